// bamextract.hip -- UMI extraction straight from the BAM records that the region split keeps (SURVEY.md §8f row
// f4+f1).
//
// The two-step path writes every kept read to region_cluster<k>.fasta (k_bam_emit, regionsplit.hip) and reads it back
// for the UMI search (extract.hip).  Here the search runs on the record where it lies: k_bam_umi_search decodes the two
// adapter windows of a kept record from its 4-bit sequence on the fly -- bam::forward_base of bam_record.h, or the
// text "None" of a sequence-less record -- and runs the two Myers passes of myers.h on each, one thread per (record,
// window), the two threads of a record in adjacent lanes.
// The window bytes come straight from global memory, a byte per two symbols: a packed window of the default 73 / 68
// symbols is at most 37 bytes at an offset only the record knows, so an LDS stage (k_extract_win's) would be filled by
// the very byte loads it is meant to replace.  The thread of the 5' window also walks the query name once (first ';',
// white space, "strand=") and writes the exact size of the record's detected-UMI text, so that the host can lay the
// output out before k_bam_emit_umi, one wave per record, writes it:
//   >{rid};strand={s};umi_fwd_dist={d5};umi_rev_dist={d3};umi_fwd_seq={u5};umi_rev_seq={u3};seq={read}\n{combined}\n
// (write_fasta, ont_tcr_consensus/extract_umis.py:154-186).  Integer VALU and byte traffic: no LDS, no atomics, no MFMA.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "bam_record.h"
#include "myers.h"
#include "umiclust_internal.h"

namespace uc {

namespace {

// the read as k_bam_emit writes it: L bytes, byte x by at(x) (bam::forward_base, or the text "None")
struct ReadText {
  const uint8_t* sq;
  int32_t lseq;
  int32_t L;
  bool rev;
  __device__ __forceinline__ char at(int x) const {
    if (lseq <= 0) return x == 0 ? 'N' : x == 1 ? 'o' : x == 2 ? 'n' : 'e';
    return bam::forward_base(sq, lseq, rev, x);
  }
};
__device__ __forceinline__ ReadText read_text(const uint8_t* rec) {
  ReadText t;
  t.lseq = bam::l_seq(rec);
  t.sq = bam::seq(rec, bam::l_read_name(rec), bam::n_cigar_op(rec));
  t.L = t.lseq > 0 ? t.lseq : 4;
  t.rev = (bam::flag(rec) & bam::kFlagReverse) != 0;
  return t;
}

constexpr int kUmiFixed = 71;  // the bytes of a record's text that are neither name, digits, UMIs nor read

}  // namespace

// res[(r * 2 + w) * 3 + {0, 1, 2}] = edit distance (-1: none <= k), start, end within window w of kept record r;
// len[r] = bytes of its detected-UMI text, 0 if either UMI is missing or the record is not kept, kUmiHostName if its
// name holds "strand=" (the host formats it), kUmiBadName if its name holds white space
__global__ __launch_bounds__(256) void k_bam_umi_search(const uint8_t* __restrict__ raw, const int64_t* __restrict__ roff,
                                                        int64_t n, const int8_t* __restrict__ cls, int32_t a5,
                                                        int32_t a3, int32_t k, const ExtractPatterns* __restrict__ P,
                                                        int32_t* __restrict__ res, int64_t* __restrict__ len) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t r = t >> 1;
  const int w = (int)(t & 1);
  const bool kept = r < n && cls[r] == kBamKept;
  int32_t o[3] = {-1, -1, -1};
  int64_t total = 0;
  if (kept) {
    const uint8_t* rec = raw + roff[r];
    const ReadText T = read_text(rec);
    // Python slicing: seq[:a5] and seq[-a3:] (a3 == 0 is the whole read)
    int w0, wl;
    if (w == 0) {
      w0 = 0;
      wl = a5 < T.L ? a5 : T.L;
    } else {
      wl = (a3 == 0 || a3 > T.L) ? T.L : a3;
      w0 = T.L - wl;
    }
    myers_locate([&](int j) { return T.at(w0 + j); }, wl, P, w, k, o);
    int32_t* q = res + t * 3;
    q[0] = o[0], q[1] = o[1], q[2] = o[2];
    if (w == 0) {
      const uint8_t* name = bam::name(rec);
      const int nl = (int)bam::l_read_name(rec) - 1;
      const uint64_t pat = 0x3d646e61727473ull;  // "strand=", byte x = its symbol x
      int rid = nl, match = 0;
      bool space = false, strand = false;
      for (int x = 0; x < nl; x++) {
        const uint8_t ch = name[x];
        if (ch == ';' && rid == nl) rid = x;
        space |= ch == ' ' || (ch >= 9 && ch <= 13);
        match = ch == (uint8_t)(pat >> (8 * match)) ? match + 1 : (ch == 's' ? 1 : 0);
        if (match == 7) strand = true, match = 0;
      }
      total = space ? kUmiBadName : strand ? kUmiHostName : (int64_t)kUmiFixed + rid + T.L;
    }
  }
  // the 3' thread's distance and UMI length, to the 5' thread in the lane below it
  const int d3 = __shfl_xor(o[0], 1), l3 = __shfl_xor(o[2] - o[1] + 1, 1);
  if (r < n && w == 0) {
    if (kept && total != kUmiBadName) {
      if (o[0] < 0 || d3 < 0) total = 0;
      else if (total > 0) total += (o[0] >= 10 ? 2 : 1) + (d3 >= 10 ? 2 : 1) + 2 * (int64_t)(o[2] - o[1] + 1 + l3);
    }
    len[r] = total;
  }
}

// one wave per record with len[r] > 0: its detected-UMI text at pos[r]
__global__ __launch_bounds__(256) void k_bam_emit_umi(const uint8_t* __restrict__ raw, const int64_t* __restrict__ roff,
                                                      int64_t n, const int64_t* __restrict__ len,
                                                      const int32_t* __restrict__ res, const int64_t* __restrict__ pos,
                                                      int32_t a3, char* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= n || len[r] <= 0) return;
  const uint8_t* rec = raw + roff[r];
  const ReadText T = read_text(rec);
  const uint8_t* name = bam::name(rec);
  const int nl = (int)bam::l_read_name(rec) - 1;
  int rid = nl;  // get_read_name: the name up to its first ';'
  for (int x0 = 0; x0 < nl && rid == nl; x0 += 64) {
    const unsigned long long m = __ballot(x0 + lane < nl && name[x0 + lane] == ';');
    if (m) rid = x0 + __ffsll(m) - 1;
  }
  const int32_t* q = res + r * 6;
  const int d5 = q[0], d3 = q[3], l5 = q[2] - q[1] + 1, l3 = q[5] - q[4] + 1;
  const int w3 = (a3 == 0 || a3 > T.L) ? T.L : a3;
  const int b5 = q[1], b3 = T.L - w3 + q[4];  // the UMIs' first bytes in the read
  const int n5 = d5 >= 10 ? 2 : 1, n3 = d3 >= 10 ? 2 : 1;
  char* o = out + pos[r];
  // field offsets: ">" rid ";strand=" s ";umi_fwd_dist=" d5 ";umi_rev_dist=" d3 ";umi_fwd_seq=" u5 ";umi_rev_seq=" u3
  // ";seq=" read "\n" combined "\n"
  const int64_t A = 1 + rid, B = A + 9, C = B + 14 + n5, D = C + 14 + n3, E = D + 13 + l5, F = E + 13 + l3,
                G = F + 5 + T.L;
  for (int x = lane; x < rid; x += 64) o[1 + x] = (char)name[x];
  if (lane == 0) {
    auto put = [&](int64_t at, const char* s, int m) {
      for (int x = 0; x < m; x++) o[at + x] = s[x];
    };
    auto num = [&](int64_t at, int v, int nd) {
      if (nd == 2) o[at++] = (char)('0' + v / 10);
      o[at] = (char)('0' + v % 10);
    };
    o[0] = '>';
    put(A, ";strand=", 8);
    o[A + 8] = T.rev ? '-' : '+';
    put(B, ";umi_fwd_dist=", 14);
    num(B + 14, d5, n5);
    put(C, ";umi_rev_dist=", 14);
    num(C + 14, d3, n3);
    put(D, ";umi_fwd_seq=", 13);
    put(E, ";umi_rev_seq=", 13);
    put(F, ";seq=", 5);
    o[G] = '\n';
    o[G + 1 + l5 + l3] = '\n';
  }
  for (int x = lane; x < l5; x += 64) o[D + 13 + x] = T.at(b5 + x);
  for (int x = lane; x < l3; x += 64) o[E + 13 + x] = T.at(b3 + x);
  for (int x = lane; x < T.L; x += 64) o[F + 5 + x] = T.at(x);
  char* cmb = o + G + 1;  // combine_umis_fasta
  if (!T.rev) {
    for (int x = lane; x < l5; x += 64) cmb[x] = T.at(b5 + x);
    for (int x = lane; x < l3; x += 64) cmb[l5 + x] = T.at(b3 + x);
  } else {
    for (int x = lane; x < l3; x += 64) cmb[x] = bam::complement(T.at(b3 + l3 - 1 - x));
    for (int x = lane; x < l5; x += 64) cmb[l3 + x] = bam::complement(T.at(b5 + l5 - 1 - x));
  }
}

hipError_t launch_bam_umi_search(const uint8_t* raw, const int64_t* roff, int64_t n, const int8_t* cls, int32_t a5,
                                 int32_t a3, int32_t k, const ExtractPatterns* P, int32_t* res, int64_t* len,
                                 hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_bam_umi_search, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, st, raw, roff, n, cls, a5,
                     a3, k, P, res, len);
  return hipGetLastError();
}

hipError_t launch_bam_emit_umi(const uint8_t* raw, const int64_t* roff, int64_t n, const int64_t* len,
                               const int32_t* res, const int64_t* pos, int32_t a3, char* out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_bam_emit_umi, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, raw, roff, n, len, res, pos, a3,
                     out);
  return hipGetLastError();
}

}  // namespace uc
