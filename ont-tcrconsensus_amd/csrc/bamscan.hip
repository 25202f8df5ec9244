// bamscan.hip -- the BAM record scan with aux tags and the exact group-by of cs:Z strings (SURVEY.md §8f row f6,
// DESIGN.md §9b).
//
// Replaces the per-record Python loops of ont_tcr_consensus/minimap2_align.py: count_cs_tags (:21-37), calculate_blast_id
// (:13-18) and the record loop of filter_consensus_alignments (:209-245).  The BGZF blocks are inflated on the device (bgzf.hip)
// and the host finds the record offsets (bam_host.cpp); here one wave per record decodes the fixed fields, sums the CIGAR
// lane-strided (reference_length = M/D/N/=/X, cols = M/I/D), and walks the aux fields of a primary record with a
// wave-uniform cursor: fixed-size types advance by their size, B arrays by subtype size x count, Z/H strings are
// searched for their NUL 64 bytes a step with a ballot.  The cs string is hashed in the pass that finds its NUL (a sum
// of mixed per-position terms, so the lanes of a step add independently).  k_cs_group claims a slot per distinct
// hash in an open-addressing table (overlap.hip's scheme: CAS claim, atomicMin of the record index into the slot's
// representative, atomicAdd on its count) and k_cs_verify compares every record's bytes with its representative's; a
// mismatch raises the collision flag and the host re-runs with the next seed, so the groups are exact.  Byte-streaming
// integer work: HBM-bound, no MFMA.  bam_host.cpp scan_record is the serial walk over the same rules (bam_record.h).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "bam_host.h"
#include "umiclust_internal.h"

namespace uc {

namespace {

__device__ __forceinline__ int64_t wave_sum(int64_t v) {
  for (int d = 32; d > 0; d >>= 1) v += (int64_t)__shfl_xor((long long)v, d, 64);
  return v;
}

constexpr int kScanWaves = 4;  // records per workgroup

}  // namespace

// one wave per record; every byte read lies in [roff[r], min(record end, raw_len))
__global__ __launch_bounds__(kScanWaves * 64) void k_bam_scan(const uint8_t* __restrict__ raw, int64_t raw_len,
                                                              const int64_t* __restrict__ roff, int64_t n,
                                                              uint64_t seed, uint64_t hmask, BamScanCols o) {
  const int64_t r = (int64_t)blockIdx.x * kScanWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= n) return;
  const int64_t ro = roff[r];
  const uint8_t* rec = raw + ro;
  int64_t end = ro + 4 + (int64_t)bam::block_size(rec);
  if (end > raw_len) end = raw_len;
  const uint32_t lrn = bam::l_read_name(rec), ncig = bam::n_cigar_op(rec), flag = bam::flag(rec);
  const int32_t lseq = bam::l_seq(rec);
  const int8_t cls = (flag & bam::kFlagUnmapped) ? bam::kScanUnmapped
                     : (flag & bam::kFlagNotPrimary) ? bam::kScanSecondary : bam::kScanPrimary;
  const uint8_t* cig = bam::cigar(rec, lrn);
  const int64_t aux = ro + bam::aux_offset(lrn, ncig, lseq);
  int8_t bad = 0;
  int64_t rl = 0, cols = 0, nm = 0, cs_off = 0;
  int32_t cs_len = -1;
  uint8_t nm_present = 0;
  uint64_t cs_hash = 0;
  if (lseq < 0 || aux > end) {
    bad = 1;
  } else {
    for (uint32_t x = (uint32_t)lane; x < ncig; x += 64) {
      const uint32_t v = bam::le32(cig + 4 * (int64_t)x), op = v & 15u;
      if (bam::op_on_reference(op)) rl += v >> 4;
      if (bam::op_in_columns(op)) cols += v >> 4;
    }
    rl = bam::reference_span(wave_sum(rl));
    cols = wave_sum(cols);
    if (cls == bam::kScanPrimary) {
      bool have_nm = false, have_cs = false;
      int64_t cur = aux;  // wave-uniform: every lane reads the same tag and type bytes
      while (cur < end && !bad) {
        if (cur + 3 > end) {
          bad = 1;
          break;
        }
        const uint8_t t0 = raw[cur], t1 = raw[cur + 1], ty = raw[cur + 2];
        const bool is_nm = t0 == 'N' && t1 == 'M' && !have_nm, is_cs = t0 == 'c' && t1 == 's' && !have_cs;
        const int64_t v = cur + 3;
        const int sz = bam::aux_fixed_size(ty);
        if (sz) {
          if (v + sz > end || is_cs || (is_nm && (ty == 'A' || ty == 'f'))) {
            bad = 1;
            break;
          }
          if (is_nm) {
            nm = bam::aux_int_value(ty, raw + v);
            nm_present = 1;
            have_nm = true;
          }
          cur = v + sz;
        } else if (ty == 'B') {
          if (v + 5 > end || is_nm || is_cs) {
            bad = 1;
            break;
          }
          const int64_t cnt = (int64_t)bam::le32(raw + v + 1);
          const int ss = bam::aux_array_elem_size(raw[v]);
          if (!ss || v + 5 + ss * cnt > end) {
            bad = 1;
            break;
          }
          cur = v + 5 + ss * cnt;
        } else if (ty == 'Z' || ty == 'H') {
          if (is_nm || (is_cs && ty != 'Z')) {
            bad = 1;
            break;
          }
          int64_t z = v, nul = -1;
          uint64_t sum = 0;
          while (z < end) {  // 64 bytes a step; a lane past the record end reads nothing
            const int64_t idx = z + lane;
            const bool in = idx < end;
            const uint8_t b = in ? raw[idx] : (uint8_t)1;
            const unsigned long long m = __ballot(in && b == 0);
            const int first = m ? __ffsll(m) - 1 : 64;
            if (is_cs && in && lane < first) sum += bam::cs_term(seed, (uint64_t)(idx - v), b);
            if (m) {
              nul = z + first;
              break;
            }
            z += 64;
          }
          if (nul < 0) {  // no NUL before the record end
            bad = 1;
            break;
          }
          if (is_cs) {
            sum = (uint64_t)wave_sum((int64_t)sum);
            cs_off = v;
            cs_len = (int32_t)(nul - v);
            cs_hash = bam::cs_finish(sum, (uint64_t)(nul - v), hmask);
            have_cs = true;
          }
          cur = nul + 1;
        } else {
          bad = 1;
        }
      }
    }
  }
  if (lane == 0) {
    o.cls[r] = cls;
    o.ref[r] = bam::ref_id(rec);
    o.l_seq[r] = lseq;
    o.reflen[r] = rl;
    o.cols[r] = cols;
    o.nm[r] = nm;
    o.nm_present[r] = nm_present;
    o.cs_off[r] = cs_off;
    o.cs_len[r] = cs_len;
    o.cs_hash[r] = cs_hash;
    o.bad[r] = bad;
  }
}

// every primary record with a cs tag: claim the slot of its hash (linear probing), representative = lowest record
__global__ void k_cs_group(const BamScanCols o, int64_t n, uint64_t mask, unsigned long long* __restrict__ keys,
                           unsigned long long* __restrict__ rep, uint32_t* __restrict__ cnt,
                           int64_t* __restrict__ slot) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  if (o.cls[r] != bam::kScanPrimary || o.bad[r] || o.cs_len[r] < 0) {
    slot[r] = -1;
    return;
  }
  const uint64_t h = o.cs_hash[r];
  uint64_t s = h & mask;
  while (true) {
    const unsigned long long prev = atomicCAS(&keys[s], (unsigned long long)bam::kCsEmpty, (unsigned long long)h);
    if (prev == bam::kCsEmpty || prev == h) break;
    s = (s + 1) & mask;
  }
  atomicMin(&rep[s], (unsigned long long)r);
  atomicAdd(&cnt[s], 1u);
  slot[r] = (int64_t)s;
}

// one wave per grouped record: length first, then the bytes against the representative's
__global__ __launch_bounds__(kScanWaves * 64) void k_cs_verify(const uint8_t* __restrict__ raw, const BamScanCols o,
                                                               int64_t n, const int64_t* __restrict__ slot,
                                                               const unsigned long long* __restrict__ rep,
                                                               uint32_t* __restrict__ collision) {
  const int64_t r = (int64_t)blockIdx.x * kScanWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= n) return;
  const int64_t s = slot[r];
  if (s < 0) return;
  const int64_t q = (int64_t)rep[s];
  if (q == r) return;
  const int32_t len = o.cs_len[r];
  bool ne = len != o.cs_len[q];
  if (!ne) {
    const uint8_t* a = raw + o.cs_off[r];
    const uint8_t* b = raw + o.cs_off[q];
    for (int32_t x = lane; x < len; x += 64) ne |= a[x] != b[x];
  }
  if (__ballot(ne) && lane == 0) atomicOr(collision, 1u);
}

hipError_t launch_bam_scan(const uint8_t* raw, int64_t raw_len, const int64_t* roff, int64_t n, uint64_t seed,
                           uint64_t hmask, const BamScanCols& o, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_bam_scan, dim3((unsigned)((n + kScanWaves - 1) / kScanWaves)), dim3(kScanWaves * 64), 0, st, raw,
                     raw_len, roff, n, seed, hmask, o);
  return hipGetLastError();
}

hipError_t launch_cs_group(const uint8_t* raw, const BamScanCols& o, int64_t n, uint64_t mask, unsigned long long* keys,
                           unsigned long long* rep, uint32_t* cnt, int64_t* slot, uint32_t* collision,
                           hipStream_t st) {
  hipError_t e = hipMemsetAsync(keys, 0xff, (size_t)(mask + 1) * 8, st);
  if (e == hipSuccess) e = hipMemsetAsync(rep, 0xff, (size_t)(mask + 1) * 8, st);
  if (e == hipSuccess) e = hipMemsetAsync(cnt, 0, (size_t)(mask + 1) * 4, st);
  if (e == hipSuccess) e = hipMemsetAsync(collision, 0, 4, st);
  if (e != hipSuccess || n <= 0) return e;
  hipLaunchKernelGGL(k_cs_group, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, o, n, mask, keys, rep, cnt, slot);
  hipLaunchKernelGGL(k_cs_verify, dim3((unsigned)((n + kScanWaves - 1) / kScanWaves)), dim3(kScanWaves * 64), 0, st, raw,
                     o, n, slot, rep, collision);
  return hipGetLastError();
}

}  // namespace uc
