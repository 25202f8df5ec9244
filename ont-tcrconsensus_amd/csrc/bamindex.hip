// bamindex.hip -- the .bai index and flagstat of the session's kept records, on the device.
//
// The rules are those of bam_index.h, which bai::build_host runs serially on the host; here one thread takes a record.
//   keys    k_bai_mark / k_scan_i64 twice: which records are kept, where each starts in the written stream and which
//           kept record it is.  k_bai_keys: per kept record its reference, bin, windows, the virtual offsets of its
//           start and end (a binary search of the block table), its own status, the 32 flagstat counters and the
//           per-reference counts -- each reduced over the wave, then one atomic per wave and counter.
//   runs    k_bai_heads: the order test against the kept record before, and the head flag where (reference, bin)
//           changes; k_scan_i64; k_bai_runs scatters one (reference, bin, start, end) per run and its sort key.
//   sort    the stable radix sort of samsort.hip over the keys, then k_bai_gather.
//   linear  k_bai_linear: a 64-bit atomicMin per window a record touches; k_bai_fill: a wave per reference walks its
//           windows from the right, 64 a step, and gives every untouched one the next touched one's value.
// Plain C++ with wave intrinsics, vector stores only.  Integer work on a few dozen bytes a record: no MFMA.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "bam_index.h"
#include "umiclust_internal.h"

namespace uc {

namespace {

typedef unsigned long long u64;

__global__ __launch_bounds__(256) void k_bai_mark(BaiIn I, int64_t* __restrict__ kf, int64_t* __restrict__ sz) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= I.n) return;
  const bool kept = !I.keep || I.keep[r];
  kf[r] = kept ? 1 : 0;
  sz[r] = kept ? 4 + (int64_t)bam::block_size(I.raw + I.roff[r]) : 0;
}

// kidx[r] = the kept records before r, spos[r] = where record r starts in the written stream
__global__ __launch_bounds__(256) void k_bai_keys(BaiIn I, const int64_t* __restrict__ kidx,
                                                  const int64_t* __restrict__ spos, BaiCols o, BaiAcc A) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63);
  const bool kept = r < I.n && (!I.keep || I.keep[r]);
  bai::Rec R{};
  uint32_t rows = 0;
  bool placed = false, ok = false;
  int32_t w1 = 0;
  if (kept) {
    const uint8_t* p = I.raw + I.roff[r];
    R = bai::read_record(p);
    rows = bai::flagstat_rows(R);
    const int32_t st = bai::range_status(R, I.nref);
    placed = R.tid >= 0 && R.tid < I.nref;
    ok = placed && st != bai::kRange;
    w1 = ok ? (int32_t)((R.end - 1) >> 14) : 0;
    const int64_t j = kidx[r], at = spos[r], size = 4 + (int64_t)bam::block_size(p);
    o.rec[j] = (uint32_t)r, o.tid[j] = R.tid, o.beg[j] = (int32_t)R.beg, o.status[j] = st;
    o.bin[j] = ok ? bam::reg2bin(R.beg, R.end) : 0;
    o.w0[j] = ok ? (int32_t)(R.beg >> 14) : 0, o.w1[j] = w1;
    o.u[j] = I.nblocks ? bai::voffset(at, I.coff, I.ustart, I.nblocks) : 0;
    o.v[j] = I.nblocks ? bai::voffset(at + size, I.coff, I.ustart, I.nblocks) : 0;
  }
  const bool qcfail = (R.flag & bam::kFlagQcFail) != 0;
  for (int k = 0; k < 16; k++) {
    const bool hit = (rows >> k) & 1u;
    const int all = __popcll(__ballot(hit)), fail = __popcll(__ballot(hit && qcfail));
    if (lane == 0 && all != fail) atomicAdd((u64*)&A.counters[2 * k], (u64)(all - fail));
    if (lane == 0 && fail) atomicAdd((u64*)&A.counters[2 * k + 1], (u64)fail);
  }
  const int nocoor = __popcll(__ballot(kept && R.tid < 0));
  if (lane == 0 && nocoor) atomicAdd((u64*)A.n_no_coor, (u64)nocoor);
  // per reference: the lanes of one reference answer together (sorted input: one or two references a wave)
  u64 todo = __ballot(placed);
  while (todo) {
    const int lead = __ffsll((long long)todo) - 1;
    const int32_t t = __shfl(R.tid, lead);
    const bool mine = placed && R.tid == t;
    const u64 group = __ballot(mine);
    const int nmapped = __popcll(__ballot(mine && !(R.flag & bam::kFlagUnmapped))), nunmapped = __popcll(group) - nmapped;
    int intv = mine && ok ? w1 + 1 : 0;
    for (int d = 32; d; d >>= 1) intv = max(intv, __shfl_xor(intv, d));
    if (lane == lead) {
      if (nmapped) atomicAdd((u64*)&A.mapped[t], (u64)nmapped);
      if (nunmapped) atomicAdd((u64*)&A.unmapped[t], (u64)nunmapped);
      if (intv) atomicMax((u64*)&A.n_intv[t], (u64)intv);
    }
    todo &= ~group;
  }
}

__global__ __launch_bounds__(256) void k_bai_heads(BaiCols o, const int64_t* __restrict__ nk,
                                                   int64_t* __restrict__ head, u64* first_bad) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= nk[0]) return;
  int32_t st = o.status[j];
  const int32_t tid = o.tid[j];
  if (!st && j > 0 && bai::out_of_order(o.tid[j - 1], o.beg[j - 1], tid, o.beg[j])) o.status[j] = st = bai::kUnsorted;
  if (st) atomicMin(first_bad, ((u64)o.rec[j] << 2) | (u64)st);
  head[j] = (tid >= 0 && (j == 0 || tid != o.tid[j - 1] || o.bin[j] != o.bin[j - 1])) ? 1 : 0;
}

// hx = the exclusive scan of head: a record's run is hx[j] + head[j] - 1
__global__ __launch_bounds__(256) void k_bai_runs(BaiCols o, const int64_t* __restrict__ nk,
                                                  const int64_t* __restrict__ head, const int64_t* __restrict__ hx,
                                                  bai::Run* __restrict__ runs, u64* __restrict__ key) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= nk[0] || o.tid[j] < 0) return;
  const int64_t run = hx[j] + head[j] - 1;
  if (run < 0) return;  // (unsorted input only: a placed record after one without a reference that starts no run)
  if (head[j]) {
    runs[run].tid = o.tid[j], runs[run].bin = o.bin[j], runs[run].u = o.u[j];
    key[run] = ((u64)(uint32_t)o.tid[j] << 16) | (u64)(uint32_t)o.bin[j];
  }
  if (j + 1 == nk[0] || head[j + 1] || o.tid[j + 1] < 0) runs[run].v = o.v[j];
}

__global__ __launch_bounds__(256) void k_bai_gather(const bai::Run* __restrict__ runs, const uint32_t* __restrict__ idx,
                                                    int64_t n, bai::Run* __restrict__ sorted) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s < n) sorted[s] = runs[idx[s]];
}

__global__ __launch_bounds__(256) void k_bai_linear(BaiCols o, const int64_t* __restrict__ nk,
                                                    const int64_t* __restrict__ base, const uint64_t* __restrict__ n_intv,
                                                    int32_t nref, u64* win) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= nk[0]) return;
  const int32_t tid = o.tid[j];
  if (tid < 0 || tid >= nref) return;
  const int64_t hi = min((int64_t)o.w1[j], (int64_t)n_intv[tid] - 1);
  const u64 u = o.u[j];
  for (int64_t w = o.w0[j]; w <= hi; w++) atomicMin(&win[base[tid] + w], u);
}

__global__ __launch_bounds__(64) void k_bai_fill(const int64_t* __restrict__ base, const uint64_t* __restrict__ n_intv,
                                                 int32_t nref, u64* win) {
  const int32_t t = (int32_t)blockIdx.x;
  if (t >= nref) return;
  const int lane = (int)threadIdx.x;
  u64* const w = win + base[t];
  u64 carry = ~0ull;  // the value of the nearest touched window to the right of this step
  for (int64_t hi = (int64_t)n_intv[t]; hi > 0; hi -= 64) {
    const int64_t i = hi - 64 + lane;  // this step: windows [hi - 64, hi), lane 0 the leftmost
    const u64 x = i >= 0 ? w[i] : ~0ull;
    const u64 touched = __ballot(i >= 0 && x != ~0ull) >> lane;  // bit 0: this lane; the next set bit: its source
    const int src = touched ? lane + __ffsll((long long)touched) - 1 : lane;
    const u64 got = (u64)__shfl((long long)x, src);
    const u64 val = touched ? got : carry;
    if (i >= 0 && x == ~0ull) w[i] = val;
    carry = (u64)__shfl((long long)val, 0);
  }
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

hipError_t launch_bai_keys(const BaiIn& I, int64_t* scratch, int64_t* nk, const BaiCols& o, const BaiAcc& A,
                           hipStream_t st) {
  int64_t *kf = scratch, *sz = kf + I.n + 1, *kidx = sz + I.n + 1, *spos = kidx + I.n + 1;
  if (I.n > 0) hipLaunchKernelGGL(k_bai_mark, dim3(blocks_of(I.n)), dim3(256), 0, st, I, kf, sz);
  hipError_t e = launch_scan_i64(kf, kidx, I.n, 0, nk, st);
  if (e == hipSuccess) e = launch_scan_i64(sz, spos, I.n, I.header_end, nullptr, st);
  if (e != hipSuccess || I.n <= 0) return e;
  hipLaunchKernelGGL(k_bai_keys, dim3(blocks_of(I.n)), dim3(256), 0, st, I, kidx, spos, o, A);
  return hipGetLastError();
}

hipError_t launch_bai_runs(const BaiCols& o, int64_t n, const int64_t* nk, int64_t* head, int64_t* hx, int64_t* nruns,
                           uint64_t* first_bad, bai::Run* runs, uint64_t* key, hipStream_t st) {
  if (n > 0) {
    hipError_t e = hipMemsetAsync(head, 0, (size_t)n * 8, st);  // past the kept records: no head
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_bai_heads, dim3(blocks_of(n)), dim3(256), 0, st, o, nk, head, (u64*)first_bad);
  }
  const hipError_t e = launch_scan_i64(head, hx, n, 0, nruns, st);
  if (e != hipSuccess || n <= 0) return e;
  hipLaunchKernelGGL(k_bai_runs, dim3(blocks_of(n)), dim3(256), 0, st, o, nk, head, hx, runs, (u64*)key);
  return hipGetLastError();
}

hipError_t launch_bai_gather(const bai::Run* runs, const uint32_t* idx, int64_t nruns, bai::Run* sorted, hipStream_t st) {
  if (nruns <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_bai_gather, dim3(blocks_of(nruns)), dim3(256), 0, st, runs, idx, nruns, sorted);
  return hipGetLastError();
}

hipError_t launch_bai_linear(const BaiCols& o, int64_t n, const int64_t* nk, const int64_t* base, const uint64_t* n_intv,
                             int32_t nref, uint64_t* win, int64_t nwin, hipStream_t st) {
  if (n <= 0 || nwin <= 0 || nref <= 0) return hipSuccess;
  const hipError_t e = hipMemsetAsync(win, 0xff, (size_t)nwin * 8, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_bai_linear, dim3(blocks_of(n)), dim3(256), 0, st, o, nk, base, n_intv, nref, (u64*)win);
  hipLaunchKernelGGL(k_bai_fill, dim3((unsigned)nref), dim3(64), 0, st, base, n_intv, nref, (u64*)win);
  return hipGetLastError();
}

}  // namespace uc
