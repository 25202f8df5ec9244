// samsort.hip -- a BAM session's raw and roff from SAM text, on the device.
//
// Four steps on the text after the header, each a few small kernels:
//   lines    k_sam_count_lines / k_scan_i64 / k_sam_scatter_lines: the start of every record line.  A wave takes
//            kChunk bytes, 64 a step, and finds the newlines by ballot.
//   measure  k_sam_measure: one wave per line on sam::measure of sam_text.h -- the code sam::encode_host runs on the
//            host -- with an Io whose 64 lanes work together: a field's end is the first tab of a 64-byte step's
//            ballot, names are hashed and compared lane-strided, CIGAR and aux are sized.  Per line: the field table,
//            size, key, status; per launch: the first refused line, the OR of all keys, the count of aux f values.
//   sort     k_iota, then per 8-bit digit that the OR of the keys has a bit in: k_radix_hist / k_scan_i64 /
//            k_radix_scatter, a stable LSD radix sort of (key, line).  8 bytes of key a record against kilobytes of
//            text: written for simplicity.
//   encode   k_gather_size / k_scan_i64 give roff; k_sam_encode takes one wave per record in sorted order on
//            sam::encode: the fixed fields by lane 0, name, CIGAR, packed bases, qualities and aux lane-strided.  The
//            aux f values are listed for the host, which parses them; k_sam_put_f stores what it parsed.
// Plain C++ with wave intrinsics, vector stores only.  Integer byte-streaming work: no MFMA.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "sam_text.h"
#include "umiclust_internal.h"

namespace uc {

namespace {

constexpr int kChunk = 4096;  // text bytes of one wave of the line kernels
constexpr int kSortTile = 256;    // keys of one workgroup of the sort, one a thread

__device__ inline uint64_t wave_sum(uint64_t v) {
  for (int d = 32; d; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d);
  return v;
}

struct WaveIo {
  const uint8_t* body;
  uint8_t* rec;           // the record being written (encode)
  int64_t rec_at, line;   // its offset in raw, its input line
  sam::FSlot* slots;      // the aux f values of the launch, appended through *nslots, at most cap of them
  unsigned long long* nslots;
  int64_t cap;
  int ln;

  __device__ int lane() const { return ln; }
  __device__ int lanes() const { return 64; }
  __device__ uint8_t at(int64_t p) const { return body[p]; }
  // the first c in [s, e), else e: 64 bytes a step
  __device__ int64_t find(int64_t s, int64_t e, uint8_t c) const {
    for (int64_t q = s; q < e; q += 64) {
      const int64_t i = q + ln;
      const unsigned long long m = __ballot(i < e && body[i] == c);
      if (m) return q + (__ffsll((long long)m) - 1);
    }
    return e;
  }
  __device__ uint64_t sum(uint64_t v) const { return wave_sum(v); }
  __device__ bool any(bool v) const { return __ballot(v) != 0; }
  __device__ int rank(bool v, int& total) const {
    const unsigned long long m = __ballot(v);
    total = __popcll(m);
    return __popcll(m & ((1ull << ln) - 1));
  }
  __device__ void put(int64_t o, uint8_t b) { rec[o] = b; }
  __device__ void fslot(int64_t o, int64_t text) {
    const unsigned long long k = atomicAdd(nslots, 1ull);
    if ((int64_t)k < cap) slots[k] = {rec_at + o, text, line};
  }
};

// ---------------------------------------------------------------- lines
// a line starts after every '\n' that is not the text's last byte
__global__ __launch_bounds__(64) void k_sam_count_lines(const uint8_t* __restrict__ body, int64_t n,
                                                        int64_t* __restrict__ count) {
  const int64_t base = (int64_t)blockIdx.x * kChunk, end = min(base + kChunk, n);
  int64_t c = 0;
  for (int64_t q = base; q < end; q += 64) {
    const int64_t i = q + threadIdx.x;
    c += __popcll(__ballot(i < end && i + 1 < n && body[i] == '\n'));
  }
  if (threadIdx.x == 0) count[blockIdx.x] = c;
}
// start[0] = 0, start[1 + k] = the byte after the k-th such '\n', start[nlines] = one past the last line's end + 1
__global__ __launch_bounds__(64) void k_sam_scatter_lines(const uint8_t* __restrict__ body, int64_t n,
                                                          const int64_t* __restrict__ first, int64_t nlines,
                                                          int64_t* __restrict__ start) {
  const int64_t base = (int64_t)blockIdx.x * kChunk, end = min(base + kChunk, n);
  int64_t k = 1 + first[blockIdx.x];
  for (int64_t q = base; q < end; q += 64) {
    const int64_t i = q + threadIdx.x;
    const bool hit = i < end && i + 1 < n && body[i] == '\n';
    const unsigned long long m = __ballot(hit);
    if (hit) start[k + __popcll(m & ((1ull << threadIdx.x) - 1))] = i + 1;
    k += __popcll(m);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    start[0] = 0;
    start[nlines] = n + (body[n - 1] != '\n');
  }
}

// out[i] = base + in[0] + .. + in[i - 1], *total = base + the sum: one workgroup, 8 adjacent entries a thread and
// 2048 a step.  in may be out.
__global__ __launch_bounds__(256) void k_scan_i64(const int64_t* in, int64_t* out, int64_t n, int64_t base,
                                                  int64_t* total) {
  __shared__ int64_t sh[256];
  __shared__ int64_t carry;
  const int t = (int)threadIdx.x;
  if (t == 0) carry = base;
  __syncthreads();
  for (int64_t i0 = 0; i0 < n; i0 += 2048) {
    const int64_t b = i0 + t * 8;
    int64_t v[8], mine = 0;
    for (int k = 0; k < 8; k++) mine += v[k] = b + k < n ? in[b + k] : 0;
    sh[t] = mine;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const int64_t add = t >= d ? sh[t - d] : 0;
      __syncthreads();
      sh[t] += add;
      __syncthreads();
    }
    int64_t run = carry + sh[t] - mine;
    for (int k = 0; k < 8; k++)
      if (b + k < n) out[b + k] = run, run += v[k];
    __syncthreads();
    if (t == 255) carry += sh[255];
    __syncthreads();
  }
  if (t == 0 && total) *total = carry;
}

// ---------------------------------------------------------------- measure
// acc[0] = the first refused line (min), acc[1] = the OR of the accepted lines' keys, acc[2] = their aux f values
__global__ __launch_bounds__(64) void k_sam_measure(const uint8_t* __restrict__ body, const int64_t* __restrict__ start,
                                                    int64_t n, sam::Names N, sam::Fields* __restrict__ fields,
                                                    int64_t* __restrict__ size, unsigned long long* __restrict__ key,
                                                    int32_t* __restrict__ status, unsigned long long* acc) {
  __shared__ sam::Fields F;
  const int64_t l = blockIdx.x;
  if (l >= n) return;
  WaveIo io{body, nullptr, 0, l, nullptr, nullptr, 0, (int)threadIdx.x};
  const sam::Measured M = sam::measure(io, N, start[l], start[l + 1] - 1, F);
  __syncthreads();
  if (threadIdx.x < 12) fields[l].f[threadIdx.x] = F.f[threadIdx.x];
  if (threadIdx.x == 0) {
    size[l] = M.size, key[l] = M.key, status[l] = M.status;
    if (M.status) {
      atomicMin(&acc[0], (unsigned long long)l);
    } else {
      atomicOr(&acc[1], (unsigned long long)M.key);
      if (M.nf) atomicAdd(&acc[2], (unsigned long long)M.nf);
    }
  }
}

// ---------------------------------------------------------------- sort
__global__ __launch_bounds__(256) void k_iota(uint32_t* __restrict__ idx, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) idx[i] = (uint32_t)i;
}
// hist[d * nb + b] = keys of tile b whose digit is d
__global__ __launch_bounds__(kSortTile) void k_radix_hist(const unsigned long long* __restrict__ key, int64_t n, int shift,
                                                      int64_t* __restrict__ hist, int64_t nb) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kSortTile + threadIdx.x;
  if (i < n) atomicAdd(&h[(key[i] >> shift) & 255], 1u);
  __syncthreads();
  hist[(int64_t)threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];
}
// first = the exclusive scan of hist: where the first key of tile b with digit d goes.  A key's place among its
// tile's keys of the same digit is its rank among them in its wave plus their counts in the waves before it.
__global__ __launch_bounds__(kSortTile) void k_radix_scatter(const unsigned long long* __restrict__ key,
                                                         const uint32_t* __restrict__ idx, int64_t n, int shift,
                                                         const int64_t* __restrict__ first, int64_t nb,
                                                         unsigned long long* __restrict__ key_out,
                                                         uint32_t* __restrict__ idx_out) {
  __shared__ uint32_t per_wave[kSortTile / 64][256];
  const int t = (int)threadIdx.x, w = t >> 6, ln = t & 63;
  for (int x = 0; x < kSortTile / 64; x++) per_wave[x][t] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kSortTile + t;
  const bool valid = i < n;
  const unsigned long long k = valid ? key[i] : 0;
  const uint32_t d = (uint32_t)(k >> shift) & 255u;
  unsigned long long peers = __ballot(valid);  // the lanes of this wave that hold the same digit
  for (int b = 0; b < 8; b++) {
    const bool bit = (d >> b) & 1u;
    const unsigned long long m = __ballot(bit);
    peers &= bit ? m : ~m;
  }
  const int rank = __popcll(peers & ((1ull << ln) - 1));
  if (valid && rank == 0) per_wave[w][d] = (uint32_t)__popcll(peers);
  __syncthreads();
  if (valid) {
    int64_t o = first[(int64_t)d * nb + blockIdx.x] + rank;
    for (int x = 0; x < w; x++) o += per_wave[x][d];
    key_out[o] = k;
    idx_out[o] = idx[i];
  }
}

// ---------------------------------------------------------------- encode
__global__ __launch_bounds__(256) void k_gather_size(const int64_t* __restrict__ size, const uint32_t* __restrict__ idx,
                                                     int64_t n, int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = size[idx[i]];
}
// record r = line idx[r] at raw + roff[r]; every byte written lies in [roff[r], roff[r] + size[idx[r]])
__global__ __launch_bounds__(64) void k_sam_encode(const uint8_t* __restrict__ body, const int64_t* __restrict__ start,
                                                   const uint32_t* __restrict__ idx, const int64_t* __restrict__ roff,
                                                   int64_t n, sam::Names N, const sam::Fields* __restrict__ fields,
                                                   const int64_t* __restrict__ size, uint8_t* __restrict__ raw,
                                                   sam::FSlot* slots, unsigned long long* nslots, int64_t cap) {
  const int64_t r = blockIdx.x;
  if (r >= n) return;
  const int64_t l = idx[r];
  WaveIo io{body, raw + roff[r], roff[r], l, slots, nslots, cap, (int)threadIdx.x};
  sam::encode(io, N, start[l], start[l + 1] - 1, fields[l], size[l]);
}
__global__ __launch_bounds__(256) void k_sam_put_f(uint8_t* __restrict__ raw, const int64_t* __restrict__ at,
                                                   const uint32_t* __restrict__ bits, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  for (int k = 0; k < 4; k++) raw[at[i] + k] = (uint8_t)(bits[i] >> (8 * k));
}

unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

hipError_t launch_scan_i64(const int64_t* in, int64_t* out, int64_t n, int64_t base, int64_t* total, hipStream_t st) {
  hipLaunchKernelGGL(k_scan_i64, dim3(1), dim3(256), 0, st, in, out, n, base, total);
  return hipGetLastError();
}

int64_t sam_line_chunks(int64_t n) { return (n + kChunk - 1) / kChunk; }

hipError_t launch_sam_count_lines(const uint8_t* body, int64_t n, int64_t* count, int64_t* first, int64_t* total,
                                  hipStream_t st) {
  const int64_t nc = sam_line_chunks(n);
  if (nc <= 0) return hipSuccess;
  if (nc > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_sam_count_lines, dim3((unsigned)nc), dim3(64), 0, st, body, n, count);
  return launch_scan_i64(count, first, nc, 0, total, st);
}

hipError_t launch_sam_scatter_lines(const uint8_t* body, int64_t n, const int64_t* first, int64_t nlines,
                                    int64_t* start, hipStream_t st) {
  const int64_t nc = sam_line_chunks(n);
  if (nc <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_sam_scatter_lines, dim3((unsigned)nc), dim3(64), 0, st, body, n, first, nlines, start);
  return hipGetLastError();
}

hipError_t launch_sam_measure(const uint8_t* body, const int64_t* start, int64_t n, const sam::Names& N,
                              sam::Fields* fields, int64_t* size, uint64_t* key, int32_t* status, uint64_t* acc,
                              hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (n > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_sam_measure, dim3((unsigned)n), dim3(64), 0, st, body, start, n, N, fields, size,
                     (unsigned long long*)key, status, (unsigned long long*)acc);
  return hipGetLastError();
}

hipError_t launch_sam_sort(uint64_t* key_a, uint32_t* idx_a, uint64_t* key_b, uint32_t* idx_b, int64_t n,
                           uint64_t key_bits, int64_t* hist, const uint32_t** sorted_idx, hipStream_t st) {
  *sorted_idx = idx_a;
  if (n <= 0) return hipSuccess;
  const int64_t nb = (n + kSortTile - 1) / kSortTile;
  hipLaunchKernelGGL(k_iota, dim3(blocks_of(n, 256)), dim3(256), 0, st, idx_a, n);
  auto *ka = (unsigned long long*)key_a, *kb = (unsigned long long*)key_b;
  for (int shift = 0; shift < 64; shift += 8) {
    if (!((key_bits >> shift) & 255)) continue;  // every key has the same digit here: the pass would move nothing
    hipLaunchKernelGGL(k_radix_hist, dim3((unsigned)nb), dim3(kSortTile), 0, st, ka, n, shift, hist, nb);
    const hipError_t e = launch_scan_i64(hist, hist, 256 * nb, 0, nullptr, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_radix_scatter, dim3((unsigned)nb), dim3(kSortTile), 0, st, ka, idx_a, n, shift, hist, nb, kb,
                       idx_b);
    std::swap(ka, kb), std::swap(idx_a, idx_b);
  }
  *sorted_idx = idx_a;
  return hipGetLastError();
}

hipError_t launch_sam_roff(const int64_t* size, const uint32_t* idx, int64_t n, int64_t base, int64_t* roff,
                           int64_t* total, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(k_gather_size, dim3(blocks_of(n, 256)), dim3(256), 0, st, size, idx, n, roff);
  return launch_scan_i64(roff, roff, n > 0 ? n : 0, base, total, st);
}

hipError_t launch_sam_encode(const uint8_t* body, const int64_t* start, const uint32_t* idx, const int64_t* roff,
                             int64_t n, const sam::Names& N, const sam::Fields* fields, const int64_t* size,
                             uint8_t* raw, sam::FSlot* slots, uint64_t* nslots, int64_t cap, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_sam_encode, dim3((unsigned)n), dim3(64), 0, st, body, start, idx, roff, n, N, fields, size, raw,
                     slots, (unsigned long long*)nslots, cap);
  return hipGetLastError();
}

hipError_t launch_sam_put_f(uint8_t* raw, const int64_t* at, const uint32_t* bits, int64_t n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_sam_put_f, dim3(blocks_of(n, 256)), dim3(256), 0, st, raw, at, bits, n);
  return hipGetLastError();
}

}  // namespace uc
