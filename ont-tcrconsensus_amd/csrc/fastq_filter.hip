// fastq_filter.hip -- the quality kernel of the `vsearch --fastq_filter` drop-in (row f5), gfx950.
//
// Per record: ee_fx = sum over its quality bytes b of table[b] (u64 fixed point, 2^-40 units; the ascii offset is
// folded into the table and out-of-range bytes map to 0) and the smallest / largest raw byte.  Integer sums do not
// depend on the order of the additions, so the result is deterministic whatever the lane mapping.
//
// One wave per record, four records per 256-thread block.  ONT reads are ~1.5 kb, so a record is one or two
// 1 KiB wave loads and the launch has tens of thousands of waves per chunk; sub-wave groups would only help records
// below 256 bases, which the step's own --fastq_minlen discards unread.  Lane l of iteration k loads the 16 aligned
// bytes at (start & ~15) + 16 * (64 k + l): consecutive lanes read consecutive 16-byte slots (one global_load_dwordx4
// per lane, 1 KiB per wave).  Records start at arbitrary byte offsets of the concatenated buffer, so a lane whose slot
// straddles the record's first or last byte masks the bytes outside it; the buffer carries 16 bytes of padding at
// both ends, so every slot read lies inside the allocation.
//
// The 256-entry table (2 KiB) sits in LDS and is read with ds_read_b64: entry q lies on banks 2q and 2q + 1 (mod 64),
// so q and q + 32 share a bank pair within a 32-lane group.  ONT qualities put almost all of a group's bytes within a
// 32-value window, see DESIGN.md §9a for the measured rate.
#include <hip/hip_runtime.h>

#include "umiclust_internal.h"

namespace uc {

namespace {

constexpr int kFqWaves = 4;  // records per block

__device__ __forceinline__ void fq_byte(uint32_t b, const unsigned long long* tab, unsigned long long& acc, uint32_t& lo,
                                        uint32_t& hi) {
  acc += tab[b];
  lo = min(lo, b);
  hi = max(hi, b);
}

__global__ __launch_bounds__(256) void k_fastq_ee(const uint8_t* __restrict__ qual, const int64_t* __restrict__ offs,
                                                  int64_t n, const unsigned long long* __restrict__ table,
                                                  long long* __restrict__ ee, uint8_t* __restrict__ qlo,
                                                  uint8_t* __restrict__ qhi) {
  __shared__ unsigned long long tab[256];
  tab[threadIdx.x] = table[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kFqWaves + (threadIdx.x >> 6);
  if (r >= n) return;
  const int64_t s = offs[r], e = offs[r + 1];
  unsigned long long acc = 0;
  uint32_t lo = 255, hi = 0;
  for (int64_t base = (s & ~(int64_t)15) + 16 * lane; base < e; base += 16 * 64) {
    const uint4 v = *reinterpret_cast<const uint4*>(qual + base);  // qual is 16-byte aligned
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    if (base >= s && base + 16 <= e) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        fq_byte(w[j] & 0xff, tab, acc, lo, hi);
        fq_byte((w[j] >> 8) & 0xff, tab, acc, lo, hi);
        fq_byte((w[j] >> 16) & 0xff, tab, acc, lo, hi);
        fq_byte(w[j] >> 24, tab, acc, lo, hi);
      }
    } else {  // the record's first or last slot: bytes outside [s, e) belong to its neighbours or the padding
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const int64_t at = base + j;
        if (at >= s && at < e) fq_byte((w[j >> 2] >> (8 * (j & 3))) & 0xff, tab, acc, lo, hi);
      }
    }
  }
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    acc += __shfl_xor(acc, m);
    lo = min(lo, (uint32_t)__shfl_xor((int)lo, m));
    hi = max(hi, (uint32_t)__shfl_xor((int)hi, m));
  }
  if (lane == 0) {
    ee[r] = (long long)acc;
    qlo[r] = (uint8_t)lo;
    qhi[r] = (uint8_t)hi;
  }
}

}  // namespace

hipError_t launch_fastq_ee(const uint8_t* qual, const int64_t* offs, int64_t n, const uint64_t* table, int64_t* ee,
                           uint8_t* qlo, uint8_t* qhi, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const int64_t blocks = (n + kFqWaves - 1) / kFqWaves;
  if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_fastq_ee, dim3((unsigned)blocks), dim3(256), 0, st, qual, offs, n,
                     reinterpret_cast<const unsigned long long*>(table), reinterpret_cast<long long*>(ee), qlo, qhi);
  return hipGetLastError();
}

}  // namespace uc
