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
//
// k_fastq_stats (row f5b) is the same walk over the qualities and, slot for slot, over the sequence bytes: besides
// ee_fx, qlo and qhi it counts what seqkit's `stat -a` table is made of.  It runs only when the tables are asked for.
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

// ---- k_fastq_stats (row f5b): k_fastq_ee's per-record outputs plus the five counts of seqkit's `stat -a` table ----
// The sequence bytes are classified by compares on the packed words, not by a table: a class table in LDS would add
// 16 byte-wide reads per lane and slot to the 16 ds_read_b64 of the error table (conflict-free for ACGT, but twice the
// LDS instructions); the compares touch no LDS at all, so the kernel's bank behaviour is k_fastq_ee's.

// 0x80 in every byte of x that is zero, 0 in the others (exact: no carry crosses a byte)
__device__ __forceinline__ uint32_t fq_zero_bytes(uint32_t x) {
  return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}
__device__ __forceinline__ uint32_t fq_eq_bytes(uint32_t w, uint32_t c) { return fq_zero_bytes(w ^ (c * 0x01010101u)); }

// counts of one sequence word's bytes under m (0x80 in each byte that belongs to the record)
__device__ __forceinline__ void fq_seq_word(uint32_t w, uint32_t m, uint32_t& gc, uint32_t& nn, uint32_t& gap) {
  const uint32_t f = w | 0x20202020u;  // 'G' and 'g' -> 'g', and no other byte
  gc += __popc((fq_eq_bytes(f, 'g') | fq_eq_bytes(f, 'c')) & m);
  nn += __popc(fq_eq_bytes(f, 'n') & m);
  gap += __popc((fq_eq_bytes(w, '-') | fq_eq_bytes(w, '.') | fq_eq_bytes(w, ' ')) & m);
}

__device__ __forceinline__ void fq_byte_stats(uint32_t b, const unsigned long long* tab, uint32_t t20, uint32_t t30,
                                              unsigned long long& acc, uint32_t& lo, uint32_t& hi, uint32_t& q20,
                                              uint32_t& q30) {
  fq_byte(b, tab, acc, lo, hi);
  q20 += b >= t20;
  q30 += b >= t30;
}

__global__ __launch_bounds__(256) void k_fastq_stats(const uint8_t* __restrict__ qual, const uint8_t* __restrict__ seq,
                                                     const int64_t* __restrict__ offs, int64_t n,
                                                     const unsigned long long* __restrict__ table, int ascii,
                                                     long long* __restrict__ ee, uint8_t* __restrict__ qlo,
                                                     uint8_t* __restrict__ qhi, uint32_t* __restrict__ counts) {
  __shared__ unsigned long long tab[256];
  tab[threadIdx.x] = table[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kFqWaves + (threadIdx.x >> 6);
  if (r >= n) return;
  const int64_t s = offs[r], e = offs[r + 1];
  const uint32_t t20 = (uint32_t)ascii + 20, t30 = (uint32_t)ascii + 30;  // b - ascii >= 20 as b >= ascii + 20
  unsigned long long acc = 0;
  uint32_t lo = 255, hi = 0, q20 = 0, q30 = 0, gc = 0, nn = 0, gap = 0;
  for (int64_t base = (s & ~(int64_t)15) + 16 * lane; base < e; base += 16 * 64) {
    const uint4 v = *reinterpret_cast<const uint4*>(qual + base);  // both buffers are 16-byte aligned
    const uint4 u = *reinterpret_cast<const uint4*>(seq + base);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    const uint32_t x[4] = {u.x, u.y, u.z, u.w};
    if (base >= s && base + 16 <= e) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        fq_byte_stats(w[j] & 0xff, tab, t20, t30, acc, lo, hi, q20, q30);
        fq_byte_stats((w[j] >> 8) & 0xff, tab, t20, t30, acc, lo, hi, q20, q30);
        fq_byte_stats((w[j] >> 16) & 0xff, tab, t20, t30, acc, lo, hi, q20, q30);
        fq_byte_stats(w[j] >> 24, tab, t20, t30, acc, lo, hi, q20, q30);
        fq_seq_word(x[j], 0x80808080u, gc, nn, gap);
      }
    } else {  // the record's first or last slot: bytes outside [s, e) belong to its neighbours or the padding
      uint32_t m[4] = {0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const int64_t at = base + j;
        if (at >= s && at < e) {
          fq_byte_stats((w[j >> 2] >> (8 * (j & 3))) & 0xff, tab, t20, t30, acc, lo, hi, q20, q30);
          m[j >> 2] |= 0x80u << (8 * (j & 3));
        }
      }
#pragma unroll
      for (int j = 0; j < 4; j++) fq_seq_word(x[j], m[j], gc, nn, gap);
    }
  }
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) {
    acc += __shfl_xor(acc, k);
    lo = min(lo, (uint32_t)__shfl_xor((int)lo, k));
    hi = max(hi, (uint32_t)__shfl_xor((int)hi, k));
    q20 += (uint32_t)__shfl_xor((int)q20, k);
    q30 += (uint32_t)__shfl_xor((int)q30, k);
    gc += (uint32_t)__shfl_xor((int)gc, k);
    nn += (uint32_t)__shfl_xor((int)nn, k);
    gap += (uint32_t)__shfl_xor((int)gap, k);
  }
  if (lane == 0) {
    ee[r] = (long long)acc;
    qlo[r] = (uint8_t)lo;
    qhi[r] = (uint8_t)hi;
    uint32_t* c = counts + 5 * r;  // record-major: n_q20, n_q30, n_gc, n_n, n_gap
    c[0] = q20;
    c[1] = q30;
    c[2] = gc;
    c[3] = nn;
    c[4] = gap;
  }
}

}  // namespace

hipError_t launch_fastq_stats(const uint8_t* qual, const uint8_t* seq, const int64_t* offs, int64_t n,
                              const uint64_t* table, int ascii, int64_t* ee, uint8_t* qlo, uint8_t* qhi,
                              uint32_t* counts, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const int64_t blocks = (n + kFqWaves - 1) / kFqWaves;
  if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_fastq_stats, dim3((unsigned)blocks), dim3(256), 0, st, qual, seq, offs, n,
                     reinterpret_cast<const unsigned long long*>(table), ascii, reinterpret_cast<long long*>(ee), qlo,
                     qhi, counts);
  return hipGetLastError();
}

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
