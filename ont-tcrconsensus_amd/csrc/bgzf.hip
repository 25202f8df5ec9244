// bgzf.hip -- BGZF blocks inflated on the device.
//
// A BGZF file is a list of independent DEFLATE streams of at most 64 KiB each, far more of them than the device has
// wave slots; k_bgzf_inflate gives each to one wave (one wave per workgroup, so a barrier is the wave's own).  The
// decoder is inf::run of inflate.h -- the code uc::inflate_block runs on the host -- on an Io whose lanes work
// together: every decision (bit cursor, symbol, lengths, output cursor, status) is the same on all 64 lanes; the
// lanes split the filling of the lookup tables in LDS, each hold 4 bytes of a 256-byte window of the input in a
// register (the bit reader takes two of them by v_readlane), each hold one pending literal until 64 lie side by side
// or a copy needs them in memory, and copy stored blocks and LZ77 matches 64 bytes a step.
//
// A match reads bytes that other lanes of this wave stored earlier -- with distance < length, bytes of the same
// match -- from the output in global memory.  Every such store is separated from the read by a wavefront-scope
// fence.  The fence emits no instruction: it keeps the compiler from moving the load above the store, and the order
// on the hardware is that of the wave's own vector memory path -- a wave's global stores and loads are issued to the
// CU's write-through L1 in program order, so a load issued after a store of the same wave to the same bytes returns
// them.  No wait for the stores' completion stands between them (the code object's match loop is load, wait for the
// load, store, branch), and no other wave touches a block's output bytes.  Integer byte-streaming work: no MFMA.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "inflate.h"
#include "umiclust_internal.h"

namespace uc {

namespace {

struct WaveIo {
  const uint32_t* words;  // the compressed buffer, 4-byte aligned
  int64_t nwords;         // its size: no word at or past it is read
  uint64_t pos, end;      // bit cursor and the payload's end, as bit offsets into `words`
  uint8_t* out;           // the block's first output byte
  int ln;
  uint64_t chunk;      // the window: lane l holds word chunk + l in w
  uint32_t w;
  uint32_t pend_from;  // literals at [pend_from, cursor) wait in pb of lane (position & 63); all in one 64-byte group
  uint8_t pb;

  __device__ int lane() const { return ln; }
  __device__ int lanes() const { return 64; }
  __device__ void sync() { __syncthreads(); }
  // orders this wave's stores to `out` before its later loads from it, for the compiler; see the note at the top
  __device__ static void fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

  // the next 32 stream bits, the first one lowest; bits past the payload's end are other bytes of the buffer or
  // zero, and consume() refuses them
  __device__ uint32_t peek() {
    const uint64_t wi = pos >> 5;
    if (wi < chunk || wi + 1 >= chunk + 64) {
      chunk = wi;
      const int64_t x = (int64_t)wi + ln;
      w = x < nwords ? words[x] : 0u;
    }
    const int i = (int)(wi - chunk);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)w, i);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)w, i + 1);
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (pos & 31));
  }
  __device__ bool consume(uint32_t n) {
    if (pos + n > end) return false;
    pos += n;
    return true;
  }
  __device__ void align_byte() { pos = (pos + 7) & ~(uint64_t)7; }
  __device__ uint32_t bytes_left() const { return (uint32_t)((end - pos) >> 3); }

  // the pending literals below `upto` (the cursor) to memory: one store of up to 64 adjacent bytes
  __device__ void flush(uint32_t upto) {
    if (pend_from < upto) {
      const uint32_t p = (pend_from & ~63u) + (uint32_t)ln;
      if (p >= pend_from && p < upto) out[p] = pb;
    }
    pend_from = upto;
  }
  __device__ void literal(uint32_t o, uint8_t c) {
    if ((uint32_t)ln == (o & 63u)) pb = c;
    if ((o & 63u) == 63u) flush(o + 1);
  }
  // len <= bytes_left(): the source lies in the payload
  __device__ void stored(uint32_t o, uint32_t len) {
    flush(o);
    const uint8_t* src = (const uint8_t*)words + (pos >> 3);
    for (uint32_t k = (uint32_t)ln; k < len; k += 64) out[o + k] = src[k];
    pos += (uint64_t)len * 8;
    pend_from = o + len;
  }
  // dist <= o: the source lies in the block.  A step copies up to 64 bytes from bytes every earlier step (and every
  // earlier store of the wave) has put: a distance below 64 repeats its own period, so lane i reads byte i % dist of
  // the period that ends at the step's first byte.
  __device__ void match(uint32_t o, uint32_t len, uint32_t dist) {
    flush(o);
    for (uint32_t k = 0; k < len; k += 64) {
      fence();
      const uint32_t base = o + k, i = (uint32_t)ln;
      if (i < len - k) out[base + i] = out[base - dist + (dist >= 64 ? i : i % dist)];
    }
    pend_from = o + len;
  }
  __device__ void finish(uint32_t o) { flush(o); }
};

}  // namespace

// one wave per block with ISIZE > 0; every byte written lies in out[blk.out_off, + isize), every byte read in the
// nwords words of comp or in what this wave wrote
__global__ __launch_bounds__(64) void k_bgzf_inflate(const uint32_t* __restrict__ comp, int64_t nwords,
                                                     const BgzfBlock* __restrict__ blk, int32_t n, uint8_t* out,
                                                     int32_t* __restrict__ status) {
  __shared__ inf::Tables T;
  const int32_t b = (int32_t)blockIdx.x;
  if (b >= n) return;
  const BgzfBlock B = blk[b];
  WaveIo io;
  io.words = comp, io.nwords = nwords;
  io.pos = (uint64_t)B.in_off * 8, io.end = io.pos + (uint64_t)B.in_len * 8;
  io.out = out + B.out_off;
  io.ln = (int)threadIdx.x;
  io.chunk = ~(uint64_t)0, io.w = 0;
  io.pend_from = 0, io.pb = 0;
  const int32_t st = inf::run(io, T, B.isize);
  if (threadIdx.x == 0) status[b] = st;
}

hipError_t launch_bgzf_inflate(const uint8_t* comp, int64_t comp_bytes, const BgzfBlock* blk, int64_t n, uint8_t* out,
                               int32_t* status, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (n > INT32_MAX || ((uintptr_t)comp & 3) != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned)n), dim3(64), 0, st, (const uint32_t*)comp, comp_bytes / 4, blk,
                     (int32_t)n, out, status);
  return hipGetLastError();
}

}  // namespace uc
