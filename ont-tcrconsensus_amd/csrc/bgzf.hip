// bgzf.hip -- BGZF blocks inflated and deflated (the second half of this file) on the
// device.
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

#include "deflate.h"
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

// ---------------------------------------------------------------- deflate
// k_bgzf_deflate gives each block of at most 0xff00 input bytes to one wave, as the inflate kernel does, on
// dfl::run of deflate.h -- the code uc::deflate_block runs on the host -- with an Io that is the wave: a per-lane
// value is a register, another lane's value comes by v_readlane, the scan by __shfl_up, and the hash table, the
// histograms and the staging window are updated by LDS atomics (ds_max_u32 / ds_add_u32 / ds_or_b32 without return),
// whose results do not depend on the order of the lanes.  The grid is persistent: a workgroup takes blocks
// blockIdx.x, + gridDim.x, ... and owns one token store of 0xff00 words in global memory, so the token memory is
// bounded by the grid (kDeflateGrid x 255 KiB), not by the file.  The tokens a lane stores are read back by other lanes
// of the same wave after a barrier; the input is only read.  Integer byte-streaming work: no MFMA.
namespace {

struct DeflateWaveIo {
  template <class T>
  struct Lanes {
    T v;
    __device__ T& operator[](int) { return v; }
  };
  const uint8_t* src;  // the block's input bytes
  uint8_t* out;        // the block's output slot, 4-byte aligned: cap = n + 5 bytes of it may be written
  uint32_t cap;
  uint32_t* tok;  // this workgroup's token store
  uint32_t tok_cap;
  int ln;
  int err;  // a store that the bounds refused (never seen: the block's status, and the host redoes the block)

  template <class F>
  __device__ __forceinline__ void each(F f) { f(ln); }
  __device__ bool lead() const { return ln == 0; }
  __device__ void sync() { __syncthreads(); }
  __device__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
  __device__ uint32_t in(uint32_t p) const { return src[p]; }
  __device__ uint32_t in4(uint32_t p) const {
    uint32_t v;
    __builtin_memcpy(&v, src + p, 4);
    return v;
  }
  __device__ uint32_t read(Lanes<uint32_t>& x, uint32_t i) {
    return (uint32_t)__builtin_amdgcn_readlane((int)x.v, __builtin_amdgcn_readfirstlane((int)i));
  }
  __device__ Lanes<uint32_t> excl_scan(Lanes<uint32_t>& x, uint32_t& total) {
    uint32_t s = x.v;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t t = __shfl_up(s, d, 64);
      if (ln >= d) s += t;
    }
    total = (uint32_t)__builtin_amdgcn_readlane((int)s, 63);
    return {s - x.v};
  }
  __device__ void lds_max(uint32_t* w, uint32_t v) { atomicMax(w, v); }
  __device__ void lds_add(uint32_t* w, uint32_t v) { atomicAdd(w, v); }
  __device__ void lds_or(uint32_t* w, uint32_t v) { atomicOr(w, v); }
  __device__ void tok_put(uint32_t i, uint32_t v) {
    if (i < tok_cap) tok[i] = v;
    else err = 1;
  }
  __device__ uint32_t tok_get(uint32_t i) const { return tok[i]; }
  __device__ void store32(uint32_t w, uint32_t v) {
    if (4 * w + 4 <= cap) reinterpret_cast<uint32_t*>(out)[w] = v;
    else err = 1;
  }
  __device__ void store8(uint32_t k, uint8_t v) {
    if (k < cap) out[k] = v;
    else err = 1;
  }
};

}  // namespace

// Every byte written lies in slots[b * kDeflateSlot, + blk[b].n + 5) or in this workgroup's tok[blockIdx.x * 0xff00,
// + blk[b].n); every byte read in in[blk[b].in_off, + blk[b].n) or in what this wave wrote.  meta[4 b ..] = kind,
// payload bytes, status (0 = ok), flags; fsize[b] = the framed size (26 + payload bytes; 0 for a block with a status)
__global__ __launch_bounds__(64) void k_bgzf_deflate(const uint8_t* __restrict__ in,
                                                     const DeflateBlock* __restrict__ blk, int32_t n, uint8_t* slots,
                                                     uint32_t* tok, int32_t* __restrict__ meta,
                                                     int64_t* __restrict__ fsize) {
  __shared__ dfl::Work W;
  for (int32_t b = (int32_t)blockIdx.x; b < n; b += (int32_t)gridDim.x) {
    const DeflateBlock B = blk[b];
    const uint32_t len = B.n <= dfl::kMaxBlock ? B.n : 0u;  // (a longer block is refused below)
    DeflateWaveIo io;
    io.src = in + B.in_off;
    io.out = slots + (size_t)b * kDeflateSlot, io.cap = len + 5;
    io.tok = tok + (size_t)blockIdx.x * dfl::kMaxBlock, io.tok_cap = len;
    io.ln = (int)threadIdx.x, io.err = 0;
    const dfl::Result R = dfl::run(io, W, len);
    const bool bad = __ballot(io.err) != 0 || R.bytes > len + 5 || len != B.n;
    if (threadIdx.x == 0) {
      meta[4 * b] = (int32_t)R.kind, meta[4 * b + 1] = bad ? 0 : (int32_t)R.bytes;
      meta[4 * b + 2] = bad ? 1 : 0, meta[4 * b + 3] = (int32_t)R.flags;
      fsize[b] = bad ? 0 : 26 + (int64_t)R.bytes;
    }
    __syncthreads();
  }
}

// The framed file bytes of a batch: block b's 18-byte header (BC, BSIZE), its payload from its slot, CRC32 and ISIZE
// at out[foff[b], foff[b + 1]) -- nothing for a block with a status.  One workgroup per block; a thread assembles the
// 4 bytes of an aligned word of `out` and stores them as one word where the word lies wholly in the block's range,
// byte by byte at the two ends, which neighbouring blocks share.
__global__ __launch_bounds__(256) void k_bgzf_frame(const uint8_t* __restrict__ slots,
                                                    const DeflateBlock* __restrict__ blk,
                                                    const int32_t* __restrict__ meta, const int64_t* __restrict__ foff,
                                                    const uint32_t* __restrict__ crc, int32_t n, uint8_t* out) {
  const int32_t b = (int32_t)blockIdx.x;
  if (b >= n || meta[4 * b + 2]) return;
  const uint32_t bytes = (uint32_t)meta[4 * b + 1], total = bytes + 26, isize = blk[b].n, c = crc[b];
  const uint8_t* const src = slots + (size_t)b * kDeflateSlot;
  const int64_t lo = foff[b], hi = lo + total;
  auto byte_at = [&](uint32_t k) -> uint32_t {  // k < total
    constexpr uint8_t hdr[16] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0};
    if (k < 16) return hdr[k];
    if (k < 18) return ((total - 1) >> (8 * (k - 16))) & 0xffu;
    if (k < 18 + bytes) return src[k - 18];
    if (k < 22 + bytes) return (c >> (8 * (k - 18 - bytes))) & 0xffu;
    return (isize >> (8 * (k - 22 - bytes))) & 0xffu;
  };
  for (int64_t w = (lo & ~(int64_t)3) + 4 * (int64_t)threadIdx.x; w < hi; w += 4 * 256) {
    if (w >= lo && w + 4 <= hi) {
      const uint32_t k = (uint32_t)(w - lo);
      *reinterpret_cast<uint32_t*>(out + w) = byte_at(k) | byte_at(k + 1) << 8 | byte_at(k + 2) << 16 | byte_at(k + 3) << 24;
    } else {
      for (int x = 0; x < 4; x++)
        if (w + x >= lo && w + x < hi) out[w + x] = (uint8_t)byte_at((uint32_t)(w + x - lo));
    }
  }
}

hipError_t launch_bgzf_deflate(const uint8_t* in, const DeflateBlock* blk, int64_t n, uint8_t* slots, uint32_t* tok,
                               int32_t* meta, int64_t* fsize, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (n > INT32_MAX || ((uintptr_t)slots & 3) != 0) return hipErrorInvalidValue;
  const unsigned grid = (unsigned)(n < kDeflateGrid ? n : kDeflateGrid);
  hipLaunchKernelGGL(k_bgzf_deflate, dim3(grid), dim3(64), 0, st, in, blk, (int32_t)n, slots, tok, meta, fsize);
  return hipGetLastError();
}

hipError_t launch_bgzf_frame(const uint8_t* slots, const DeflateBlock* blk, const int32_t* meta, const int64_t* foff,
                             const uint32_t* crc, int64_t n, uint8_t* out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (n > INT32_MAX || ((uintptr_t)out & 3) != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_bgzf_frame, dim3((unsigned)n), dim3(256), 0, st, slots, blk, meta, foff, crc, (int32_t)n, out);
  return hipGetLastError();
}

}  // namespace uc
