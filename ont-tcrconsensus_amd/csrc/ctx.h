// ctx.h -- the context core: what every entry point of the C ABI (include/umiclust.h) needs of a context, and the
// state of the drop-ins (dropin_*.cpp), which share nothing else with clustering.  cluster_ctx.h derives umiclust_ctx
// from uc::Ctx; the drop-ins see umiclust_ctx only as the ABI's incomplete type and reach this base through uc::core.
#pragma once
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <memory>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/umiclust.h"
#include "bam_host.h"
#include "host_io.h"
#include "tunables.h"
#include "umiclust_internal.h"

namespace uc {

inline double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// An owned array in device memory (DevBuf) or in pinned host memory (PinBuf), grown by ensure() and never shrunk.
// Kernels write pinned buffers directly (pinned host memory is device-accessible); the host reads them only after the
// writing kernel's completion event, and copies what it scans into pageable vectors first.
template <typename T, bool kPinned>
struct HipBuf {
  T* p = nullptr;
  size_t n = 0;
  HipBuf() = default;
  HipBuf(const HipBuf&) = delete;
  HipBuf& operator=(const HipBuf&) = delete;
  ~HipBuf() { release(); }
  void release() {
    if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    n = 0;
  }
  hipError_t ensure(size_t count) {
    if (count <= n && p) return hipSuccess;
    release();
    const size_t c = count ? count : 1;
    void** q = reinterpret_cast<void**>(&p);
    const hipError_t e = kPinned ? hipHostMalloc(q, c * sizeof(T), hipHostMallocDefault) : hipMalloc(q, c * sizeof(T));
    if (e == hipSuccess) n = c;
    return e;
  }
};
template <typename T>
using DevBuf = HipBuf<T, false>;
template <typename T>
using PinBuf = HipBuf<T, true>;
// c->hip(b.ensure(count), "alloc") for each buffer, in order
template <typename C, typename... B>
void alloc_each(C* c, size_t count, B&... b) {
  (c->hip(b.ensure(count), "alloc"), ...);
}

// An owned HIP event (Event) or stream (Stream): move-only, destroyed with its owner, read as the raw handle.
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
  Event& operator=(Event&& o) noexcept {
    std::swap(e, o.e);
    return *this;
  }
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
  operator hipEvent_t() const { return e; }
  // creates the event unless it exists
  hipError_t create(unsigned flags = hipEventDefault) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
  // the handle, created on first use (a failure is the context's)
  template <typename C>
  hipEvent_t get(C* c, unsigned flags = hipEventDefault) {
    c->hip(create(flags), "event");
    return e;
  }
};
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
  // (a replaced stream -- umiclust_set_priority -- leaves in `o` and is destroyed with it)
  Stream& operator=(Stream&& o) noexcept {
    std::swap(s, o.s);
    return *this;
  }
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
  operator hipStream_t() const { return s; }
  hipError_t create(unsigned flags) { return hipStreamCreateWithFlags(&s, flags); }
  hipError_t create(unsigned flags, int priority) { return hipStreamCreateWithPriority(&s, flags, priority); }
};

struct Fail {
  int code;
};

// UMI extraction (f1): gathered adapter windows, kept across calls
struct ExtractState {
  PinBuf<char> win;
  PinBuf<uint8_t> len;
  DevBuf<char> dwin;
  DevBuf<uint8_t> dlen;
  DevBuf<int32_t> dout;
  DevBuf<ExtractPatterns> dpat;
};

// quality filtering (f5): two pinned staging slots (one being gathered while the other is on the device), one set
// of device buffers, kept across calls.  seq / cnt and dseq / dcnt (the sequence bytes and the five counts per record
// of row f5b) are allocated by the first call that asks for the statistics tables.
struct FqState {
  struct Slot {
    PinBuf<uint8_t> q, lo, hi, seq;
    PinBuf<int64_t> offs, ee;
    PinBuf<uint32_t> cnt;
  } slot[2];
  DevBuf<uint8_t> dq, dlo, dhi, dseq;
  DevBuf<int64_t> doffs, dee;
  DevBuf<uint32_t> dcnt;
  DevBuf<uint64_t> dtab;
  Event ev[3];  // copy begin, kernel begin, kernel end
};

// The device writer of the BAM session.
constexpr size_t kDeflateIn = bam::kBgzfPayload;       // a block's input bytes at most
constexpr size_t kDeflateFramed = kDeflateIn + 5 + 26;  // its framed bytes at most: stored form, header and trailer
// The device buffers of one batch of at most `cap` blocks and the host copies of its tables.
struct DeflateDev {
  DevBuf<uint8_t> d_in, d_slots, d_out;
  DevBuf<uint32_t> d_tok, d_crc;
  DevBuf<DeflateBlock> d_blk;
  DevBuf<int32_t> d_meta;
  DevBuf<int64_t> d_fsize, d_foff;
  std::vector<DeflateBlock> blk;
  std::vector<int32_t> meta;  // per block: kind, payload bytes, status, flags
  std::vector<int64_t> foff;  // per block: its framed bytes' offset; foff[nb] = the batch's framed bytes
  Event e[4];
  void release() {
    d_in.release(), d_slots.release(), d_out.release(), d_tok.release(), d_crc.release(), d_blk.release();
    d_meta.release(), d_fsize.release(), d_foff.release();
  }
  // an allocation failure is returned, not thrown: the writer then takes the host path
  hipError_t ensure(size_t cap) {
    const size_t grid = std::min<size_t>(cap, (size_t)kDeflateGrid);
    hipError_t r = hipSuccess;
    auto on = [&](hipError_t x) { r = r == hipSuccess ? x : r; };
    on(d_in.ensure(cap * kDeflateIn + 8)), on(d_slots.ensure(cap * (size_t)kDeflateSlot)), on(d_out.ensure(cap * kDeflateFramed + 8));
    on(d_tok.ensure(grid * kDeflateIn)), on(d_crc.ensure(cap)), on(d_blk.ensure(cap)), on(d_meta.ensure(4 * cap));
    on(d_fsize.ensure(cap)), on(d_foff.ensure(cap + 1));
    for (Event& x : e) on(x.create());
    if (r != hipSuccess) (void)hipGetLastError();
    return r;
  }
};
// The writer's buffers, kept across calls: one batch on the device, two pinned staging slots (one being gathered
// while the other is on the device) and the pinned framed bytes of a batch.
struct BgzfWriteState {
  DeflateDev dev;
  struct Slot {
    PinBuf<uint8_t> in;
    PinBuf<uint32_t> crc;
  } slot[2];
  PinBuf<uint8_t> out;
  void release() {
    dev.release(), out.release();
    for (Slot& s : slot) s.in.release(), s.crc.release();
  }
};

// The inflated file on the host: a byte array that is not zero-filled when it is made, because the copy from the
// device writes every byte of it (zero-filling 540 MB on one thread cost more than inflating them)
struct RawBuf {
  std::unique_ptr<uint8_t[]> p;
  size_t n = 0;
  RawBuf() = default;
  RawBuf(RawBuf&& o) noexcept : p(std::move(o.p)), n(o.n) { o.n = 0; }  // a moved-from buffer is empty: size() == 0
  RawBuf& operator=(RawBuf&& o) noexcept {
    p = std::move(o.p);
    n = o.n;
    o.n = 0;
    return *this;
  }
  void alloc(size_t bytes) {
    p.reset(new uint8_t[bytes ? bytes : 1]);
    n = bytes;
  }
  uint8_t* data() { return p.get(); }
  const uint8_t* data() const { return p.get(); }
  size_t size() const { return n; }
  uint8_t operator[](size_t i) const { return p[i]; }
};

// BAM session (f6, umiclust_bam_open .. umiclust_bam_close): the inflated file, its header, the record offsets and
// the columns of the device scan.  The open inflates the file on the device and copies it back; what
// stays is host memory only: umiclust_bam_split and umiclust_bam_name_suffix (f4b / f6b)
// upload what their kernels read and free it on return
struct BamSession {
  bool open = false;
  RawBuf raw;
  bam::Header hdr;
  std::vector<int64_t> roff, reflen, cols, nm, cs_off, g_count, g_rep;
  std::vector<int32_t> ref, l_seq, cs_len, cs_group;
  std::vector<int8_t> cls;
  std::vector<uint8_t> nm_present;
  int64_t n_reruns = 0, first_bad = -1;
  int64_t inflate_info[3] = {0, 0, 0};  // BGZF blocks, blocks inflated on the device, compressed bytes uploaded
  double t_inflate = 0, t_h2d = 0, t_dev = 0;
  // the last umiclust_bam_write: blocks, blocks deflated on the device, of them stored / fixed /
  // dynamic, blocks redone on the host, batches, compressed bytes; seconds of upload, kernels, copy back (HIP events)
  // and of the host's gather + CRC32
  bool wrote = false;
  int64_t write_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double write_times[4] = {0, 0, 0, 0};
  // the compressed offset of every block that write framed, the EOF block's last: what
  // umiclust_bam_write_index reads the virtual offsets from
  std::vector<int64_t> write_coff;
  // a session opened from SAM text (umiclust_sam_open): lines, records, text bytes uploaded, aux f
  // values the host parsed; seconds of upload, lines + measure, sort, encode, copy back
  bool from_sam = false;
  int64_t sam_info[4] = {0, 0, 0, 0};
  double sam_times[5] = {0, 0, 0, 0, 0};
};

struct Ctx {
  int dev = 0;
  Stream st;
  Event ev0, ev1;
  std::string err;
  Tunables tun;  // the UMICLUST_* switches, as umiclust_create read them (tunables.h)
  umiclust_stats stats{};
  ExtractState ex;
  FqState fq;
  BamSession bs;
  BgzfWriteState bw;
  // the last index or flagstat call: kept records, runs, chunks after the finish, windows; seconds of
  // upload, kernels, copy back (HIP events) and of the host's finish
  struct IndexInfo {
    bool have = false;
    int64_t out[4] = {0, 0, 0, 0};
    double times[4] = {0, 0, 0, 0};
  } ix;
  // (the members go after the derived context's destructor, which selects the device)

  void fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    err = buf;
    throw Fail{code};
  }
  void hip(hipError_t e, const char* what) {
    if (e != hipSuccess) fail(UMICLUST_EDEVICE, "%s: %s", what, hipGetErrorString(e));
  }
  // a copy to or from the device queued on st; nothing for 0 bytes
  void h2d(void* dst, const void* src, size_t bytes) {
    if (bytes) hip(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st), "h2d");
  }
  void d2h(void* dst, const void* src, size_t bytes) {
    if (bytes) hip(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st), "d2h");
  }
};

// the core of a context (driver.cpp: the upcast); null for null
Ctx* core(umiclust_ctx* c);

// the match masks of the two UMI patterns (dropin_extract.cpp): 1..64 symbols each, the reference's IUPAC equalities
void build_patterns(Ctx* c, const char* fwd, const char* rev, ExtractPatterns& P);

// seconds between two recorded events that have completed
inline double elapsed_s(Ctx* c, hipEvent_t a, hipEvent_t b) {
  float ms = 0;
  c->hip(hipEventElapsedTime(&ms, a, b), "elapsed");
  return ms * 1e-3;
}

// A packed sequence set on the device: the bytes of records [0, n) into d_seq and their offsets, relative to offs[0],
// into d_off, both copies queued on st.  `rel` is what the offset copy reads: it must live until st has run it.
inline void upload_seqs(Ctx* c, const char* seqs, const int64_t* offs, int64_t n, DevBuf<char>& d_seq,
                        DevBuf<int64_t>& d_off, std::vector<int64_t>& rel, hipStream_t st) {
  const int64_t bytes = n > 0 ? offs[n] - offs[0] : 0;
  rel.resize((size_t)n + 1);
  for (int64_t i = 0; i <= n; i++) rel[i] = n > 0 ? offs[i] - offs[0] : 0;
  c->hip(d_seq.ensure((size_t)bytes + 1), "alloc");
  c->hip(d_off.ensure((size_t)n + 1), "alloc");
  if (bytes > 0) c->hip(hipMemcpyAsync(d_seq.p, seqs + offs[0], (size_t)bytes, hipMemcpyHostToDevice, st), "h2d");
  c->hip(hipMemcpyAsync(d_off.p, rel.data(), rel.size() * 8, hipMemcpyHostToDevice, st), "h2d");
}

// the records of one packed set appended to `all`, their end offsets to `off` (which starts as {0})
inline void append_set(const char* s, const int64_t* o, int64_t n, std::vector<char>& all, std::vector<int64_t>& off) {
  for (int64_t i = 0; i < n; i++) {
    all.insert(all.end(), s + o[i], s + o[i + 1]);
    off.push_back((int64_t)all.size());
  }
}

// Region overlap (f3, dropin_overlap.cpp): n sequences of nreg regions on the device and the buffers of the accepted
// hash-table pass.  overlap_table checks the arguments (UMICLUST_EINVAL: null arguments, region boundaries that do not
// span [0, n] or decrease), sizes the table (m = mask + 1 = the smallest power of two >= max(1024, 2 n)), uploads, and
// runs launch_overlap_table under one seed after another until no two different sequences share a hash.  hash_bits
// < 64 keeps that many low bits of the first pass's hashes (umiclust_overlap_probe; UMICLUST_OVERLAP_TEST_COLLIDE
// keeps 8); `passes` and `seed` tell how many passes ran and which seed was accepted.
struct OvRun {
  DevBuf<char> d_seq;
  DevBuf<int64_t> d_off, d_rs, d_slot;
  DevBuf<uint64_t> d_hash;
  DevBuf<int32_t> d_reg;
  DevBuf<unsigned long long> d_keys, d_rep;
  DevBuf<uint32_t> d_cnt, d_start, d_cursor, d_bsum, d_members, d_coll, d_big, d_nbig;
  OvBuffers B{};
  uint64_t mask = 0, seed = 0;
  int passes = 0;
};
void overlap_table(Ctx* c, OvRun& R, const char* seqs, const int64_t* offs, int64_t n, const int64_t* rstart,
                   int32_t nreg, bool csr, int hash_bits = 64);

}  // namespace uc

// Body of an entry point: selects the device; what the body throws becomes the ABI's error code and last-error text.
#define UC_GUARD(c, ...)                                \
  do {                                                  \
    if (!(c)) return UMICLUST_EINVAL;                   \
    try {                                               \
      (void)hipSetDevice((c)->dev);                     \
      __VA_ARGS__                                       \
    } catch (const uc::Fail& f__) {                     \
      return f__.code;                                  \
    } catch (const uc::io::IoError& e__) {              \
      (c)->err = e__.msg;                               \
      return e__.code;                                  \
    } catch (const std::bad_alloc&) {                   \
      (c)->err = "host allocation failed";              \
      return UMICLUST_ENOMEM;                           \
    } catch (...) {                                     \
      (c)->err = "unexpected exception";                \
      return UMICLUST_EDEVICE;                          \
    }                                                   \
  } while (0)
