// dropin_bam.cpp -- the two BAM readers: region binning (§8f f4, regionsplit.hip) and the BAM session with its scan,
// cs group-by and writer (§8f f6, DESIGN.md §9b, bamscan.hip), and on the session the round-2 region split and the
// name suffix (§8f f4b / f6b, DESIGN.md §9c, bamsplit.hip), and on both readers the region split fused with the UMI
// extraction (§8f f4+f1, DESIGN.md §9d, bamextract.hip).  Both readers inflate the file on the device (DESIGN.md §9e,
// bgzf.hip on inflate.h), which umiclust_bgzf_inflate runs alone.  Their HIP-free halves are in bam_host.h.  The
// session also opens from SAM text, parsed, encoded and coordinate-sorted on the device (samsort.hip on
// sam_text.h), and the round-1 split then runs on it (umiclust_bam_region_split[_extract]).  The session's writer
// deflates its blocks on the device (bgzf.hip on deflate.h), which umiclust_bgzf_deflate runs alone.
#include <errno.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "ctx.h"
#include "deflate.h"
#include "inflate.h"
#include "sam_text.h"

using namespace uc;
using namespace uc::io;

namespace {
int32_t rd_i32(const uint8_t* p) { int32_t v; memcpy(&v, p, 4); return v; }
// the query name of record r: at most l_read_name bytes and never past the record, up to its NUL
std::string_view record_name(const RawBuf& raw, const std::vector<int64_t>& roff, int64_t r) {
  const uint8_t* f = raw.data() + roff[r] + 4;
  const size_t lrn = std::min<size_t>(f[8], (size_t)bam::rd_block(raw.data() + roff[r]) - 32);
  return {(const char*)f + 32, lrn ? strnlen((const char*)f + 32, lrn) : 0};
}
BamSession* bam_session(Ctx* c) {
  if (!c->bs.open) c->fail(UMICLUST_ESTATE, "no BAM session is open (umiclust_bam_open)");
  return &c->bs;
}
// ---- BGZF blocks inflated on the device (bgzf.hip)
// The block table of a BGZF byte string: the blocks with ISIZE > 0 (the others are not launched), their index among
// all blocks, and the inflated size.
struct BgzfPlan {
  std::vector<BgzfBlock> blk;
  std::vector<int64_t> file_idx;
  int64_t n_blocks = 0, total = 0;
};
bool bgzf_plan(const uint8_t* d, size_t N, BgzfPlan& P) {
  std::vector<size_t> boff, bsz;
  std::vector<uint32_t> isz;
  if (!io::bgzf_blocks(d, N, boff, bsz, isz)) return false;
  P.n_blocks = (int64_t)boff.size();
  for (size_t b = 0; b < boff.size(); b++) {
    const size_t xlen = (size_t)d[boff[b] + 10] | ((size_t)d[boff[b] + 11] << 8);
    if (isz[b]) {
      P.blk.push_back({(int64_t)(boff[b] + 12 + xlen), P.total, (uint32_t)(bsz[b] - 12 - xlen - 8), isz[b]});
      P.file_idx.push_back((int64_t)b);
    }
    P.total += isz[b];
  }
  return true;
}
// d[0 .. N) uploaded (with 8 zero bytes of padding, rounded up to whole words), P's blocks inflated into d_raw
// (P.total + 1 bytes, as the scan kernels want it), their statuses into `status`, and the inflated bytes copied to
// host_dst(), which is called once the upload and the kernel are queued, so what it does (allocating, touching the
// pages) runs beside them.  Returns after the stream has drained.  times (may be null): upload, kernel, download in
// seconds by HIP events.
template <typename HostDst>
void bgzf_inflate_device(Ctx* c, const uint8_t* d, size_t N, const BgzfPlan& P, DevBuf<uint8_t>& d_raw,
                         std::vector<int32_t>& status, HostDst host_dst, double* times) {
  const size_t nb = P.blk.size(), padded = (N + 8 + 3) & ~(size_t)3;
  DevBuf<uint8_t> d_comp;
  DevBuf<BgzfBlock> d_blk;
  DevBuf<int32_t> d_st;
  Event e[4];
  c->hip(d_comp.ensure(padded), "alloc");
  c->hip(d_raw.ensure((size_t)P.total + 1), "alloc");
  alloc_each(c, nb + 1, d_blk, d_st);
  status.assign(nb, 0);
  c->hip(hipEventRecord(e[0].get(c), c->st), "event");
  const size_t tail = std::min<size_t>(padded, 12);  // covers the padding whatever N % 4 is
  c->hip(hipMemsetAsync(d_comp.p + (padded - tail), 0, tail, c->st), "memset");
  if (N) c->hip(hipMemcpyAsync(d_comp.p, d, N, hipMemcpyHostToDevice, c->st), "h2d");
  if (nb) c->hip(hipMemcpyAsync(d_blk.p, P.blk.data(), nb * sizeof(BgzfBlock), hipMemcpyHostToDevice, c->st), "h2d");
  c->hip(hipEventRecord(e[1].get(c), c->st), "event");
  c->hip(launch_bgzf_inflate(d_comp.p, (int64_t)padded, d_blk.p, (int64_t)nb, d_raw.p, d_st.p, c->st), "bgzf inflate");
  c->hip(hipEventRecord(e[2].get(c), c->st), "event");
  if (nb) c->hip(hipMemcpyAsync(status.data(), d_st.p, nb * 4, hipMemcpyDeviceToHost, c->st), "d2h");
  uint8_t* const host_out = host_dst();
  if (host_out && P.total)
    c->hip(hipMemcpyAsync(host_out, d_raw.p, (size_t)P.total, hipMemcpyDeviceToHost, c->st), "d2h");
  c->hip(hipEventRecord(e[3].get(c), c->st), "event");
  c->hip(hipStreamSynchronize(c->st), "sync");
  if (times)
    for (int x = 0; x < 3; x++) times[x] = elapsed_s(c, e[x], e[x + 1]);
}

// ---- BGZF blocks deflated on the device (bgzf.hip on deflate.h)
constexpr size_t kBlk = kDeflateIn, kFramedMax = kDeflateFramed;
// nb blocks -- in[0 .. in_bytes), cut every 0xff00 bytes -- uploaded with their CRC32s, deflated, framed and copied
// back to out (nb * kFramedMax bytes at most): the bytes a file takes as they are.  D.meta and D.foff say what each
// block became; a block with a status has no bytes in out.  Returns the framed bytes; times (may be null): upload,
// kernels, copy back in seconds by HIP events, added to what is there.
size_t deflate_batch(Ctx* c, DeflateDev& D, const uint8_t* in, size_t in_bytes, size_t nb, const uint32_t* crc,
                     uint8_t* out, double* times) {
  D.blk.resize(nb), D.meta.assign(4 * nb, 0), D.foff.assign(nb + 1, 0);
  for (size_t b = 0; b < nb; b++) D.blk[b] = {(int64_t)(b * kBlk), (uint32_t)std::min(kBlk, in_bytes - b * kBlk), 0};
  c->hip(hipEventRecord(D.e[0], c->st), "event");
  c->hip(hipMemcpyAsync(D.d_in.p, in, in_bytes, hipMemcpyHostToDevice, c->st), "h2d");
  c->hip(hipMemcpyAsync(D.d_blk.p, D.blk.data(), nb * sizeof(DeflateBlock), hipMemcpyHostToDevice, c->st), "h2d");
  c->hip(hipMemcpyAsync(D.d_crc.p, crc, nb * 4, hipMemcpyHostToDevice, c->st), "h2d");
  c->hip(hipEventRecord(D.e[1], c->st), "event");
  c->hip(launch_bgzf_deflate(D.d_in.p, D.d_blk.p, (int64_t)nb, D.d_slots.p, D.d_tok.p, D.d_meta.p, D.d_fsize.p, c->st),
         "bgzf deflate");
  c->hip(launch_scan_i64(D.d_fsize.p, D.d_foff.p, (int64_t)nb, 0, D.d_foff.p + nb, c->st), "scan");
  c->hip(launch_bgzf_frame(D.d_slots.p, D.d_blk.p, D.d_meta.p, D.d_foff.p, D.d_crc.p, (int64_t)nb, D.d_out.p, c->st),
         "bgzf frame");
  c->hip(hipEventRecord(D.e[2], c->st), "event");
  c->hip(hipMemcpyAsync(D.meta.data(), D.d_meta.p, 4 * nb * 4, hipMemcpyDeviceToHost, c->st), "d2h");
  c->hip(hipMemcpyAsync(D.foff.data(), D.d_foff.p, (nb + 1) * 8, hipMemcpyDeviceToHost, c->st), "d2h");
  c->hip(hipStreamSynchronize(c->st), "sync");
  const size_t total = (size_t)D.foff[nb];
  if (total > nb * kFramedMax) c->fail(UMICLUST_EDEVICE, "bgzf deflate: %zu framed bytes from %zu blocks", total, nb);
  if (total) c->hip(hipMemcpyAsync(out, D.d_out.p, total, hipMemcpyDeviceToHost, c->st), "d2h");
  c->hip(hipEventRecord(D.e[3], c->st), "event");
  c->hip(hipStreamSynchronize(c->st), "sync");
  if (times)
    for (int x = 0; x < 3; x++) times[x] += elapsed_s(c, D.e[x], D.e[x + 1]);
  return total;
}

// umiclust_bam_write on the device: the stream cut into batches of c->tun.bgzf_batch blocks; while the device deflates
// batch k and its bytes are written, the I/O threads gather batch k + 1 into the other staging slot and compute its
// CRC32s.  A block with a status is redone by zlib in place.  Returns the records written, -1 + err on an I/O
// failure, -2 where device or pinned memory could not be had (nothing has been written: the caller takes the host
// writer).
int64_t write_bgzf_device(Ctx* c, BamSession& S, const uint8_t* keep, const char* path, std::string& err) {
  const bam::BgzfStream Z = bam::bgzf_stream(S.raw.data(), S.hdr.end, S.roff, keep);
  const size_t nb = Z.blocks(), batch = std::max<size_t>(1, std::min<size_t>((size_t)c->tun.bgzf_batch, std::max<size_t>(nb, 1)));
  // the context's buffers, kept across calls as the fastq_filter drop-in keeps its own: allocating the pinned ones
  // anew cost each write more than its kernels
  typedef BgzfWriteState::Slot Slot;
  DeflateDev& D = c->bw.dev;
  Slot* const slot = c->bw.slot;
  PinBuf<uint8_t>& out = c->bw.out;
  bool have = D.ensure(batch) == hipSuccess && out.ensure(batch * kFramedMax) == hipSuccess;
  for (int k = 0; k < 2; k++) have = have && slot[k].in.ensure(batch * kBlk) == hipSuccess && slot[k].crc.ensure(batch) == hipSuccess;
  if (!have) {
    (void)hipGetLastError();
    c->bw.release();
    return -2;
  }
  const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0666);
  if (fd < 0) {
    err = std::string("cannot create ") + path;
    return -1;
  }
  struct Fd {
    int fd;
    ~Fd() {
      if (fd >= 0) close(fd);
    }
  } guard{fd};
  // the gather of one batch on a thread of its own (which spreads it over the I/O threads); joined before the batch is
  // used and before this function is left, however it is left
  struct Gather {
    std::thread th;
    double seconds = 0;
    void join() {
      if (th.joinable()) th.join();
    }
    ~Gather() { join(); }
  } g;
  const int threads = io_threads();
  auto start_gather = [&](size_t b0) {
    Slot& s = slot[(b0 / batch) & 1];
    const size_t b1 = std::min(nb, b0 + batch);
    g.th = std::thread([&Z, &s, &g, b0, b1, threads]() {
      const double t0 = now_s();
      bam::bgzf_gather_crc(Z, b0, b1, s.in.p, s.crc.p, threads);
      g.seconds += now_s() - t0;
    });
  };
  int64_t* const I = S.write_info;
  std::fill(I, I + 8, 0);
  std::fill(S.write_times, S.write_times + 4, 0.0);
  I[0] = (int64_t)nb;
  size_t bytes = 0;
  bool ok = true;
  std::vector<uint8_t> redo;
  if (nb) start_gather(0);
  for (size_t b0 = 0; b0 < nb && ok; b0 += batch) {
    const size_t b1 = std::min(nb, b0 + batch), n = b1 - b0;
    Slot& s = slot[(b0 / batch) & 1];
    g.join();
    if (b1 < nb) start_gather(b1);
    const size_t in_bytes = std::min(Z.total, b1 * kBlk) - b0 * kBlk;
    const size_t total = deflate_batch(c, D, s.in.p, in_bytes, n, s.crc.p, out.p, S.write_times);
    I[6]++;
    int64_t bad = 0;
    for (size_t b = 0; b < n; b++) {
      if (D.meta[4 * b + 2]) bad++;
      else I[2 + std::min(2, std::max(0, D.meta[4 * b]))]++;
    }
    I[1] += (int64_t)n - bad, I[5] += bad;
    if (!bad) {
      ok = bam::write_fd(fd, out.p, total);
      bytes += total;
      continue;
    }
    for (size_t b = 0; b < n && ok; b++) {  // block by block: a refused block by zlib, in its place
      if (!D.meta[4 * b + 2]) {
        const size_t len = (size_t)(D.foff[b + 1] - D.foff[b]);
        ok = bam::write_fd(fd, out.p + D.foff[b], len);
        bytes += len;
      } else {
        ok = bam::bgzf_block(s.in.p + b * kBlk, D.blk[b].n, redo) && bam::write_fd(fd, redo.data(), redo.size());
        bytes += redo.size();
      }
    }
  }
  g.join();
  S.write_times[3] = g.seconds;
  ok = ok && bam::write_fd(fd, bam::kBgzfEof, sizeof bam::kBgzfEof);
  guard.fd = -1;
  ok = (close(fd) == 0) && ok;
  if (!ok) {
    err = std::string("cannot write ") + path;
    return -1;
  }
  I[7] = (int64_t)(bytes + sizeof bam::kBgzfEof);
  return Z.nkept;
}

// raw sized to `bytes` with its pages touched by the I/O threads (first touch is the cost of a fresh array this size,
// and one thread takes several times the inflate kernel's time over it)
uint8_t* alloc_touched(RawBuf& raw, size_t bytes) {
  raw.alloc(bytes);
  uint8_t* const p = raw.data();
  const size_t n = raw.size(), page = 4096;
  const int T = std::max(1, std::min<int>(io_threads(), (int)(n >> 22)));
  parallel_for(T, [&](int th) {
    const size_t lo = n / (size_t)T * (size_t)th, hi = th + 1 == T ? n : n / (size_t)T * (size_t)(th + 1);
    for (size_t o = lo; o < hi; o += page) p[o] = 0;
  });
  return p;
}

// What both BAM readers start with: the file mapped and its block table built, the compressed bytes uploaded, the
// blocks inflated into d_raw, and `raw` copied back to the host, where the header parser, record_offsets, the session
// and the writer read it.  info: BGZF blocks, blocks inflated on the device, compressed bytes uploaded; *t_upload:
// seconds of the compressed upload (HIP events).  False for a file that cannot be read, is not BGZF, or has a block
// the decoder refuses -- what io::inflate_bgzf returned false for.
bool read_bam_on_device(Ctx* c, const char* path, RawBuf& raw, DevBuf<uint8_t>& d_raw, int64_t info[3],
                        double* t_upload) {
  struct Map {
    void* p = nullptr;
    size_t n = 0;
    ~Map() {
      if (p) munmap(p, n);
    }
  } map;
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return false;
  struct stat sb;
  if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) {
    close(fd);
    return false;
  }
  map.n = (size_t)sb.st_size;
  if (map.n) map.p = mmap(nullptr, map.n, PROT_READ, MAP_PRIVATE | MAP_POPULATE, fd, 0);
  close(fd);
  if (map.p == MAP_FAILED) {
    map.p = nullptr;
    return false;
  }
  BgzfPlan P;
  if (!bgzf_plan((const uint8_t*)map.p, map.n, P)) return false;
  std::vector<int32_t> status;
  double t[3] = {0, 0, 0};
  // while the device inflates: the host's array, its pages touched by the I/O threads
  const auto host_dst = [&]() { return alloc_touched(raw, (size_t)P.total); };
  bgzf_inflate_device(c, (const uint8_t*)map.p, map.n, P, d_raw, status, host_dst, t);
  info[0] = P.n_blocks, info[1] = (int64_t)P.blk.size(), info[2] = (int64_t)map.n;
  if (t_upload) *t_upload = t[0];
  for (int32_t s : status)
    if (s) return false;
  return true;
}

// ---- SAM text to raw on the device (samsort.hip on sam_text.h)
// The bytes of `path`: a regular file is mapped, any other readable path (a FIFO, /dev/fd/N) is read to its end.
struct TextInput {
  void* map = nullptr;
  size_t map_n = 0;
  std::vector<uint8_t> buf;
  const uint8_t* p = nullptr;
  size_t n = 0;
  ~TextInput() {
    if (map) munmap(map, map_n);
  }
  bool read(const char* path) {
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return false;
    struct stat sb;
    if (fstat(fd, &sb) != 0) return close(fd), false;
    if (S_ISREG(sb.st_mode)) {
      map_n = (size_t)sb.st_size;
      if (map_n) map = mmap(nullptr, map_n, PROT_READ, MAP_PRIVATE | MAP_POPULATE, fd, 0);
      close(fd);
      if (map == MAP_FAILED) return map = nullptr, false;
      p = (const uint8_t*)map, n = map_n;
      return true;
    }
    for (size_t have = 0;;) {
      if (buf.size() - have < (1u << 20)) buf.resize(std::max<size_t>(buf.size() * 2, 1u << 22));
      const ssize_t k = ::read(fd, buf.data() + have, buf.size() - have);
      if (k < 0 && errno == EINTR) continue;
      if (k < 0) return close(fd), false;
      if (k == 0) {
        n = have;
        break;
      }
      have += (size_t)k;
    }
    close(fd);
    p = buf.data();
    return true;
  }
};

// The sibling of read_bam_on_device for SAM text: the text uploaded, its lines split, measured, sorted and encoded on
// the device into d_raw -- the BAM header the host built, then the records in coordinate order -- and `raw` copied back
// to the host.  Text and raw are both on the device until this returns.  info: lines (header included), records, text
// bytes uploaded, aux f values the host parsed; times: upload, lines + measure, sort, encode, copy back in seconds by
// HIP events.  Fails the context: UMICLUST_EIO for a path that cannot be read, UMICLUST_EFORMAT / UMICLUST_ERANGE for
// a refused header or line (named), UMICLUST_ENOMEM for a device allocation that fails.
void read_sam_on_device(Ctx* c, const char* path, RawBuf& raw, DevBuf<uint8_t>& d_raw, int64_t info[4],
                        double times[5]) {
  TextInput in;
  if (!in.read(path)) c->fail(UMICLUST_EIO, "cannot read SAM %s", path);
  sam::Header H;
  std::string herr;
  if (!sam::build_header(in.p, in.n, H, herr)) c->fail(UMICLUST_EFORMAT, "%s: %s", path, herr.c_str());
  sam::NameTable T;
  T.build(H.ref_name);
  const uint8_t* const body = in.p + H.body;
  const int64_t N = (int64_t)(in.n - H.body), hdr_len = (int64_t)H.bam.size();
  const auto dev = [&](hipError_t e) {
    if (e == hipErrorOutOfMemory) {
      (void)hipGetLastError();
      c->fail(UMICLUST_ENOMEM, "device allocation failed");
    }
    c->hip(e, "alloc");
  };
  const auto h2d = [&](void* dst, const void* src, size_t bytes) {
    if (bytes) c->hip(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->st), "h2d");
  };
  const auto d2h = [&](void* dst, const void* src, size_t bytes) {
    if (bytes) c->hip(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->st), "d2h");
  };
  Event e[6];
  const auto mark = [&](int k) { c->hip(hipEventRecord(e[k].get(c), c->st), "event"); };
  // upload: the text after the header and the name table
  DevBuf<uint8_t> d_text, d_nbytes;
  DevBuf<int32_t> d_noff, d_nslot;
  dev(d_text.ensure((size_t)N + 1)), dev(d_nbytes.ensure(T.bytes.size())), dev(d_noff.ensure(T.off.size()));
  dev(d_nslot.ensure(T.slot.size()));
  mark(0);
  h2d(d_text.p, body, (size_t)N), h2d(d_nbytes.p, T.bytes.data(), T.bytes.size());
  h2d(d_noff.p, T.off.data(), T.off.size() * 4), h2d(d_nslot.p, T.slot.data(), T.slot.size() * 4);
  const sam::Names names{d_nbytes.p, d_noff.p, d_nslot.p, T.mask, (int32_t)H.ref_name.size()};
  mark(1);
  // lines
  int64_t n = 0;
  DevBuf<int64_t> d_cnt, d_first, d_start, d_one;
  dev(d_one.ensure(1));
  if (N > 0) {
    const size_t nc = (size_t)sam_line_chunks(N);
    dev(d_cnt.ensure(nc)), dev(d_first.ensure(nc));
    c->hip(launch_sam_count_lines(d_text.p, N, d_cnt.p, d_first.p, d_one.p, c->st), "sam lines");
    d2h(&n, d_one.p, 8);
    c->hip(hipStreamSynchronize(c->st), "sync");
    n += 1;
    if (n > INT32_MAX) c->fail(UMICLUST_ERANGE, "%s: more than 2^31 - 1 lines", path);
    dev(d_start.ensure((size_t)n + 1));
    c->hip(launch_sam_scatter_lines(d_text.p, N, d_first.p, n, d_start.p, c->st), "sam lines");
  }
  // measure: per line the field table, size, key and status
  const int64_t nb = (n + 255) / 256;
  DevBuf<sam::Fields> d_fields;
  DevBuf<int64_t> d_size, d_roff, d_hist;
  DevBuf<uint64_t> d_key, d_key2, d_acc;
  DevBuf<uint32_t> d_idx, d_idx2;
  DevBuf<int32_t> d_status;
  dev(d_fields.ensure((size_t)n)), dev(d_size.ensure((size_t)n)), dev(d_roff.ensure((size_t)n));
  dev(d_hist.ensure((size_t)nb * 256)), dev(d_key.ensure((size_t)n)), dev(d_key2.ensure((size_t)n));
  dev(d_acc.ensure(4)), dev(d_idx.ensure((size_t)n)), dev(d_idx2.ensure((size_t)n)), dev(d_status.ensure((size_t)n));
  uint64_t acc[4] = {~0ull, 0, 0, 0};  // first refused line, OR of the keys, aux f values, slots appended by encode
  h2d(d_acc.p, acc, sizeof(acc));
  c->hip(launch_sam_measure(d_text.p, d_start.p, n, names, d_fields.p, d_size.p, d_key.p, d_status.p, d_acc.p, c->st),
         "sam measure");
  d2h(acc, d_acc.p, sizeof(acc));
  mark(2);
  c->hip(hipStreamSynchronize(c->st), "sync");
  if (acc[0] != ~0ull) {
    // the refusal's text comes from the host restatement of the same rules, on that line alone
    int64_t be[2] = {0, 0};
    d2h(be, d_start.p + acc[0], 16);
    c->hip(hipStreamSynchronize(c->st), "sync");
    int32_t status = 0;
    const std::string what = sam::describe(body, be[0], be[1] - 1, T.view(), H.lines + (int64_t)acc[0] + 1, &status);
    c->fail((status & 0xff) == sam::kERange ? UMICLUST_ERANGE : UMICLUST_EFORMAT, "%s: %s", path, what.c_str());
  }
  // sort: stable by key
  const uint32_t* d_order = d_idx.p;
  c->hip(launch_sam_sort(d_key.p, d_idx.p, d_key2.p, d_idx2.p, n, acc[1], d_hist.p, &d_order, c->st), "sam sort");
  mark(3);
  // encode: roff, the header bytes, the records, the f values
  int64_t total = hdr_len;
  c->hip(launch_sam_roff(d_size.p, d_order, n, hdr_len, d_roff.p, d_one.p, c->st), "sam roff");
  d2h(&total, d_one.p, 8);
  c->hip(hipStreamSynchronize(c->st), "sync");
  const int64_t nf = (int64_t)acc[2];
  DevBuf<sam::FSlot> d_slots;
  dev(d_raw.ensure((size_t)total + 1)), dev(d_slots.ensure((size_t)nf));
  h2d(d_raw.p, H.bam.data(), H.bam.size());
  c->hip(launch_sam_encode(d_text.p, d_start.p, d_order, d_roff.p, n, names, d_fields.p, d_size.p, d_raw.p, d_slots.p,
                           d_acc.p + 3, nf, c->st),
         "sam encode");
  DevBuf<int64_t> d_at;
  DevBuf<uint32_t> d_bits;
  std::vector<int64_t> at((size_t)nf);
  std::vector<uint32_t> bits((size_t)nf);
  if (nf) {
    std::vector<sam::FSlot> slots((size_t)nf);
    d2h(slots.data(), d_slots.p, (size_t)nf * sizeof(sam::FSlot)), d2h(acc, d_acc.p, sizeof(acc));
    c->hip(hipStreamSynchronize(c->st), "sync");
    if ((int64_t)acc[3] != nf) c->fail(UMICLUST_EDEVICE, "%s: the encode pass listed %lld f values, the measure pass %lld",
                                       path, (long long)acc[3], (long long)nf);
    for (int64_t k = 0; k < nf; k++) {
      uint8_t b[4];
      if (!sam::float_bytes(body, (size_t)N, slots[k].text, b))
        c->fail(UMICLUST_EFORMAT, "%s: line %lld: aux: an f value is no number", path,
                (long long)(H.lines + slots[k].line + 1));
      at[k] = slots[k].at;
      memcpy(&bits[k], b, 4);
    }
    dev(d_at.ensure((size_t)nf)), dev(d_bits.ensure((size_t)nf));
    h2d(d_at.p, at.data(), (size_t)nf * 8), h2d(d_bits.p, bits.data(), (size_t)nf * 4);
    c->hip(launch_sam_put_f(d_raw.p, d_at.p, d_bits.p, nf, c->st), "sam put f");
  }
  mark(4);
  d2h(alloc_touched(raw, (size_t)total), d_raw.p, (size_t)total);
  mark(5);
  c->hip(hipStreamSynchronize(c->st), "sync");
  info[0] = H.lines + n, info[1] = n, info[2] = N, info[3] = nf;
  for (int x = 0; x < 5; x++) times[x] = elapsed_s(c, e[x], e[x + 1]);
}

// The text of the kept records among [0, stop), grouped by bucket and in BAM order within a bucket: the slots are laid
// out here from olen (a kept record may have none), the bytes written by `launch(d_pos, d_out)` (k_bam_emit or
// k_bam_emit_umi) and then by `patch(pos, out)` on the host, and every bucket's text goes to path_of(bucket), opened
// with O_WRONLY | O_CREAT | mode: O_APPEND for the region FASTA (the reference opens it with "a" for every record),
// O_TRUNC for the detected-UMI FASTA (opened with "w").  d_pos: room for a slot per record.  Returns the buckets that
// hold a kept record, each of which got its file; a file that cannot be written is UMICLUST_EIO.
template <typename PathOf, typename Launch, typename Patch>
std::vector<int32_t> emit_buckets(Ctx* c, DevBuf<int64_t>& d_pos, const std::vector<int8_t>& cls,
                                  const std::vector<int32_t>& bkt, const std::vector<int64_t>& olen, int64_t stop,
                                  PathOf path_of, int mode, Launch launch, Patch patch) {
  const int64_t n = (int64_t)cls.size();
  int32_t nb = 0;
  for (int64_t r = 0; r < stop; r++)
    if (cls[r] == kBamKept) nb = std::max(nb, bkt[r] + 1);
  std::vector<int64_t> cbase((size_t)nb + 1, 0), pos(n, -1);
  std::vector<uint8_t> has((size_t)nb, 0);
  for (int64_t r = 0; r < stop; r++)
    if (cls[r] == kBamKept) cbase[bkt[r] + 1] += olen[r], has[bkt[r]] = 1;
  for (int32_t k = 0; k < nb; k++) cbase[k + 1] += cbase[k];
  {
    std::vector<int64_t> cur(cbase.begin(), cbase.end() - 1);
    for (int64_t r = 0; r < stop; r++)
      if (cls[r] == kBamKept) {
        pos[r] = cur[bkt[r]];
        cur[bkt[r]] += olen[r];
      }
  }
  std::vector<char> outb((size_t)cbase[nb] + 1);
  DevBuf<char> d_out;
  c->hip(d_out.ensure(outb.size()), "alloc");
  if (stop) {
    c->hip(hipMemcpyAsync(d_pos.p, pos.data(), (size_t)stop * 8, hipMemcpyHostToDevice, c->st), "h2d");
    c->hip(launch(d_pos.p, d_out.p), "bam emit");
    c->hip(hipMemcpyAsync(outb.data(), d_out.p, (size_t)cbase[nb], hipMemcpyDeviceToHost, c->st), "d2h");
  }
  c->hip(hipStreamSynchronize(c->st), "sync");
  patch(pos, outb.data());
  std::vector<int32_t> used;
  for (int32_t k = 0; k < nb; k++)
    if (has[k]) used.push_back(k);
  const int T = std::max(1, std::min<int>(io_threads(), (int)used.size()));
  std::vector<int32_t> bad(T, -1);
  parallel_for(T, [&](int t) {
    for (size_t u = (size_t)t; u < used.size(); u += (size_t)T) {
      const int32_t k = used[u];
      const std::string fn = path_of(k);
      const int fd = open(fn.c_str(), O_WRONLY | O_CREAT | mode, 0666);
      bool ok = fd >= 0 && io::write_all(fd, outb.data() + cbase[k], (size_t)(cbase[k + 1] - cbase[k]));
      if (fd >= 0) ok = (close(fd) == 0) && ok;
      if (!ok) bad[t] = k;
    }
  });
  for (int32_t v : bad)
    if (v >= 0) c->fail(UMICLUST_EIO, "cannot write %s", path_of(v).c_str());
  return used;
}

// the region FASTA of the kept records (rows f4 / f4b): k_bam_emit, appended
template <typename PathOf>
std::vector<int32_t> emit_fasta(Ctx* c, const uint8_t* d_raw, const int64_t* d_roff, const int8_t* d_cls,
                                DevBuf<int64_t>& d_pos, const std::vector<int8_t>& cls, const std::vector<int32_t>& bkt,
                                const std::vector<int64_t>& olen, int64_t stop, PathOf path_of) {
  return emit_buckets(
      c, d_pos, cls, bkt, olen, stop, path_of, O_APPEND,
      [&](const int64_t* pos, char* out) { return launch_bam_emit(d_raw, d_roff, stop, d_cls, pos, out, c->st); },
      [](const std::vector<int64_t>&, char*) {});
}

// The five extraction parameters of umiclust_region_split_extract / umiclust_bam_split_extract.
struct UmiArgs {
  int32_t a5, a3, k;
  const char* fwd;
  const char* rev;
};
void check_umi_args(Ctx* c, const UmiArgs& u, ExtractPatterns& P) {
  if (u.a5 < 0 || u.a3 < 0 || u.k < 0) c->fail(UMICLUST_EINVAL, "bad argument");
  build_patterns(c, u.fwd, u.rev, P);
}

// The detected-UMI FASTA of the kept records among [0, stop) (row f4+f1): the UMI search on the records
// in place (k_bam_umi_search), the slots from its sizes, the text by k_bam_emit_umi -- by bam::format_umi_record for a
// record whose name holds "strand=" -- and one truncated file per bucket that holds a kept record.  A kept record
// whose name holds white space is refused before any file is opened.  per_bucket[b] (b < cap) = records written.
template <typename PathOf>
std::vector<int32_t> emit_umis(Ctx* c, const RawBuf& raw, const std::vector<int64_t>& roff,
                               const uint8_t* d_raw, const int64_t* d_roff, const int8_t* d_cls, DevBuf<int64_t>& d_pos,
                               const std::vector<int8_t>& cls, const std::vector<int32_t>& bkt, int64_t stop,
                               const UmiArgs& u, const ExtractPatterns& P, PathOf path_of, int64_t* per_bucket,
                               int32_t cap) {
  const int64_t n = (int64_t)cls.size();
  DevBuf<ExtractPatterns> d_pat;
  DevBuf<int32_t> d_res;
  DevBuf<int64_t> d_len;
  c->hip(d_pat.ensure(1), "alloc");
  c->hip(d_res.ensure((size_t)stop * 6 + 1), "alloc");
  c->hip(d_len.ensure((size_t)stop + 1), "alloc");
  std::vector<int64_t> olen((size_t)n, 0);
  c->hip(hipMemcpyAsync(d_pat.p, &P, sizeof(P), hipMemcpyHostToDevice, c->st), "h2d");
  c->hip(launch_bam_umi_search(d_raw, d_roff, stop, d_cls, u.a5, u.a3, u.k, d_pat.p, d_res.p, d_len.p, c->st),
         "bam umi search");
  if (stop) c->hip(hipMemcpyAsync(olen.data(), d_len.p, (size_t)stop * 8, hipMemcpyDeviceToHost, c->st), "d2h");
  c->hip(hipStreamSynchronize(c->st), "sync");
  std::vector<std::pair<int64_t, std::string>> host_text;  // the records the host formats, in BAM order
  for (int64_t r = 0; r < stop; r++) {
    if (olen[r] == kUmiBadName) {
      const std::string name(record_name(raw, roff, r));
      c->fail(UMICLUST_EFORMAT, "BAM record %lld: white space in the query name '%s'", (long long)r, name.c_str());
    }
    if (olen[r] == kUmiHostName) host_text.emplace_back(r, std::string());
  }
  if (!host_text.empty()) {
    std::vector<int32_t> res((size_t)stop * 6);
    c->hip(hipMemcpyAsync(res.data(), d_res.p, res.size() * 4, hipMemcpyDeviceToHost, c->st), "d2h");
    c->hip(hipStreamSynchronize(c->st), "sync");
    for (auto& [r, text] : host_text) {
      text = bam::format_umi_record(raw.data() + roff[r], res.data() + r * 6, u.a3);
      olen[r] = (int64_t)text.size();
    }
  }
  if (cap > 0) memset(per_bucket, 0, sizeof(int64_t) * (size_t)cap);
  for (int64_t r = 0; r < stop; r++)
    if (cls[r] == kBamKept && olen[r] > 0 && bkt[r] < cap) per_bucket[bkt[r]]++;
  return emit_buckets(
      c, d_pos, cls, bkt, olen, stop, path_of, O_TRUNC,
      [&](const int64_t* pos, char* out) {
        return launch_bam_emit_umi(d_raw, d_roff, stop, d_len.p, d_res.p, pos, u.a3, out, c->st);
      },
      [&](const std::vector<int64_t>& pos, char* out) {
        for (const auto& [r, text] : host_text) memcpy(out + pos[r], text.data(), text.size());
      });
}

// What the round-1 split reads: the inflated file on the host and on the device, its header and its record offsets.
// The path-based entries fill it from read_bam_on_device and own what they made; the session entries point into the
// open session and upload its raw, as umiclust_bam_split does.
struct SplitSource {
  const RawBuf* raw = nullptr;
  const bam::Header* hdr = nullptr;
  const std::vector<int64_t>* roff = nullptr;
  const uint8_t* d_raw = nullptr;
  std::string what;  // the file's name in a refusal
  RawBuf own_raw;
  bam::Header own_hdr;
  std::vector<int64_t> own_roff;
  DevBuf<uint8_t> own_d_raw;

  void from_path(Ctx* c, const char* bam_file) {
    // the file inflated on the device: raw there (d_raw) and on the host
    int64_t inflate_info[3];
    if (!read_bam_on_device(c, bam_file, own_raw, own_d_raw, inflate_info, nullptr))
      c->fail(UMICLUST_EIO, "cannot read BGZF/BAM %s", bam_file);
    std::string herr;
    if (!bam::parse_header(own_raw.data(), own_raw.size(), own_hdr, herr)) c->fail(UMICLUST_EFORMAT, "%s is not BAM", bam_file);
    if (!bam::record_offsets(own_raw.data(), own_raw.size(), own_hdr.end, own_roff, herr))
      c->fail(UMICLUST_EFORMAT, "truncated BAM record");
    raw = &own_raw, hdr = &own_hdr, roff = &own_roff, d_raw = own_d_raw.p, what = bam_file;
  }
  void from_session(Ctx* c) {
    const BamSession& S = *bam_session(c);
    c->hip(own_d_raw.ensure(S.raw.size() + 1), "alloc");
    if (S.raw.size())
      c->hip(hipMemcpyAsync(own_d_raw.p, S.raw.data(), S.raw.size(), hipMemcpyHostToDevice, c->st), "h2d");
    raw = &S.raw, hdr = &S.hdr, roff = &S.roff, d_raw = own_d_raw.p, what = "the BAM session";
  }
};

// umiclust_region_split (umi null: region_cluster<k>.fasta in out_dir) and umiclust_region_split_extract (umi set:
// region_cluster<k>_detected_umis.fasta in out_dir, their record counts in umis_per_cluster); session: the open
// session is the file and bam_file is not read (umiclust_bam_region_split[_extract])
int64_t region_split_impl(umiclust_ctx* ctx, bool session, const char* bam_file, int32_t nregions,
                          const char* const* region_names,
                          const int64_t* region_lengths, const int32_t* region_clusters, double minimal_region_overlap,
                          int32_t max_softclip_5_end, int32_t max_softclip_3_end, const UmiArgs* umi,
                          const char* out_dir, int64_t* counts, int64_t* reads_per_cluster, int64_t* umis_per_cluster,
                          int32_t ncluster_cap, uint8_t* region_detected, char* missing_name, int32_t missing_cap) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    if (umi && ncluster_cap > 0 && !umis_per_cluster) c->fail(UMICLUST_EINVAL, "bad argument");
    ExtractPatterns pat;
    if (umi) check_umi_args(c, *umi, pat);
    if ((!session && !bam_file) || !out_dir || nregions < 0 || (nregions > 0 && (!region_names || !region_lengths || !region_clusters)) ||
        !counts || ncluster_cap < 0 || (ncluster_cap > 0 && !reads_per_cluster))
      c->fail(UMICLUST_EINVAL, "bad argument");
    SplitSource src;
    if (session)
      src.from_session(c);
    else
      src.from_path(c, bam_file);
    const RawBuf& raw = *src.raw;
    const bam::Header& hdr = *src.hdr;
    const std::vector<int64_t>& roff = *src.roff;
    const uint8_t* const d_raw = src.d_raw;
    std::string herr;
    // the reference names of the header, matched to the regions of the reference FASTA
    std::unordered_map<std::string, int32_t> rid;
    for (int32_t r = 0; r < nregions; r++) rid.emplace(region_names[r], r);
    const int32_t nref = (int32_t)hdr.ref_name.size();
    const std::vector<std::string>& refname = hdr.ref_name;
    std::vector<int64_t> rlen(nref, -1);
    std::vector<int32_t> rclu(nref, -1), rreg(nref, -1);
    for (int32_t r = 0; r < nref; r++) {
      auto it = rid.find(refname[r]);
      if (it != rid.end()) {
        rreg[r] = it->second;
        rlen[r] = region_lengths[it->second];
        rclu[r] = region_clusters[it->second];
      }
    }
    // the kernels index each record by its own l_read_name, n_cigar_op and l_seq
    if (!bam::check_record_fields(raw.data(), roff, herr)) c->fail(UMICLUST_EFORMAT, "%s: %s", src.what.c_str(), herr.c_str());
    const int64_t n = (int64_t)roff.size();
    // device: classify every record where the decoder wrote it
    DevBuf<int64_t> d_roff, d_rlen, d_outlen, d_pos;
    DevBuf<int32_t> d_rclu, d_clu;
    DevBuf<int8_t> d_cls;
    alloc_each(c, (size_t)n + 1, d_roff, d_cls, d_clu, d_outlen, d_pos);
    alloc_each(c, (size_t)nref + 1, d_rlen, d_rclu);
    if (n) c->hip(hipMemcpyAsync(d_roff.p, roff.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->st), "h2d");
    if (nref) {
      c->hip(hipMemcpyAsync(d_rlen.p, rlen.data(), (size_t)nref * 8, hipMemcpyHostToDevice, c->st), "h2d");
      c->hip(hipMemcpyAsync(d_rclu.p, rclu.data(), (size_t)nref * 4, hipMemcpyHostToDevice, c->st), "h2d");
    }
    c->hip(launch_bam_classify(d_raw, d_roff.p, n, nref, d_rlen.p, d_rclu.p, minimal_region_overlap,
                               max_softclip_5_end, max_softclip_3_end, d_cls.p, d_clu.p, d_outlen.p, c->st),
           "bam classify");
    std::vector<int8_t> cls(n);
    std::vector<int32_t> clu(n);
    std::vector<int64_t> olen(n);
    if (n) {
      c->hip(hipMemcpyAsync(cls.data(), d_cls.p, (size_t)n, hipMemcpyDeviceToHost, c->st), "d2h");
      c->hip(hipMemcpyAsync(clu.data(), d_clu.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->st), "d2h");
      c->hip(hipMemcpyAsync(olen.data(), d_outlen.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->st), "d2h");
    }
    c->hip(hipStreamSynchronize(c->st), "sync");
    // the reference raises KeyError at the first record whose region is unknown, after the records before it
    int64_t stop = n;
    for (int64_t r = 0; r < n && stop == n; r++)
      if (cls[r] == kBamNoRegion || cls[r] == kBamNoCluster) stop = r;
    int32_t ncl = 0;
    for (int64_t r = 0; r < stop; r++)
      if (cls[r] == kBamKept) ncl = std::max(ncl, clu[r] + 1);
    // output grouped by cluster, records in BAM order within a cluster
    const auto cluster_fasta = [&](int32_t k) { return pjoin(out_dir, "region_cluster" + std::to_string(k) + ".fasta"); };
    const auto cluster_umis = [&](int32_t k) {
      return pjoin(out_dir, "region_cluster" + std::to_string(k) + "_detected_umis.fasta");
    };
    // (the reference's KeyError ends the pipeline before extract_umis starts: no UMI file then)
    std::vector<int32_t> used;
    if (!umi)
      used = emit_fasta(c, d_raw, d_roff.p, d_cls.p, d_pos, cls, clu, olen, stop, cluster_fasta);
    else if (stop == n)
      used = emit_umis(c, raw, roff, d_raw, d_roff.p, d_cls.p, d_pos, cls, clu, stop, *umi, pat, cluster_umis,
                       umis_per_cluster, ncluster_cap);
    // counters of the records the reference reached
    int64_t cnt[4] = {0, 0, 0, 0};  // unmapped, primary mapped, short, long
    if (reads_per_cluster) memset(reads_per_cluster, 0, sizeof(int64_t) * (size_t)ncluster_cap);
    if (region_detected) memset(region_detected, 0, (size_t)nregions);
    const int64_t last = stop < n ? stop + 1 : n;  // the failing record counts as a primary alignment too
    for (int64_t r = 0; r < last; r++) {
      const int8_t k = cls[r];
      if (k == kBamUnmapped) cnt[0]++;
      if (k >= kBamShort) cnt[1]++;
      if (k == kBamShort) cnt[2]++;
      if (k == kBamLong) cnt[3]++;
      if (k == kBamKept && r < stop) {
        if (clu[r] < ncluster_cap) reads_per_cluster[clu[r]]++;
        const int32_t ref = rd_i32(raw.data() + roff[r] + 4);
        if (region_detected && rreg[ref] >= 0) region_detected[rreg[ref]] = 1;
      }
    }
    for (int x = 0; x < 4; x++) counts[x] = cnt[x];
    if (stop < n) {
      const int32_t ref = rd_i32(raw.data() + roff[stop] + 4);
      const std::string nm = ref >= 0 && ref < nref ? refname[ref] : std::string("None");
      if (missing_name && missing_cap > 0) snprintf(missing_name, (size_t)missing_cap, "%s", nm.c_str());
      c->fail(UMICLUST_EFORMAT, "KeyError: '%s'", nm.c_str());
    }
    if (ncl > ncluster_cap) c->fail(UMICLUST_ERANGE, "cluster ids up to %d exceed the counter capacity", ncl - 1);
    return (int64_t)used.size();
  });
}
}  // namespace

int64_t umiclust_region_split(umiclust_ctx* ctx, const char* bam_file, int32_t nregions, const char* const* region_names,
                              const int64_t* region_lengths, const int32_t* region_clusters,
                              double minimal_region_overlap, int32_t max_softclip_5_end, int32_t max_softclip_3_end,
                              const char* out_dir, int64_t* counts, int64_t* reads_per_cluster, int32_t ncluster_cap,
                              uint8_t* region_detected, char* missing_name, int32_t missing_cap) {
  return region_split_impl(ctx, false, bam_file, nregions, region_names, region_lengths, region_clusters,
                           minimal_region_overlap, max_softclip_5_end, max_softclip_3_end, nullptr, out_dir, counts, reads_per_cluster, nullptr,
                           ncluster_cap, region_detected, missing_name, missing_cap);
}

int64_t umiclust_region_split_extract(umiclust_ctx* ctx, const char* bam_file, int32_t nregions,
                                      const char* const* region_names, const int64_t* region_lengths,
                                      const int32_t* region_clusters, double minimal_region_overlap,
                                      int32_t max_softclip_5_end, int32_t max_softclip_3_end,
                                      int32_t adapter_length_5_end, int32_t adapter_length_3_end, int32_t max_pattern_dist,
                                      const char* umi_fwd, const char* umi_rev, const char* umi_out_dir, int64_t* counts,
                                      int64_t* reads_per_cluster, int64_t* umis_per_cluster, int32_t ncluster_cap,
                                      uint8_t* region_detected, char* missing_name, int32_t missing_cap) {
  const UmiArgs umi{adapter_length_5_end, adapter_length_3_end, max_pattern_dist, umi_fwd, umi_rev};
  return region_split_impl(ctx, false, bam_file, nregions, region_names, region_lengths, region_clusters,
                           minimal_region_overlap, max_softclip_5_end, max_softclip_3_end, &umi, umi_out_dir, counts, reads_per_cluster,
                           umis_per_cluster, ncluster_cap, region_detected, missing_name, missing_cap);
}

// the same two on the open session: no bam_file, everything else as above
int64_t umiclust_bam_region_split(umiclust_ctx* ctx, int32_t nregions, const char* const* region_names,
                                  const int64_t* region_lengths, const int32_t* region_clusters,
                                  double minimal_region_overlap, int32_t max_softclip_5_end, int32_t max_softclip_3_end,
                                  const char* out_dir, int64_t* counts, int64_t* reads_per_cluster,
                                  int32_t ncluster_cap, uint8_t* region_detected, char* missing_name,
                                  int32_t missing_cap) {
  return region_split_impl(ctx, true, nullptr, nregions, region_names, region_lengths, region_clusters,
                           minimal_region_overlap, max_softclip_5_end, max_softclip_3_end, nullptr, out_dir, counts,
                           reads_per_cluster, nullptr, ncluster_cap, region_detected, missing_name, missing_cap);
}

int64_t umiclust_bam_region_split_extract(umiclust_ctx* ctx, int32_t nregions, const char* const* region_names,
                                          const int64_t* region_lengths, const int32_t* region_clusters,
                                          double minimal_region_overlap, int32_t max_softclip_5_end,
                                          int32_t max_softclip_3_end, int32_t adapter_length_5_end,
                                          int32_t adapter_length_3_end, int32_t max_pattern_dist, const char* umi_fwd,
                                          const char* umi_rev, const char* umi_out_dir, int64_t* counts,
                                          int64_t* reads_per_cluster, int64_t* umis_per_cluster, int32_t ncluster_cap,
                                          uint8_t* region_detected, char* missing_name, int32_t missing_cap) {
  const UmiArgs umi{adapter_length_5_end, adapter_length_3_end, max_pattern_dist, umi_fwd, umi_rev};
  return region_split_impl(ctx, true, nullptr, nregions, region_names, region_lengths, region_clusters,
                           minimal_region_overlap, max_softclip_5_end, max_softclip_3_end, &umi, umi_out_dir, counts,
                           reads_per_cluster, umis_per_cluster, ncluster_cap, region_detected, missing_name,
                           missing_cap);
}

// ---------------------------------------------------------------- k_bgzf_inflate alone (kernel-level entry point, §9e)
int64_t umiclust_bgzf_inflate(umiclust_ctx* ctx, const uint8_t* file, int64_t n, uint8_t* out, int64_t cap,
                              int32_t* block_status, int64_t* n_blocks, double* times) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    if (n < 0 || (n > 0 && !file)) c->fail(UMICLUST_EINVAL, "bad argument");
    BgzfPlan P;
    if (!bgzf_plan(file, (size_t)n, P)) c->fail(UMICLUST_EFORMAT, "malformed BGZF framing");
    if (n_blocks) *n_blocks = P.n_blocks;
    if (cap == 0) return P.total;
    if (!out || cap < P.total)
      c->fail(UMICLUST_ERANGE, "buffer of %lld bytes, %lld needed", (long long)cap, (long long)P.total);
    DevBuf<uint8_t> d_raw;
    std::vector<int32_t> status;
    bgzf_inflate_device(c, file, (size_t)n, P, d_raw, status, [&]() { return out; }, times);
    if (block_status) {
      std::fill(block_status, block_status + P.n_blocks, 0);
      for (size_t b = 0; b < status.size(); b++) block_status[P.file_idx[b]] = status[b];
    }
    for (size_t b = 0; b < status.size(); b++)
      if (status[b])
        c->fail(UMICLUST_EFORMAT, "BGZF block %lld: %s (class %d)", (long long)P.file_idx[b],
                inf::status_name(status[b]), status[b]);
    return P.total;
  });
}

// ---------------------------------------------------------------- k_bgzf_deflate alone (kernel-level entry point, §9g)
int64_t umiclust_bgzf_deflate(umiclust_ctx* ctx, const uint8_t* data, int64_t n, uint8_t* out, int64_t cap,
                              int32_t* block_kind, int64_t* n_blocks, double* times) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    if (n < 0 || (n > 0 && !data)) c->fail(UMICLUST_EINVAL, "bad argument");
    const size_t nb = ((size_t)n + kBlk - 1) / kBlk;
    const int64_t bound = (int64_t)(nb * kFramedMax + sizeof bam::kBgzfEof);
    if (n_blocks) *n_blocks = (int64_t)nb;
    if (cap == 0) return bound;
    if (!out || cap < bound) c->fail(UMICLUST_ERANGE, "buffer of %lld bytes, %lld needed", (long long)cap, (long long)bound);
    if (times) times[0] = times[1] = times[2] = 0;
    size_t total = 0;
    if (nb) {
      DeflateDev D;
      c->hip(D.ensure(nb), "alloc");
      std::vector<uint32_t> crc(nb);
      const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)io_threads(), nb));
      parallel_for(T, [&](int t) {
        for (size_t b = (size_t)t; b < nb; b += (size_t)T)
          crc[b] = bam::bgzf_crc32(data + b * kBlk, std::min(kBlk, (size_t)n - b * kBlk));
      });
      total = deflate_batch(c, D, data, (size_t)n, nb, crc.data(), out, times);
      for (size_t b = 0; b < nb; b++) {
        if (D.meta[4 * b + 2]) c->fail(UMICLUST_EDEVICE, "BGZF block %zu: the encoder refused it (status %d)", b, D.meta[4 * b + 2]);
        if (block_kind) block_kind[b] = D.meta[4 * b];
      }
    }
    memcpy(out + total, bam::kBgzfEof, sizeof bam::kBgzfEof);
    return (int64_t)(total + sizeof bam::kBgzfEof);
  });
}

// ---------------------------------------------------------------- BAM session: scan with tags, cs group-by, writer (§8f f6)
namespace {
// What every open ends with, once S.raw holds the inflated file and d_raw the same bytes on the device: the header,
// the record offsets, the scan with tags, the cs group-by, and the session put in place.  t_upload: the seconds the
// open has already spent uploading.  Returns the number of records.
int64_t finish_open(Ctx* c, BamSession& S, DevBuf<uint8_t>& d_raw, const char* bam_file, int32_t hash_bits,
                    double t_upload) {
  DevBuf<uint8_t> d_nmp;
  std::string herr;
  if (!bam::parse_header(S.raw.data(), S.raw.size(), S.hdr, herr)) c->fail(UMICLUST_EFORMAT, "%s: %s", bam_file, herr.c_str());
  if (!bam::record_offsets(S.raw.data(), S.raw.size(), S.hdr.end, S.roff, herr))
    c->fail(UMICLUST_EFORMAT, "%s: %s", bam_file, herr.c_str());
  const int64_t n = (int64_t)S.roff.size();
  uint64_t m = 1024;
  while (m < 2 * (uint64_t)n) m <<= 1;
  DevBuf<int64_t> d_roff, d_reflen, d_cols, d_nm, d_csoff, d_slot;
  DevBuf<int32_t> d_ref, d_lseq, d_cslen;
  DevBuf<int8_t> d_cls, d_bad;
  DevBuf<uint64_t> d_hash;
  DevBuf<unsigned long long> d_keys, d_rep;
  DevBuf<uint32_t> d_cnt, d_coll;
  alloc_each(c, (size_t)n + 1, d_roff, d_reflen, d_cols, d_nm, d_csoff, d_slot, d_ref, d_lseq, d_cslen, d_cls, d_bad,
             d_nmp, d_hash);
  alloc_each(c, (size_t)m, d_keys, d_rep, d_cnt);
  c->hip(d_coll.ensure(1), "alloc");
  float ms = 0.f;
  c->hip(hipEventRecord(c->ev0, c->st), "event");
  if (n) c->hip(hipMemcpyAsync(d_roff.p, S.roff.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->st), "h2d");
  c->hip(hipEventRecord(c->ev1, c->st), "event");
  c->hip(hipEventSynchronize(c->ev1), "sync");
  c->hip(hipEventElapsedTime(&ms, c->ev0, c->ev1), "elapsed");
  S.t_h2d = t_upload + ms * 1e-3;  // the compressed bytes and roff
  const BamScanCols o{d_cls.p, d_ref.p, d_lseq.p, d_reflen.p, d_cols.p, d_nm.p, d_nmp.p, d_csoff.p, d_cslen.p, d_hash.p,
                      d_bad.p};
  // hash, group, verify; a detected collision (two different strings, one hash) moves on to the next seed
  constexpr int kMaxSeeds = 8;
  int pass = 0;
  for (;; pass++) {
    if (pass == kMaxSeeds) c->fail(UMICLUST_EDEVICE, "cs hash collisions under %d seeds", kMaxSeeds);
    const uint64_t hmask = (pass == 0 && hash_bits < 64) ? ((1ull << hash_bits) - 1) : ~0ull;
    uint32_t coll = 0;
    c->hip(hipEventRecord(c->ev0, c->st), "event");
    c->hip(launch_bam_scan(d_raw.p, (int64_t)S.raw.size(), d_roff.p, n, bam::cs_seed(pass), hmask, o, c->st), "bam scan");
    c->hip(launch_cs_group(d_raw.p, o, n, m - 1, d_keys.p, d_rep.p, d_cnt.p, d_slot.p, d_coll.p, c->st), "cs group");
    c->hip(hipEventRecord(c->ev1, c->st), "event");
    c->hip(hipMemcpyAsync(&coll, d_coll.p, 4, hipMemcpyDeviceToHost, c->st), "d2h");
    c->hip(hipStreamSynchronize(c->st), "sync");
    c->hip(hipEventElapsedTime(&ms, c->ev0, c->ev1), "elapsed");
    S.t_dev += ms * 1e-3;
    if (!coll) break;
  }
  S.n_reruns = pass;
  S.cls.resize(n), S.ref.resize(n), S.l_seq.resize(n), S.reflen.resize(n), S.cols.resize(n), S.nm.resize(n);
  S.nm_present.resize(n), S.cs_off.resize(n), S.cs_len.resize(n), S.cs_group.assign(n, -1);
  std::vector<int8_t> bad(n);
  std::vector<int64_t> slot(n);
  std::vector<unsigned long long> rep((size_t)m);
  std::vector<uint32_t> cnt((size_t)m);
  if (n) {
    auto d2h = [&](void* dst, const void* src, size_t bytes) {
      c->hip(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->st), "d2h");
    };
    d2h(S.cls.data(), d_cls.p, (size_t)n), d2h(S.ref.data(), d_ref.p, (size_t)n * 4);
    d2h(S.l_seq.data(), d_lseq.p, (size_t)n * 4), d2h(S.reflen.data(), d_reflen.p, (size_t)n * 8);
    d2h(S.cols.data(), d_cols.p, (size_t)n * 8), d2h(S.nm.data(), d_nm.p, (size_t)n * 8);
    d2h(S.nm_present.data(), d_nmp.p, (size_t)n), d2h(S.cs_off.data(), d_csoff.p, (size_t)n * 8);
    d2h(S.cs_len.data(), d_cslen.p, (size_t)n * 4), d2h(bad.data(), d_bad.p, (size_t)n);
    d2h(slot.data(), d_slot.p, (size_t)n * 8), d2h(rep.data(), d_rep.p, (size_t)m * 8);
    d2h(cnt.data(), d_cnt.p, (size_t)m * 4);
    c->hip(hipStreamSynchronize(c->st), "sync");
  }
  for (int64_t r = 0; r < n; r++)
    if (bad[r] && S.first_bad < 0) S.first_bad = r;  // a primary one fails below: what stays is a record never read
  for (int64_t r = 0; r < n; r++)
    if (S.cls[r] == bam::kScanPrimary && bad[r]) {
      const std::string name(record_name(S.raw, S.roff, r));
      c->fail(UMICLUST_EFORMAT, "malformed BAM record %lld (%s): a field or an aux tag does not fit the record",
              (long long)r, name.c_str());
    }
  // dense group ids in order of the representative = first-seen order (a representative is its group's first record)
  std::vector<int32_t> gid_of_slot;
  gid_of_slot.assign((size_t)m, -1);
  for (int64_t r = 0; r < n; r++) {
    const int64_t s = slot[r];
    if (s < 0) continue;
    if ((int64_t)rep[s] == r) {
      gid_of_slot[s] = (int32_t)S.g_rep.size();
      S.g_rep.push_back(r);
      S.g_count.push_back((int64_t)cnt[s]);
    }
    S.cs_group[r] = gid_of_slot[s];
  }
  S.open = true;
  c->bs = std::move(S);
  return n;
}
}  // namespace

int64_t umiclust_bam_open(umiclust_ctx* ctx, const char* bam_file, int32_t hash_bits) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    if (!bam_file || hash_bits < 1 || hash_bits > 64) c->fail(UMICLUST_EINVAL, "bad argument");
    c->bs = BamSession();
    BamSession S;
    DevBuf<uint8_t> d_raw;
    const double t0 = now_s();
    double t_upload = 0;
    if (!read_bam_on_device(c, bam_file, S.raw, d_raw, S.inflate_info, &t_upload))
      c->fail(UMICLUST_EIO, "cannot read BGZF/BAM %s", bam_file);
    S.t_inflate = now_s() - t0;  // from mapping the file until raw is on the host
    return finish_open(c, S, d_raw, bam_file, hash_bits, t_upload);
  });
}

int64_t umiclust_sam_open(umiclust_ctx* ctx, const char* sam_file, int32_t hash_bits) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    if (!sam_file || hash_bits < 1 || hash_bits > 64) c->fail(UMICLUST_EINVAL, "bad argument");
    c->bs = BamSession();
    BamSession S;
    DevBuf<uint8_t> d_raw;
    const double t0 = now_s();
    S.from_sam = true;
    read_sam_on_device(c, sam_file, S.raw, d_raw, S.sam_info, S.sam_times);
    S.t_inflate = now_s() - t0;  // from reading the text until raw is on the host
    return finish_open(c, S, d_raw, sam_file, hash_bits, S.sam_times[0]);
  });
}

int32_t umiclust_sam_info(umiclust_ctx* ctx, int64_t* out, double* times) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    auto& S = *bam_session(c);
    if (!S.from_sam) c->fail(UMICLUST_ESTATE, "the session was not opened from SAM text (umiclust_sam_open)");
    if (out)
      for (int x = 0; x < 4; x++) out[x] = S.sam_info[x];
    if (times)
      for (int x = 0; x < 5; x++) times[x] = S.sam_times[x];
    return UMICLUST_OK;
  });
}

int32_t umiclust_bam_counts(umiclust_ctx* ctx, int64_t* out) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    auto& S = *bam_session(c);
    if (!out) c->fail(UMICLUST_EINVAL, "null argument");
    out[0] = (int64_t)S.roff.size();
    out[1] = (int64_t)S.hdr.ref_name.size();
    out[2] = (int64_t)S.g_rep.size();
    out[3] = S.n_reruns;
    out[4] = S.first_bad;
    return UMICLUST_OK;
  });
}

int32_t umiclust_bam_times(umiclust_ctx* ctx, double* out) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    auto& S = *bam_session(c);
    if (!out) c->fail(UMICLUST_EINVAL, "null argument");
    out[0] = S.t_inflate, out[1] = S.t_h2d, out[2] = S.t_dev;
    return UMICLUST_OK;
  });
}

int32_t umiclust_bam_inflate_info(umiclust_ctx* ctx, int64_t* out) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    auto& S = *bam_session(c);
    if (!out) c->fail(UMICLUST_EINVAL, "null argument");
    for (int x = 0; x < 3; x++) out[x] = S.inflate_info[x];
    return UMICLUST_OK;
  });
}

int32_t umiclust_bam_columns(umiclust_ctx* ctx, int8_t* cls, int32_t* ref, int32_t* l_seq, int64_t* reference_length,
                             int64_t* cols, int64_t* nm, uint8_t* nm_present, int32_t* cs_group) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    auto& S = *bam_session(c);
    const size_t n = S.roff.size();
    if (n) {
      if (cls) memcpy(cls, S.cls.data(), n);
      if (ref) memcpy(ref, S.ref.data(), n * 4);
      if (l_seq) memcpy(l_seq, S.l_seq.data(), n * 4);
      if (reference_length) memcpy(reference_length, S.reflen.data(), n * 8);
      if (cols) memcpy(cols, S.cols.data(), n * 8);
      if (nm) memcpy(nm, S.nm.data(), n * 8);
      if (nm_present) memcpy(nm_present, S.nm_present.data(), n);
      if (cs_group) memcpy(cs_group, S.cs_group.data(), n * 4);
    }
    return UMICLUST_OK;
  });
}

int32_t umiclust_bam_refs(umiclust_ctx* ctx, char* buf, int64_t cap, int64_t* off, int64_t* len) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    auto& S = *bam_session(c);
    int64_t need = 0;
    for (const std::string& s : S.hdr.ref_name) need += (int64_t)s.size() + 1;
    if (need > INT32_MAX) c->fail(UMICLUST_ERANGE, "reference names exceed 2 GiB");
    if (cap == 0) return (int32_t)need;
    if (!buf || !off || cap < need) c->fail(UMICLUST_ERANGE, "buffer of %lld bytes, %lld needed", (long long)cap, (long long)need);
    int64_t o = 0;
    for (size_t r = 0; r < S.hdr.ref_name.size(); r++) {
      off[r] = o;
      memcpy(buf + o, S.hdr.ref_name[r].c_str(), S.hdr.ref_name[r].size() + 1);
      o += (int64_t)S.hdr.ref_name[r].size() + 1;
      if (len) len[r] = S.hdr.ref_len[r];
    }
    off[S.hdr.ref_name.size()] = o;
    return (int32_t)need;
  });
}

int64_t umiclust_bam_strings(umiclust_ctx* ctx, int32_t kind, const int64_t* rec, int64_t m, char* buf, int64_t cap,
                             int64_t* off) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    auto& S = *bam_session(c);
    const int64_t n = (int64_t)S.roff.size();
    if ((kind != 0 && kind != 1) || m < 0 || (m > 0 && !rec)) c->fail(UMICLUST_EINVAL, "bad argument");
    auto span = [&](int64_t r, const uint8_t*& p) -> int64_t {
      if (kind == 1) {
        p = S.raw.data() + S.cs_off[r];
        return std::max<int64_t>(0, S.cs_len[r]);
      }
      const std::string_view name = record_name(S.raw, S.roff, r);
      p = (const uint8_t*)name.data();
      return (int64_t)name.size();
    };
    int64_t need = 0;
    const uint8_t* p = nullptr;
    for (int64_t x = 0; x < m; x++) {
      if (rec[x] < 0 || rec[x] >= n) c->fail(UMICLUST_EINVAL, "record %lld out of range", (long long)rec[x]);
      need += span(rec[x], p);
    }
    if (cap == 0) return need;
    if (!buf || !off || cap < need) c->fail(UMICLUST_ERANGE, "buffer of %lld bytes, %lld needed", (long long)cap, (long long)need);
    int64_t o = 0;
    for (int64_t x = 0; x < m; x++) {
      const int64_t ln = span(rec[x], p);
      off[x] = o;
      if (ln) memcpy(buf + o, p, (size_t)ln);
      o += ln;
    }
    off[m] = o;
    return need;
  });
}

int32_t umiclust_bam_cs_groups(umiclust_ctx* ctx, int64_t* count, int64_t* rep) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    auto& S = *bam_session(c);
    const size_t g = S.g_rep.size();
    if (g && count) memcpy(count, S.g_count.data(), g * 8);
    if (g && rep) memcpy(rep, S.g_rep.data(), g * 8);
    return UMICLUST_OK;
  });
}

int64_t umiclust_bam_write(umiclust_ctx* ctx, const uint8_t* keep, const char* out_bam) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    auto& S = *bam_session(c);
    if (!out_bam || (!keep && !S.roff.empty())) c->fail(UMICLUST_EINVAL, "null argument");
    std::string err;
    static const uint8_t none = 0;
    if (!keep) keep = &none;  // (no records: nothing reads it)
    int64_t k = c->tun.bgzf_device ? write_bgzf_device(c, S, keep, out_bam, err) : -2;
    if (k == -2) {  // the host writer: by the switch, or without the memory for a batch
      k = bam::write_bgzf(out_bam, S.raw.data(), S.hdr.end, S.roff, keep, io_threads(), err);
      std::fill(S.write_info, S.write_info + 8, 0);
      std::fill(S.write_times, S.write_times + 4, 0.0);
      struct stat sb;
      if (k >= 0 && stat(out_bam, &sb) == 0) {
        S.write_info[0] = (int64_t)bam::bgzf_stream(S.raw.data(), S.hdr.end, S.roff, keep).blocks();
        S.write_info[7] = (int64_t)sb.st_size;
      }
    }
    if (k < 0) c->fail(UMICLUST_EIO, "%s", err.c_str());
    S.wrote = true;
    return k;
  });
}

int32_t umiclust_bam_write_info(umiclust_ctx* ctx, int64_t* out, double* times) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    auto& S = *bam_session(c);
    if (!S.wrote) c->fail(UMICLUST_ESTATE, "the session has written no file (umiclust_bam_write)");
    if (out) memcpy(out, S.write_info, sizeof S.write_info);
    if (times) memcpy(times, S.write_times, sizeof S.write_times);
    return UMICLUST_OK;
  });
}

// ---------------------------------------------------------------- region split and name suffix on the session (§8f f4b / f6b)
// The session holds the inflated file and its columns on the host only (ctx.h BamSession), so each of the two calls
// below uploads what its kernel reads -- the raw bytes and record offsets, and for the split the four columns and the
// keep mask -- and frees it on return: no device memory outlives a call.
namespace {
// umiclust_bam_split (umi null: bucket_paths are region FASTA files, appended to) and umiclust_bam_split_extract (umi
// set: bucket_paths are detected-UMI FASTA files, truncated, their record counts in umis_per_bucket)
int64_t bam_split_impl(umiclust_ctx* ctx, const uint8_t* keep, int32_t nregions, const char* const* region_names,
                       const int64_t* region_lengths, const int32_t* region_buckets, int32_t nbuckets,
                       const char* const* bucket_paths, double minimal_region_overlap, int32_t max_softclip_5_end,
                       int32_t max_softclip_3_end, const UmiArgs* umi, int64_t* counts, int64_t* reads_per_bucket,
                       int64_t* umis_per_bucket, uint8_t* region_detected, char* missing_name, int32_t missing_cap) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    auto& S = *bam_session(c);
    if (umi && nbuckets > 0 && !umis_per_bucket) c->fail(UMICLUST_EINVAL, "bad argument");
    ExtractPatterns pat;
    if (umi) check_umi_args(c, *umi, pat);
    if (nregions < 0 || (nregions > 0 && (!region_names || !region_lengths || !region_buckets)) || nbuckets < 0 ||
        (nbuckets > 0 && (!bucket_paths || !reads_per_bucket)) || !counts)
      c->fail(UMICLUST_EINVAL, "bad argument");
    for (int32_t r = 0; r < nregions; r++)
      if (region_buckets[r] >= nbuckets) c->fail(UMICLUST_EINVAL, "region %d: bucket %d of %d", r, region_buckets[r], nbuckets);
    std::unordered_map<std::string, int32_t> rid;
    for (int32_t r = 0; r < nregions; r++) rid.emplace(region_names[r], r);
    const int32_t nref = (int32_t)S.hdr.ref_name.size();
    std::vector<int64_t> rlen(nref, -1);
    std::vector<int32_t> rbkt(nref, -1), rreg(nref, -1);
    for (int32_t r = 0; r < nref; r++) {
      auto it = rid.find(S.hdr.ref_name[r]);
      if (it != rid.end()) {
        rreg[r] = it->second;
        rlen[r] = region_lengths[it->second];
        rbkt[r] = region_buckets[it->second];
      }
    }
    const int64_t n = (int64_t)S.roff.size();
    DevBuf<uint8_t> d_raw, d_keep;
    DevBuf<int64_t> d_roff, d_reflen, d_rlen, d_outlen, d_pos;
    DevBuf<int32_t> d_ref, d_lseq, d_rbkt, d_bkt;
    DevBuf<int8_t> d_scan, d_cls;
    c->hip(d_raw.ensure(S.raw.size() + 1), "alloc");
    alloc_each(c, (size_t)n + 1, d_keep, d_roff, d_reflen, d_outlen, d_pos, d_ref, d_lseq, d_bkt, d_scan, d_cls);
    alloc_each(c, (size_t)nref + 1, d_rlen, d_rbkt);
    auto h2d = [&](void* dst, const void* src, size_t bytes) {
      if (bytes) c->hip(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->st), "h2d");
    };
    h2d(d_raw.p, S.raw.data(), S.raw.size()), h2d(d_roff.p, S.roff.data(), (size_t)n * 8);
    h2d(d_scan.p, S.cls.data(), (size_t)n), h2d(d_ref.p, S.ref.data(), (size_t)n * 4);
    h2d(d_lseq.p, S.l_seq.data(), (size_t)n * 4), h2d(d_reflen.p, S.reflen.data(), (size_t)n * 8);
    if (keep) h2d(d_keep.p, keep, (size_t)n);
    h2d(d_rlen.p, rlen.data(), (size_t)nref * 8), h2d(d_rbkt.p, rbkt.data(), (size_t)nref * 4);
    BamScanCols o{};
    o.cls = d_scan.p, o.ref = d_ref.p, o.l_seq = d_lseq.p, o.reflen = d_reflen.p;
    c->hip(launch_split_cols(o, d_raw.p, d_roff.p, keep ? d_keep.p : nullptr, n, nref, d_rlen.p, d_rbkt.p,
                             minimal_region_overlap, max_softclip_5_end, max_softclip_3_end, d_cls.p, d_bkt.p,
                             d_outlen.p, c->st),
           "split cols");
    std::vector<int8_t> cls(n);
    std::vector<int32_t> bkt(n);
    std::vector<int64_t> olen(n);
    if (n) {
      c->hip(hipMemcpyAsync(cls.data(), d_cls.p, (size_t)n, hipMemcpyDeviceToHost, c->st), "d2h");
      c->hip(hipMemcpyAsync(bkt.data(), d_bkt.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->st), "d2h");
      c->hip(hipMemcpyAsync(olen.data(), d_outlen.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->st), "d2h");
    }
    c->hip(hipStreamSynchronize(c->st), "sync");
    // the reference raises KeyError at the first primary record whose region is unknown, after the records before it
    int64_t stop = n;
    for (int64_t r = 0; r < n && stop == n; r++)
      if (cls[r] == kBamNoRegion || cls[r] == kBamNoCluster) stop = r;
    // k_bam_emit indexes the name, the CIGAR and the sequence of a kept record by its own fields.  Kept records are
    // primary, and the open has refused every primary record whose l_seq is negative or whose fields overrun its
    // block_size, so no second field check is made here; what the open does not look at is an empty name field.
    for (int64_t r = 0; r < stop; r++)
      if (cls[r] == kBamKept && S.raw[(size_t)S.roff[r] + 12] == 0)
        c->fail(UMICLUST_EFORMAT, "BAM record %lld: l_read_name 0", (long long)r);
    const auto bucket_path = [&](int32_t b) { return std::string(bucket_paths[b]); };
    std::vector<int32_t> used;
    if (!umi)
      used = emit_fasta(c, d_raw.p, d_roff.p, d_cls.p, d_pos, cls, bkt, olen, stop, bucket_path);
    else if (stop == n)
      used = emit_umis(c, S.raw, S.roff, d_raw.p, d_roff.p, d_cls.p, d_pos, cls, bkt, stop, *umi, pat, bucket_path,
                       umis_per_bucket, nbuckets);
    // counters of the records the reference reached
    int64_t cnt[4] = {0, 0, 0, 0};  // unmapped, primary mapped, short, long
    if (nbuckets) memset(reads_per_bucket, 0, sizeof(int64_t) * (size_t)nbuckets);
    if (region_detected && nregions) memset(region_detected, 0, (size_t)nregions);
    const int64_t last = stop < n ? stop + 1 : n;  // the failing record counts as a primary alignment too
    for (int64_t r = 0; r < last; r++) {
      const int8_t k = cls[r];
      if (k == kBamUnmapped) cnt[0]++;
      if (k >= kBamShort && k != kBamAbsent) cnt[1]++;
      if (k == kBamShort) cnt[2]++;
      if (k == kBamLong) cnt[3]++;
      if (k == kBamKept && r < stop) {
        reads_per_bucket[bkt[r]]++;
        if (region_detected) region_detected[rreg[S.ref[r]]] = 1;
      }
    }
    for (int x = 0; x < 4; x++) counts[x] = cnt[x];
    if (stop < n) {
      const int32_t ref = S.ref[stop];
      const std::string nm = ref >= 0 && ref < nref ? S.hdr.ref_name[ref] : std::string("None");
      if (missing_name && missing_cap > 0) snprintf(missing_name, (size_t)missing_cap, "%s", nm.c_str());
      c->fail(UMICLUST_EFORMAT, "KeyError: '%s'", nm.c_str());
    }
    return (int64_t)used.size();
  });
}
}  // namespace

int64_t umiclust_bam_split(umiclust_ctx* ctx, const uint8_t* keep, int32_t nregions, const char* const* region_names,
                           const int64_t* region_lengths, const int32_t* region_buckets, int32_t nbuckets,
                           const char* const* bucket_paths, double minimal_region_overlap, int32_t max_softclip_5_end,
                           int32_t max_softclip_3_end, int64_t* counts, int64_t* reads_per_bucket,
                           uint8_t* region_detected, char* missing_name, int32_t missing_cap) {
  return bam_split_impl(ctx, keep, nregions, region_names, region_lengths, region_buckets, nbuckets, bucket_paths,
                        minimal_region_overlap, max_softclip_5_end, max_softclip_3_end, nullptr, counts,
                        reads_per_bucket, nullptr, region_detected, missing_name, missing_cap);
}

int64_t umiclust_bam_split_extract(umiclust_ctx* ctx, const uint8_t* keep, int32_t nregions,
                                   const char* const* region_names, const int64_t* region_lengths,
                                   const int32_t* region_buckets, int32_t nbuckets, const char* const* bucket_umi_paths,
                                   double minimal_region_overlap, int32_t max_softclip_5_end, int32_t max_softclip_3_end,
                                   int32_t adapter_length_5_end, int32_t adapter_length_3_end, int32_t max_pattern_dist,
                                   const char* umi_fwd, const char* umi_rev, int64_t* counts, int64_t* reads_per_bucket,
                                   int64_t* umis_per_bucket, uint8_t* region_detected, char* missing_name,
                                   int32_t missing_cap) {
  const UmiArgs umi{adapter_length_5_end, adapter_length_3_end, max_pattern_dist, umi_fwd, umi_rev};
  return bam_split_impl(ctx, keep, nregions, region_names, region_lengths, region_buckets, nbuckets, bucket_umi_paths,
                        minimal_region_overlap, max_softclip_5_end, max_softclip_3_end, &umi, counts, reads_per_bucket,
                        umis_per_bucket, region_detected, missing_name, missing_cap);
}

int32_t umiclust_bam_name_suffix(umiclust_ctx* ctx, int64_t* value, uint8_t* status) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    auto& S = *bam_session(c);
    const int64_t n = (int64_t)S.roff.size();
    if (!n) return UMICLUST_OK;
    DevBuf<uint8_t> d_raw, d_status;
    DevBuf<int64_t> d_roff, d_value;
    c->hip(d_raw.ensure(S.raw.size() + 1), "alloc");
    alloc_each(c, (size_t)n, d_roff, d_value, d_status);
    c->hip(hipMemcpyAsync(d_raw.p, S.raw.data(), S.raw.size(), hipMemcpyHostToDevice, c->st), "h2d");
    c->hip(hipMemcpyAsync(d_roff.p, S.roff.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->st), "h2d");
    c->hip(launch_name_suffix(d_raw.p, d_roff.p, n, d_value.p, d_status.p, c->st), "name suffix");
    if (value) c->hip(hipMemcpyAsync(value, d_value.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->st), "d2h");
    if (status) c->hip(hipMemcpyAsync(status, d_status.p, (size_t)n, hipMemcpyDeviceToHost, c->st), "d2h");
    c->hip(hipStreamSynchronize(c->st), "sync");
    return UMICLUST_OK;
  });
}

int32_t umiclust_bam_close(umiclust_ctx* ctx) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    (void)bam_session(c);
    c->bs = BamSession();
    return UMICLUST_OK;
  });
}
