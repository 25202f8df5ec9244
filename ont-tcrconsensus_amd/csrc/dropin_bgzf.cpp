// dropin_bgzf.cpp -- BGZF on the device for the BAM drop-ins: the blocks of a file inflated (bgzf.hip on
// inflate.h), which is how both BAM readers start (read_bam_on_device) and what umiclust_bgzf_inflate runs alone; and
// the session's writer, which deflates its blocks there (bgzf.hip on deflate.h: write_bgzf_device),
// which umiclust_bgzf_deflate runs alone.  The HIP-free halves are in bam_host.h and host_io.h.
#include <errno.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstring>
#include <thread>

#include "bam_dev.h"
#include "deflate.h"
#include "inflate.h"

using namespace uc;
using namespace uc::io;

namespace {
// ---- BGZF blocks inflated on the device (bgzf.hip)
// The block table of a BGZF byte string: the blocks with ISIZE > 0 (the others are not launched), their index among
// all blocks, and the inflated size.
struct BgzfPlan {
  std::vector<BgzfBlock> blk;
  std::vector<int64_t> file_idx;
  BlockTable table;  // every block, the empty ones too
  int64_t n_blocks = 0, total = 0;
};
bool bgzf_plan(const uint8_t* d, size_t N, BgzfPlan& P) {
  std::vector<size_t> boff, bsz;
  std::vector<uint32_t> isz;
  if (!io::bgzf_blocks(d, N, boff, bsz, isz)) return false;
  P.n_blocks = (int64_t)boff.size();
  for (size_t b = 0; b < boff.size(); b++) {
    const size_t xlen = (size_t)d[boff[b] + 10] | ((size_t)d[boff[b] + 11] << 8);
    P.table.coff.push_back((int64_t)boff[b]), P.table.ustart.push_back(P.total);
    if (isz[b]) {
      P.blk.push_back({(int64_t)(boff[b] + 12 + xlen), P.total, (uint32_t)(bsz[b] - 12 - xlen - 8), isz[b]});
      P.file_idx.push_back((int64_t)b);
    }
    P.total += isz[b];
  }
  if (isz.empty() || isz.back()) P.table.coff.push_back((int64_t)N), P.table.ustart.push_back(P.total);  // no EOF block
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
  c->h2d(d_comp.p, d, N), c->h2d(d_blk.p, P.blk.data(), nb * sizeof(BgzfBlock));
  c->hip(hipEventRecord(e[1].get(c), c->st), "event");
  c->hip(launch_bgzf_inflate(d_comp.p, (int64_t)padded, d_blk.p, (int64_t)nb, d_raw.p, d_st.p, c->st), "bgzf inflate");
  c->hip(hipEventRecord(e[2].get(c), c->st), "event");
  c->d2h(status.data(), d_st.p, nb * 4);
  uint8_t* const host_out = host_dst();
  if (host_out) c->d2h(host_out, d_raw.p, (size_t)P.total);
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
  c->h2d(D.d_in.p, in, in_bytes), c->h2d(D.d_blk.p, D.blk.data(), nb * sizeof(DeflateBlock));
  c->h2d(D.d_crc.p, crc, nb * 4);
  c->hip(hipEventRecord(D.e[1], c->st), "event");
  c->hip(launch_bgzf_deflate(D.d_in.p, D.d_blk.p, (int64_t)nb, D.d_slots.p, D.d_tok.p, D.d_meta.p, D.d_fsize.p, c->st),
         "bgzf deflate");
  c->hip(launch_scan_i64(D.d_fsize.p, D.d_foff.p, (int64_t)nb, 0, D.d_foff.p + nb, c->st), "scan");
  c->hip(launch_bgzf_frame(D.d_slots.p, D.d_blk.p, D.d_meta.p, D.d_foff.p, D.d_crc.p, (int64_t)nb, D.d_out.p, c->st),
         "bgzf frame");
  c->hip(hipEventRecord(D.e[2], c->st), "event");
  c->d2h(D.meta.data(), D.d_meta.p, 4 * nb * 4), c->d2h(D.foff.data(), D.d_foff.p, (nb + 1) * 8);
  c->hip(hipStreamSynchronize(c->st), "sync");
  const size_t total = (size_t)D.foff[nb];
  if (total > nb * kFramedMax) c->fail(UMICLUST_EDEVICE, "bgzf deflate: %zu framed bytes from %zu blocks", total, nb);
  c->d2h(out, D.d_out.p, total);
  c->hip(hipEventRecord(D.e[3], c->st), "event");
  c->hip(hipStreamSynchronize(c->st), "sync");
  if (times)
    for (int x = 0; x < 3; x++) times[x] += elapsed_s(c, D.e[x], D.e[x + 1]);
  return total;
}
}  // namespace

// umiclust_bam_write on the device: the stream cut into batches of c->tun.bgzf_batch blocks; while the device deflates
// batch k and its bytes are written, the I/O threads gather batch k + 1 into the other staging slot and compute its
// CRC32s.  A block with a status is redone by zlib in place.  Returns the records written, -1 + err on an I/O
// failure, -2 where device or pinned memory could not be had (nothing has been written: the caller takes the host
// writer).
int64_t uc::write_bgzf_device(Ctx* c, BamSession& S, const uint8_t* keep, const char* path, std::string& err) {
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
  S.write_coff.assign(nb + 1, 0);
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
      for (size_t b = 0; b < n; b++) S.write_coff[b0 + b] = (int64_t)bytes + D.foff[b];
      ok = bam::write_fd(fd, out.p, total);
      bytes += total;
      continue;
    }
    for (size_t b = 0; b < n && ok; b++) {  // block by block: a refused block by zlib, in its place
      S.write_coff[b0 + b] = (int64_t)bytes;
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
  S.write_coff[nb] = (int64_t)bytes;
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
uint8_t* uc::alloc_touched(RawBuf& raw, size_t bytes) {
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

uc::InputBytes::~InputBytes() {
  if (map) munmap(map, map_n);
}
bool uc::InputBytes::read(const char* path, bool regular_only) {
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
  if (regular_only) return close(fd), false;
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

// The file mapped and its block table built, the compressed bytes uploaded, the blocks inflated into d_raw, and `raw`
// copied back to the host, where the header parser, record_offsets, the session and the writer read it.  False for
// what io::inflate_bgzf returned false for, and for a path that is no regular file.
bool uc::read_bam_on_device(Ctx* c, const char* path, RawBuf& raw, DevBuf<uint8_t>& d_raw, int64_t info[3],
                            double* t_upload, BlockTable* table) {
  InputBytes in;
  BgzfPlan P;
  if (!in.read(path, true) || !bgzf_plan(in.p, in.n, P)) return false;
  std::vector<int32_t> status;
  double t[3] = {0, 0, 0};
  // while the device inflates: the host's array, its pages touched by the I/O threads
  const auto host_dst = [&]() { return alloc_touched(raw, (size_t)P.total); };
  bgzf_inflate_device(c, in.p, in.n, P, d_raw, status, host_dst, t);
  info[0] = P.n_blocks, info[1] = (int64_t)P.blk.size(), info[2] = (int64_t)in.n;
  if (t_upload) *t_upload = t[0];
  if (table) *table = std::move(P.table);
  for (int32_t s : status)
    if (s) return false;
  return true;
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
