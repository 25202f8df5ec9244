// dropin_fastq.cpp -- quality filtering (row f5): fastq_filter.h's device Backend and its entry points.
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "fastq_filter.h"

using namespace uc;
using uc::io::io_threads;

namespace {
// The device behind fq::run_filter: a chunk's gathered qualities and offsets go up in two copies, k_fastq_ee runs,
// the per-record sums and byte ranges come back.  In stats mode (row f5b) the gathered sequence bytes go up in a third
// copy, k_fastq_stats runs in k_fastq_ee's place and the five counts per record come back as well.  reserve() runs on
// the parsing thread, run() / run_stats() on the caller's.
struct FqDevice : fq::Backend {
  Ctx* c;
  explicit FqDevice(Ctx* ctx) : c(ctx) {}
  template <typename B>
  static bool grow(B& b, size_t count) {  // with slack: chunks differ by a few records
    return (b.p && count <= b.n) || b.ensure(count + count / 8 + 64) == hipSuccess;
  }
  bool reserve(int slot, size_t qual_bytes, size_t nrec, bool stats, fq::Slot& s, std::string& err) override {
    FqState::Slot& h = c->fq.slot[slot];
    if (hipSetDevice(c->dev) != hipSuccess || !grow(h.q, qual_bytes + 2 * fq::kPad) || !grow(h.offs, nrec + 1) ||
        !grow(h.ee, nrec + 1) || !grow(h.lo, nrec + 1) || !grow(h.hi, nrec + 1) ||
        (stats && !(grow(h.seq, qual_bytes + 2 * fq::kPad) && grow(h.cnt, fq::kCounts * (nrec + 1))))) {
      (void)hipGetLastError();
      err = "cannot allocate the pinned staging buffers";
      return false;
    }
    s = fq::Slot{h.q.p, h.offs.p, h.ee.p, h.lo.p, h.hi.p};
    if (stats) s.seq = h.seq.p, s.cnt = h.cnt.p;
    return true;
  }
  bool run(int slot, size_t qual_bytes, int64_t nrec, const uint64_t* table, double* t_h2d_s, double* t_kernel_s,
           std::string& err) override {
    return go(slot, qual_bytes, nrec, table, false, 0, t_h2d_s, t_kernel_s, err);
  }
  bool run_stats(int slot, size_t qual_bytes, int64_t nrec, const uint64_t* table, int ascii, double* t_h2d_s,
                 double* t_kernel_s, std::string& err) override {
    return go(slot, qual_bytes, nrec, table, true, ascii, t_h2d_s, t_kernel_s, err);
  }
  bool go(int slot, size_t qual_bytes, int64_t nrec, const uint64_t* table, bool stats, int ascii, double* t_h2d_s,
          double* t_kernel_s, std::string& err) {
    FqState::Slot& h = c->fq.slot[slot];
    const size_t n = (size_t)nrec;
    hipError_t e = hipSuccess;
    auto ok = [&](hipError_t x) { return e == hipSuccess && (e = x) == hipSuccess; };
    for (uc::Event& ev : c->fq.ev) ok(ev.create());
    if (e == hipSuccess && !(grow(c->fq.dq, qual_bytes + 2 * fq::kPad) && grow(c->fq.doffs, n + 1) &&
                             grow(c->fq.dee, n + 1) && grow(c->fq.dlo, n + 1) && grow(c->fq.dhi, n + 1) &&
                             grow(c->fq.dtab, 256) &&
                             (!stats || (grow(c->fq.dseq, qual_bytes + 2 * fq::kPad) &&
                                         grow(c->fq.dcnt, fq::kCounts * (n + 1))))))
      e = hipErrorOutOfMemory;
    hipStream_t st = c->st;
    ok(hipMemcpyAsync(c->fq.dtab.p, table, 256 * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    ok(hipEventRecord(c->fq.ev[0], st));
    ok(hipMemcpyAsync(c->fq.dq.p, h.q.p, qual_bytes + 2 * fq::kPad, hipMemcpyHostToDevice, st));
    if (stats) ok(hipMemcpyAsync(c->fq.dseq.p, h.seq.p, qual_bytes + 2 * fq::kPad, hipMemcpyHostToDevice, st));
    ok(hipMemcpyAsync(c->fq.doffs.p, h.offs.p, (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    ok(hipEventRecord(c->fq.ev[1], st));
    if (e == hipSuccess && stats)
      ok(launch_fastq_stats(c->fq.dq.p + fq::kPad, c->fq.dseq.p + fq::kPad, c->fq.doffs.p, nrec, c->fq.dtab.p, ascii,
                            c->fq.dee.p, c->fq.dlo.p, c->fq.dhi.p, c->fq.dcnt.p, st));
    else if (e == hipSuccess)
      ok(launch_fastq_ee(c->fq.dq.p + fq::kPad, c->fq.doffs.p, nrec, c->fq.dtab.p, c->fq.dee.p, c->fq.dlo.p,
                         c->fq.dhi.p, st));
    ok(hipEventRecord(c->fq.ev[2], st));
    ok(hipMemcpyAsync(h.ee.p, c->fq.dee.p, n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ok(hipMemcpyAsync(h.lo.p, c->fq.dlo.p, n, hipMemcpyDeviceToHost, st));
    ok(hipMemcpyAsync(h.hi.p, c->fq.dhi.p, n, hipMemcpyDeviceToHost, st));
    if (stats) ok(hipMemcpyAsync(h.cnt.p, c->fq.dcnt.p, fq::kCounts * n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    ok(hipStreamSynchronize(st));
    float ms0 = 0.f, ms1 = 0.f;
    ok(hipEventElapsedTime(&ms0, c->fq.ev[0], c->fq.ev[1]));
    ok(hipEventElapsedTime(&ms1, c->fq.ev[1], c->fq.ev[2]));
    if (e != hipSuccess) {
      err = std::string("fastq_filter device step: ") + hipGetErrorString(e);
      return false;
    }
    *t_h2d_s = ms0 * 1e-3;
    *t_kernel_s = ms1 * 1e-3;
    return true;
  }
};

int64_t fastq_filter_impl(Ctx* c, const umiclust_fastq_filter_params* p, const char* in_fastq,
                          const char* fastqout, const char* fastqout_discarded, const char* log_path,
                          umiclust_fastq_filter_result* result, const fq::StatsReq* stats = nullptr) {
  if (!p || !in_fastq) c->fail(UMICLUST_EINVAL, "null params or input path");
  FqDevice dev(c);
  fq::Paths paths;
  paths.in = in_fastq;
  paths.out = fastqout;
  paths.discarded = fastqout_discarded;
  paths.log = log_path;
  std::string err;
  const int64_t rc = fq::run_filter(*p, paths, io_threads(), c->tun.fq_chunk, dev, result, err, stats);
  if (rc < 0) c->fail((int)rc, "%s", err.c_str());
  return rc;
}

}  // namespace

int64_t umiclust_fastq_filter(umiclust_ctx* ctx, const umiclust_fastq_filter_params* p, const char* in_fastq,
                              const char* fastqout, const char* fastqout_discarded, const char* log_path,
                              umiclust_fastq_filter_result* result) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, { return fastq_filter_impl(c, p, in_fastq, fastqout, fastqout_discarded, log_path, result); });
}

int64_t umiclust_fastq_filter_argv(umiclust_ctx* ctx, int32_t argc, const char* const* argv,
                                   umiclust_fastq_filter_result* result) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    umiclust_fastq_filter_params p;
    std::vector<char> in(4096), out(4096), dis(4096), lg(4096);
    const int32_t rc =
        umiclust_fastq_filter_params_from_argv(&p, argc, argv, in.data(), out.data(), dis.data(), lg.data(), 4096);
    if (rc != UMICLUST_OK) c->fail(rc, "cannot parse the vsearch --fastq_filter argv");
    return fastq_filter_impl(c, &p, in.data(), out[0] ? out.data() : nullptr, dis[0] ? dis.data() : nullptr,
                             lg[0] ? lg.data() : nullptr, result);
  });
}

int64_t umiclust_fastq_filter_stats(umiclust_ctx* ctx, const umiclust_fastq_filter_params* p, const char* in_fastq,
                                    const char* fastqout, const char* fastqout_discarded, const char* log_path,
                                    const char* stats_before_txt, const char* stats_after_txt,
                                    umiclust_fastq_filter_result* result, umiclust_fastq_stats* before,
                                    umiclust_fastq_stats* after) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    const fq::StatsReq req{stats_before_txt, stats_after_txt, before, after};
    return fastq_filter_impl(c, p, in_fastq, fastqout, fastqout_discarded, log_path, result, &req);
  });
}

int64_t umiclust_fastq_filter_stats_argv(umiclust_ctx* ctx, int32_t argc, const char* const* argv,
                                         const char* stats_before_txt, const char* stats_after_txt,
                                         umiclust_fastq_filter_result* result, umiclust_fastq_stats* before,
                                         umiclust_fastq_stats* after) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    umiclust_fastq_filter_params p;
    std::vector<char> in(4096), out(4096), dis(4096), lg(4096);
    const int32_t rc =
        umiclust_fastq_filter_params_from_argv(&p, argc, argv, in.data(), out.data(), dis.data(), lg.data(), 4096);
    if (rc != UMICLUST_OK) c->fail(rc, "cannot parse the vsearch --fastq_filter argv");
    const fq::StatsReq req{stats_before_txt, stats_after_txt, before, after};
    return fastq_filter_impl(c, &p, in.data(), out[0] ? out.data() : nullptr, dis[0] ? dis.data() : nullptr,
                             lg[0] ? lg.data() : nullptr, result, &req);
  });
}

int32_t umiclust_fastq_ee(umiclust_ctx* ctx, const uint8_t* quals, const int64_t* offsets, int64_t n,
                          int32_t fastq_ascii, int64_t* ee_fx, uint8_t* qlo, uint8_t* qhi) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    if (n < 0 || (n > 0 && (!quals || !offsets || !ee_fx || !qlo || !qhi)) || (fastq_ascii != 33 && fastq_ascii != 64))
      c->fail(UMICLUST_EINVAL, "bad argument");
    if (n == 0) return UMICLUST_OK;
    for (int64_t i = 0; i < n; i++) {
      const int64_t len = offsets[i + 1] - offsets[i];
      if (len < 0) c->fail(UMICLUST_EINVAL, "offsets decrease at record %lld", (long long)i);
      if (len > fq::kDevMaxLen) c->fail(UMICLUST_ERANGE, "record %lld is longer than 2^22 bytes", (long long)i);
    }
    fq::Tables tab;
    fq::build_tables(fastq_ascii, 0, 93, tab);
    FqDevice dev(c);
    fq::Slot s;
    std::string err;
    const size_t bytes = (size_t)(offsets[n] - offsets[0]);
    if (!dev.reserve(0, bytes, (size_t)n, false, s, err)) c->fail(UMICLUST_ENOMEM, "%s", err.c_str());
    memset(s.qual, 0, (size_t)fq::kPad);
    memcpy(s.qual + fq::kPad, quals + offsets[0], bytes);
    memset(s.qual + fq::kPad + bytes, 0, (size_t)fq::kPad);
    for (int64_t i = 0; i <= n; i++) s.offs[i] = offsets[i] - offsets[0];
    double t0, t1;
    if (!dev.run(0, bytes, n, tab.fx, &t0, &t1, err)) c->fail(UMICLUST_EDEVICE, "%s", err.c_str());
    memcpy(ee_fx, s.ee, (size_t)n * sizeof(int64_t));
    memcpy(qlo, s.qlo, (size_t)n);
    memcpy(qhi, s.qhi, (size_t)n);
    return UMICLUST_OK;
  });
}

int32_t umiclust_fastq_record_stats(umiclust_ctx* ctx, const uint8_t* seqs, const uint8_t* quals,
                                    const int64_t* offsets, int64_t n, int32_t fastq_ascii, int64_t* ee_fx, uint8_t* qlo, uint8_t* qhi,
                                    uint32_t* counts) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    if (n < 0 || (n > 0 && (!seqs || !quals || !offsets || !ee_fx || !qlo || !qhi || !counts)) ||
        (fastq_ascii != 33 && fastq_ascii != 64))
      c->fail(UMICLUST_EINVAL, "bad argument");
    if (n == 0) return UMICLUST_OK;
    for (int64_t i = 0; i < n; i++) {
      const int64_t len = offsets[i + 1] - offsets[i];
      if (len < 0) c->fail(UMICLUST_EINVAL, "offsets decrease at record %lld", (long long)i);
      if (len > fq::kDevMaxLen) c->fail(UMICLUST_ERANGE, "record %lld is longer than 2^22 bytes", (long long)i);
    }
    fq::Tables tab;
    fq::build_tables(fastq_ascii, 0, 93, tab);
    FqDevice dev(c);
    fq::Slot s;
    std::string err;
    const size_t bytes = (size_t)(offsets[n] - offsets[0]);
    if (!dev.reserve(0, bytes, (size_t)n, true, s, err)) c->fail(UMICLUST_ENOMEM, "%s", err.c_str());
    uint8_t* dst[2] = {s.qual, s.seq};
    const uint8_t* src[2] = {quals, seqs};
    for (int k = 0; k < 2; k++) {
      memset(dst[k], 0, (size_t)fq::kPad);
      memcpy(dst[k] + fq::kPad, src[k] + offsets[0], bytes);
      memset(dst[k] + fq::kPad + bytes, 0, (size_t)fq::kPad);
    }
    for (int64_t i = 0; i <= n; i++) s.offs[i] = offsets[i] - offsets[0];
    double t0, t1;
    if (!dev.run_stats(0, bytes, n, tab.fx, fastq_ascii, &t0, &t1, err)) c->fail(UMICLUST_EDEVICE, "%s", err.c_str());
    memcpy(ee_fx, s.ee, (size_t)n * sizeof(int64_t));
    memcpy(qlo, s.qlo, (size_t)n);
    memcpy(qhi, s.qhi, (size_t)n);
    memcpy(counts, s.cnt, (size_t)n * fq::kCounts * sizeof(uint32_t));
    return UMICLUST_OK;
  });
}
