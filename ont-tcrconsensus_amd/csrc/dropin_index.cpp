// dropin_index.cpp -- the .bai index and flagstat of the BAM session (bamindex.hip on bam_index.h):
// umiclust_bam_write_index (the write, then the index of exactly that file), umiclust_bam_index_file (`samtools index`
// of a file, beside an open session), umiclust_bam_flagstat, the kernel-level umiclust_bam_index_probe and the
// diagnostic umiclust_bam_index_info.  The kernels leave the sorted runs, the linear arrays and the counters; the
// finish over the runs and the file's bytes are bam_index.h's host code.
#include <unistd.h>

#include <algorithm>
#include <cstring>

#include "bam_dev.h"
#include "bam_index.h"

using namespace uc;
using namespace uc::io;

namespace {

// The records an index call works on: a session's, or those of a file read for the call.
struct Records {
  const RawBuf& raw;
  const std::vector<int64_t>& roff;
  int64_t header_end;
  int32_t nref;
};

// bai::build_host on the device: d_raw and d_roff hold R's bytes and offsets.  keep: host memory, may be null.  An
// empty block table (nblocks = 0) stops after the keys: counters, per-reference counts and statuses.  cols: the
// per-record arrays and the runs in file order are copied back too (the probe).  A refused record (K.first_bad) stops
// before the sort.  times[0..2] += seconds of the uploads made here, the kernels, the copies back.
void index_on_device(Ctx* c, const Records& R, const uint8_t* d_raw, const int64_t* d_roff, const uint8_t* keep,
                     const int64_t* coff, const int64_t* ustart, int64_t nblocks, bool cols, bai::Keys& K,
                     double* times) {
  const int64_t n = (int64_t)R.roff.size();
  const int32_t nref = R.nref;
  const size_t N = (size_t)n + 1, NR = (size_t)nref + 1;
  K = bai::Keys();
  DevBuf<uint8_t> d_keep;
  DevBuf<int64_t> d_table, d_scratch, d_head, d_hx, d_small, d_base, d_hist;
  DevBuf<uint32_t> d_rec, d_idx, d_idx2;
  DevBuf<int32_t> d_i32;
  DevBuf<uint64_t> d_u, d_v, d_acc, d_key, d_key2, d_win;
  DevBuf<bai::Run> d_runs, d_sorted;
  Event e[7];  // upload, first kernels, first copy back | second kernels, second copy back
  alloc_each(c, N, d_keep, d_rec, d_u, d_v);
  if (nblocks) alloc_each(c, N, d_head, d_hx, d_key, d_key2, d_idx, d_idx2, d_runs, d_sorted);  // the runs and their sort
  alloc_each(c, 4 * N, d_scratch);
  alloc_each(c, 6 * N, d_i32);
  alloc_each(c, 2 * (size_t)nblocks + 1, d_table);
  alloc_each(c, 8, d_small);
  alloc_each(c, NR, d_base);
  // the accumulators: first_bad, n_no_coor, the 32 counters, then mapped, unmapped, n_intv per reference
  const size_t acc_n = 34 + 3 * NR;
  alloc_each(c, acc_n, d_acc);
  std::vector<uint64_t> acc(acc_n, 0);
  acc[0] = ~0ull;
  c->hip(hipEventRecord(e[0].get(c), c->st), "event");
  if (keep) c->h2d(d_keep.p, keep, (size_t)n);
  c->h2d(d_table.p, coff, (size_t)nblocks * 8), c->h2d(d_table.p + nblocks, ustart, (size_t)nblocks * 8);
  c->h2d(d_acc.p, acc.data(), acc_n * 8);
  c->hip(hipEventRecord(e[1].get(c), c->st), "event");
  const BaiIn I{d_raw, d_roff, keep ? d_keep.p : nullptr, n, R.header_end, d_table.p, d_table.p + nblocks, nblocks, nref};
  int32_t* const i32 = d_i32.p;
  const BaiCols o{d_rec.p, i32, i32 + N, i32 + 2 * N, i32 + 3 * N, i32 + 4 * N, i32 + 5 * N, d_u.p, d_v.p};
  uint64_t* const a = d_acc.p;
  const BaiAcc A{a, a + 2, a + 34, a + 34 + NR, a + 34 + 2 * NR, a + 1};
  int64_t* const d_nk = d_small.p;  // [0] kept records, [1] runs, [2] windows
  c->hip(launch_bai_keys(I, d_scratch.p, d_nk, o, A, c->st), "bai keys");
  c->hip(launch_scan_i64((const int64_t*)A.n_intv, d_base.p, nref, 0, d_nk + 2, c->st), "scan");
  if (nblocks) c->hip(launch_bai_runs(o, n, d_nk, d_head.p, d_hx.p, d_nk + 1, A.first_bad, d_runs.p, d_key.p, c->st), "bai runs");
  else c->hip(hipMemsetAsync(d_nk + 1, 0, 8, c->st), "memset");
  c->hip(hipEventRecord(e[2].get(c), c->st), "event");
  int64_t small[3] = {0, 0, 0};
  c->d2h(small, d_small.p, sizeof small), c->d2h(acc.data(), d_acc.p, acc_n * 8);
  c->hip(hipEventRecord(e[3].get(c), c->st), "event");
  c->hip(hipStreamSynchronize(c->st), "sync");
  const int64_t nk = small[0], nruns = small[1], nwin = small[2];
  K.nkept = nk, K.n_no_coor = (int64_t)acc[1];
  for (int k = 0; k < bai::kCounters; k++) K.counters[k] = (int64_t)acc[2 + k];
  K.mapped.assign(acc.begin() + 34, acc.begin() + 34 + nref);
  K.unmapped.assign(acc.begin() + 34 + NR, acc.begin() + 34 + NR + nref);
  K.n_intv.assign(acc.begin() + 34 + 2 * NR, acc.begin() + 34 + 2 * NR + nref);
  K.base.assign(NR, 0);
  for (int32_t t = 0; t < nref; t++) K.base[(size_t)t + 1] = K.base[(size_t)t] + K.n_intv[(size_t)t];
  if (acc[0] != ~0ull) K.first_bad = (int64_t)(acc[0] >> 2), K.first_status = (int32_t)(acc[0] & 3);
  if (nk < 0 || nk > n || nruns < 0 || nruns > nk || nwin != K.base[(size_t)nref])
    c->fail(UMICLUST_EDEVICE, "bam index: %lld kept records, %lld runs, %lld windows from the device", (long long)nk,
            (long long)nruns, (long long)nwin);
  const bool rest = nblocks && K.first_bad < 0;
  if (rest) {
    c->hip(d_win.ensure((size_t)nwin + 1), "alloc");
    c->hip(d_hist.ensure(256 * (size_t)((nruns + 255) / 256) + 1), "alloc");
    c->hip(hipEventRecord(e[4].get(c), c->st), "event");
    const uint32_t* d_order = d_idx.p;
    // the sort skips a digit that no key has a bit in, and wants the OR of the keys: every bit a tid below nref or a
    // bin can have is a superset of it (the largest tid is no mask: 256 has no bit where 1 .. 255 differ)
    uint64_t tid_bits = 0;
    while (tid_bits < (uint64_t)std::max(nref - 1, 0)) tid_bits = (tid_bits << 1) | 1;
    const uint64_t key_bits = (tid_bits << 16) | 0xffffull;
    // (the sort scatters the keys it is given: the runs keep their own copy in d_runs)
    c->hip(launch_sam_sort(d_key.p, d_idx.p, d_key2.p, d_idx2.p, nruns, key_bits, d_hist.p, &d_order, c->st), "bai sort");
    c->hip(launch_bai_gather(d_runs.p, d_order, nruns, d_sorted.p, c->st), "bai gather");
    c->hip(launch_bai_linear(o, n, d_nk, d_base.p, A.n_intv, nref, d_win.p, nwin, c->st), "bai linear");
    c->hip(hipEventRecord(e[5].get(c), c->st), "event");
    K.sorted.resize((size_t)nruns), K.linear.resize((size_t)nwin);
    c->d2h(K.sorted.data(), d_sorted.p, (size_t)nruns * sizeof(bai::Run)), c->d2h(K.linear.data(), d_win.p, (size_t)nwin * 8);
    if (cols) {
      K.runs.resize((size_t)nruns);
      c->d2h(K.runs.data(), d_runs.p, (size_t)nruns * sizeof(bai::Run));
    }
    c->hip(hipEventRecord(e[6].get(c), c->st), "event");
    c->hip(hipStreamSynchronize(c->st), "sync");
  }
  if (cols) {
    const size_t k = (size_t)nk;
    K.tid.resize(k), K.bin.resize(k), K.w0.resize(k), K.w1.resize(k), K.status.resize(k), K.u.resize(k), K.v.resize(k);
    c->d2h(K.tid.data(), o.tid, k * 4), c->d2h(K.bin.data(), o.bin, k * 4), c->d2h(K.w0.data(), o.w0, k * 4);
    c->d2h(K.w1.data(), o.w1, k * 4), c->d2h(K.status.data(), o.status, k * 4);
    c->d2h(K.u.data(), o.u, k * 8), c->d2h(K.v.data(), o.v, k * 8);
    c->hip(hipStreamSynchronize(c->st), "sync");
  }
  if (times) {
    times[0] += elapsed_s(c, e[0], e[1]);
    times[1] += elapsed_s(c, e[1], e[2]) + (rest ? elapsed_s(c, e[4], e[5]) : 0.0);
    times[2] += elapsed_s(c, e[2], e[3]) + (rest ? elapsed_s(c, e[5], e[6]) : 0.0);
  }
}

// the error of a refused record, named
void fail_refused(Ctx* c, const Records& R, const bai::Keys& K, const char* what) {
  const std::string name(record_name(R.raw, R.roff, K.first_bad));
  const bai::Rec rec = bai::read_record(R.raw.data() + R.roff[(size_t)K.first_bad]);
  if (K.first_status == bai::kUnsorted)
    c->fail(UMICLUST_EFORMAT, "%s: unsorted: record %lld (%s) at reference %d position %lld comes after a later one",
            what, (long long)K.first_bad, name.c_str(), rec.tid, (long long)rec.beg);
  if (K.first_status == bai::kRange)
    c->fail(UMICLUST_ERANGE, "%s: record %lld (%s) spans [%lld, %lld): a .bai index holds 0 .. 2^29", what,
            (long long)K.first_bad, name.c_str(), (long long)rec.beg, (long long)rec.end);
  c->fail(UMICLUST_EFORMAT, "%s: record %lld (%s) names reference %d of %d", what, (long long)K.first_bad, name.c_str(),
          rec.tid, R.nref);
}

// the finish and the file; the chunks left
int64_t write_bai(Ctx* c, const bai::Keys& K, int32_t nref, const std::string& path) {
  int64_t chunks = 0;
  const std::vector<uint8_t> bytes = bai::serialise(K, nref, &chunks);
  FILE* f = fopen(path.c_str(), "wb");
  const bool ok = f && fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
  if ((f && fclose(f) != 0) || !ok) {
    unlink(path.c_str());
    c->fail(UMICLUST_EIO, "cannot write %s", path.c_str());
  }
  return chunks;
}

void put_info(Ctx* c, const bai::Keys& K, int64_t chunks, const double* times) {
  c->ix.have = true;
  c->ix.out[0] = K.nkept, c->ix.out[1] = (int64_t)K.sorted.size(), c->ix.out[2] = chunks;
  c->ix.out[3] = K.base.empty() ? 0 : K.base.back();
  for (int x = 0; x < 4; x++) c->ix.times[x] = times[x];
}

double upload_timed(Ctx* c, const BamSession& S, DevBuf<uint8_t>& d_raw, DevBuf<int64_t>& d_roff) {
  Event e[2];
  c->hip(hipEventRecord(e[0].get(c), c->st), "event");
  upload_session(c, S, d_raw, d_roff);
  c->hip(hipEventRecord(e[1].get(c), c->st), "event");
  c->hip(hipStreamSynchronize(c->st), "sync");
  return elapsed_s(c, e[0], e[1]);
}

}  // namespace

int64_t umiclust_bam_write_index(umiclust_ctx* ctx, const uint8_t* keep, const char* out_bam, const char* out_bai) {
  uc::Ctx* c = uc::core(ctx);
  if (!c) return UMICLUST_EINVAL;
  const int64_t k = umiclust_bam_write(ctx, keep, out_bam);
  if (k < 0) return k;
  const std::string bai_path = out_bai ? std::string(out_bai) : std::string(out_bam) + ".bai";
  const int64_t rc = [&]() -> int64_t {
    UC_GUARD(c, {
      auto& S = *bam_session(c);
      const Records R{S.raw, S.roff, (int64_t)S.hdr.end, (int32_t)S.hdr.ref_name.size()};
      // the table of the file just written: a block every 0xff00 stream bytes, then the EOF block
      const size_t nb = S.write_coff.size();
      size_t total = S.hdr.end;
      for (size_t r = 0; r < S.roff.size(); r++)
        if (keep[r]) total += 4 + (size_t)bam::block_size(S.raw.data() + S.roff[r]);
      if (nb != (total + bam::kBgzfPayload - 1) / bam::kBgzfPayload + 1)
        c->fail(UMICLUST_ESTATE, "the writer recorded %zu blocks for a stream of %zu bytes", nb, total);
      std::vector<int64_t> ustart(nb);
      for (size_t b = 0; b < nb; b++) ustart[b] = (int64_t)std::min(b * bam::kBgzfPayload, total);
      double times[4] = {0, 0, 0, 0};
      DevBuf<uint8_t> d_raw;
      DevBuf<int64_t> d_roff;
      times[0] = upload_timed(c, S, d_raw, d_roff);
      bai::Keys K;
      index_on_device(c, R, d_raw.p, d_roff.p, S.roff.empty() ? nullptr : keep, S.write_coff.data(), ustart.data(),
                      (int64_t)nb, false, K, times);
      if (K.first_bad >= 0) fail_refused(c, R, K, out_bam);
      const double t0 = now_s();
      const int64_t chunks = write_bai(c, K, R.nref, bai_path);
      times[3] = now_s() - t0;
      put_info(c, K, chunks, times);
      return 0;
    });
  }();
  if (rc < 0) {
    unlink(bai_path.c_str());
    return rc;
  }
  return k;
}

int64_t umiclust_bam_index_file(umiclust_ctx* ctx, const char* bam_file, const char* out_bai) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    if (!bam_file) c->fail(UMICLUST_EINVAL, "null argument");
    const std::string bai_path = out_bai ? std::string(out_bai) : std::string(bam_file) + ".bai";
    RawBuf raw;
    DevBuf<uint8_t> d_raw;
    DevBuf<int64_t> d_roff;
    BlockTable T;
    int64_t info[3];
    double times[4] = {0, 0, 0, 0};
    if (!read_bam_on_device(c, bam_file, raw, d_raw, info, &times[0], &T))
      c->fail(UMICLUST_EIO, "cannot read BGZF/BAM %s", bam_file);
    bam::Header hdr;
    std::vector<int64_t> roff;
    std::string herr;
    if (!bam::parse_header(raw.data(), raw.size(), hdr, herr) || !bam::record_offsets(raw.data(), raw.size(), hdr.end, roff, herr))
      c->fail(UMICLUST_EFORMAT, "%s: %s", bam_file, herr.c_str());
    c->hip(d_roff.ensure(roff.size() + 1), "alloc");
    c->h2d(d_roff.p, roff.data(), roff.size() * 8);
    const Records R{raw, roff, (int64_t)hdr.end, (int32_t)hdr.ref_name.size()};
    bai::Keys K;
    index_on_device(c, R, d_raw.p, d_roff.p, nullptr, T.coff.data(), T.ustart.data(), (int64_t)T.coff.size(), false, K,
                    times);
    if (K.first_bad >= 0) {
      unlink(bai_path.c_str());
      fail_refused(c, R, K, bam_file);
    }
    const double t0 = now_s();
    const int64_t chunks = write_bai(c, K, R.nref, bai_path);
    times[3] = now_s() - t0;
    put_info(c, K, chunks, times);
    return (int64_t)roff.size();
  });
}

int32_t umiclust_bam_flagstat(umiclust_ctx* ctx, const uint8_t* keep, int64_t* out, char* text, int64_t cap) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    auto& S = *bam_session(c);
    if (cap < 0 || (cap > 0 && !text)) c->fail(UMICLUST_EINVAL, "bad argument");
    const Records R{S.raw, S.roff, (int64_t)S.hdr.end, (int32_t)S.hdr.ref_name.size()};
    double times[4] = {0, 0, 0, 0};
    DevBuf<uint8_t> d_raw;
    DevBuf<int64_t> d_roff;
    times[0] = upload_timed(c, S, d_raw, d_roff);
    bai::Keys K;
    index_on_device(c, R, d_raw.p, d_roff.p, keep, nullptr, nullptr, 0, false, K, times);
    put_info(c, K, 0, times);
    if (out) memcpy(out, K.counters, sizeof K.counters);
    const std::string t = bai::flagstat_text(K.counters);
    const int64_t need = (int64_t)t.size() + 1;
    if (need > INT32_MAX) c->fail(UMICLUST_ERANGE, "flagstat text");
    if (cap == 0) return (int32_t)need;
    if (cap < need) c->fail(UMICLUST_ERANGE, "buffer of %lld bytes, %lld needed", (long long)cap, (long long)need);
    memcpy(text, t.c_str(), (size_t)need);
    return (int32_t)need;
  });
}

int32_t umiclust_bam_index_probe(umiclust_ctx* ctx, const uint8_t* keep, const int64_t* coff, const int64_t* ustart,
                                 int64_t nblocks, int32_t* bin, uint64_t* u, uint64_t* v, int32_t* status,
                                 int64_t* runs, int64_t* sorted_runs, int64_t run_cap, int64_t* n_intv,
                                 uint64_t* linear, int64_t linear_cap, int64_t* mapped, int64_t* unmapped,
                                 int64_t* counters, int64_t* info) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    auto& S = *bam_session(c);
    if (nblocks < 1 || !coff || !ustart || run_cap < 0 || linear_cap < 0) c->fail(UMICLUST_EINVAL, "bad argument");
    int64_t total = (int64_t)S.hdr.end;
    for (size_t r = 0; r < S.roff.size(); r++)
      if (!keep || keep[r]) total += 4 + (int64_t)bam::block_size(S.raw.data() + S.roff[r]);
    bool good = ustart[0] == 0 && ustart[nblocks - 1] == total && coff[0] >= 0 && coff[nblocks - 1] < ((int64_t)1 << 47);
    for (int64_t b = 1; b < nblocks && good; b++) good = ustart[b] >= ustart[b - 1] && coff[b] > coff[b - 1] && ustart[b] - ustart[b - 1] <= 0x10000;
    if (!good)
      c->fail(UMICLUST_EINVAL, "the block table does not list increasing blocks of at most 64 KiB over the %lld stream bytes",
              (long long)total);
    const Records R{S.raw, S.roff, (int64_t)S.hdr.end, (int32_t)S.hdr.ref_name.size()};
    double times[4] = {0, 0, 0, 0};
    DevBuf<uint8_t> d_raw;
    DevBuf<int64_t> d_roff;
    times[0] = upload_timed(c, S, d_raw, d_roff);
    bai::Keys K;
    index_on_device(c, R, d_raw.p, d_roff.p, keep, coff, ustart, nblocks, true, K, times);
    const size_t nk = (size_t)K.nkept, nref = (size_t)R.nref, nruns = K.sorted.size(), nwin = K.linear.size();
    if (info) info[0] = K.nkept, info[1] = (int64_t)nruns, info[2] = (int64_t)nwin, info[3] = K.first_bad, info[4] = K.first_status, info[5] = K.n_no_coor;
    if ((int64_t)nruns > run_cap || (int64_t)nwin > linear_cap)
      c->fail(UMICLUST_ERANGE, "%zu runs and %zu windows, room for %lld and %lld", nruns, nwin, (long long)run_cap, (long long)linear_cap);
    if (nk && bin) memcpy(bin, K.bin.data(), nk * 4);
    if (nk && u) memcpy(u, K.u.data(), nk * 8);
    if (nk && v) memcpy(v, K.v.data(), nk * 8);
    if (nk && status) memcpy(status, K.status.data(), nk * 4);
    const auto put_runs = [](const std::vector<bai::Run>& from, int64_t* to) {
      for (size_t x = 0; to && x < from.size(); x++)
        to[4 * x] = from[x].tid, to[4 * x + 1] = from[x].bin, to[4 * x + 2] = (int64_t)from[x].u, to[4 * x + 3] = (int64_t)from[x].v;
    };
    put_runs(K.runs, runs), put_runs(K.sorted, sorted_runs);
    if (nref && n_intv) memcpy(n_intv, K.n_intv.data(), nref * 8);
    if (nref && mapped) memcpy(mapped, K.mapped.data(), nref * 8);
    if (nref && unmapped) memcpy(unmapped, K.unmapped.data(), nref * 8);
    if (nwin && linear) memcpy(linear, K.linear.data(), nwin * 8);
    if (counters) memcpy(counters, K.counters, sizeof K.counters);
    put_info(c, K, 0, times);
    return UMICLUST_OK;
  });
}

int32_t umiclust_bam_index_info(umiclust_ctx* ctx, int64_t* out, double* times) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    if (!c->ix.have) c->fail(UMICLUST_ESTATE, "no index or flagstat call has run on this context");
    if (out) memcpy(out, c->ix.out, sizeof c->ix.out);
    if (times) memcpy(times, c->ix.times, sizeof c->ix.times);
    return UMICLUST_OK;
  });
}
