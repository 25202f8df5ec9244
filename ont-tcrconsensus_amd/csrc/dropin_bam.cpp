// dropin_bam.cpp -- the BAM session (§8f f6, DESIGN.md §9b, bamscan.hip): the open from a BAM file (inflated on the
// device, dropin_bgzf.cpp) or from SAM text (dropin_sam.cpp) with its scan and cs group-by, the accessors, the writer's
// entry point (umiclust_bam_write; its device half is in dropin_bgzf.cpp), the name suffix (§8f f6b, DESIGN.md §9c,
// bamsplit.hip) and the close.  The region split on the session is in dropin_split.cpp.
#include <sys/stat.h>

#include <algorithm>
#include <cstring>

#include "bam_dev.h"

using namespace uc;
using namespace uc::io;

std::string_view uc::record_name(const RawBuf& raw, const std::vector<int64_t>& roff, int64_t r) {
  const uint8_t* rec = raw.data() + roff[r];
  const size_t lrn = std::min<size_t>(bam::l_read_name(rec), (size_t)bam::block_size(rec) - 32);
  return {(const char*)bam::name(rec), lrn ? strnlen((const char*)bam::name(rec), lrn) : 0};
}
BamSession* uc::bam_session(Ctx* c) {
  if (!c->bs.open) c->fail(UMICLUST_ESTATE, "no BAM session is open (umiclust_bam_open)");
  return &c->bs;
}
void uc::upload_session(Ctx* c, const BamSession& S, DevBuf<uint8_t>& d_raw, DevBuf<int64_t>& d_roff) {
  c->hip(d_raw.ensure(S.raw.size() + 1), "alloc");
  c->hip(d_roff.ensure(S.roff.size() + 1), "alloc");
  c->h2d(d_raw.p, S.raw.data(), S.raw.size()), c->h2d(d_roff.p, S.roff.data(), S.roff.size() * 8);
}

// ---------------------------------------------------------------- the open: scan with tags, cs group-by
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
  c->h2d(d_roff.p, S.roff.data(), (size_t)n * 8);
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
    c->d2h(&coll, d_coll.p, 4);
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
    c->d2h(S.cls.data(), d_cls.p, (size_t)n), c->d2h(S.ref.data(), d_ref.p, (size_t)n * 4);
    c->d2h(S.l_seq.data(), d_lseq.p, (size_t)n * 4), c->d2h(S.reflen.data(), d_reflen.p, (size_t)n * 8);
    c->d2h(S.cols.data(), d_cols.p, (size_t)n * 8), c->d2h(S.nm.data(), d_nm.p, (size_t)n * 8);
    c->d2h(S.nm_present.data(), d_nmp.p, (size_t)n), c->d2h(S.cs_off.data(), d_csoff.p, (size_t)n * 8);
    c->d2h(S.cs_len.data(), d_cslen.p, (size_t)n * 4), c->d2h(bad.data(), d_bad.p, (size_t)n);
    c->d2h(slot.data(), d_slot.p, (size_t)n * 8), c->d2h(rep.data(), d_rep.p, (size_t)m * 8);
    c->d2h(cnt.data(), d_cnt.p, (size_t)m * 4);
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
      k = bam::write_bgzf(out_bam, S.raw.data(), S.hdr.end, S.roff, keep, io_threads(), err, &S.write_coff);
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

int32_t umiclust_bam_name_suffix(umiclust_ctx* ctx, int64_t* value, uint8_t* status) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    auto& S = *bam_session(c);
    const int64_t n = (int64_t)S.roff.size();
    if (!n) return UMICLUST_OK;
    DevBuf<uint8_t> d_raw, d_status;
    DevBuf<int64_t> d_roff, d_value;
    alloc_each(c, (size_t)n, d_value, d_status);
    upload_session(c, S, d_raw, d_roff);
    c->hip(launch_name_suffix(d_raw.p, d_roff.p, n, d_value.p, d_status.p, c->st), "name suffix");
    if (value) c->d2h(value, d_value.p, (size_t)n * 8);
    if (status) c->d2h(status, d_status.p, (size_t)n);
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
