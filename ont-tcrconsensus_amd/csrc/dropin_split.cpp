// dropin_split.cpp -- the region split of a BAM, round 1 and round 2, plain and fused with the UMI extraction: one core
// (split_core) behind six entry points.  Round 1 classifies the record bytes, CIGAR and all (§8f f4, regionsplit.hip),
// of a file (umiclust_region_split[_extract]) or of the open session (umiclust_bam_region_split[_extract], DESIGN.md
// §9f); round 2 classifies the session's columns under a keep mask (umiclust_bam_split[_extract], §8f f4b, DESIGN.md
// §9c, bamsplit.hip).  Both end in the same emitters: the region FASTA (k_bam_emit) or the detected-UMI FASTA (§8f
// f4+f1, DESIGN.md §9d, bamextract.hip).
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cstring>
#include <unordered_map>

#include "bam_dev.h"

using namespace uc;
using namespace uc::io;

namespace {
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
    c->h2d(d_pos.p, pos.data(), (size_t)stop * 8);
    c->hip(launch(d_pos.p, d_out.p), "bam emit");
    c->d2h(outb.data(), d_out.p, (size_t)cbase[nb]);
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
  c->h2d(d_pat.p, &P, sizeof(P));
  c->hip(launch_bam_umi_search(d_raw, d_roff, stop, d_cls, u.a5, u.a3, u.k, d_pat.p, d_res.p, d_len.p, c->st),
         "bam umi search");
  c->d2h(olen.data(), d_len.p, (size_t)stop * 8);
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
    c->d2h(res.data(), d_res.p, res.size() * 4);
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

// What the split reads: the inflated file on the host and on the device, its header and its record offsets, there
// too.  The path-based entries fill it from read_bam_on_device and own what they made; the session entries point into
// the open session and upload its raw and roff.
struct SplitSource {
  const RawBuf* raw = nullptr;
  const bam::Header* hdr = nullptr;
  const std::vector<int64_t>* roff = nullptr;
  const BamSession* session = nullptr;
  DevBuf<uint8_t> d_raw;
  DevBuf<int64_t> d_roff;
  std::string what;  // the file's name in a refusal
  RawBuf own_raw;
  bam::Header own_hdr;
  std::vector<int64_t> own_roff;

  void from_path(Ctx* c, const char* bam_file) {
    // the file inflated on the device: raw there (d_raw) and on the host
    int64_t inflate_info[3];
    if (!read_bam_on_device(c, bam_file, own_raw, d_raw, inflate_info, nullptr))
      c->fail(UMICLUST_EIO, "cannot read BGZF/BAM %s", bam_file);
    std::string herr;
    if (!bam::parse_header(own_raw.data(), own_raw.size(), own_hdr, herr)) c->fail(UMICLUST_EFORMAT, "%s is not BAM", bam_file);
    if (!bam::record_offsets(own_raw.data(), own_raw.size(), own_hdr.end, own_roff, herr))
      c->fail(UMICLUST_EFORMAT, "truncated BAM record");
    raw = &own_raw, hdr = &own_hdr, roff = &own_roff, what = bam_file;
  }
  void from_session(const BamSession& S) { raw = &S.raw, hdr = &S.hdr, roff = &S.roff, session = &S, what = "the BAM session"; }
  // raw and roff to the device, what of them is not there yet; after the caller's allocations, as it always was
  void upload(Ctx* c) {
    if (session) return upload_session(c, *session, d_raw, d_roff);
    c->hip(d_roff.ensure(roff->size() + 1), "alloc");
    c->h2d(d_roff.p, roff->data(), roff->size() * 8);
  }
};

// What the six entries share of their arguments.  bucket: region_clusters / region_buckets; cap: ncluster_cap /
// nbuckets, the room in reads_per and umis_per; umi null: the region FASTA, set: the detected-UMI FASTA.
struct SplitArgs {
  int32_t nregions;
  const char* const* region_names;
  const int64_t* region_lengths;
  const int32_t* bucket;
  double minov;
  int32_t s5, s3;
  const UmiArgs* umi;
  int64_t *counts, *reads_per, *umis_per;
  int32_t cap;
  uint8_t* region_detected;
  char* missing_name;
  int32_t missing_cap;
  bool bad_regions() const {
    return nregions < 0 || (nregions > 0 && (!region_names || !region_lengths || !bucket)) || !counts;
  }
};
// what every entry checks ahead of its other arguments: the room for the UMI counts and the extraction parameters
void check_umi(Ctx* c, const SplitArgs& a, ExtractPatterns& pat) {
  if (!a.umi) return;
  if ((a.cap > 0 && !a.umis_per) || a.umi->a5 < 0 || a.umi->a3 < 0 || a.umi->k < 0) c->fail(UMICLUST_EINVAL, "bad argument");
  build_patterns(c, a.umi->fwd, a.umi->rev, pat);
}

// The split itself, the same for round 1 and round 2.  classify(nref, d_rlen, d_rbkt, d_cls, d_bkt, d_outlen) queues
// the kernel that turns the region map by refID into every record's class, bucket and output bytes -- on the record
// bytes (launch_bam_classify) or on the session's columns (launch_split_cols): the one place where the rounds differ
// -- and path_of(bucket) names a bucket's file.  Returns the number of files written.
template <typename Classify, typename PathOf>
int64_t split_core(Ctx* c, SplitSource& src, const SplitArgs& a, const ExtractPatterns& pat, Classify classify,
                   PathOf path_of) {
  const RawBuf& raw = *src.raw;
  const std::vector<int64_t>& roff = *src.roff;
  const std::vector<std::string>& refname = src.hdr->ref_name;
  // the reference names of the header, matched to the regions of the reference FASTA
  std::unordered_map<std::string, int32_t> rid;
  for (int32_t r = 0; r < a.nregions; r++) rid.emplace(a.region_names[r], r);
  const int32_t nref = (int32_t)refname.size();
  std::vector<int64_t> rlen(nref, -1);
  std::vector<int32_t> rbkt(nref, -1), rreg(nref, -1);
  for (int32_t r = 0; r < nref; r++) {
    auto it = rid.find(refname[r]);
    if (it != rid.end()) {
      rreg[r] = it->second;
      rlen[r] = a.region_lengths[it->second];
      rbkt[r] = a.bucket[it->second];
    }
  }
  const int64_t n = (int64_t)roff.size();
  DevBuf<int64_t> d_rlen, d_outlen, d_pos;
  DevBuf<int32_t> d_rbkt, d_bkt;
  DevBuf<int8_t> d_cls;
  alloc_each(c, (size_t)n + 1, d_cls, d_bkt, d_outlen, d_pos);
  alloc_each(c, (size_t)nref + 1, d_rlen, d_rbkt);
  src.upload(c);
  c->h2d(d_rlen.p, rlen.data(), (size_t)nref * 8), c->h2d(d_rbkt.p, rbkt.data(), (size_t)nref * 4);
  classify(nref, d_rlen.p, d_rbkt.p, d_cls.p, d_bkt.p, d_outlen.p);
  std::vector<int8_t> cls(n);
  std::vector<int32_t> bkt(n);
  std::vector<int64_t> olen(n);
  c->d2h(cls.data(), d_cls.p, (size_t)n), c->d2h(bkt.data(), d_bkt.p, (size_t)n * 4);
  c->d2h(olen.data(), d_outlen.p, (size_t)n * 8);
  c->hip(hipStreamSynchronize(c->st), "sync");
  // the reference raises KeyError at the first primary record whose region is unknown, after the records before it
  int64_t stop = n;
  for (int64_t r = 0; r < n && stop == n; r++)
    if (cls[r] == kBamNoRegion || cls[r] == kBamNoCluster) stop = r;
  // One pass over the kept records' fixed fields: the regions they are on (a kept record is on one), and the name
  // field.  k_bam_emit indexes a kept record by its own fields: round 1 has checked them all (check_record_fields); in
  // round 2 kept records are primary, and the open has refused every primary record whose l_seq is negative or whose
  // fields overrun its block_size, but it does not look at an empty name field.
  std::vector<uint8_t> detected((size_t)a.nregions, 0);
  int32_t nb = 0;  // the kept records' buckets are [0, nb)
  for (int64_t r = 0; r < stop; r++)
    if (cls[r] == kBamKept) {
      const uint8_t* rec = raw.data() + roff[r];
      if (bam::l_read_name(rec) == 0) c->fail(UMICLUST_EFORMAT, "BAM record %lld: l_read_name 0", (long long)r);
      detected[rreg[bam::ref_id(rec)]] = 1;
      nb = std::max(nb, bkt[r] + 1);
    }
  // output grouped by bucket (the reference's KeyError ends the pipeline before extract_umis starts: no UMI file then)
  std::vector<int32_t> used;
  if (!a.umi)
    used = emit_fasta(c, src.d_raw.p, src.d_roff.p, d_cls.p, d_pos, cls, bkt, olen, stop, path_of);
  else if (stop == n)
    used = emit_umis(c, raw, roff, src.d_raw.p, src.d_roff.p, d_cls.p, d_pos, cls, bkt, stop, *a.umi, pat, path_of,
                     a.umis_per, a.cap);
  // counters of the records the reference reached
  int64_t cnt[4] = {0, 0, 0, 0};  // unmapped, primary mapped, short, long
  if (a.cap > 0) memset(a.reads_per, 0, sizeof(int64_t) * (size_t)a.cap);
  if (a.region_detected && a.nregions) memcpy(a.region_detected, detected.data(), (size_t)a.nregions);
  const int64_t last = stop < n ? stop + 1 : n;  // the failing record counts as a primary alignment too
  for (int64_t r = 0; r < last; r++) {
    const int8_t k = cls[r];
    if (k == kBamUnmapped) cnt[0]++;
    if (k >= kBamShort && k != kBamAbsent) cnt[1]++;
    if (k == kBamShort) cnt[2]++;
    if (k == kBamLong) cnt[3]++;
    if (k == kBamKept && r < stop && bkt[r] < a.cap) a.reads_per[bkt[r]]++;
  }
  for (int x = 0; x < 4; x++) a.counts[x] = cnt[x];
  if (stop < n) {
    const int32_t ref = bam::ref_id(raw.data() + roff[stop]);
    const std::string nm = ref >= 0 && ref < nref ? refname[ref] : std::string("None");
    if (a.missing_name && a.missing_cap > 0) snprintf(a.missing_name, (size_t)a.missing_cap, "%s", nm.c_str());
    c->fail(UMICLUST_EFORMAT, "KeyError: '%s'", nm.c_str());
  }
  // (round 2 has refused a bucket past the capacity up front)
  if (nb > a.cap) c->fail(UMICLUST_ERANGE, "cluster ids up to %d exceed the counter capacity", nb - 1);
  return (int64_t)used.size();
}

// Round 1, on the record bytes of a file or (bam_file null) of the open session: region_cluster<k>.fasta or
// region_cluster<k>_detected_umis.fasta in out_dir.
int64_t round1(umiclust_ctx* ctx, const char* bam_file, bool session, const SplitArgs& a, const char* out_dir) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    ExtractPatterns pat;
    check_umi(c, a, pat);
    if ((!session && !bam_file) || !out_dir || a.bad_regions() || a.cap < 0 || (a.cap > 0 && !a.reads_per))
      c->fail(UMICLUST_EINVAL, "bad argument");
    SplitSource src;
    if (session) src.from_session(*bam_session(c));
    if (!session) src.from_path(c, bam_file);
    // the kernels index each record by its own l_read_name, n_cigar_op and l_seq
    std::string herr;
    if (!bam::check_record_fields(src.raw->data(), *src.roff, herr))
      c->fail(UMICLUST_EFORMAT, "%s: %s", src.what.c_str(), herr.c_str());
    const auto classify = [&](int32_t nref, const int64_t* d_rlen, const int32_t* d_rbkt, int8_t* d_cls, int32_t* d_bkt,
                              int64_t* d_outlen) {
      c->hip(launch_bam_classify(src.d_raw.p, src.d_roff.p, (int64_t)src.roff->size(), nref, d_rlen, d_rbkt, a.minov,
                                 a.s5, a.s3, d_cls, d_bkt, d_outlen, c->st),
             "bam classify");
    };
    const std::string tail = a.umi ? "_detected_umis.fasta" : ".fasta";
    return split_core(c, src, a, pat, classify,
                      [&](int32_t k) { return pjoin(out_dir, "region_cluster" + std::to_string(k) + tail); });
  });
}

// Round 2, on the session's columns under a keep mask (null: every record): bucket b goes to bucket_paths[b].
int64_t round2(umiclust_ctx* ctx, const uint8_t* keep, const SplitArgs& a, const char* const* bucket_paths) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    const BamSession& S = *bam_session(c);
    ExtractPatterns pat;
    check_umi(c, a, pat);
    if (a.bad_regions() || a.cap < 0 || (a.cap > 0 && (!bucket_paths || !a.reads_per)))
      c->fail(UMICLUST_EINVAL, "bad argument");
    for (int32_t r = 0; r < a.nregions; r++)
      if (a.bucket[r] >= a.cap) c->fail(UMICLUST_EINVAL, "region %d: bucket %d of %d", r, a.bucket[r], a.cap);
    SplitSource src;
    src.from_session(S);
    const size_t n = S.roff.size();
    DevBuf<uint8_t> d_keep;
    DevBuf<int64_t> d_reflen;
    DevBuf<int32_t> d_ref, d_lseq;
    DevBuf<int8_t> d_scan;
    alloc_each(c, n + 1, d_keep, d_reflen, d_ref, d_lseq, d_scan);
    const auto classify = [&](int32_t nref, const int64_t* d_rlen, const int32_t* d_rbkt, int8_t* d_cls, int32_t* d_bkt,
                              int64_t* d_outlen) {
      c->h2d(d_scan.p, S.cls.data(), n), c->h2d(d_ref.p, S.ref.data(), n * 4);
      c->h2d(d_lseq.p, S.l_seq.data(), n * 4), c->h2d(d_reflen.p, S.reflen.data(), n * 8);
      if (keep) c->h2d(d_keep.p, keep, n);
      BamScanCols col{};
      col.cls = d_scan.p, col.ref = d_ref.p, col.l_seq = d_lseq.p, col.reflen = d_reflen.p;
      c->hip(launch_split_cols(col, src.d_raw.p, src.d_roff.p, keep ? d_keep.p : nullptr, (int64_t)n, nref, d_rlen,
                               d_rbkt, a.minov, a.s5, a.s3, d_cls, d_bkt, d_outlen, c->st),
             "split cols");
    };
    return split_core(c, src, a, pat, classify, [&](int32_t b) { return std::string(bucket_paths[b]); });
  });
}
}  // namespace

int64_t umiclust_region_split(umiclust_ctx* ctx, const char* bam_file, int32_t nregions, const char* const* region_names,
                              const int64_t* region_lengths, const int32_t* region_clusters,
                              double minimal_region_overlap, int32_t max_softclip_5_end, int32_t max_softclip_3_end,
                              const char* out_dir, int64_t* counts, int64_t* reads_per_cluster, int32_t ncluster_cap,
                              uint8_t* region_detected, char* missing_name, int32_t missing_cap) {
  return round1(ctx, bam_file, false,
                {nregions, region_names, region_lengths, region_clusters, minimal_region_overlap, max_softclip_5_end,
                 max_softclip_3_end, nullptr, counts, reads_per_cluster, nullptr, ncluster_cap, region_detected,
                 missing_name, missing_cap},
                out_dir);
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
  return round1(ctx, bam_file, false,
                {nregions, region_names, region_lengths, region_clusters, minimal_region_overlap, max_softclip_5_end,
                 max_softclip_3_end, &umi, counts, reads_per_cluster, umis_per_cluster, ncluster_cap, region_detected,
                 missing_name, missing_cap},
                umi_out_dir);
}

// the same two on the open session: no bam_file, everything else as above
int64_t umiclust_bam_region_split(umiclust_ctx* ctx, int32_t nregions, const char* const* region_names,
                                  const int64_t* region_lengths, const int32_t* region_clusters,
                                  double minimal_region_overlap, int32_t max_softclip_5_end, int32_t max_softclip_3_end,
                                  const char* out_dir, int64_t* counts, int64_t* reads_per_cluster,
                                  int32_t ncluster_cap, uint8_t* region_detected, char* missing_name,
                                  int32_t missing_cap) {
  return round1(ctx, nullptr, true,
                {nregions, region_names, region_lengths, region_clusters, minimal_region_overlap, max_softclip_5_end,
                 max_softclip_3_end, nullptr, counts, reads_per_cluster, nullptr, ncluster_cap, region_detected,
                 missing_name, missing_cap},
                out_dir);
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
  return round1(ctx, nullptr, true,
                {nregions, region_names, region_lengths, region_clusters, minimal_region_overlap, max_softclip_5_end,
                 max_softclip_3_end, &umi, counts, reads_per_cluster, umis_per_cluster, ncluster_cap, region_detected,
                 missing_name, missing_cap},
                umi_out_dir);
}

// round 2: the region FASTA files are appended to, the detected-UMI FASTA files truncated
int64_t umiclust_bam_split(umiclust_ctx* ctx, const uint8_t* keep, int32_t nregions, const char* const* region_names,
                           const int64_t* region_lengths, const int32_t* region_buckets, int32_t nbuckets,
                           const char* const* bucket_paths, double minimal_region_overlap, int32_t max_softclip_5_end,
                           int32_t max_softclip_3_end, int64_t* counts, int64_t* reads_per_bucket,
                           uint8_t* region_detected, char* missing_name, int32_t missing_cap) {
  return round2(ctx, keep,
                {nregions, region_names, region_lengths, region_buckets, minimal_region_overlap, max_softclip_5_end,
                 max_softclip_3_end, nullptr, counts, reads_per_bucket, nullptr, nbuckets, region_detected, missing_name,
                 missing_cap},
                bucket_paths);
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
  return round2(ctx, keep,
                {nregions, region_names, region_lengths, region_buckets, minimal_region_overlap, max_softclip_5_end,
                 max_softclip_3_end, &umi, counts, reads_per_bucket, umis_per_bucket, nbuckets, region_detected,
                 missing_name, missing_cap},
                bucket_umi_paths);
}
