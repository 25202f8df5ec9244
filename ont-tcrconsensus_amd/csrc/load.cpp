// load.cpp -- a load's way onto the device: parameter checks, the acceptance / rank tables, staging the raw records
// (umiclust_stage) and vsearch's length filter, sort, DUST and k-mers over them (umiclust_prepare).
#include <algorithm>
#include <cstdio>

#include "cluster_ctx.h"

namespace uc {

Scoring to_scoring(const umiclust_params& p) {
  Scoring s{};
  s.match = p.match;
  s.mismatch = p.mismatch;
  for (int k = 0; k < 6; k++) {
    s.go[k] = p.gap_open[k];
    s.ge[k] = p.gap_ext[k];
  }
  s.boundary_open = p.policy_boundary_open;
  return s;
}

void validate(umiclust_ctx* c, const umiclust_params& p) {
  if (p.wordlength != 8) c->fail(UMICLUST_EINVAL, "wordlength %d unsupported (8 required)", p.wordlength);
  if (p.maxaccepts != 1 || p.maxrejects != 32)
    c->fail(UMICLUST_EINVAL, "maxaccepts/maxrejects must be 1/32 (got %d/%d)", p.maxaccepts, p.maxrejects);
  if (p.minseqlength < 1 || p.minseqlength > p.maxseqlength)
    c->fail(UMICLUST_EINVAL, "bad length window [%d,%d]", p.minseqlength, p.maxseqlength);
  if (!(p.id > 0.0 && p.id <= 1.0)) c->fail(UMICLUST_EINVAL, "--id must be in (0,1]");
  if (p.minwordmatches < 0) c->fail(UMICLUST_EINVAL, "minwordmatches < 0");
  if (p.policy_threads != 0 && p.policy_threads != 1) c->fail(UMICLUST_EINVAL, "policy_threads must be 0 or 1");
  if (p.policy_threads && (p.threads < 1 || p.threads > kMaxBlock))
    c->fail(UMICLUST_EINVAL, "policy_threads = 1 needs 1 <= threads <= %d", kMaxBlock);
  // The alignment kernels' 16-bit cells (DESIGN.md section 6, K3P range argument).  Gap penalties are costs: a
  // negative component passes a bound on the sums alone and does not fit the cells.
  int64_t mx = (int64_t)std::abs((int64_t)p.match) + std::abs((int64_t)p.mismatch);
  for (int k = 0; k < 6; k++) {
    if (p.gap_open[k] < 0) c->fail(UMICLUST_EINVAL, "gap_open[%d] = %d is negative", k, p.gap_open[k]);
    if (p.gap_ext[k] < 0) c->fail(UMICLUST_EINVAL, "gap_ext[%d] = %d is negative", k, p.gap_ext[k]);
    mx = std::max(mx, (int64_t)p.gap_open[k] + p.gap_ext[k]);
  }
  if (mx * 2 * kMaxLen > 15000)
    c->fail(UMICLUST_EINVAL, "scores too large for 16-bit DP (|match| + |mismatch| and every gap_open + gap_ext <= %d)",
            15000 / (2 * kMaxLen));
  // The closed boundary's state is the constant -16000 in the packed kernels' frame H'' = H - (mismatch + ge[QI]) (row
  // + 1) + ...; it has to stay below column 0's real cells, the lowest of which is the boundary column's last row
  // plus one diagonal move.  Only a positive mismatch score beside large extension penalties comes near.
  if (!p.policy_boundary_open) {
    const int64_t low = p.gap_open[1] + (int64_t)(kMaxLen - 1) * (p.gap_ext[1] + p.mismatch + p.gap_ext[2]) +
                        std::max(0, p.mismatch - p.match) + std::max(p.gap_open[2], p.gap_open[4]);
    if (low > 16000)
      c->fail(UMICLUST_EINVAL, "policy_boundary_open = 0 with mismatch %d, gap_ext[1] %d and gap_ext[2] %d: column 0 "
              "falls below the 16-bit boundary state (use policy_boundary_open = 1)", p.mismatch, p.gap_ext[1],
              p.gap_ext[2]);
  }
}

namespace {

// exact acceptance / id-order tables: id2 = 100.0*m/L (align_trim, iddef 2),
// accept iff id2 >= 100.0*opt_id, both in IEEE double exactly as vsearch evaluates them.
void build_tables(umiclust_ctx* c) {
  const int NL = kTabL, NM = kTabM;
  c->h_acc.assign((size_t)NL * NM, 0);
  c->h_rank.assign((size_t)NL * NM, 0);
  std::vector<std::pair<double, int>> v;
  v.reserve((size_t)NL * NM);
  const double thr = 100.0 * c->p.id;
  for (int L = 0; L < NL; L++)
    for (int m = 0; m < NM; m++) {
      const double id = L > 0 ? 100.0 * m / L : 0.0;
      c->h_acc[(size_t)L * NM + m] = (L > 0 && m <= L && id >= thr) ? 1 : 0;
      v.push_back({id, L * NM + m});
    }
  std::sort(v.begin(), v.end());
  uint16_t r = 0;
  for (size_t i = 0; i < v.size(); i++) {
    if (i > 0 && v[i].first != v[i - 1].first) r++;
    c->h_rank[(size_t)v[i].second] = r;
  }
  c->hip(c->d_acc.ensure(c->h_acc.size()), "alloc acc");
  c->hip(c->d_rank.ensure(c->h_rank.size()), "alloc rank");
  c->hip(hipMemcpyAsync(c->d_acc.p, c->h_acc.data(), c->h_acc.size(), hipMemcpyHostToDevice, c->st), "acc");
  c->hip(hipMemcpyAsync(c->d_rank.p, c->h_rank.data(), c->h_rank.size() * 2, hipMemcpyHostToDevice, c->st),
         "rank");
}

}  // namespace

// ---------------------------------------------------------------- load
// bin_in: nbins + 1 input record boundaries (NULL: one bin of all n records)
// Stage the raw records of a load in HBM (umiclust_stage): the ASCII bytes and record offsets, and the record lengths
// and bin boundaries on the host.  Nothing of A3 (length filter, sort, DUST, k-mers) happens here: that is
// prepare_impl's, from these resident records.
void stage_impl(umiclust_ctx* c, const char* seqs, const int64_t* offs, int64_t n, const int64_t* bin_in,
                int32_t nbins) {
  if ((!seqs && n > 0) || !offs || n < 0 || nbins < 1) c->fail(UMICLUST_EINVAL, "null argument");
  c->staged = false;
  c->loaded = false;
  c->clustered = false;
  c->n_input = n;
  c->bin_in.assign((size_t)nbins + 1, 0);
  if (bin_in) {
    if (bin_in[0] != 0 || bin_in[nbins] != n) c->fail(UMICLUST_EINVAL, "bin boundaries must span [0, n]");
    for (int32_t b = 0; b < nbins; b++)
      if (bin_in[b + 1] < bin_in[b]) c->fail(UMICLUST_EINVAL, "bin boundaries must not decrease");
    for (int32_t b = 0; b <= nbins; b++) c->bin_in[b] = bin_in[b];
  } else {
    c->bin_in[1] = n;
  }
  c->rec_len.resize((size_t)n);
  for (int64_t i = 0; i < n; i++) {
    const int64_t L = offs[i + 1] - offs[i];
    if (L < 0) c->fail(UMICLUST_EINVAL, "record offsets must not decrease");
    c->rec_len[i] = (uint32_t)std::min<int64_t>(L, UINT32_MAX);
  }
  const int64_t bytes = n > 0 ? offs[n] - offs[0] : 0;
  c->hip(c->d_ascii.ensure((size_t)bytes + 1), "alloc ascii");
  c->hip(c->d_offs.ensure((size_t)n + 1), "alloc offs");
  std::vector<int64_t> rel;
  upload_seqs(c, seqs, offs, n, c->d_ascii, c->d_offs, rel, c->st);  // allocated above: the same two copies
  c->hip(hipStreamSynchronize(c->st), "sync stage");  // `rel` goes out of scope
  c->staged = true;
}

// vsearch's load, length filter, DUST and length sort over the staged records
// (umiclust_prepare): the stable counting sort by length on the host (perm, hlen: the host's resolve and writers
// use them), then K1 k_prep on the device (DUST, 4-bit codes, unique 8-mers of both strands) from the resident
// ASCII.  One stream synchronisation at the end.
void prepare_impl(umiclust_ctx* c, const umiclust_params* p) {
  if (!p) c->fail(UMICLUST_EINVAL, "null argument");
  if (!c->staged) c->fail(UMICLUST_ESTATE, "umiclust_prepare before umiclust_stage");
  validate(c, *p);
  c->loaded = false;
  c->clustered = false;
  c->p = *p;
  c->sc = to_scoring(*p);
  c->both = p->strand_both ? 2 : 1;
  c->o4_T = (p->policy_threads && p->threads > 1) ? p->threads : 0;
  const double tp0 = now_s();
  build_tables(c);
  const int64_t n = c->n_input;
  const int32_t nbins = (int32_t)c->bin_in.size() - 1;
  const uint32_t* rl = c->rec_len.data();
  // length filter + stable sort by length desc within every bin (db_sortbylength; ties keep input order, O1), bins
  // laid out one after another: io::sort_by_length (host_io.cpp)
  if (n > (int64_t)INT32_MAX) c->fail(UMICLUST_ERANGE, "too many sequences in one load");  // perm holds int32
  c->hip(c->h_perm.ensure((size_t)n + 1), "pin perm");
  c->hlen.resize((size_t)n);
  c->bin_s.assign((size_t)nbins + 1, 0);
  const io::LenSort ls = io::sort_by_length(rl, c->bin_in.data(), nbins, p->minseqlength, p->maxseqlength,
                                            io::io_threads(), c->h_perm.p, c->hlen.data(), c->bin_s.data());
  const int64_t kept = ls.kept;
  if (ls.bad >= 0) {  // the first input record whose length is out of range
    if (rl[ls.bad] > kMaxLen) c->fail(UMICLUST_ERANGE, "sequence longer than %d", kMaxLen);
    c->fail(UMICLUST_ERANGE, "sequence shorter than %d (minseqlength)", kMinTplLen);
  }
  if (kept > (int64_t)INT32_MAX / 2) c->fail(UMICLUST_ERANGE, "too many sequences in one load");
  c->n = (int32_t)kept;
  c->hlen.resize((size_t)kept);
  const size_t ns = (size_t)c->n + 1;
  c->hip(c->d_perm.ensure(ns), "alloc perm");
  if (c->n > 0)
    c->hip(hipMemcpyAsync(c->d_perm.p, c->h_perm.p, (size_t)c->n * 4, hipMemcpyHostToDevice, c->st), "h2d");
  c->hip(c->d_codes.ensure(ns * 2 * kCodeWords), "alloc");
  c->hip(c->d_lens.ensure(ns), "alloc");
  c->hip(c->d_kmers.ensure(ns * 2 * kKmerStride), "alloc");
  c->hip(c->d_nk.ensure(ns * 2), "alloc");
  c->hip(c->d_masked.ensure(ns * kMaxLen), "alloc");
  if (c->iota_n < ns) {  // 0, 1, 2, ... (peer tiles index sequences by seqno); the same for every load
    c->hip(c->d_iota.ensure(ns), "alloc");
    c->hip(launch_iota(c->d_iota.p, (int32_t)ns, c->st), "iota");
    c->iota_n = ns;
  }
  c->hip(c->d_amb.ensure(2), "alloc");
  c->hip(c->h_amb.ensure(2), "pin");
  c->hip(hipMemsetAsync(c->d_amb.p, 0, 8, c->st), "memset");
  c->hip(c->d_mchg.ensure((size_t)std::max(c->n, 1)), "alloc");
  const double tp1 = now_s();
  c->hip(launch_prep(c->d_ascii.p, c->d_offs.p, c->d_perm.p, c->n, p->qmask_dust, c->d_codes.p,
                     c->d_lens.p, c->d_kmers.p, c->d_nk.p, c->d_masked.p, c->d_amb.p, c->st, c->d_mchg.p),
         "prep");
  c->hip(hipMemcpyAsync(c->h_amb.p, c->d_amb.p, 8, hipMemcpyDeviceToHost, c->st), "d2h");
  // the host's per-sequence state is filled while K1 runs
  c->perm.assign(c->h_perm.p, c->h_perm.p + c->n);
  c->cno.assign(c->n, -1);
  c->strand.assign(c->n, 0);
  c->target.assign(c->n, -1);
  c->ocl.assign(c->n, -1);
  c->bout.assign(nbins, umiclust_ctx::BinOut());
  c->cur_bin = -1;
  c->hqbin.clear();
  if (nbins > 1 && c->n > 0) {
    // packs: per-bin XOR masks on the k-mers (a bijection within a bin: counts within a bin are unchanged; other
    // bins' structured k-mers land on unrelated lists), sorted seqno -> bin, each bin's first seqno
    c->hqbin.resize(c->n);
    c->hip(c->h_xm.ensure((size_t)nbins), "pin");
    for (int32_t b = 0; b < nbins; b++) {
      for (int32_t s = c->bin_s[b]; s < c->bin_s[b + 1]; s++) c->hqbin[s] = b;
      uint32_t h = (uint32_t)b * 0x9E3779B1u + 0x7F4A7C15u;  // murmur3 finaliser
      h ^= h >> 16;
      h *= 0x85EBCA6Bu;
      h ^= h >> 13;
      h *= 0xC2B2AE35u;
      h ^= h >> 16;
      c->h_xm.p[b] = (uint16_t)(h ^ (h >> 16));
    }
    c->hip(c->d_qbin.ensure(c->n), "alloc");
    alloc_each(c, nbins, c->d_bin_seq0, c->d_bin_ord0);
    c->hip(c->h_bin_ord0.ensure(nbins), "pin");
    c->hip(c->d_xm.ensure(nbins), "alloc");
    c->hip(hipMemcpyAsync(c->d_qbin.p, c->hqbin.data(), (size_t)c->n * 4, hipMemcpyHostToDevice, c->st), "h2d");
    c->hip(hipMemcpyAsync(c->d_bin_seq0.p, c->bin_s.data(), (size_t)nbins * 4, hipMemcpyHostToDevice, c->st), "h2d");
    c->hip(hipMemcpyAsync(c->d_xm.p, c->h_xm.p, (size_t)nbins * 2, hipMemcpyHostToDevice, c->st), "h2d");
    c->hip(launch_kmer_xor(c->d_kmers.p, c->d_nk.p, c->n, c->d_qbin.p, c->d_xm.p, c->st), "k-mer masks");
  }
  const double tp2 = now_s();
  c->hip(hipStreamSynchronize(c->st), "sync load");
  if (c->tun.debug)
    fprintf(stderr, "umiclust: prepare: host sort %.4f s, after the K1 launch %.4f s, sync %.4f s\n", tp1 - tp0,
            tp2 - tp1, now_s() - tp2);
  c->ambig = c->h_amb.p[0] != 0;
  c->n_changed = (int64_t)c->h_amb.p[1];
  c->loaded = true;
  c->clustered = false;
}

void load_impl(umiclust_ctx* c, const umiclust_params* p, const char* seqs, const int64_t* offs, int64_t n,
               const int64_t* bin_in, int32_t nbins) {
  if (!p) c->fail(UMICLUST_EINVAL, "null argument");
  validate(c, *p);
  stage_impl(c, seqs, offs, n, bin_in, nbins);
  prepare_impl(c, p);
}

}  // namespace uc
