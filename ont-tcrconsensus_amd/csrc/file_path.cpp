// file_path.cpp -- the file path of the C ABI: a FASTA in, vsearch's cluster files, consout and log out
// (umiclust_run_fasta, umiclust_run_argv), optionally with the in-process parse_umi_clusters (umiclust_run_fasta_parse).
#include <sys/mman.h>

#include <algorithm>
#include <cstdio>
#include <exception>
#include <memory>
#include <thread>

#include "cluster_ctx.h"

using namespace uc;
using uc::io::Fasta;

namespace {

// a thread joined when its owner goes out of scope
struct Joiner {
  std::thread t;
  ~Joiner() {
    if (t.joinable()) t.join();
  }
};

int64_t run_fasta_impl(umiclust_ctx* c, const umiclust_params* p, const char* in_fasta,
                       const char* clusters_prefix, const char* consout, const char* log_path,
                       umiclust_stats* stats, const umiclust_parse_params* pp = nullptr,
                       const char* work_dir = nullptr, umiclust_parse_result* pr = nullptr) {
  const double t0 = now_s();
  c->join_release();
  std::unique_ptr<Fasta> fin(new Fasta());
  Fasta& f = *fin;
  // output mappings handed over by the writers (released with the input; at once if the call fails)
  struct Unmaps {
    std::vector<std::pair<void*, size_t>> v;
    ~Unmaps() {
      for (auto& m : v) munmap(m.first, m.second);
    }
  } unmaps;
  if (!in_fasta || !io::read_fasta(in_fasta, f)) c->fail(UMICLUST_EIO, "cannot read %s", in_fasta ? in_fasta : "(null)");
  const int64_t n = (int64_t)f.hdr_off.size();
  for (int64_t i = 0; i < n; i++) {
    const int64_t L = f.seq_off[i + 1] - f.seq_off[i];
    if (L > kMaxLen && L <= p->maxseqlength) c->fail(UMICLUST_ERANGE, "sequence longer than %d", kMaxLen);
  }
  const double t_read = now_s() - t0;
  // the fused drop-in: the headers' fields parse_clusters needs, computed on a few host threads while the GPU
  // clusters (the resolve pool keeps the rest of the CPUs)
  std::vector<io::RecFields> pre;
  Joiner pre_th;
  if (pp) pre_th.t = std::thread([&] { io::precompute_fields(f, pre, std::max(1, std::min(4, io::host_cpus() / 4))); });
  load_impl(c, p, f.seq.data(), f.seq_off.data(), n);
  if (c->bin_s.size() != 2) c->fail(UMICLUST_EINVAL, "file path: one bin per load");
  cluster_pinned(c, 0);  // the same host placement as the session API (umiclust_cluster)
  const double t1 = now_s();
  const int32_t K = c->nclusters;
  const int width = p->fasta_width;
  const io::ClusterView cv{K, c->num.ostart.data(), c->num.omemb.data(), c->perm.data()};
  // both writers build and write disjoint cluster ranges on io_threads() threads; the consout (one file: bound by its
  // page allocation or inode lock, 0.12 s of a config-2 bin on the GPU box) is written beside the cluster<N> files
  double t_cons = 0.0;
  std::exception_ptr cons_err;
  Joiner cons_th;
  if (consout)
    cons_th.t = std::thread([&] {
      try {
        io::write_consout(consout, f, cv, c->cons.data(), c->cons_off.data(), p->clusterout_id != 0, width);
      } catch (...) {
        cons_err = std::current_exception();
      }
      t_cons = now_s() - t1;
    });
  double t_mask = 0.0;
  int64_t n_rows = 0;  // masked rows downloaded for the cluster files: none, the changed rows alone, or every row
  if (clusters_prefix) {
    // vsearch prints the DUST-masked (upper-cased) db sequence.  Where no sequence changed (prepare counted them:
    // nothing masked, input already upper case) that is the input's own bytes, so the 112 B-per-UMI masked
    // buffer is downloaded only when some sequence changed
    std::vector<char> masked;
    std::vector<int32_t> mrow;
    if (c->n > 0 && c->n_changed > 0) {
      const double tm = now_s();
      if (c->n_changed * 16 < c->n) {  // a few changed rows (config 2: one): their flags, then those rows alone
        std::vector<uint8_t> chg((size_t)c->n);
        c->hip(hipMemcpy(chg.data(), c->d_mchg.p, chg.size(), hipMemcpyDeviceToHost), "d2h masked flags");
        mrow.assign((size_t)c->n, -1);
        int32_t r = 0;
        for (int32_t s = 0; s < c->n; s++)
          if (chg[s]) mrow[s] = r++;
        masked.resize((size_t)r * kMaxLen);
        n_rows = r;
        for (int32_t s = 0; s < c->n; s++)
          if (mrow[s] >= 0)
            c->hip(hipMemcpyAsync(masked.data() + (size_t)mrow[s] * kMaxLen, c->d_masked.p + (size_t)s * kMaxLen,
                                  kMaxLen, hipMemcpyDeviceToHost, c->st), "d2h masked row");
        c->hip(hipStreamSynchronize(c->st), "sync");
      } else {
        masked.resize((size_t)c->n * kMaxLen);
        n_rows = c->n;
        c->hip(hipMemcpy(masked.data(), c->d_masked.p, masked.size(), hipMemcpyDeviceToHost), "d2h masked");
      }
      t_mask = now_s() - tm;
    }
    io::write_cluster_files(clusters_prefix, f, cv, masked.empty() ? nullptr : masked.data(), kMaxLen,
                            c->hlen.data(), width, mrow.empty() ? nullptr : mrow.data());
  }
  const double t_files = now_s() - t1;
  if (cons_th.t.joinable()) cons_th.t.join();
  if (cons_err) std::rethrow_exception(cons_err);
  const double t_write = now_s() - t1;
  if (c->tun.debug)
    fprintf(stderr, "umiclust: file path: read %.3f s, cluster %.3f s, masked download %.3f s (%lld changed, %lld of %lld "
                    "rows), cluster files done at %.3f s, consout (beside them) at %.3f s\n", t_read, t1 - t0 - t_read,
            t_mask, (long long)c->n_changed, (long long)n_rows, (long long)c->n, t_files, t_cons);
  if (log_path) {
    const umiclust_stats& s = c->stats;
    int64_t nt = 0, singles = 0;
    int32_t smin = 0, smax = 0;
    for (int32_t x = 0; x < c->n; x++) nt += c->hlen[x];
    for (int32_t k = 0; k < K; k++) {
      const int32_t sz = c->num.ostart[k + 1] - c->num.ostart[k];
      singles += sz == 1;
      smin = k ? std::min(smin, sz) : sz;
      smax = std::max(smax, sz);
    }
    char buf[2048];
    snprintf(buf, sizeof(buf),
             "umiclust-mi355x (vsearch --cluster_fast drop-in, ABI %d)\n"
             "Reading file %s\n"
             "%lld nt in %lld seqs, min %d, max %d, avg %.0f\n"
             "%lld sequences discarded by the length window [%d, %d]\n"
             "Masking (dust), sorting by length, clustering (id %.4f, strand %s)\n"
             "Clusters: %d Size min %d, max %d, avg %.1f\n"
             "Singletons: %lld, %.1f%% of seqs, %.1f%% of clusters\n"
             "Alignments: %lld, cells: %lld, k-mer postings: %lld, blocks: %lld\n"
             "Time: read %.3f s, cluster %.3f s (prefilter %.3f, align %.3f, consensus %.3f, host %.3f), write %.3f s\n",
             UMICLUST_ABI_VERSION, in_fasta, (long long)nt, (long long)c->n,
             c->n ? (int)c->hlen[c->n - 1] : 0, c->n ? (int)c->hlen[0] : 0, c->n ? (double)nt / c->n : 0.0,
             (long long)(n - c->n), p->minseqlength, p->maxseqlength, p->id, p->strand_both ? "both" : "plus",
             K, smin, smax, K ? (double)c->n / K : 0.0, (long long)singles,
             c->n ? 100.0 * singles / c->n : 0.0, K ? 100.0 * singles / K : 0.0,
             (long long)s.n_alignments, (long long)s.cells, (long long)s.kmer_postings, (long long)s.n_blocks,
             t_read, s.t_total_s, s.t_prefilter_s, s.t_align_s, s.t_consensus_s, s.t_host_s, t_write);
    io::write_text(log_path, buf);
  }
  if (pp) {
    if (!c->p.clusterout_sort || !c->p.clusterout_id)
      c->fail(UMICLUST_EINVAL, "in-process parse needs --clusterout_sort and --clusterout_id numbering");
    const double tj = now_s();
    if (pre_th.t.joinable()) pre_th.t.join();
    if (c->tun.debug == 1) fprintf(stderr, "umiclust: fused: waited %.3f s for the header fields\n", now_s() - tj);
    io::parse_clusters(f, cv, pp, work_dir, pr, pre.empty() ? nullptr : pre.data(), &unmaps.v);
  }
  c->stats.t_read_s = t_read;
  c->stats.t_write_s = t_write + (pp ? now_s() - t1 - t_write : 0.0);
  // the outputs are written: the input goes on a thread of its own (UMICLUST_DEBUG prints how long it takes)
  {
    Fasta* in = fin.release();
    std::vector<std::pair<void*, size_t>> outs;
    outs.swap(unmaps.v);
    c->in_release = std::thread([in, outs, debug = c->tun.debug] {
      const double tr = now_s();
      for (auto& m : outs) munmap(m.first, m.second);
      delete in;
      if (debug) fprintf(stderr, "umiclust: file path: input released in %.3f s\n", now_s() - tr);
    });
  }
  c->stats.t_run_s = now_s() - t0;
  if (stats) *stats = c->stats;
  return K;
}

}  // namespace

extern "C" {

int64_t umiclust_run_fasta(umiclust_ctx* c, const umiclust_params* p, const char* in_fasta,
                           const char* clusters_prefix, const char* consout, const char* log_path,
                           umiclust_stats* stats) {
  UC_GUARD(c, {
    if (!p) c->fail(UMICLUST_EINVAL, "null params");
    return run_fasta_impl(c, p, in_fasta, clusters_prefix, consout, log_path, stats);
  });
}

int64_t umiclust_run_fasta_parse(umiclust_ctx* c, const umiclust_params* p, const char* in_fasta,
                                 const char* clusters_prefix, const char* consout, const char* log_path,
                                 const umiclust_parse_params* pp, const char* work_dir,
                                 umiclust_parse_result* result, umiclust_stats* stats) {
  UC_GUARD(c, {
    if (!p || !pp || !result) c->fail(UMICLUST_EINVAL, "null params");
    if (!p->clusterout_sort || !p->clusterout_id)
      c->fail(UMICLUST_EINVAL, "in-process parse needs --clusterout_sort and --clusterout_id numbering");
    if (pp->max_reads_per_cluster < 0 || pp->min_reads_per_cluster < 0) c->fail(UMICLUST_EINVAL, "read caps");
    return run_fasta_impl(c, p, in_fasta, clusters_prefix, consout, log_path, stats, pp, work_dir, result);
  });
}

int64_t umiclust_run_argv(umiclust_ctx* c, int32_t argc, const char* const* argv, umiclust_stats* stats) {
  UC_GUARD(c, {
    umiclust_params p;
    std::vector<char> in(4096), cl(4096), co(4096), lg(4096);
    int32_t rc = umiclust_params_from_argv(&p, argc, argv, in.data(), cl.data(), co.data(), lg.data(), 4096);
    if (rc != UMICLUST_OK) c->fail(rc, "cannot parse vsearch argv");
    return run_fasta_impl(c, &p, in.data(), cl[0] ? cl.data() : nullptr, co[0] ? co.data() : nullptr,
                          lg[0] ? lg.data() : nullptr, stats);
  });
}

}  // extern "C"
