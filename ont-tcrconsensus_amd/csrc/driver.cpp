// driver.cpp -- the MI355X UMI clustering pipeline (ClusterRun, cluster_all), the context's life cycle and the session
// entries of the C ABI (include/umiclust.h).  Its parts are beside it on cluster_ctx.h: the index (index.cpp), one
// pass and its resolution (pass.cpp), load and prepare (load.cpp), the file path (file_path.cpp), the kernel-level
// probes (probes.cpp) and the timeline (timeline.cpp).  The drop-ins (f1, f3-f6) are dropin_*.cpp, on the context
// core of ctx.h.
//
// Replaces the `vsearch --cluster_fast` subprocess of
// /root/reference/ont_tcr_consensus/vsearch_umi_cluster.py:21-54 (round 1) and :71-97 (round 2).
// vsearch's greedy is sequential: query k (length-sorted) is compared with the centroids created
// by queries 0..k-1.  This driver keeps that definition exactly while batching on the GPU:
//
//   for each block of B consecutive sorted queries of one length:
//     K2  prefilter every (query, strand) against C_old (the index: centroids of the blocks before
//         the peer window) -> exact top-41 list T_old, and against the earlier queries of the peer
//         window (previous block + this block) -> peer list P (count >= threshold)
//     K3W walk T_old on the device in batches of 8 (vsearch's pop loop), aligning with K3, and
//         align every (query, peer) pair speculatively
//     host pass 1: in sorted order, a query whose centroid peers cannot change its walk takes the
//         device outcome; otherwise it runs the exact merged walk over T_old u centroid peers,
//         deferred only if that walk needs a T_old entry the device did not align
//     round B (side stream): align what deferred queries need; host pass 2 resolves them
//     new centroids are appended to the LSM index (sealed / base / delta tiles)
//
// The passes form a software pipeline: pass k+1 is queued before the host resolves block k, so
// the host work hides behind device work.  Pass k+1's index lacks block k, which is why its peer
// window includes block k.  top-41 of (C_old u N) = top-41 of (top-41(C_old) u N), and a walk
// touches at most 32 entries, so every alignment a query can need exists: the result is
// identical to the sequential definition (vsearch --threads 1).
#include <algorithm>
#include <cstdio>
#include <sched.h>

#include "cluster_ctx.h"

using namespace uc;

std::atomic<int> uc::g_live_ctx{0};

// Keep the host resolve -- the calling thread and the resolve pool -- inside the L3 domain the caller runs on,
// for the duration of one call; the caller's and the pool's affinity are restored afterwards.  Only while this
// is the process's one live context and the process is its node's only rank (LOCAL_WORLD_SIZE <= 1): several
// contexts (bin-set lanes) or ranks pinned by where their callers happen to run could all land on one CCD.
// UMICLUST_PIN=0 turns it off, UMICLUST_PIN=1 forces it on.
// CPUs the calling thread may run on (its affinity mask: taskset, cgroup cpusets, L3Pin's narrowing), bounded by
// the process's cgroup CPU quota
int uc::affinity_cpus() {
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof set, &set) != 0) return io::host_cpus();
  return std::max(1, std::min(CPU_COUNT(&set), io::host_cpus()));
}

// 8 resolve threads (4 beside other contexts), never more than the caller's affinity mask holds: the in-order
// phase's workers spin on each other's flags, so more threads than CPUs would only take slices from the worker
// the others wait on
int uc::pool_threads(const umiclust_ctx* c) {
  const int want = c->tun.resolve_threads > 0 ? c->tun.resolve_threads : (g_live_ctx.load() > 1 ? 4 : 8);
  return std::max(1, std::min(want, affinity_cpus()));
}

namespace {

struct L3Pin {
  cpu_set_t saved;
  bool on = false;
  umiclust_ctx* c = nullptr;
  explicit L3Pin(umiclust_ctx* ctx) : c(ctx) {
    if (!c->tun.pin || (g_live_ctx.load() > 1 && !c->tun.pin_forced) || sched_getaffinity(0, sizeof saved, &saved) != 0)
      return;
    // the pool is created with the caller's own mask before the caller is narrowed, so restoring `saved` on
    // both undoes the call's pinning completely
    if (!c->pool) c->pool.reset(new WorkPool(pool_threads(c)));
    const int cpu = sched_getcpu();
    char path[96], buf[256];
    snprintf(path, sizeof path, "/sys/devices/system/cpu/cpu%d/cache/index3/shared_cpu_list", cpu);
    FILE* f = cpu >= 0 ? fopen(path, "r") : nullptr;
    if (!f) return;
    const bool got = fgets(buf, sizeof buf, f) != nullptr;
    fclose(f);
    if (!got) return;
    cpu_set_t want;
    CPU_ZERO(&want);
    for (char* p = buf; *p;) {  // "a-b,c,d-e"
      char* e;
      const long a = strtol(p, &e, 10);
      if (e == p) break;
      long b = a;
      if (*e == '-') b = strtol(e + 1, &e, 10);
      for (long x = a; x <= b && x < CPU_SETSIZE; x++)
        if (CPU_ISSET((int)x, &saved)) CPU_SET((int)x, &want);
      p = *e == ',' ? e + 1 : e;
      if (*p == '\n') break;
    }
    if (CPU_COUNT(&want) == 0 || sched_setaffinity(0, sizeof want, &want) != 0) return;
    c->pool->set_affinity(want);
    on = true;
  }
  ~L3Pin() {
    if (!on) return;
    sched_setaffinity(0, sizeof saved, &saved);
    c->pool->set_affinity(saved);
  }
};

}  // namespace

// After its queued work; no other handle of the stream is kept (ix_st is st_b or null, events recorded on it have
// completed), and the old stream is destroyed once the new one is in place.
hipError_t uc::main_stream_priority(umiclust_ctx* c, int level) {
  if (c->st_level == level) return hipSuccess;
  int lo = 0, hi = 0;
  hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);
  Stream s;
  if (e == hipSuccess) e = hipStreamSynchronize(c->st);  // work queued since the caller's drain (memsets) first
  if (e == hipSuccess) e = level ? s.create(hipStreamNonBlocking, hi) : s.create(hipStreamNonBlocking);
  if (e != hipSuccess) return e;
  c->st = std::move(s);
  c->st_level = level;
  return hipSuccess;
}

// ---- member tracebacks and consensus: the launches ClusterRun and umiclust_consensus share.  Both work in the
// context's traceback / consensus buffers, on sequences the caller names by `ds`.
// the buffers for at most n members
void uc::ensure_traceback_buffers(umiclust_ctx* c, int32_t n) {
  alloc_each(c, (size_t)std::max(n, 1), c->h_mpq, c->h_mpt);
  alloc_each(c, n, c->t_mpq, c->t_mpt, c->t_mout);
  c->hip(c->t_ops.ensure((size_t)std::max(n, 1) * kOpsStride), "alloc");
  c->hip(c->t_nops.ensure(n), "alloc");
}

// The two launches of a TracePlan (plan.h) whose pairs are in h_mpq / h_mpt: ops, op counts and results go to the
// members' slots of t_ops / t_nops / t_mout.  maxl: the longest sequence any pair can hold.
void uc::launch_tracebacks(umiclust_ctx* c, const DevSeqs& ds, const Scoring& sc, const TracePlan& tp, int32_t maxl,
                           hipStream_t stq) {
  const int32_t x0 = tp.x0, nm1 = tp.x0 + tp.n1, nall = tp.n1 + tp.n2;
  if (nall == 0) return;
  c->hip(hipMemcpyAsync(c->t_mpq.p + x0, c->h_mpq.p + x0, (size_t)nall * 4, hipMemcpyHostToDevice, stq), "h2d");
  c->hip(hipMemcpyAsync(c->t_mpt.p + x0, c->h_mpt.p + x0, (size_t)nall * 4, hipMemcpyHostToDevice, stq), "h2d");
  c->hip(launch_traceback(ds, c->t_mpq.p + x0, c->t_mpt.p + x0, tp.n1, sc, c->t_ops.p + (size_t)x0 * kOpsStride,
                          c->t_nops.p + x0, c->t_mout.p + x0, stq, maxl, tp.maxq1),
         "traceback");
  c->hip(launch_traceback(ds, c->t_mpq.p + nm1, c->t_mpt.p + nm1, tp.n2, sc, c->t_ops.p + (size_t)nm1 * kOpsStride,
                          c->t_nops.p + nm1, c->t_mout.p + nm1, stq, maxl, tp.maxq2),
         "traceback");
}

// the pinned consensus inputs of n members in K clusters, for the caller to fill: h_cstart[K + 1], and per member in
// cluster order (centroid first) h_mseq (seqno), h_mops (traceback slot, a centroid's is not read), h_mstr (strand)
void uc::ensure_consensus_inputs(umiclust_ctx* c, int32_t n, int32_t K) {
  alloc_each(c, (size_t)std::max(n, 1), c->h_mseq, c->h_mops, c->h_mstr);
  c->hip(c->h_cstart.ensure((size_t)K + 1), "pin");
}

// Uploads those inputs, runs k_consensus on the main stream behind whatever wrote t_ops / t_nops (ev, if given, is
// recorded behind the kernel), downloads the lengths into h_clen and the sequences into h_craw (kConsCap bytes per
// cluster) and waits.  Returns the clusters whose MSA is wider than kMsaCols (their length is 0): the caller fails with
// kConsOverMsg.
int32_t uc::run_consensus(umiclust_ctx* c, const DevSeqs& ds, int32_t n, int32_t K, hipEvent_t ev) {
  c->hip(c->t_cstart.ensure((size_t)K + 1), "alloc");
  alloc_each(c, n, c->t_mseq, c->t_mops, c->t_mstrand);
  c->hip(c->t_cons.ensure((size_t)std::max(K, 1) * kConsCap), "alloc");
  c->hip(c->t_conslen.ensure((size_t)std::max(K, 1)), "alloc");
  c->hip(c->t_over.ensure(1), "alloc");
  c->hip(hipMemsetAsync(c->t_over.p, 0, 4, c->st), "memset");
  c->hip(hipMemcpyAsync(c->t_cstart.p, c->h_cstart.p, ((size_t)K + 1) * 4, hipMemcpyHostToDevice, c->st), "h2d");
  if (n > 0) {
    c->hip(hipMemcpyAsync(c->t_mseq.p, c->h_mseq.p, (size_t)n * 4, hipMemcpyHostToDevice, c->st), "h2d");
    c->hip(hipMemcpyAsync(c->t_mops.p, c->h_mops.p, (size_t)n * 4, hipMemcpyHostToDevice, c->st), "h2d");
    c->hip(hipMemcpyAsync(c->t_mstrand.p, c->h_mstr.p, (size_t)n, hipMemcpyHostToDevice, c->st), "h2d");
  }
  c->hip(launch_consensus(ds, c->t_cstart.p, K, c->t_mseq.p, c->t_mops.p, c->t_mstrand.p, c->t_ops.p, c->t_nops.p,
                          c->t_cons.p, c->t_conslen.p, c->t_over.p, c->st),
         "consensus");
  if (ev) c->hip(hipEventRecord(ev, c->st), "event");
  c->hip(c->h_clen.ensure((size_t)std::max(K, 1)), "pin");
  c->hip(c->h_craw.ensure((size_t)std::max(K, 1) * kConsCap), "pin");
  c->hip(c->h_over.ensure(1), "pin");
  if (K > 0) {
    c->hip(hipMemcpyAsync(c->h_clen.p, c->t_conslen.p, (size_t)K * 2, hipMemcpyDeviceToHost, c->st), "d2h");
    c->hip(hipMemcpyAsync(c->h_craw.p, c->t_cons.p, (size_t)K * kConsCap, hipMemcpyDeviceToHost, c->st), "d2h");
  }
  c->hip(hipMemcpyAsync(c->h_over.p, c->t_over.p, 4, hipMemcpyDeviceToHost, c->st), "d2h");
  c->hip(hipStreamSynchronize(c->st), "sync");
  return *c->h_over.p;
}

// ================================================================ ClusterRun (cluster_ctx.h): the steps of one call

// ---- step 1: a clean slate for the bin
void ClusterRun::reset_bin() {
  c->pack_on = npk > 1;
  c->cur_bin = bin;
  std::fill(c->cno.begin() + s0, c->cno.begin() + s1, -1);
  std::fill(c->strand.begin() + s0, c->strand.begin() + s1, 0);
  std::fill(c->target.begin() + s0, c->target.begin() + s1, -1);
  c->nclusters = 0;
  c->ix.reset(n);
  c->stats = umiclust_stats{};
  c->stats.n_input = c->bin_in[bin + npk] - c->bin_in[bin];
  if (c->pack_on) {
    for (int32_t b = bin; b < bin + npk; b++) c->h_bin_ord0.p[b] = INT32_MAX;  // no centroid of the bin indexed yet
    c->hip(hipMemcpyAsync(c->d_bin_ord0.p + bin, c->h_bin_ord0.p + bin, (size_t)npk * 4, hipMemcpyHostToDevice, c->st),
           "h2d bin ord0");
  }
  c->stats.n_kept = n;
  state_buf.assign((size_t)n, ST_UNDET);
  state = StateView{state_buf.data(), s0};
  if (c->tun.walk_dump) c->wd.assign((size_t)n * 4, -1);
}

// the block size and the pass buffers for it, then the bin's blocks
void ClusterRun::plan_blocks() {
  // blocks of at most B queries of one length (the aligner is compiled per query length); a block's
  // peer tile fills one kPeerRegion of the prefilter counters, so B <= kMaxBlock
  int32_t B = std::max(1, std::min<int32_t>(c->tun.block_size, kMaxBlock));
  if (c->tun.block_div > 0) B = std::min<int32_t>(B, std::max<int32_t>(kBlockMin, ((s1 - s0) / c->tun.block_div + 255) & ~255));
  c->pass_B = B;
  for (Pass& P : c->pass) ensure_pass_buffers(c, P, B);
  plan.hlen = c->hlen.data();
  plan.s0 = s0;
  plan.s1 = s1;
  plan.B = B;
  // blocks across length changes: bins below the full block size (config 3: 4.15 vs 3.61 M UMIs/s; a 2M-read bin
  // gains nothing, its length runs are many blocks long: profiles/r03/mixlen_ab.json)
  plan.mix = c->tun.mix_len > 0 || (c->tun.mix_len < 0 && (B < kMaxBlock || c->pack_on));
  plan.o4_T = T4;
  plan.hqbin = c->pack_on ? c->hqbin.data() : nullptr;
  plan.bin_s = c->bin_s.data();
  plan.regrow = c->tun.regrow;
  plan.start(c->b_hint);
}

void ClusterRun::alloc_traceback() {
  c->t_opsidx.assign(n, -1);  // member -> its traceback slot
  ensure_traceback_buffers(c, n);
  ds = dev_seqs(c);
  tw_maxl = traceback_maxl(c->hlen.data(), s0, s1);
}

// ---- the O4 round window
// Policy O4 batched rounds (T4 queries each, counted from the first sorted query of q's bin): query q's search
// sees only the centroids before its round start rstart(q), and the centroids of its round before it are the
// re-check's extras -- both must be in its pass's peer window, and the index must hold nothing from the round.
// Every pass that may still run or re-run counts: a queued pass is re-run alone when its block overflows a peer
// list (run_alone), against the index as it stands then.  So the index only ever holds the centroids before
// W = rstart(first query of the earliest block not yet resolved) -- the oldest window tile's first query -- and a
// *round tile* over [W, that query) joins the window in front of the nominal tiles; resolved centroids wait in
// `pending` until W has passed them.  (Round 4 synced the index to min(nominal window start, round start of the
// pass's own first query): when block k overflowed after pass k+1 had been queued, block k's re-run met centroids
// of its own first round in the index -- config 5 under --threads 25 aligned 15-50 more pairs than the oracle and
// moved reads between clusters, tests/test_gpu_o4.py::test_o4_config_vs_oracle_golden.)
int32_t ClusterRun::rstart(int32_t q) const { return round_start(c, s0, q); }
void ClusterRun::sync_index(int32_t X) {  // the index gets the pending centroids before seqno X
  size_t m = 0;
  while (m < pending.size() && pending[m] < X) m++;
  if (!m) return;
  std::vector<int32_t> a(pending.begin(), pending.begin() + (ptrdiff_t)m);
  c->ix.append(a);
  pending.erase(pending.begin(), pending.begin() + (ptrdiff_t)m);
}
// the window of a pass starting at query q with the nprev tiles prevs (oldest first), adjusted for the rounds:
// the round tile (counter region 2; the block tiles of the D = 2 ring use 0 and 1) goes in front
void ClusterRun::round_window(int32_t q, const Tile** prevs, int& nprev, int slot) {
  const int32_t first = nprev ? prevs[0]->base : q;
  const int32_t W = rstart(first);
  if (W < first) {
    Tile& rt = c->round_tile[slot & 1];
    build_tile(c, rt, c->d_iota.p, W, first - W, 0, (kPeerTiles - 1) * kPeerRegion, 1 << 30);
    rt.base = W;
    rt.seg = kPeerTiles - 1;
    rt.len = 0;  // several lengths
    rt.prebuilt = false;
    for (int i = nprev; i > 0; i--) prevs[i] = prevs[i - 1];
    prevs[0] = &rt;
    nprev++;
  }
  sync_index(W);
}

// ---- what both pipelines share
// the resolved block's (or prefix's) new centroids join the index -- under O4 once the window start has passed them
void ClusterRun::keep_new_cents() {
  if (T4) pending.insert(pending.end(), new_cents.begin(), new_cents.end());
  else c->ix.append(new_cents);
  c->stats.n_blocks++;
}
// block k is resolved: are the next passes lazy?  (`ahead`: the pass enqueued next is block k + ahead's)
void ClusterRun::count_lazy(int32_t k, int32_t ahead) {
  lazy = (int64_t)new_cents.size() * 1000 < (int64_t)plan.blocks[k].second * kLazyPermille;
  c->stats.n_lazy_passes += (lazy && k + ahead < plan.nb()) ? 1 : 0;
}
// A block whose peer list overflowed: re-run it alone (window = itself, index complete up to it)
// in halving pieces, synchronously.
void ClusterRun::run_alone(int32_t q0, int32_t nq) {
  Pass& P = c->pass[0];
  int32_t piece = nq;
  for (int32_t q = q0; q < q0 + nq;) {
    const int32_t m = std::min(piece, q0 + nq - q);
    const Tile* prevs[kPeerTiles];
    int nprev = 0;
    if (T4) round_window(q, prevs, nprev, 0);
    enqueue_pass(c, P, q, m, prevs, nprev, c->solo_tile, 0);
    c->stats.n_reruns++;
    int32_t done = 0;
    const bool all = resolve_pass(c, P, state, new_cents, t_pf, t_al, t_host, &done);
    if (done > 0) {  // the whole piece, or its prefix before the first overflowing query
      keep_new_cents();
      q += done;
    }
    if (!all && done == 0) {
      if (m == 1) c->fail(UMICLUST_EDEVICE, "peer overflow with block of 1");
      piece = std::max(1, m / 2);
    }
  }
}

// ---- step 2a: whole passes
// Software pipeline over blocks, D passes in flight: passes k+1 .. k+D-1 are queued before
// the host resolves block k.  Pass j runs against the index of the blocks before its peer window (blocks
// j-D+1 .. j), and the window covers every later query before block j's, so C_old u window = all queries
// before j: the merged walk is exact.  Invariant at the top of iteration k: passes k .. k+D-1 (those that
// exist) are queued, the index holds blocks < k.  Block k's peer tile lives in blk_tile[k % (D + 1)] (tile_of;
// read by passes k .. k+D-1) and counts into peer region k % D of the prefilter counters.
// enqueue block k's pass with the nprev blocks before it in its peer window
void ClusterRun::enqueue(int32_t k, int nprev) {
  const Tile* prevs[kPeerTiles];
  for (int i = 0; i < nprev; i++) prevs[i] = &tile_of(k - nprev + i);
  if (T4) round_window(plan.blocks[k].first, prevs, nprev, k);
  enqueue_pass(c, c->pass[k % D], plan.blocks[k].first, plan.blocks[k].second, prevs, nprev, tile_of(k), k % D, lazy);
}
// block k + D's peer tile depends on its queries only: build it now, while the host resolves block k (its ring
// slot was last read by pass k's prefilter).  Since round 6 on the side stream (after pass k's prefilter), so
// the build runs beside the main stream's counting instead of between two counting launches; the pass that
// next enqueues on the main stream waits for it (wait_index_and_tiles, pt_ev).  Before, it sat on the main stream.
void ClusterRun::prebuild_peer(int32_t k) {
  const auto& blk = plan.blocks[k + D];
  Tile& t = tile_of(k + D);
  hipStream_t bst = multi_bin ? nullptr : (hipStream_t)c->st_b;  // config 2 +1.6 %, multi-lane config 3 -2 %
  if (bst) {
    c->hip(hipStreamWaitEvent(bst, c->pass[k % D].ev[1], 0), "wait");
    c->pt_ev.get(c, hipEventDisableTiming);
  }
  build_tile(c, t, c->d_iota.p, blk.first, blk.second, 0, ((k + D) % D) * kPeerRegion, 1 << 30, bst);
  if (bst) {
    c->hip(hipEventRecord(c->pt_ev, bst), "event");
    c->pt_pending = true;
  }
  t.base = blk.first;
  t.seg = (k + D) % D;
  t.prebuilt = true;
}
void ClusterRun::run_whole() {
  for (int32_t i = 0; i < D && i < plan.nb(); i++) enqueue(i, i);
  for (int32_t k = 0; k < plan.nb(); k++) {
    Pass& P = c->pass[k % D];
    const double te0 = now_s();
    if (k + D < plan.nb()) prebuild_peer(k);
    c->dbg.t.enqueue += now_s() - te0;
    int32_t done = 0;
    if (!resolve_pass(c, P, state, new_cents, t_pf, t_al, t_host, &done)) {
      // drain the queued passes k+1 .. k+D-1 (their windows include block k) and restart the pipeline
      for (int i = 1; i < D; i++) {
        Pass& Q = c->pass[(k + i) % D];
        if (Q.live) {
          c->hip(hipEventSynchronize(Q.ev[4]), "sync");
          Q.live = false;
        }
      }
      // the block's prefix before its first overflowing query is resolved (its queries' peers are all earlier)
      if (done > 0) keep_new_cents();
      // an overflowing bin runs synchronous re-runs from here on: with other lanes sharing the GPU they queue behind
      // every lane's work unless its main stream goes first (config 4: a 792k-read bin with a giant molecule took
      // 7.2 s among 8 lanes, 0.6 s alone)
      run_alone(plan.blocks[k].first + done, plan.blocks[k].second - done);
      plan.overflowed(k);
      for (int i = 1; i <= D; i++)
        if (k + i < plan.nb()) enqueue(k + i, i - 1);
      continue;
    }
    keep_new_cents();
    count_lazy(k, D);
    if (plan.resolved(k, D, c->last_max_npeer)) {  // regrowth: the blocks from k + D on were re-cut
      c->stats.n_regrows++;
      tile_of(k + D).prebuilt = false;
    }
    const double te1 = now_s();
    if (k + D < plan.nb()) enqueue(k + D, D - 1);
    c->dbg.t.enqueue += now_s() - te1;
  }
}

// ---- step 2b: split passes
// Pass j = counting half A(j) (index of blocks <= j-3, window j-2 .. j with block j-2
// flagged) enqueued after block j-3 is resolved, and second half R(j) (the full kernel over A's
// overflowed units against index <= j-2 / window j-1 .. j, the merge keeping the flagged hits that are
// centroids, then walk / align / pack) after block j-2 is.  Block j's peer tile: blk_tile[j % 4] (stile),
// counter region j % 3 (three consecutive blocks share a counting window).
// Unlike run_whole, this loop never regrows the blocks (plan.resolved is not called, so the planner's clean count
// is never read here) and resolves without partial resolution: an overflowing block is re-run whole.
void ClusterRun::build_peer(int32_t j, bool side) {
  const auto& blk = plan.blocks[j];
  Tile& t = stile(j);
  const int32_t region = j % kPeerTiles;
  if (!(t.prebuilt && t.base == blk.first && t.n == blk.second && t.seg == region)) {
    hipStream_t bs = c->st;
    if (side && c->ix_st) {
      bs = c->ix_st;
      if (c->last_r_ev) c->hip(hipStreamWaitEvent(bs, c->last_r_ev, 0), "wait");
    }
    build_tile(c, t, c->d_iota.p, blk.first, blk.second, 0, region * kPeerRegion, 1 << 30, bs);
    if (bs != c->st) c->hip(hipEventRecord(c->ix_done.get(c), bs), "event");
  }
  t.base = blk.first;
  t.seg = region;
  t.len = c->hlen[blk.first];
  t.prebuilt = true;
}
// R(j) with the window's blocks from `first` (first = j - 1 in the steady state)
void ClusterRun::second_half(int32_t j, int32_t first, bool after_count, PfCapture* cap) {
  const Tile* prevs[kPeerTiles];
  int np = 0;
  for (int32_t i = first; i < j; i++) prevs[np++] = &stile(i);
  enqueue_pass(c, c->pass[j % 2], plan.blocks[j].first, plan.blocks[j].second, prevs, np, stile(j), j % kPeerTiles, lazy,
               after_count, cap);
}
void ClusterRun::count_half(int32_t j, int32_t first, int flag, PfCapture* cap) {
  const Tile* wins[kPeerTiles];
  int nw = 0;
  for (int32_t i = first; i <= j; i++) wins[nw++] = &stile(i);
  enqueue_count(c, c->pass[j % 2], plan.blocks[j].first, plan.blocks[j].second, wins, nw, flag, j % 4, cap);
}
// the index holds the blocks before r and nothing is queued: classic passes r (window r) and r+1 (window
// r, r+1), then A(r+2) with block r flagged
void ClusterRun::prime(int32_t r) {
  const int32_t nb = plan.nb();
  for (int32_t j = r; j < r + 3 && j < nb; j++) build_peer(j, false);
  if (r < nb) second_half(r, r, false);
  if (r + 1 < nb) second_half(r + 1, r, false);
  if (r + 2 < nb) count_half(r + 2, r, 0);
}
void ClusterRun::run_split() {
  prime(0);
  for (int32_t k = 0; k < plan.nb(); k++) {
    Pass& P = c->pass[k % 2];
    const double tb0 = now_s();
    if (k + 3 < plan.nb()) build_peer(k + 3, true);  // queries only: built while the host resolves block k
    c->dbg.t.enqueue += now_s() - tb0;
    if (!resolve_pass(c, P, state, new_cents, t_pf, t_al, t_host, nullptr)) {
      // drain everything queued (its windows include block k) and restart the pipeline after block k
      c->hip(hipStreamSynchronize(c->st_al), "sync");
      c->hip(hipStreamSynchronize(c->st_b), "sync");
      c->hip(hipStreamSynchronize(c->st), "sync");
      for (Pass& Q : c->pass) {
        Q.live = false;
        Q.a_live = false;
        c->hip(hipMemsetAsync(Q.d_anunits.p, 0, 4, c->st), "memset");
      }
      run_alone(plan.blocks[k].first, plan.blocks[k].second);
      plan.overflowed(k);
      for (Tile& t : c->blk_tile) t.prebuilt = false;
      prime(k + 1);
      continue;
    }
    const double ta0 = now_s();
    keep_new_cents();
    const double ta1 = now_s();
    count_lazy(k, 2);
    if (k + 2 < plan.nb()) second_half(k + 2, k + 1, true);
    if (k + 3 < plan.nb()) count_half(k + 3, k + 1, 0);
    c->dbg.t.appends += ta1 - ta0;          // UMICLUST_DEBUG: index appends (host side)
    c->dbg.t.enqueue += now_s() - ta1;      // and the next passes' enqueue
  }
}

// ---- step 2: cluster the blocks
void ClusterRun::run_pipeline() {
  // split passes shorten the host <-> device cycle of one bin at the price of a wider counting window;
  // multi-bin sets run several lanes on one GPU, which is throughput-bound: there the whole passes win
  // (configs 2 / 5: +12 % / +2 %, config 3: -6 %; profiles/r02/split_ab.json)
  const bool split = !T4 && (c->tun.split_env >= 0 ? c->tun.split_env != 0 : !multi_bin) && D == 2;
  c->ix_st = split ? (hipStream_t)c->st_b : nullptr;
  c->last_r_ev = nullptr;
  if (split) run_split();
  else run_whole();
  c->b_hint = plan.b_eff;
  // centroids still pending (O4): creation numbers only, no index is needed any more
  c->ix.add_unindexed(pending);
}

// ---- step 3: drain the streams; the main stream gets the caller's priority back
void ClusterRun::drain() {
  c->hip(hipStreamSynchronize(c->st_b), "sync");
  c->ix_st = nullptr;
  c->hip(hipStreamSynchronize(c->st_al), "sync");
  c->hip(hipStreamSynchronize(c->st), "sync");
  c->hip(main_stream_priority(c, c->prio_user), "stream priority");
  c->stats.t_index_s += c->ix.t_index_s();
}

// ---- step 4: member tracebacks
// tw_launch(lo, hi, stream) traces the members among seqnos [lo, hi) (their targets are final), queries of <= 64 nt
// in a launch of their own (a one-stripe direction store: more waves per CU; one launch for all measured equal:
// round 4 twsplit_ab/), appending to the pair arrays at tw_n; t_opsidx maps a member to its traceback slot.
// (Tracing the first blocks' members early on a least-priority stream while later blocks are clustered measured no
// faster: round 4 cumask_early_ab/.)
void ClusterRun::tw_launch(int32_t lo, int32_t hi, hipStream_t stq) {
  const TracePlan tp = plan_traceback(c->hlen.data(), c->target.data(), c->strand.data(), lo, hi, tw_n,
                                      c->t_opsidx.data() + (lo - s0), c->h_mpq.p, c->h_mpt.p);
  tw_n += tp.n1 + tp.n2;
  launch_tracebacks(c, ds, c->sc, tp, tw_maxl, stq);
}
// The tracebacks go first: their pairs (sorted seqno order) need only the targets, so the launch goes out
// before the host numbers the clusters, which then overlaps the traceback (round 4: the numbering and the
// pageable pair uploads were ~16 ms of idle GPU before the traceback of a 2M-read bin).
void ClusterRun::trace_members() {
  tw_launch(s0, s1, c->st);
  c->hip(hipEventRecord(c->tev[0].get(c), c->st), "event");
}

// ---- step 5: creation and output numbers (plan.h)
void ClusterRun::number() {
  c->nclusters = (int32_t)c->ix.cent.size();
  number_clusters(s0, s1, c->ix.cent, c->target.data(), c->p.clusterout_sort != 0, c->pack_on ? c->hqbin.data() : nullptr,
                  bin, npk, c->cno.data(), c->ocl.data(), c->num);
}

// ---- step 6: consensus (behind the traceback on the same stream) and its download
void ClusterRun::consensus() {
  const int32_t K = c->nclusters;
  // consensus inputs in output-cluster order (pinned: the uploads are queued, not staged)
  ensure_consensus_inputs(c, n, K);
  for (int32_t x = 0; x < n; x++) {
    const int32_t s = c->num.omemb[x];
    c->h_mseq.p[x] = s;
    c->h_mops.p[x] = c->t_opsidx[s - s0];
    c->h_mstr.p[x] = c->strand[s];
  }
  std::copy(c->num.ostart.begin(), c->num.ostart.end(), c->h_cstart.p);
  const int32_t over = run_consensus(c, ds, n, K, c->tev[1].get(c));
  const uint16_t* clen = c->h_clen.p;
  const char* craw = c->h_craw.p;
  t_cons = elapsed_s(c, c->tev[0], c->tev[1]);
  if (over) c->fail(UMICLUST_ERANGE, kConsOverMsg, over);
  c->cons_off.assign((size_t)K + 1, 0);
  for (int32_t k = 0; k < K; k++) c->cons_off[k + 1] = c->cons_off[k] + clen[k];
  c->cons.resize((size_t)c->cons_off[K]);
  for (int32_t k = 0; k < K; k++)
    memcpy(c->cons.data() + c->cons_off[k], craw + (size_t)k * kConsCap, clen[k]);
}

// ---- step 7: every bin keeps its own clusters' consensus sequences (umiclust_fetch_bin)
void ClusterRun::store_outputs() {
  for (int32_t b = bin; b < bin + npk; b++) {
    const int32_t k0 = c->num.bin_k[b - bin], k1 = c->num.bin_k[b - bin + 1];
    auto& bo = c->bout[b];
    bo.done = true;
    bo.K = k1 - k0;
    bo.cons_off.assign((size_t)bo.K + 1, 0);
    for (int32_t k = 0; k <= bo.K; k++) bo.cons_off[k] = c->cons_off[k0 + k] - c->cons_off[k0];
    bo.cons.assign(c->cons.begin() + c->cons_off[k0], c->cons.begin() + c->cons_off[k1]);
  }
}

// ---- step 8: the call's statistics and the measurement-only reports
void ClusterRun::report_pf_prof() {
  unsigned long long h[24];
  c->hip(hipMemcpy(h, c->pf_prof.p, sizeof(h), hipMemcpyDeviceToHost), "d2h");
  const double nwg = h[8] ? (double)h[8] : 1.0;
  fprintf(stderr,
          "prefilter phase clocks per workgroup (%llu): query %.0f views %.0f offsets %.0f table %.0f count %.0f "
          "scan %.0f select %.0f out %.0f\n",
          h[8], h[5] / nwg, h[6] / nwg, h[7] / nwg, h[0] / nwg, h[1] / nwg, h[2] / nwg, h[3] / nwg, h[4] / nwg);
  const double nc = h[14] ? (double)h[14] : 1.0;
  fprintf(stderr,
          "k_pf_count phase clocks per workgroup (%llu sampled): zero %.0f table %.0f count %.0f scan %.0f "
          "peers+out %.0f; chunks per workgroup %.1f; table = offsets %.0f + block scan %.0f + writes\n",
          h[14], h[9] / nc, h[10] / nc, h[11] / nc, h[12] / nc, h[13] / nc, h[15] / nc, h[16] / nc, h[17] / nc);
  if (h[19])
    fprintf(stderr, "k_pf_count sampled workgroups: %.0f shader cycles in %.2f us real time = %.2f GHz in the pipeline\n",
            h[18] / nc, h[19] / nc / 100.0, (double)h[18] / ((double)h[19] / 100e6) / 1e9);
  c->hip(hipMemset(c->pf_prof.p, 0, 24 * sizeof(unsigned long long)), "memset");
}
void ClusterRun::report_debug() const {  // UMICLUST_DEBUG: the per-bin summary
  const DebugSums& d = c->dbg;
  fprintf(stderr, "bin %d: n %d mispredicted %lld saved(seen) %lld blocked %lld deferred %lld\n", bin, n,
          (long long)d.mispredicted, (long long)d.saved, (long long)d.blocked, (long long)c->stats.n_deferred);
  fprintf(stderr, "bin %d: queries no-record %lld earlier-block-only %lld in-block %lld; pass-1 host %.3f s\n", bin,
          (long long)d.q_no_record, (long long)d.q_earlier_only, (long long)d.q_in_block, d.q_host_ns * 1e-9);
  fprintf(stderr, "bin %d: strands inline %lld many-relevant %lld record-read %lld peers-scanned %lld\n", bin,
          (long long)d.s_inline, (long long)d.s_many_relevant, (long long)d.s_record_read,
          (long long)d.s_peers_scanned);
  fprintf(stderr, "bin %d: resolve wait %.3f hq-copy %.3f rec-copy %.3f classify %.3f in-order %.3f total %.3f s "
          "(round B and the rest %.3f: round-B round trips %.3f, rest of resolve_block %.3f, outside it %.3f)\n", bin,
          d.t.wait, d.t.hq_copy, d.t.rec_copy, d.t.classify, d.t.inorder, d.t.total,
          d.t.total - d.t.wait - d.t.hq_copy - d.t.rec_copy - d.t.classify - d.t.inorder, d.t.round_b,
          d.t.resolve_block - d.t.classify - d.t.inorder - d.t.round_b,
          d.t.total - d.t.wait - d.t.hq_copy - d.t.rec_copy - d.t.resolve_block);
  fprintf(stderr, "bin %d: host: split-pass appends %.3f, enqueue (peer tiles, appends, launches) %.3f s; bin %.3f s\n",
          bin, d.t.appends, d.t.enqueue, now_s() - t0);
  fprintf(stderr, "bin %d: round B: %.0f round trips, %.0f launches, %.0f pairs, %.4f s between its first and last "
          "launch's events\n", bin, d.rb.trips, d.rb.launches, d.rb.pairs, d.rb.dev_s);
}
void ClusterRun::report() {
  c->stats.n_clusters = c->nclusters;
  c->stats.t_prefilter_s = t_pf;
  c->stats.t_align_s = t_al;
  c->stats.t_consensus_s = t_cons;
  c->stats.t_host_s = t_host;
  if (c->pf_prof.p) report_pf_prof();
  c->stats.t_total_s = now_s() - t0;
  c->clustered = true;
  if (c->tun.walk_dump && !c->wd.empty()) {
    if (FILE* f = fopen(c->tun.walk_dump, "wb")) {
      fwrite(c->wd.data(), 2, c->wd.size(), f);
      fclose(f);
    }
    c->wd.clear();
  }
  if (c->tun.debug) report_debug();
  c->dbg = DebugSums{};
}

// Cluster bin `bin` -- or, npk > 1, the pack of bins [bin, bin + npk) in one greedy order (each bin's queries in
// its own sorted order, the bins one after another: bins never interact, so this is every bin's own vsearch run):
// blocks then span bin boundaries and small bins share passes; the prefilter keeps only a query's own bin
// (PrefilterArgs::qbin) and the results are split per bin.
static void cluster_all(umiclust_ctx* c, int32_t bin, bool multi_bin, int32_t npk) {
  c->rec_direct = g_live_ctx.load() > 1;
  if (bin < 0 || npk < 1 || bin + npk >= (int32_t)c->bin_s.size())
    c->fail(UMICLUST_EINVAL, "bins [%d, %d) out of range", bin, bin + npk);
  ClusterRun r(c, bin, npk, multi_bin);
  r.reset_bin();
  r.plan_blocks();
  c->ix.layout(r.n, r.T4);
  r.alloc_traceback();
  r.run_pipeline();
  r.drain();
  r.trace_members();
  r.number();
  r.consensus();
  r.store_outputs();
  r.report();
}

void uc::cluster_pinned(umiclust_ctx* c, int32_t bin, bool multi_bin, int32_t npk) {
  L3Pin pin(c);  // only with one live context (a bin-set runner's lanes each own one: then it stays off)
  cluster_all(c, bin, multi_bin, npk);
}

uc::Ctx* uc::core(umiclust_ctx* c) { return c; }

umiclust_ctx::~umiclust_ctx() {
  join_release();
  (void)hipSetDevice(dev);
  if (counted) io::set_live_contexts(--g_live_ctx);
}

// what the three clustering entries share: the load must be there (`unloaded` names what is missing)
static int64_t cluster_entry(umiclust_ctx* c, const char* unloaded, int32_t bin, bool multi_bin, int32_t npk,
                             umiclust_stats* stats) {
  UC_GUARD(c, {
    if (!c->loaded) c->fail(UMICLUST_ESTATE, "%s", unloaded);
    if (!multi_bin && c->bin_s.size() != 2) c->fail(UMICLUST_EINVAL, "umiclust_cluster: the load holds several bins");
    cluster_pinned(c, bin, multi_bin, npk);
    if (stats) *stats = c->stats;
    return c->nclusters;
  });
}

// ====================================================================== C ABI
extern "C" {

int32_t umiclust_abi_version(void) { return UMICLUST_ABI_VERSION; }

// The alignment stream is created with the device's greatest stream priority: a pass's walk/align/pack chain gates
// the host's resolution of its block and through it the next passes.  A prioritised stream also gets a hardware
// queue of its own class instead of sharing the normal-priority queues with the other lanes' streams (config 3, 4
// lanes on one MI355X: 1.73 -> 3.1 M UMIs/s; least priority or a plain stream measured no better, round 4
// al_prio_ab/; a CU-masked stream slower, cumask_early_ab/).
static int al_priority() {
  int lo = 0, hi = 0;
  if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) return 0;
  if (env_debug()) fprintf(stderr, "stream priorities: least %d greatest %d\n", lo, hi);
  return hi;
}

umiclust_ctx* umiclust_create(int32_t device_id, int32_t* err) {
  // every early return: the context, if there is one, releases what it holds so far and gives its count back
  auto failed = [&](umiclust_ctx* c, int32_t code) -> umiclust_ctx* {
    delete c;
    if (err) *err = code;
    return nullptr;
  };
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev)
    return failed(nullptr, UMICLUST_EDEVICE);
  umiclust_ctx* c = new (std::nothrow) umiclust_ctx();
  if (!c) return failed(nullptr, UMICLUST_ENOMEM);
  c->dev = device_id;
  if (hipSetDevice(device_id) != hipSuccess || c->st.create(hipStreamNonBlocking) != hipSuccess ||
      c->st_b.create(hipStreamNonBlocking) != hipSuccess || c->st_copy.create(hipStreamNonBlocking) != hipSuccess ||
      c->st_al.create(hipStreamNonBlocking, al_priority()) != hipSuccess || c->ev0.create() != hipSuccess ||
      c->ev1.create() != hipSuccess || c->evb[0].create() != hipSuccess || c->evb[1].create() != hipSuccess || [&] {
        for (Pass& P : c->pass)
          for (Event& e : P.ev)
            if (e.create() != hipSuccess) return true;
        return false;
      }())
    return failed(c, UMICLUST_EDEVICE);
  warn_unknown_env();
  c->tun = read_tunables();
  io::set_live_contexts(++g_live_ctx);
  c->counted = true;
  if (c->tun.pf_prof &&
      (c->pf_prof.ensure(24) != hipSuccess || hipMemset(c->pf_prof.p, 0, 24 * sizeof(unsigned long long)) != hipSuccess))
    return failed(c, UMICLUST_EDEVICE);
  if (err) *err = UMICLUST_OK;
  return c;
}

int32_t umiclust_set_priority(umiclust_ctx* c, int32_t level) {
  if (!c || level < -1 || level > 1) return UMICLUST_EINVAL;
  if (hipSetDevice(c->dev) != hipSuccess || hipStreamSynchronize(c->st) != hipSuccess) return UMICLUST_EDEVICE;
  // level -1 (background): the alignment stream loses its priority too; 0 / 1 give it back
  const int al = level < 0 ? -1 : 0;
  if (al != c->al_level) {
    Stream s;
    if (hipStreamSynchronize(c->st_al) != hipSuccess ||
        (al < 0 ? s.create(hipStreamNonBlocking) : s.create(hipStreamNonBlocking, al_priority())) != hipSuccess)
      return UMICLUST_EDEVICE;
    c->st_al = std::move(s);  // (the old stream goes with `s`)
    c->al_level = al;
  }
  c->prio_user = level < 0 ? 0 : level;
  return main_stream_priority(c, c->prio_user) == hipSuccess ? UMICLUST_OK : UMICLUST_EDEVICE;
}

int32_t umiclust_wait_host(umiclust_ctx* c) {
  if (!c) return UMICLUST_EINVAL;
  c->join_release();
  return UMICLUST_OK;
}

void umiclust_destroy(umiclust_ctx* c) { delete c; }

const char* umiclust_last_error(const umiclust_ctx* c) { return c ? c->err.c_str() : "null context"; }

int32_t umiclust_load(umiclust_ctx* c, const umiclust_params* p, const char* seqs, const int64_t* offs,
                      int64_t n) {
  UC_GUARD(c, {
    for (int64_t i = 0; i < n; i++) {
      const int64_t L = offs[i + 1] - offs[i];
      if (p && L > kMaxLen && L <= p->maxseqlength) c->fail(UMICLUST_ERANGE, "sequence longer than %d", kMaxLen);
    }
    load_impl(c, p, seqs, offs, n);
    return UMICLUST_OK;
  });
}

int64_t umiclust_cluster(umiclust_ctx* c, umiclust_stats* stats) {
  return cluster_entry(c, "umiclust_cluster before umiclust_load", 0, false, 1, stats);
}

int64_t umiclust_fetch(umiclust_ctx* c, int32_t* cluster, uint8_t* strand, uint8_t* centroid, char* cons,
                       int64_t cons_cap, int64_t* cons_off) {
  if (!c) return UMICLUST_EINVAL;
  if (c->bin_s.size() != 2) {
    c->err = "umiclust_fetch: the load holds several bins (umiclust_fetch_bin)";
    return UMICLUST_EINVAL;
  }
  return umiclust_fetch_bin(c, 0, cluster, strand, centroid, cons, cons_cap, cons_off);
}

int64_t umiclust_fetch_bin(umiclust_ctx* c, int32_t bin, int32_t* cluster, uint8_t* strand, uint8_t* centroid,
                           char* cons, int64_t cons_cap, int64_t* cons_off) {
  UC_GUARD(c, {
    if (!c->loaded || bin < 0 || bin >= (int32_t)c->bout.size())
      c->fail(c->loaded ? UMICLUST_EINVAL : UMICLUST_ESTATE, "umiclust_fetch_bin: no such bin");
    const auto& bo = c->bout[bin];
    if (!bo.done) c->fail(UMICLUST_ESTATE, "umiclust_fetch_bin before the bin was clustered");
    const int64_t i0 = c->bin_in[bin], n = c->bin_in[bin + 1] - i0;
    if (cluster)
      for (int64_t i = 0; i < n; i++) cluster[i] = -1;
    if (strand) memset(strand, 0, (size_t)n);
    if (centroid) memset(centroid, 0, (size_t)n);
    for (int32_t s = c->bin_s[bin]; s < c->bin_s[bin + 1]; s++) {
      const int64_t i = c->perm[s] - i0;
      if (cluster) cluster[i] = c->ocl[s];
      if (strand) strand[i] = c->strand[s];
      if (centroid) centroid[i] = c->target[s] < 0 ? 1 : 0;
    }
    const int32_t K = bo.K;
    if (cons_off)
      for (int32_t k = 0; k <= K; k++) cons_off[k] = bo.cons_off[k];
    if (cons) {
      if ((int64_t)bo.cons.size() > cons_cap) c->fail(UMICLUST_EINVAL, "consensus buffer too small");
      memcpy(cons, bo.cons.data(), bo.cons.size());
    }
    return K;
  });
}

int32_t umiclust_stage(umiclust_ctx* c, const char* seqs, const int64_t* offs, int64_t n, const int64_t* bin_start,
                       int32_t nbins) {
  UC_GUARD(c, {
    stage_impl(c, seqs, offs, n, bin_start, bin_start ? nbins : 1);
    return UMICLUST_OK;
  });
}

int32_t umiclust_prepare(umiclust_ctx* c, const umiclust_params* p) {
  UC_GUARD(c, {
    prepare_impl(c, p);
    return UMICLUST_OK;
  });
}

int32_t umiclust_load_bins(umiclust_ctx* c, const umiclust_params* p, const char* seqs, const int64_t* offs,
                           int64_t n, const int64_t* bin_start, int32_t nbins) {
  UC_GUARD(c, {
    if (!bin_start || nbins < 1) c->fail(UMICLUST_EINVAL, "bin boundaries");
    load_impl(c, p, seqs, offs, n, bin_start, nbins);
    return UMICLUST_OK;
  });
}

int64_t umiclust_cluster_bin(umiclust_ctx* c, int32_t bin, umiclust_stats* stats) {
  return cluster_entry(c, "umiclust_cluster_bin before umiclust_load_bins", bin, true, 1, stats);
}

int64_t umiclust_cluster_pack(umiclust_ctx* c, int32_t first, int32_t nbins, umiclust_stats* stats) {
  return cluster_entry(c, "umiclust_cluster_pack before umiclust_load_bins", first, true, nbins, stats);
}

}  // extern "C"
