// probes.cpp -- the kernel-level entry points of the C ABI, for the test suite: one prefilter or one whole pass
// through the pipeline's own steps (umiclust_prefilter, umiclust_prefilter_pack, umiclust_prefilter_split,
// umiclust_pass, umiclust_resolve), and the alignment, consensus and preparation
// kernels on caller-given records (umiclust_align_pairs, umiclust_consensus, umiclust_prep, umiclust_prep_outputs), and
// the region overlap join's intermediate arrays (umiclust_overlap_probe).
#include <algorithm>
#include <cstddef>

#include "cluster_ctx.h"

using namespace uc;

// What umiclust_prefilter, its siblings and umiclust_pass share.  check_block_args: the refusals (`who` names the entry
// point); npk = 0 asks for a single-bin load, npk >= 1 names the pack [bin, bin + npk) of a umiclust_load_bins load,
// whose sorted seqno range then bounds the centroids and the window; max_cent is the largest index covered.
// stage_block: the pipeline's own steps up to the pass -- the bin's (or pack's) clean slate, arena and pass buffers
// (ClusterRun), Index::append in steps of append_step, and the window's peer tiles (ClusterRun::build_peer) with the
// window's blocks as the plan, oldest first, the block under test last (index nprev), as ClusterRun::prime enqueues a
// first pass.  With `split` the appends and the tile builds go to the side stream behind ix_done, as
// ClusterRun::run_split queues them in its steady state.
static void check_block_args(umiclust_ctx* c, const char* who, const int32_t* cent, int32_t ncent, int32_t q0, int32_t nq,
                      int32_t nprev, int32_t append_step, int32_t max_cent, int32_t bin = 0, int32_t npk = 0) {
  if (!c->loaded) c->fail(UMICLUST_ESTATE, "%s before umiclust_load", who);
  if (npk == 0 && c->bin_s.size() != 2) c->fail(UMICLUST_EINVAL, "%s: the load holds several bins", who);
  if (npk != 0 && (bin < 0 || npk < 1 || (int64_t)bin + npk >= (int64_t)c->bin_s.size()))
    c->fail(UMICLUST_EINVAL, "%s: bins [%d, %d) out of range", who, bin, bin + npk);
  if (c->o4_T) c->fail(UMICLUST_EINVAL, "%s: batched rounds (policy O4) are not covered", who);
  const int32_t s0 = npk ? c->bin_s[bin] : 0, s1 = npk ? c->bin_s[bin + npk] : c->n;
  if ((!cent && ncent > 0) || ncent < 0 || nq < 1 || nq > kMaxBlock || nprev < 0 || nprev > kPeerTiles - 1 ||
      append_step < 1 || q0 < s0 || (int64_t)q0 + nq > s1 || (int64_t)q0 - (int64_t)nprev * nq < s0)
    c->fail(UMICLUST_EINVAL, "%s: block, window or append step out of range", who);
  if (ncent > max_cent)
    c->fail(UMICLUST_EINVAL, "%s: more than %d counter segment(s)", who, (max_cent + kSegCentroids - 1) / kSegCentroids);
  const int32_t w0 = q0 - nprev * nq;
  for (int32_t i = 0; i < ncent; i++)
    if (cent[i] < (i ? cent[i - 1] + 1 : s0) || cent[i] >= w0)
      c->fail(UMICLUST_EINVAL, "%s: centroid seqnos must increase and precede the window", who);
  // packs: a bin's first sequence is its first centroid (Index::append opens the bin's ordinal range with it)
  for (int32_t i = 0; npk > 1 && i < ncent; i++) {
    const int32_t b = c->hqbin[cent[i]];
    if ((i == 0 || c->hqbin[cent[i - 1]] != b) && cent[i] != c->bin_s[b])
      c->fail(UMICLUST_EINVAL, "%s: centroids of bin %d without the bin's first sequence", who, b);
  }
  if (block_maxlen(c, q0, nq) - block_minlen(c, q0, nq) + 1 > kSegLens)
    c->fail(UMICLUST_EINVAL, "%s: block spans more than %d query lengths", who, kSegLens);
}
static void stage_block(umiclust_ctx* c, ClusterRun& r, const int32_t* cent, int32_t ncent, int32_t q0, int32_t nq,
                 int32_t nprev, int32_t append_step, bool split = false) {
  const int32_t w0 = q0 - nprev * nq;
  c->rec_direct = g_live_ctx.load() > 1;
  c->clustered = false;
  for (auto& bo : c->bout) bo.done = false;
  r.reset_bin();
  r.plan_blocks();
  c->ix.layout(r.n, r.T4);
  if (nq > c->pass_B)
    for (Pass& P : c->pass) ensure_pass_buffers(c, P, nq);
  c->ix_st = split ? (hipStream_t)c->st_b : nullptr;
  c->last_r_ev = nullptr;
  for (Pass& P : c->pass) P.live = P.a_live = false;
  std::vector<int32_t> step;
  for (int32_t i = 0; i < ncent; i += (int32_t)step.size()) {
    step.assign(cent + i, cent + std::min<int64_t>(ncent, (int64_t)i + append_step));
    c->ix.append(step);
  }
  r.plan.blocks.clear();
  for (int32_t j = 0; j <= nprev; j++) r.plan.blocks.push_back({w0 + j * nq, nq});
  for (int32_t j = 0; j <= nprev; j++) r.build_peer(j, split);
  c->hip(c->h_pf_nunits.ensure(1), "pin");
  c->h_pf_nunits.p[0] = 0;
}
static void sync_streams(umiclust_ctx* c) {
  c->hip(hipStreamSynchronize(c->st), "sync");
  c->hip(hipStreamSynchronize(c->st_al), "sync");
  c->hip(hipStreamSynchronize(c->st_b), "sync");
}
// the prefilter's lists of pass P and info[0..4], copied out
static void fetch_lists(umiclust_ctx* c, const Pass& P, const PfCapture& cap, size_t nqs, uint32_t* top_seqno,
                 uint8_t* top_count, uint8_t* ntop, uint16_t* peer_id, uint8_t* peer_count, uint8_t* npeer,
                 int64_t* info) {
  auto out = [&](void* dst, const void* src, size_t bytes) {
    if (dst) c->hip(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost), "d2h prefilter lists");
  };
  out(top_seqno, P.d_top_seqno.p, nqs * kTopHits * 4);
  out(top_count, P.d_top_count.p, nqs * kTopHits);
  out(ntop, P.d_ntop.p, nqs);
  out(peer_id, P.d_peer_id.p, nqs * kPeerCap * 2);
  out(peer_count, P.d_peer_count.p, nqs * kPeerCap);
  out(npeer, P.d_npeer.p, nqs);
  if (info) {
    info[0] = c->h_pf_nunits.p[0];
    info[1] = cap.ntiles;
    info[2] = cap.nseg;
    info[3] = cap.one_wave;
    info[4] = c->both;
  }
}
// the appends and tile builds go back to the main stream, whatever ends a split probe
struct SideStreamOff {
  umiclust_ctx* c;
  ~SideStreamOff() { c->ix_st = nullptr; }
};

// What umiclust_align_pairs, umiclust_consensus and umiclust_prep share: n records on the device, beside whatever load
// the context holds, and k_prep over them.  The uploads have completed when probe_prep returns, the kernel is queued.
// perm (n record indices, or null: the identity) names the record of each output row, as prepare_impl's sort does;
// with `changed` the per-row "output differs from input" flags are written too (they need `masked`).
struct ProbeSeqs {
  DevBuf<char> d_a, d_m;
  DevBuf<int64_t> d_o;
  DevBuf<int32_t> d_perm;
  DevBuf<uint32_t> d_codes, d_amb;
  DevBuf<uint8_t> d_lens, d_nk, d_chg;
  DevBuf<uint16_t> d_km;
  DevSeqs ds() const { return DevSeqs{d_codes.p, d_lens.p, d_km.p, d_nk.p}; }
};
static void probe_prep(umiclust_ctx* c, ProbeSeqs& S, const char* seqs, const int64_t* offs, int64_t n, int dust,
                       bool masked, bool amb, const int32_t* perm = nullptr, bool changed = false) {
  std::vector<int64_t> rel;
  upload_seqs(c, seqs, offs, n, S.d_a, S.d_o, rel, c->st);
  if (perm) {
    c->hip(S.d_perm.ensure((size_t)n + 1), "alloc");
    if (n > 0) c->hip(hipMemcpyAsync(S.d_perm.p, perm, (size_t)n * 4, hipMemcpyHostToDevice, c->st), "h2d");
  }
  c->hip(hipStreamSynchronize(c->st), "sync");  // `rel` goes out of scope
  c->hip(S.d_codes.ensure((size_t)n * 2 * kCodeWords + 1), "alloc");
  c->hip(S.d_lens.ensure((size_t)n + 1), "alloc");
  c->hip(S.d_km.ensure((size_t)n * 2 * kKmerStride + 1), "alloc");
  c->hip(S.d_nk.ensure((size_t)n * 2 + 1), "alloc");
  if (masked) c->hip(S.d_m.ensure((size_t)n * kMaxLen + 1), "alloc");
  if (changed) c->hip(S.d_chg.ensure((size_t)n + 1), "alloc");
  if (amb) {
    c->hip(S.d_amb.ensure(2), "alloc");
    c->hip(hipMemsetAsync(S.d_amb.p, 0, 8, c->st), "memset");
  }
  c->hip(launch_prep(S.d_a.p, S.d_o.p, perm ? S.d_perm.p : nullptr, (int32_t)n, dust, S.d_codes.p, S.d_lens.p,
                     S.d_km.p, S.d_nk.p, masked ? S.d_m.p : nullptr, amb ? S.d_amb.p : nullptr, c->st,
                     changed ? S.d_chg.p : nullptr),
         "prep");
}
// an alignment result word: matches, the alignment's internal length, the score
static void unpack_result(uint32_t r, int64_t k, int32_t* matches, int32_t* internal_len, int32_t* score) {
  if (matches) matches[k] = (int32_t)(r & 0xffu);
  if (internal_len) internal_len[k] = (int32_t)((r >> 8) & 0xffu);
  if (score) score[k] = (int32_t)(int16_t)(r >> 16);
}

// one whole pass (ClusterRun::second_half -> enqueue_pass) of the staged block and its lists: umiclust_prefilter and
// umiclust_prefilter_pack
static void whole_pass_lists(umiclust_ctx* c, ClusterRun& r, const int32_t* cent, int32_t ncent, int32_t q0, int32_t nq,
                             int32_t nprev, int32_t append_step, uint32_t* top_seqno, uint8_t* top_count, uint8_t* ntop,
                             uint16_t* peer_id, uint8_t* peer_count, uint8_t* npeer, int64_t* info) {
  stage_block(c, r, cent, ncent, q0, nq, nprev, append_step);
  PfCapture cap;
  cap.h_nunits = c->h_pf_nunits.p;
  r.second_half(nprev, 0, false, &cap);
  Pass& P = c->pass[nprev % 2];
  sync_streams(c);
  P.live = false;
  fetch_lists(c, P, cap, (size_t)nq * c->both, top_seqno, top_count, ntop, peer_id, peer_count, npeer, info);
}

static_assert(sizeof(umiclust_pass_qs) == sizeof(HostQs) && offsetof(umiclust_pass_qs, rel) == offsetof(HostQs, rel) &&
                  offsetof(umiclust_pass_qs, nrel) == offsetof(HostQs, nrel) &&
                  offsetof(umiclust_pass_qs, npeer) == offsetof(HostQs, npeer),
              "umiclust_pass_qs mirrors HostQs");
static_assert(sizeof(umiclust_pass_walk) == sizeof(WalkState) &&
                  offsetof(umiclust_pass_walk, best_rank) == offsetof(WalkState, best_rank) &&
                  offsetof(umiclust_pass_walk, e) == offsetof(WalkState, e),
              "umiclust_pass_walk mirrors WalkState");

extern "C" {

// The prefilter of one block against a caller-chosen index and peer window, through the pipeline's own steps
// (stage_block) and one whole pass (ClusterRun::second_half -> enqueue_pass) whose top and peer lists are copied out.
// The walk and alignments the pass also enqueues run and are dropped.
int32_t umiclust_prefilter(umiclust_ctx* c, const int32_t* cent, int32_t ncent, int32_t q0, int32_t nq, int32_t nprev,
                           int32_t append_step, uint32_t* top_seqno, uint8_t* top_count, uint8_t* ntop,
                           uint16_t* peer_id, uint8_t* peer_count, uint8_t* npeer, int64_t* info) {
  UC_GUARD(c, {
    check_block_args(c, "umiclust_prefilter", cent, ncent, q0, nq, nprev, append_step, kMaxSegs * kSegCentroids);
    ClusterRun r(c, 0, 1, false);
    whole_pass_lists(c, r, cent, ncent, q0, nq, nprev, append_step, top_seqno, top_count, ntop, peer_id, peer_count,
                     npeer, info);
    return UMICLUST_OK;
  });
}

// The same on a pack of a multi-bin load: ClusterRun over the bins [first_bin, first_bin + nbins), so the queries see
// the scrambled k-mers, the per-bin cuts of the counter sweeps and the centroid length table as a clustering of the
// pack does.
int32_t umiclust_prefilter_pack(umiclust_ctx* c, int32_t first_bin, int32_t nbins, const int32_t* cent, int32_t ncent,
                                int32_t q0, int32_t nq, int32_t nprev, int32_t append_step, uint32_t* top_seqno,
                                uint8_t* top_count, uint8_t* ntop, uint16_t* peer_id, uint8_t* peer_count,
                                uint8_t* npeer, int64_t* info) {
  UC_GUARD(c, {
    if (c->loaded && nbins < 1)
      c->fail(UMICLUST_EINVAL, "umiclust_prefilter_pack: bins [%d, %d) out of range", first_bin, first_bin + nbins);
    check_block_args(c, "umiclust_prefilter_pack", cent, ncent, q0, nq, nprev, append_step, kSegCentroids, first_bin,
                     nbins);
    ClusterRun r(c, first_bin, nbins, true);
    whole_pass_lists(c, r, cent, ncent, q0, nq, nprev, append_step, top_seqno, top_count, ntop, peer_id, peer_count,
                     npeer, info);
    return UMICLUST_OK;
  });
}

// A split pass in ClusterRun::run_split's steady state: the blocks j-2 = [w0, w0 + nq), j-1 and j = [w0 + 2 nq,
// w0 + 3 nq); the counting half of block j with block j-2 flagged, the append of block j-2's new centroids, then
// the second half of block j with the window j-1 .. j.  One synchronisation, at the end: the order of the halves,
// the append and the fold it may bring rests on the events the pipeline itself records.
int32_t umiclust_prefilter_split(umiclust_ctx* c, const int32_t* cent, int32_t ncent, const int32_t* newcent,
                                 int32_t nnew, int32_t w0, int32_t nq, int32_t append_step, uint32_t* top_seqno,
                                 uint8_t* top_count, uint8_t* ntop, uint16_t* peer_id, uint8_t* peer_count,
                                 uint8_t* npeer, int64_t* info) {
  UC_GUARD(c, {
    const char* who = "umiclust_prefilter_split";
    if (c->loaded && (w0 < 0 || w0 > c->n || nq < 1 || nq > kMaxBlock))
      c->fail(UMICLUST_EINVAL, "%s: block, window or append step out of range", who);
    const int32_t q0 = c->loaded ? w0 + 2 * nq : 0;
    check_block_args(c, who, cent, ncent, q0, nq, 2, append_step, kSegCentroids);
    if ((!newcent && nnew > 0) || nnew < 0) c->fail(UMICLUST_EINVAL, "%s: new centroids", who);
    for (int32_t i = 0; i < nnew; i++)
      if (newcent[i] < (i ? newcent[i - 1] + 1 : w0) || newcent[i] >= w0 + nq)
        c->fail(UMICLUST_EINVAL, "%s: new centroid seqnos must increase inside the window's oldest block", who);
    // (the counting half of an index past one counter segment is skipped: enqueue_count)
    if ((int64_t)ncent + nnew > kSegCentroids) c->fail(UMICLUST_EINVAL, "%s: more than one counter segment", who);
    ClusterRun r(c, 0, 1, false);
    SideStreamOff off{c};
    stage_block(c, r, cent, ncent, q0, nq, 2, append_step, true);
    PfCapture cap;
    cap.h_nunits = c->h_pf_nunits.p;
    r.count_half(2, 0, 0, &cap);
    c->ix.append(std::vector<int32_t>(newcent, newcent + nnew));
    r.second_half(2, 1, true, &cap);
    Pass& P = c->pass[0];
    sync_streams(c);
    P.live = false;
    fetch_lists(c, P, cap, (size_t)nq * c->both, top_seqno, top_count, ntop, peer_id, peer_count, npeer, info);
    if (info) {
      info[5] = cap.ntiles_count;
      info[6] = c->ix.base_end;
    }
    return UMICLUST_OK;
  });
}

// The same pass with everything the host's resolve step reads of it copied out (the walk, the peer pairs and k_pack
// against tests/pass_ref.py).  With UMICLUST_PASS_PREV the pass of the block before is queued first on the other
// buffer set, unresolved, as ClusterRun's pipelines queue consecutive passes; without it the other buffer sets are
// marked unused, so enqueue_pass's search for the block before (Q.q0 + Q.nq == q0) finds nothing an earlier
// clustering left behind.
int32_t umiclust_pass(umiclust_ctx* c, const int32_t* cent, int32_t ncent, int32_t q0, int32_t nq, int32_t nprev,
                      int32_t append_step, uint32_t flags, uint32_t* top_seqno, uint8_t* top_count, uint8_t* ntop,
                      uint16_t* peer_id, uint8_t* peer_count, uint8_t* npeer, umiclust_pass_qs* hostqs, uint32_t* rec,
                      int64_t rec_cap, int64_t* rec_total, uint32_t* res, uint64_t* aligned, umiclust_pass_walk* walk,
                      uint32_t* counters, int64_t* info) {
  UC_GUARD(c, {
    check_block_args(c, "umiclust_pass", cent, ncent, q0, nq, nprev, append_step, kSegCentroids);
    if (flags & ~(UMICLUST_PASS_LAZY | UMICLUST_PASS_PREV)) c->fail(UMICLUST_EINVAL, "umiclust_pass: unknown flag");
    if ((flags & UMICLUST_PASS_PREV) && nprev < 1)
      c->fail(UMICLUST_EINVAL, "umiclust_pass: the previous block's pass needs nprev >= 1");
    if (rec_cap < 0) c->fail(UMICLUST_EINVAL, "umiclust_pass: record buffer");
    ClusterRun r(c, 0, 1, false);
    // The set-up re-plans the bin, after which every buffer set zeroes its counters with a memset (ensure_pass_buffers).
    // A set whose last k_pack re-zeroed them, and whose counters were not reallocated, keeps that knowledge here: its
    // next pass takes the no-memset path, as every pass after a bin's first ones does in a clustering call (every
    // stream is drained first, so the counters are as that k_pack left them).
    const uint32_t* ctr_p[kPeerTiles];
    bool ctr_z[kPeerTiles];
    for (int i = 0; i < kPeerTiles; i++) {
      ctr_p[i] = c->pass[i].d_counters.p;
      ctr_z[i] = c->pass[i].ctr_zeroed;
    }
    stage_block(c, r, cent, ncent, q0, nq, nprev, append_step);
    sync_streams(c);
    for (int i = 0; i < kPeerTiles; i++)
      if (ctr_p[i] && c->pass[i].d_counters.p == ctr_p[i]) c->pass[i].ctr_zeroed = ctr_z[i];
    r.lazy = (flags & UMICLUST_PASS_LAZY) != 0;
    Pass& P = c->pass[nprev % 2];
    for (Pass& Q : c->pass)
      if (&Q != &P) Q.nq = 0;
    if (flags & UMICLUST_PASS_PREV) r.second_half(nprev - 1, 0, false);
    PfCapture cap;
    cap.h_nunits = c->h_pf_nunits.p;
    r.second_half(nprev, 0, false, &cap);
    sync_streams(c);
    for (Pass& Q : c->pass) Q.live = false;
    const size_t nqs = (size_t)nq * c->both;
    fetch_lists(c, P, cap, nqs, top_seqno, top_count, ntop, peer_id, peer_count, npeer, info);
    auto out = [&](void* dst, const void* src, size_t bytes) {
      if (dst && bytes) c->hip(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost), "d2h pass");
    };
    if (hostqs) memcpy(hostqs, P.h_hq.p, nqs * sizeof(HostQs));  // pinned: written by k_pack or copied by the pass
    const int64_t total = *P.h_reccount.p;
    if (rec_total) *rec_total = total;
    if (rec) {
      const size_t nw = (size_t)std::min<int64_t>(total, rec_cap);
      if (P.rec_direct) memcpy(rec, P.h_rec.p, nw * 4);
      else out(rec, P.d_rec.p, nw * 4);
    }
    out(res, P.d_res.p, nqs * (kWalk + kPeerCap) * 4);
    out(aligned, P.d_paligned.p, nqs * (kPeerCap / 64) * 8);
    out(walk, P.d_ws.p, nqs * sizeof(WalkState));
    if (counters) memcpy(counters, P.h_counters.p, 16 * 4);
    if (rec && total > rec_cap) c->fail(UMICLUST_ERANGE, "umiclust_pass: %lld record words, room for %lld",
                                         (long long)total, (long long)rec_cap);
    return UMICLUST_OK;
  });
}

// The same pass, queued and then resolved by the pipeline's own resolve_pass (pass.cpp): resolve_block on the pass's
// outcomes and records with the window's states as given, round B on the device, on the copy stream (the resolve step
// against tests/resolve_ref.py).  The bin's states before the window are members (never read), the block's
// undetermined; with UMICLUST_RESOLVE_PARTIAL resolve_pass may resolve the prefix before the first overflowing query,
// as ClusterRun::run_whole asks it to.
int32_t umiclust_resolve(umiclust_ctx* c, const int32_t* cent, int32_t ncent, int32_t q0, int32_t nq, int32_t nprev,
                         int32_t append_step, uint32_t flags, const uint8_t* win_state, uint8_t* state,
                         int32_t* target, uint8_t* strand, int32_t* new_cents, int64_t* info) {
  UC_GUARD(c, {
    check_block_args(c, "umiclust_resolve", cent, ncent, q0, nq, nprev, append_step, kSegCentroids);
    if (flags & ~(UMICLUST_PASS_LAZY | UMICLUST_PASS_PREV | UMICLUST_RESOLVE_PARTIAL))
      c->fail(UMICLUST_EINVAL, "umiclust_resolve: unknown flag");
    if ((flags & UMICLUST_PASS_PREV) && nprev < 1)
      c->fail(UMICLUST_EINVAL, "umiclust_resolve: the previous block's pass needs nprev >= 1");
    const int32_t w0 = q0 - nprev * nq;
    if (!win_state && q0 > w0) c->fail(UMICLUST_EINVAL, "umiclust_resolve: the window's states");
    for (int32_t x = w0; x < q0; x++)
      if (win_state[x - w0] != ST_CENT && win_state[x - w0] != ST_MEMBER)
        c->fail(UMICLUST_EINVAL, "umiclust_resolve: window query %d is neither a centroid (1) nor a member (2)", x);
    ClusterRun r(c, 0, 1, false);
    const uint32_t* ctr_p[kPeerTiles];  // (as umiclust_pass: the buffer sets' zeroed counters stay known)
    bool ctr_z[kPeerTiles];
    for (int i = 0; i < kPeerTiles; i++) {
      ctr_p[i] = c->pass[i].d_counters.p;
      ctr_z[i] = c->pass[i].ctr_zeroed;
    }
    stage_block(c, r, cent, ncent, q0, nq, nprev, append_step);
    sync_streams(c);
    for (int i = 0; i < kPeerTiles; i++)
      if (ctr_p[i] && c->pass[i].d_counters.p == ctr_p[i]) c->pass[i].ctr_zeroed = ctr_z[i];
    r.lazy = (flags & UMICLUST_PASS_LAZY) != 0;
    Pass& P = c->pass[nprev % 2];
    for (Pass& Q : c->pass)
      if (&Q != &P) Q.nq = 0;
    std::fill(r.state_buf.begin(), r.state_buf.begin() + w0, (uint8_t)ST_MEMBER);
    std::copy(win_state, win_state + (q0 - w0), r.state_buf.begin() + w0);
    if (flags & UMICLUST_PASS_PREV) r.second_half(nprev - 1, 0, false);
    r.second_half(nprev, 0, false);
    const auto rb0 = c->dbg.rb;
    int32_t done = 0;
    const bool all = resolve_pass(c, P, r.state, r.new_cents, r.t_pf, r.t_al, r.t_host,
                                  (flags & UMICLUST_RESOLVE_PARTIAL) ? &done : nullptr);
    if (!(flags & UMICLUST_RESOLVE_PARTIAL)) done = all ? nq : 0;
    sync_streams(c);
    c->hip(hipStreamSynchronize(c->st_copy), "sync");
    for (Pass& Q : c->pass) Q.live = false;
    for (int32_t i = 0; i < nq; i++) {
      if (state) state[i] = r.state[q0 + i];
      if (target) target[i] = c->target[(size_t)(q0 + i)];
      if (strand) strand[i] = c->strand[(size_t)(q0 + i)];
    }
    const int64_t nc = done > 0 ? (int64_t)r.new_cents.size() : 0;
    if (new_cents) std::copy(r.new_cents.begin(), r.new_cents.begin() + nc, new_cents);
    if (info) {
      info[0] = done;
      info[1] = all ? 1 : 0;
      info[2] = nc;
      info[3] = c->stats.n_alignments;
      info[4] = c->stats.cells;
      info[5] = c->stats.n_merged_walks;
      info[6] = c->stats.n_deferred;
      info[7] = c->stats.pairs_round_b;
      info[8] = (int64_t)(c->dbg.rb.trips - rb0.trips);
      info[9] = (int64_t)(c->dbg.rb.launches - rb0.launches);
      info[10] = (int64_t)(c->dbg.rb.pairs - rb0.pairs);
      info[11] = c->both;
      info[12] = (int64_t)(c->dbg.rb.staged - rb0.staged);
    }
    return UMICLUST_OK;
  });
}

int32_t umiclust_align_pairs(umiclust_ctx* c, const umiclust_params* p, const char* q, const int64_t* q_off,
                             const char* t, const int64_t* t_off, int64_t npairs, int32_t* score,
                             int32_t* matches, int32_t* internal_len, char* cigar_ops, int32_t ops_stride,
                             int32_t* ops_len) {
  UC_GUARD(c, {
    if (!p || npairs < 0 || (npairs > 0 && (!q || !q_off || !t || !t_off))) c->fail(UMICLUST_EINVAL, "null argument");
    umiclust_params pp = *p;
    pp.minseqlength = 1;
    pp.maxseqlength = kMaxLen;
    validate(c, pp);
    // load queries then targets as one sequence set without filtering/sorting
    std::vector<char> all;
    std::vector<int64_t> off{0};
    append_set(q, q_off, npairs, all, off);
    append_set(t, t_off, npairs, all, off);
    const int64_t ns = 2 * npairs;
    for (int64_t i = 0; i < ns; i++)
      if (off[i + 1] - off[i] < 1 || off[i + 1] - off[i] > kMaxLen) c->fail(UMICLUST_ERANGE, "pair sequence length");
    Scoring sc = to_scoring(pp);
    ProbeSeqs S;
    DevBuf<uint32_t> d_pq, d_pt, d_out;
    DevBuf<uint8_t> d_ops;
    DevBuf<uint16_t> d_nops;
    probe_prep(c, S, all.data(), off.data(), ns, 0, false, true);
    uint32_t amb = 0;
    c->hip(hipMemcpyAsync(&amb, S.d_amb.p, 4, hipMemcpyDeviceToHost, c->st), "d2h");
    c->hip(hipStreamSynchronize(c->st), "sync");
    // pairs grouped by query length (the aligner is compiled per query length)
    std::vector<int64_t> ord(npairs);
    for (int64_t k = 0; k < npairs; k++) {
      ord[k] = k;
      const int64_t ql = off[k + 1] - off[k];
      if (ql < kMinTplLen) c->fail(UMICLUST_ERANGE, "query shorter than %d", kMinTplLen);
    }
    std::stable_sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) {
      return (off[a + 1] - off[a]) < (off[b + 1] - off[b]);
    });
    std::vector<uint32_t> pq(npairs), pt(npairs);
    for (int64_t x = 0; x < npairs; x++) {
      pq[x] = (uint32_t)ord[x] << 1;
      pt[x] = (uint32_t)(npairs + ord[x]);
    }
    c->hip(d_pq.ensure(npairs + 1), "alloc");
    c->hip(d_pt.ensure(npairs + 1), "alloc");
    c->hip(d_out.ensure(npairs + 1), "alloc");
    if (npairs > 0) {
      c->hip(hipMemcpyAsync(d_pq.p, pq.data(), npairs * 4, hipMemcpyHostToDevice, c->st), "h2d");
      c->hip(hipMemcpyAsync(d_pt.p, pt.data(), npairs * 4, hipMemcpyHostToDevice, c->st), "h2d");
    }
    const DevSeqs ds = S.ds();
    std::vector<uint32_t> sres(npairs);
    std::vector<uint8_t> ops;
    std::vector<uint16_t> nops;
    if (cigar_ops) {
      if (ops_stride < kOpsStride) c->fail(UMICLUST_EINVAL, "ops_stride < %d", kOpsStride);
      c->hip(d_ops.ensure((size_t)npairs * kOpsStride + 1), "alloc");
      c->hip(d_nops.ensure(npairs + 1), "alloc");
    }
    for (int64_t b0 = 0; b0 < npairs;) {
      const int32_t ql = (int32_t)(off[ord[b0] + 1] - off[ord[b0]]);
      int64_t e = b0 + 1;
      while (e < npairs && off[ord[e] + 1] - off[ord[e]] == ql) e++;
      if (cigar_ops)
        c->hip(launch_traceback(ds, d_pq.p + b0, d_pt.p + b0, (int32_t)(e - b0), sc, d_ops.p + (size_t)b0 * kOpsStride,
                                d_nops.p + b0, d_out.p + b0, c->st, kMaxLen),
               "traceback");
      else
        c->hip(launch_align(ds, ql, amb != 0, d_pq.p + b0, d_pt.p + b0, (int32_t)(e - b0), nullptr, nullptr, sc,
                            d_out.p + b0, c->st, c->tun.band_pairs),
               "align");
      b0 = e;
    }
    if (npairs > 0)
      c->hip(hipMemcpyAsync(sres.data(), d_out.p, (size_t)npairs * 4, hipMemcpyDeviceToHost, c->st), "d2h");
    if (cigar_ops) {
      ops.resize((size_t)npairs * kOpsStride);
      nops.resize(npairs);
      c->hip(hipMemcpyAsync(ops.data(), d_ops.p, ops.size(), hipMemcpyDeviceToHost, c->st), "d2h");
      c->hip(hipMemcpyAsync(nops.data(), d_nops.p, (size_t)npairs * 2, hipMemcpyDeviceToHost, c->st), "d2h");
    }
    c->hip(hipStreamSynchronize(c->st), "sync");
    std::vector<uint32_t> res(npairs);
    for (int64_t x = 0; x < npairs; x++) {
      const int64_t k = ord[x];
      res[k] = sres[x];
      if (cigar_ops) {
        const int n = nops[x];
        memcpy(cigar_ops + (size_t)k * ops_stride, ops.data() + (size_t)x * kOpsStride + kOpsStride - n, (size_t)n);
        if (ops_len) ops_len[k] = n;
      }
    }
    for (int64_t k = 0; k < npairs; k++) unpack_result(res[k], k, matches, internal_len, score);
    return UMICLUST_OK;
  });
}

int32_t umiclust_consensus(umiclust_ctx* c, const umiclust_params* p, const char* seqs, const int64_t* offsets,
                           int64_t n, const int32_t* cstart, int32_t nclusters, const int32_t* member,
                           const uint8_t* member_strand, const char* ops_in, const int32_t* ops_in_len,
                           int32_t ops_stride, char* ops_out, int32_t* ops_out_len, int32_t* score, int32_t* matches,
                           int32_t* internal_len, char* cons, int64_t cons_cap, int64_t* cons_off) {
  UC_GUARD(c, {
    if (!p || n < 0 || nclusters < 0 || (n > 0 && (!seqs || !offsets)) ||
        (nclusters > 0 && (!cstart || !member || !member_strand)) || (ops_in && !ops_in_len) ||
        (ops_out && !ops_out_len))
      c->fail(UMICLUST_EINVAL, "null argument");
    if (n > (1 << 30)) c->fail(UMICLUST_ERANGE, "too many records");
    if ((ops_in || ops_out) && ops_stride < kOpsStride) c->fail(UMICLUST_EINVAL, "ops_stride < %d", kOpsStride);
    umiclust_params pp = *p;
    pp.minseqlength = 1;
    pp.maxseqlength = kMaxLen;
    validate(c, pp);
    const Scoring sc = to_scoring(pp);
    const int32_t ns = (int32_t)n, K = nclusters;
    std::vector<uint8_t> hlen((size_t)ns);  // the records' lengths
    for (int32_t i = 0; i < ns; i++) {
      const int64_t L = offsets[i + 1] - offsets[i];
      if (L < 1 || L > kMaxLen) c->fail(UMICLUST_ERANGE, "record %d: length %lld outside 1..%d", i, (long long)L, kMaxLen);
      hlen[i] = (uint8_t)L;
    }
    // the clusters: every record in at most one, its centroid first
    if (K > 0 && cstart[0] != 0) c->fail(UMICLUST_EINVAL, "cstart[0] must be 0");
    for (int32_t k = 0; k < K; k++)
      if (cstart[k + 1] <= cstart[k]) c->fail(UMICLUST_EINVAL, "cluster %d is empty", k);
    const int32_t nm = K > 0 ? cstart[K] : 0;  // member entries
    std::vector<int32_t> target((size_t)ns, -1);
    std::vector<uint8_t> strand((size_t)ns, 0), seen((size_t)ns, 0);
    for (int32_t k = 0; k < K; k++)
      for (int32_t x = cstart[k]; x < cstart[k + 1]; x++) {
        const int32_t r = member[x];
        if (r < 0 || r >= ns) c->fail(UMICLUST_EINVAL, "cluster %d: record %d out of range", k, r);
        if (seen[r]) c->fail(UMICLUST_EINVAL, "record %d is listed twice", r);
        seen[r] = 1;
        if (x > cstart[k]) {
          target[r] = member[cstart[k]];
          strand[r] = member_strand[x] ? 1 : 0;
        }
      }
    // given ops: the consensus kernel indexes its LDS by their counts, so nothing invalid may reach the device
    if (ops_in)
      for (int32_t k = 0; k < K; k++)
        for (int32_t x = cstart[k] + 1; x < cstart[k + 1]; x++) {
          const int32_t len = ops_in_len[x];
          if (len < 0 || len > kOpsStride) c->fail(UMICLUST_EINVAL, "member %d: %d ops (at most %d)", x, len, kOpsStride);
          const char* o = ops_in + (size_t)x * ops_stride;
          int32_t nM = 0, nD = 0, nI = 0;
          for (int32_t y = 0; y < len; y++) {
            if (o[y] == 'M') nM++;
            else if (o[y] == 'D') nD++;
            else if (o[y] == 'I') nI++;
            else c->fail(UMICLUST_EINVAL, "member %d: op %d is not one of M D I", x, y);
          }
          if (nM + nI != hlen[member[cstart[k]]] || nM + nD != hlen[member[x]])
            c->fail(UMICLUST_EINVAL, "member %d: ops cover %d centroid and %d member residues, not %d and %d", x, nM + nI,
                    nM + nD, (int)hlen[member[cstart[k]]], (int)hlen[member[x]]);
        }
    // the sequences' codes, beside whatever load the context holds
    ProbeSeqs S;
    probe_prep(c, S, seqs, offsets, ns, 0, false, true);
    const DevSeqs ds = S.ds();
    // slots and launches as ClusterRun::tw_launch plans them, records standing for the sorted seqnos
    ensure_traceback_buffers(c, ns);
    std::vector<int32_t> slot((size_t)ns, -1);
    const TracePlan tp = plan_traceback(hlen.data(), target.data(), strand.data(), 0, ns, 0, slot.data(), c->h_mpq.p,
                                        c->h_mpt.p);
    const int32_t nslots = tp.n1 + tp.n2;
    std::vector<uint8_t> hops;
    std::vector<uint16_t> hnops((size_t)nslots);
    if (ops_in) {
      hops.assign((size_t)nslots * kOpsStride, 0);
      for (int32_t k = 0; k < K; k++)
        for (int32_t x = cstart[k] + 1; x < cstart[k + 1]; x++) {
          const int32_t sl = slot[member[x]], len = ops_in_len[x];
          hnops[sl] = (uint16_t)len;
          memcpy(hops.data() + (size_t)sl * kOpsStride + kOpsStride - len, ops_in + (size_t)x * ops_stride, (size_t)len);
        }
      if (nslots > 0) {
        c->hip(hipMemcpyAsync(c->t_ops.p, hops.data(), hops.size(), hipMemcpyHostToDevice, c->st), "h2d");
        c->hip(hipMemcpyAsync(c->t_nops.p, hnops.data(), (size_t)nslots * 2, hipMemcpyHostToDevice, c->st), "h2d");
      }
    } else {
      launch_tracebacks(c, ds, sc, tp, traceback_maxl(hlen.data(), 0, ns), c->st);
    }
    ensure_consensus_inputs(c, nm, K);
    for (int32_t x = 0; x < nm; x++) {
      c->h_mseq.p[x] = member[x];
      c->h_mops.p[x] = slot[member[x]];
      c->h_mstr.p[x] = strand[member[x]];
    }
    std::copy(cstart, cstart + (K > 0 ? K + 1 : 0), c->h_cstart.p);
    if (K == 0) c->h_cstart.p[0] = 0;
    const int32_t over = run_consensus(c, ds, nm, K, nullptr);
    // what the consensus kernel read, and what the traceback reported, per member entry
    std::vector<uint32_t> res((size_t)nslots);
    if (nslots > 0) {
      hops.resize((size_t)nslots * kOpsStride);
      c->hip(hipMemcpy(hops.data(), c->t_ops.p, hops.size(), hipMemcpyDeviceToHost), "d2h");
      c->hip(hipMemcpy(hnops.data(), c->t_nops.p, (size_t)nslots * 2, hipMemcpyDeviceToHost), "d2h");
      if (!ops_in) c->hip(hipMemcpy(res.data(), c->t_mout.p, (size_t)nslots * 4, hipMemcpyDeviceToHost), "d2h");
    }
    for (int32_t x = 0; x < nm; x++) {
      const int32_t sl = slot[member[x]];  // -1: a centroid
      const int32_t len = sl < 0 ? 0 : hnops[sl];
      const uint32_t r = sl < 0 ? 0u : res[sl];
      if (ops_out) {
        if (len > kOpsStride) c->fail(UMICLUST_EDEVICE, "member %d: the traceback reported %d ops", x, len);
        ops_out_len[x] = len;
        if (len > 0) memcpy(ops_out + (size_t)x * ops_stride, hops.data() + (size_t)sl * kOpsStride + kOpsStride - len, (size_t)len);
      }
      unpack_result(r, x, matches, internal_len, score);
    }
    if (over) c->fail(UMICLUST_ERANGE, kConsOverMsg, over);
    int64_t total = 0;
    for (int32_t k = 0; k < K; k++) {
      if (cons_off) cons_off[k] = total;
      total += c->h_clen.p[k];
    }
    if (cons_off) cons_off[K] = total;
    if (cons) {
      if (total > cons_cap) c->fail(UMICLUST_EINVAL, "consensus buffer too small");
      for (int64_t k = 0, at = 0; k < K; at += c->h_clen.p[k], k++)
        memcpy(cons + at, c->h_craw.p + (size_t)k * kConsCap, c->h_clen.p[k]);
    }
    return UMICLUST_OK;
  });
}

int32_t umiclust_prep(umiclust_ctx* c, const umiclust_params* p, const char* seqs, const int64_t* offsets,
                      int64_t n, char* masked, uint16_t* kmers, int32_t kstride, int32_t* nk) {
  UC_GUARD(c, {
    if (!p || n < 0 || (n > 0 && (!seqs || !offsets))) c->fail(UMICLUST_EINVAL, "null argument");
    for (int64_t i = 0; i < n; i++)
      if (offsets[i + 1] - offsets[i] > kMaxLen) c->fail(UMICLUST_ERANGE, "sequence longer than %d", kMaxLen);
    ProbeSeqs S;
    probe_prep(c, S, seqs, offsets, n, p->qmask_dust, true, false);
    std::vector<char> m((size_t)n * kMaxLen);
    std::vector<uint16_t> km((size_t)n * 2 * kKmerStride);
    std::vector<uint8_t> nkv((size_t)n * 2);
    if (n > 0) {
      c->hip(hipMemcpyAsync(m.data(), S.d_m.p, m.size(), hipMemcpyDeviceToHost, c->st), "d2h");
      c->hip(hipMemcpyAsync(km.data(), S.d_km.p, km.size() * 2, hipMemcpyDeviceToHost, c->st), "d2h");
      c->hip(hipMemcpyAsync(nkv.data(), S.d_nk.p, nkv.size(), hipMemcpyDeviceToHost, c->st), "d2h");
    }
    c->hip(hipStreamSynchronize(c->st), "sync");
    for (int64_t i = 0; i < n; i++) {
      const int64_t L = offsets[i + 1] - offsets[i];
      if (masked) memcpy(masked + (offsets[i] - offsets[0]), m.data() + (size_t)i * kMaxLen, (size_t)L);
      for (int s = 0; s < 2; s++) {
        if (nk) nk[2 * i + s] = nkv[(size_t)2 * i + s];
        if (kmers)
          for (int x = 0; x < nkv[(size_t)2 * i + s] && x < kstride; x++)
            kmers[(size_t)(2 * i + s) * kstride + x] = km[(size_t)(2 * i + s) * kKmerStride + x];
      }
    }
    return UMICLUST_OK;
  });
}

// Everything K1 writes, as the device holds it, for n records launched the way prepare_impl launches a load's: output
// row s is record perm[s].  Every access of the kernel is bounded by the record lengths and by perm, so both are checked
// here before anything is launched.
int32_t umiclust_prep_outputs(umiclust_ctx* c, const umiclust_params* p, const char* seqs, const int64_t* offsets,
                              int64_t n, const int32_t* perm, char* masked, uint32_t* codes, uint8_t* lens,
                              uint16_t* kmers, int32_t kstride, int32_t* nk, uint8_t* changed, uint32_t* flags) {
  UC_GUARD(c, {
    if (!p || n < 0 || (n > 0 && (!seqs || !offsets))) c->fail(UMICLUST_EINVAL, "null argument");
    if (n > (1 << 30)) c->fail(UMICLUST_ERANGE, "too many records");
    if (kmers && (kstride < kMaxKmers || !nk)) c->fail(UMICLUST_EINVAL, "kmers needs nk and kstride >= %d", kMaxKmers);
    for (int64_t i = 0; i < n; i++) {
      const int64_t L = offsets[i + 1] - offsets[i];
      if (L < 0) c->fail(UMICLUST_EINVAL, "record %lld: offsets decrease", (long long)i);
      if (L > kMaxLen) c->fail(UMICLUST_ERANGE, "record %lld longer than %d", (long long)i, kMaxLen);
    }
    if (perm) {
      std::vector<uint8_t> seen((size_t)n, 0);
      for (int64_t s = 0; s < n; s++) {
        if (perm[s] < 0 || perm[s] >= n || seen[perm[s]]) c->fail(UMICLUST_EINVAL, "perm is no permutation of 0..n-1");
        seen[perm[s]] = 1;
      }
    }
    ProbeSeqs S;
    probe_prep(c, S, seqs, offsets, n, p->qmask_dust, true, true, perm, true);
    auto out = [&](void* dst, const void* src, size_t bytes) {
      if (dst && bytes) c->hip(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->st), "d2h");
    };
    std::vector<uint16_t> km(kmers ? (size_t)n * 2 * kKmerStride : 0);
    std::vector<uint8_t> nkv((size_t)n * 2);
    out(masked, S.d_m.p, (size_t)n * kMaxLen);
    out(codes, S.d_codes.p, (size_t)n * 2 * kCodeWords * 4);
    out(lens, S.d_lens.p, (size_t)n);
    out(changed, S.d_chg.p, (size_t)n);
    out(flags, S.d_amb.p, 8);
    out(kmers ? km.data() : nullptr, S.d_km.p, km.size() * 2);
    out(nk ? nkv.data() : nullptr, S.d_nk.p, nkv.size());
    c->hip(hipStreamSynchronize(c->st), "sync");
    for (int64_t r = 0; nk && r < 2 * n; r++) {
      nk[r] = nkv[(size_t)r];
      if (nkv[(size_t)r] > kMaxKmers) c->fail(UMICLUST_EDEVICE, "row %lld: the kernel reported %d k-mers", (long long)r, nk[r]);
      if (kmers) memcpy(kmers + (size_t)r * kstride, km.data() + (size_t)r * kKmerStride, (size_t)nkv[(size_t)r] * 2);
    }
    return UMICLUST_OK;
  });
}

// The region join's own sequence (overlap_table with the CSR, then launch_overlap_pairs, as umiclust_overlap_regions
// runs them) with every array the kernels leave behind copied out.  No kernel runs for n = 0, as there: start is
// then all zero by definition.
int32_t umiclust_overlap_probe(umiclust_ctx* c, const char* seqs, const int64_t* offsets, int64_t n,
                               const int64_t* region_start, int32_t nregions, int32_t hash_bits, int64_t n_cap,
                               int64_t m_cap, int64_t big_cap, uint64_t* hash, int32_t* region, int64_t* slot,
                               int64_t* rep_of, uint32_t* cnt, uint32_t* start, uint32_t* members, uint32_t* big,
                               int64_t* nbig, int64_t* total, int32_t* maxcount, uint64_t* info) {
  UC_GUARD(c, {
    if (nregions < 1 || nregions > UMICLUST_OVERLAP_MAX_REGIONS || hash_bits < 1 || hash_bits > 64 || n_cap < 0 ||
        m_cap < 0 || big_cap < 0)
      c->fail(UMICLUST_EINVAL, "umiclust_overlap_probe: 1..%d regions, 1..64 hash bits, capacities >= 0",
              UMICLUST_OVERLAP_MAX_REGIONS);
    OvRun R;
    overlap_table(c, R, seqs, offsets, n, region_start, nregions, true, hash_bits);
    const int64_t m = (int64_t)R.mask + 1;
    if (info) info[0] = (uint64_t)m, info[1] = (uint64_t)R.passes, info[2] = R.seed;
    if (n_cap < n || m_cap < m)
      c->fail(UMICLUST_ERANGE, "umiclust_overlap_probe: %lld sequences and %lld slots, room for %lld and %lld",
              (long long)n, (long long)m, (long long)n_cap, (long long)m_cap);
    const size_t cells = (size_t)nregions * nregions;
    DevBuf<unsigned long long> d_total;
    DevBuf<uint32_t> d_max;
    alloc_each(c, cells, d_total, d_max);
    c->hip(hipMemsetAsync(d_total.p, 0, cells * 8, c->st), "memset");
    c->hip(hipMemsetAsync(d_max.p, 0, cells * 4, c->st), "memset");
    c->hip(hipMemsetAsync(R.d_nbig.p, 0, 4, c->st), "memset");
    if (n > 0) c->hip(launch_overlap_pairs(R.B, R.mask, nregions, d_total.p, d_max.p, c->st), "overlap pairs");
    auto out = [&](void* dst, const void* src, size_t bytes) {
      if (dst) c->d2h(dst, src, bytes);
    };
    std::vector<unsigned long long> rep(rep_of ? (size_t)m : 0);
    std::vector<int64_t> sl(rep_of ? (size_t)n : 0);
    std::vector<uint32_t> mx(maxcount ? cells : 0);
    uint32_t nb = 0;
    out(hash, R.d_hash.p, (size_t)n * 8);
    out(region, R.d_reg.p, (size_t)n * 4);
    out(slot, R.d_slot.p, (size_t)n * 8);
    out(cnt, R.d_cnt.p, (size_t)m * 4);
    if (n > 0) out(start, R.d_start.p, ((size_t)m + 1) * 4);
    else if (start) std::fill(start, start + m + 1, 0u);
    out(members, R.d_members.p, (size_t)n * 4);  // after k_ov_pairs: the small buckets are sorted
    out(total, d_total.p, cells * 8);
    out(maxcount ? mx.data() : nullptr, d_max.p, cells * 4);
    out(rep_of ? rep.data() : nullptr, R.d_rep.p, (size_t)m * 8);
    out(rep_of ? sl.data() : nullptr, R.d_slot.p, (size_t)n * 8);
    c->d2h(&nb, R.d_nbig.p, 4);
    c->hip(hipStreamSynchronize(c->st), "sync");
    for (size_t x = 0; maxcount && x < cells; x++) maxcount[x] = (int32_t)mx[x];
    for (int64_t i = 0; rep_of && i < n; i++) {
      if (sl[i] < 0 || sl[i] >= m) c->fail(UMICLUST_EDEVICE, "sequence %lld: slot %lld", (long long)i, (long long)sl[i]);
      rep_of[i] = (int64_t)rep[(size_t)sl[i]];
    }
    if (nbig) *nbig = nb;
    if ((int64_t)nb > (int64_t)n / (kOvSmallBucket + 1))
      c->fail(UMICLUST_EDEVICE, "umiclust_overlap_probe: %u large buckets of %lld sequences", nb, (long long)n);
    if (big) {
      c->d2h(big, R.d_big.p, (size_t)std::min<int64_t>(nb, big_cap) * 4);
      c->hip(hipStreamSynchronize(c->st), "sync");
      if ((int64_t)nb > big_cap)
        c->fail(UMICLUST_ERANGE, "umiclust_overlap_probe: %u large buckets, room for %lld", nb, (long long)big_cap);
    }
    return UMICLUST_OK;
  });
}

}  // extern "C"
