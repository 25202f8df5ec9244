// pass.cpp -- one greedy block's device pass and its host resolution: the pass buffers, the prefilter launches (whole
// passes and the split passes' two halves), the walk / alignment chain, and resolve_pass with round B.  The pipeline
// that orders the passes is driver.cpp's ClusterRun.
#include <cstdio>
#include <string>

#include "cluster_ctx.h"

namespace uc {

void ensure_pass_buffers(umiclust_ctx* c, Pass& P, int32_t B) {
  const size_t nqs = (size_t)B * c->both;
  alloc_each(c, nqs * kTopHits, P.d_top_seqno, P.d_top_count);
  c->hip(P.d_ntop.ensure(nqs), "alloc");
  c->hip(P.d_pcand.ensure(nqs * kParts * kPartCand), "alloc");
  alloc_each(c, nqs * kParts, P.d_pncand, P.d_units);
  alloc_each(c, nqs * kParts * kPeerCap, P.d_ppeer_id, P.d_ppeer_count);
  alloc_each(c, nqs * kParts, P.d_pnpeer, P.d_ppost);
  alloc_each(c, nqs * kPeerCap, P.d_peer_id, P.d_peer_count);
  c->hip(P.d_npeer.ensure(nqs), "alloc");
  c->hip(P.d_counters.ensure(kCountersLen), "alloc");
  P.ctr_zeroed = false;  // (a new bin or a grown buffer set: the next pass memsets them)
  // pair lists: a launch aligns up to kWalk walk pairs plus kPeerCap peer pairs per query-strand; results
  // land in d_res: walk candidate x of qs at [qs * kWalk + x], peer y at [nqs * kWalk + qs * kPeerCap + y]
  alloc_each(c, nqs * (kWalk + kPeerCap), P.d_pq, P.d_pt, P.d_outidx, P.d_res);
  c->hip(P.d_hq.ensure(nqs), "alloc");
  c->hip(P.d_paligned.ensure((size_t)nqs * (kPeerCap / 64)), "alloc");  // 64-bit aligned-peer masks per query-strand
  c->hip(P.d_ws.ensure(nqs), "alloc");
  if (!P.d_reccount.p) {  // [0] record words allocated, [1] k_pack's workgroup tickets; k_pack leaves both zero
    c->hip(P.d_reccount.ensure(2), "alloc");
    c->hip(hipMemsetAsync(P.d_reccount.p, 0, 8, c->st), "memset");
  }
  c->hip(P.h_hq.ensure(nqs), "pin");
  c->hip(P.h_rec.ensure(nqs * kRecWords), "pin");
  c->hip(P.d_rec.ensure(nqs * kRecWords), "alloc");
  c->hip(P.h_counters.ensure(16), "pin");
  c->hip(P.h_reccount.ensure(1), "pin");
  // fixed capacities, so a pass never frees memory a queued pass still reads
  c->hip(P.h_tiles.ensure(64), "pin");
  c->hip(P.d_tiles.ensure(64), "alloc");
  c->hip(P.h_tiles_a.ensure(64), "pin");
  c->hip(P.d_tiles_a.ensure(64), "alloc");
  if (!P.d_anunits.p) {
    c->hip(P.d_anunits.ensure(1), "alloc");
    c->hip(hipMemsetAsync(P.d_anunits.p, 0, 4, c->st), "memset");
  }
  P.ev_a.get(c);
}

namespace {

// ---- what enqueue_pass and enqueue_count share of a prefilter launch ----
// Stream st waits for the side stream's index appends and peer-tile builds.
void wait_index_and_tiles(umiclust_ctx* c, hipStream_t st) {
  if (c->ix_st && c->ix_done) c->hip(hipStreamWaitEvent(st, c->ix_done, 0), "wait");  // index / peer tiles
  if (c->pt_pending) {  // whole passes: the peer tiles built ahead on the side stream (ClusterRun::run_whole)
    c->hip(hipStreamWaitEvent(st, c->pt_ev, 0), "wait");
    c->pt_pending = false;
  }
}

// The arguments that do not depend on the peer window: the sequences, the index as it stands (nv staged views), the
// block, the pass's per-part buffers, the packs' bin bounds (PrefilterArgs::qbin) and the centroid length table.
PrefilterArgs prefilter_args(umiclust_ctx* c, const Pass& P, const TileView* views, const TileView* dviews, int32_t nv,
                             int32_t q0, int32_t nq) {
  const Index& ix = c->ix;
  PrefilterArgs a{};
  for (int32_t i = 0; i < nv && nv <= kArgTiles; i++) a.tv[i] = views[i];
  a.seqs = dev_seqs(c);
  a.arena = ix.arena.p;
  a.tiles = dviews;
  a.ntiles = nv;
  a.ncent = ix.index_end;
  a.nseg = ix.nseg();
  a.cent_seqno = ix.d_cent.p;
  for (int L = 0; L <= kMaxLen; L++) a.cnt_ge[L] = ix.cnt_ge[L];
  a.q0 = q0;
  a.nq = nq;
  a.both = c->both;
  a.minwordmatches = c->p.minwordmatches;
  a.seq2ord = ix.d_seq2ord.p - c->bin_s[c->cur_bin];
  a.pcand = P.d_pcand.p;
  a.pncand = P.d_pncand.p;
  a.units = P.d_units.p;
  a.nunits = P.d_anunits.p;
  a.ppeer_id = P.d_ppeer_id.p;
  a.ppeer_count = P.d_ppeer_count.p;
  a.pnpeer = P.d_pnpeer.p;
  a.ppost = P.d_ppost.p;
  a.pf1_lds = c->tun.pf1_lds;
  a.prof = c->pf_prof.p;  // null unless UMICLUST_PFPROF is set
  a.qbin = c->pack_on ? c->d_qbin.p : nullptr;
  a.bin_seq0 = c->d_bin_seq0.p;
  a.bin_ord0 = c->d_bin_ord0.p;
  a.cent_len = ix.d_cent_len.p;
  return a;
}

// the window's tiles in the kernel's peer slots, oldest first and the newest in the last slot: tiles[0 .. n), then
// `last` if given; missing earlier blocks leave n = 0 slots in front
void fill_peer_slots(PrefilterArgs& a, const Tile* const* tiles, int n, const Tile* last) {
  const int nwin = n + (last ? 1 : 0);
  for (int i = 0; i < kPeerTiles; i++) {
    const int j = i - (kPeerTiles - nwin);
    a.peer[i] = j < 0 ? TileView{} : view_of(j < n ? *tiles[j] : *last);
  }
}

// list table of the lean kernel: every k-mer of the block's length in every tile it reads (ntiles of the index)
int32_t nlist_cap(const umiclust_ctx* c, int32_t q0, int32_t nq, int32_t ntiles) {
  return std::min(kMaxKmers * 12, std::max(1, block_maxlen(c, q0, nq) - 7) * (ntiles + kPeerTiles));
}

// UMICLUST_PFPROBE=1 (measurement only): after every counting launch, the same launch without its count loop
// (k_pf_count<2>) into scratch outputs, so a kernel trace shows what the table, zeroing, scan and output phases cost
// on their own beside the full kernel
void launch_pf_probe(umiclust_ctx* c, const PrefilterArgs& a, hipStream_t st) {
  const size_t U = (size_t)a.nq * a.both * kParts;
  const size_t words = U * kPartCand + U * (kPeerCap / 2) + 8 * U + 16 + U * (kPeerCap / 4);
  c->hip(c->d_probe.ensure(words), "alloc probe");
  uint32_t* p = c->d_probe.p;
  PrefilterArgs b = a;
  b.pcand = p;
  p += U * kPartCand;
  b.ppeer_id = reinterpret_cast<uint16_t*>(p);
  p += U * (kPeerCap / 2);
  b.ppost = p;
  b.units = p + 3 * U;
  b.pncand = reinterpret_cast<uint8_t*>(p + 4 * U);
  b.pnpeer = reinterpret_cast<uint8_t*>(p + 5 * U);
  b.nunits = p + 7 * U + 8;
  b.ppeer_count = reinterpret_cast<uint8_t*>(p + 8 * U + 16);  // U * kPeerCap bytes
  b.prof = nullptr;
  c->hip(hipMemsetAsync(b.nunits, 0, 4, st), "memset");
  c->hip(launch_prefilter(b, st, 3), "prefilter probe");
}

}  // namespace

// Enqueue the device pass of block [q0, q0+nq) against the index as it stands (centroids of the
// blocks before the peer window), with no host synchronisation: the block's own peer tile (kept
// for the next block's window), prefilter, the batch-of-8 walk over T_old (up to 4 align rounds),
// the speculative alignment of every (query, earlier window query) pair passing the k-mer
// threshold, and one download of the walk states, top lists, walked results and peer results.
// The peer window is [prev->base, q0+nq) with prev = the previous block's tile, or the block
// alone (prev == nullptr).  `cap` is null in production (PfCapture).
void enqueue_pass(umiclust_ctx* c, Pass& P, int32_t q0, int32_t nq, const Tile* const* prevs, int nprev, Tile& own,
                  int32_t region, bool lazy_peers, bool after_count, PfCapture* cap) {
  const int32_t w0 = nprev > 0 ? prevs[0]->base : q0;
  const int both = c->both;
  const int32_t nqs = nq * both;
  hipStream_t st = c->st;
  wait_index_and_tiles(c, st);
  P.q0 = q0;
  P.nq = nq;
  P.w0 = w0;
  P.live = true;
  const bool built_now = !(own.prebuilt && own.base == q0 && own.n == nq && own.seg == region);
  if (built_now) build_tile(c, own, c->d_iota.p, q0, nq, 0, region * kPeerRegion, 1 << 30);
  own.prebuilt = false;
  own.base = q0;
  own.seg = region;
  own.len = block_maxlen(c, q0, nq);  // the block's longest query
  const bool second_half = after_count && P.a_live && P.a_q0 == q0;
  // a second half's prefilter (full kernel + merge) runs on the align stream ahead of its walk, so the
  // main stream's next counting half does not queue behind it.  It needs its counting half (a_ev) and the
  // index / tiles (ix_done; index appends on the side stream wait for the latest second half, last_r_ev)
  if (second_half && c->ix_st && !built_now) {
    st = c->st_al;
    if (c->ix_done) c->hip(hipStreamWaitEvent(st, c->ix_done, 0), "wait");
  }
  const int32_t nv = c->ix.stage_views(P.h_tiles, P.d_tiles, st);
  // the counters are zero unless this buffer set's last pass launched no k_pack (which re-zeroes them at its end)
  if (!P.ctr_zeroed) c->hip(hipMemsetAsync(P.d_counters.p, 0, kCountersLen * 4, st), "memset");
  P.ctr_zeroed = false;
  PrefilterArgs a = prefilter_args(c, P, P.h_tiles.p, P.d_tiles.p, nv, q0, nq);
  // centroid tiles are in segment order (sealed tiles, then base and delta); each pass addresses its
  // postings from the lowest arena slot it reads
  if (a.nseg > kMaxSegs) c->fail(UMICLUST_ERANGE, "more than %d centroids in one bin", kMaxSegs * kSegCentroids);
  for (int s = 0, vi = 0; s <= a.nseg; s++) {
    while (vi < nv && P.h_tiles.p[vi].seg < s) vi++;
    a.seg_tile[s] = s == a.nseg ? nv : vi;
  }
  {
    uint64_t peer_lo = own.post_base;
    for (int i = 0; i < nprev; i++) peer_lo = std::min(peer_lo, prevs[i]->post_base);
    for (int s = 0; s < std::max(a.nseg, 1); s++) {
      uint64_t lo = (s == std::max(a.nseg, 1) - 1) ? peer_lo : UINT64_MAX;
      if (a.nseg > 0)
        for (int v = a.seg_tile[s]; v < a.seg_tile[s + 1]; v++) lo = std::min(lo, P.h_tiles.p[v].post_base);
      a.seg_base[s] = lo;
    }
  }
  fill_peer_slots(a, prevs, nprev, &own);
  a.peer_base = w0;
  a.flag_tile = -1;
  a.cand_base = w0;
  a.peer_shift = 0;
  a.peer_id_add = 0;
  if (second_half) {
    // the counting half ran with the window one block wider (oldest first): its peer ids are relative to
    // that window's start
    a.cand_base = P.a_base;
    a.peer_shift = w0 - P.a_base;
    a.peer_id_add = a.peer_shift;
  }
  a.nlist_cap = nlist_cap(c, q0, nq, a.nseg > 0 ? a.seg_tile[1] - a.seg_tile[0] : 0);
  a.top_seqno = P.d_top_seqno.p;
  a.top_count = P.d_top_count.p;
  a.ntop = P.d_ntop.p;
  a.peer_id = P.d_peer_id.p;
  a.peer_count = P.d_peer_count.p;
  a.npeer = P.d_npeer.p;
  a.postings_touched = P.d_counters.p;
  if (second_half) c->hip(hipStreamWaitEvent(st, c->a_ev[P.a_slot][1], 0), "wait");
  c->hip(hipEventRecord(P.ev[0], st), "event");
  P.c_timed = false;
  if (cap) {  // (one_wave: the lean kernel's layout, set where that kernel is launched)
    cap->ntiles = nv;
    cap->nseg = a.nseg;
  }
  if (second_half) {
    // (the units are the counting half's: the merge resets their count)
    if (cap) c->hip(hipMemcpyAsync(cap->h_nunits, P.d_anunits.p, 4, hipMemcpyDeviceToHost, st), "d2h units");
    c->hip(launch_prefilter(a, st, 4), "prefilter");
  } else if (a.nseg <= 1) {
    // whole pass: the lean counting (timed alone), then the full kernel over its overflowed units + merge
    c->hip(hipEventRecord(P.ev_c[0].get(c), st), "event");
    c->hip(launch_prefilter(a, st, 1), "prefilter (count)");
    c->hip(hipEventRecord(P.ev_c[1].get(c), st), "event");
    c->stats.counter_cells += (int64_t)nq * c->both * a.ncent;
    if (c->tun.pf_probe) launch_pf_probe(c, a, st);
    if (cap) {
      c->hip(hipMemcpyAsync(cap->h_nunits, P.d_anunits.p, 4, hipMemcpyDeviceToHost, st), "d2h units");
      cap->one_wave = prefilter_one_wave(a) ? 1 : 0;
    }
    c->hip(launch_prefilter(a, st, 2), "prefilter");
    P.c_timed = true;
  } else {
    c->hip(launch_prefilter(a, st, 0), "prefilter");
  }
  c->hip(hipEventRecord(P.ev[1], st), "event");
  c->last_r_ev = P.ev[1];
  P.a_timed = second_half;
  P.t_slot = P.a_slot;
  P.a_live = false;
  // The walk, its alignment rounds and the packing run on the align stream: they read only this
  // pass's buffers and the sequences, so the main stream goes on with the index append of the block
  // being resolved and the next pass's prefilter while these small launches run.
  c->hip(hipStreamWaitEvent(c->st_al, P.ev[1], 0), "wait");
  st = c->st_al;
  DevSeqs ds = dev_seqs(c);
  // the block's query lengths (sorted, non-increasing): one pair segment and one alignment launch per length
  const int32_t lmax = block_maxlen(c, q0, nq), nsg = lmax - block_minlen(c, q0, nq) + 1;
  if (nsg > kSegLens) c->fail(UMICLUST_EINVAL, "block spans %d query lengths (> %d)", nsg, kSegLens);
  int32_t nql[kSegLens] = {};
  for (int32_t q = q0; q < q0 + nq; q++) nql[lmax - c->hlen[q]]++;
  SegTab sg0{}, sg1{};
  sg0.lmax = sg1.lmax = lmax;
  sg0.nseg = sg1.nseg = nsg;
  for (int32_t i = 0, b0 = 0, b1 = 0; i < nsg; i++) {
    sg0.base[i] = (uint32_t)b0;
    sg1.base[i] = (uint32_t)b1;
    b0 += nql[i] * both * kWalk;
    b1 += nql[i] * both * (kWalk + kPeerCap);
  }
  uint32_t* segc = P.d_counters.p + kSegSlot;  // [walk round][segment]
  unsigned long long* cells_w = reinterpret_cast<unsigned long long*>(P.d_counters.p + 12);
  unsigned long long* cells_p = reinterpret_cast<unsigned long long*>(P.d_counters.p + 14);
  auto align_round = [&](const SegTab& sg, int per_qs, uint32_t* cnt, const char* what) {
    for (int32_t i = 0; i < nsg; i++)
      if (nql[i])
        c->hip(launch_align(ds, lmax - i, c->ambig, P.d_pq.p + sg.base[i], P.d_pt.p + sg.base[i], nql[i] * both * per_qs,
                            cnt + i, P.d_outidx.p + sg.base[i], c->sc, P.d_res.p, st, c->tun.band_pairs),
               what);
  };
  c->hip(launch_walk(-1, q0, nqs, both, kSpecThr, P.d_top_seqno.p, P.d_top_count.p, P.d_ntop.p, c->d_lens.p, P.d_res.p,
                     c->d_acc.p, c->d_rank.p, P.d_ws.p, P.d_pq.p, P.d_pt.p, P.d_outidx.p, sg0, segc, cells_w, st),
         "walk");
  c->hip(hipEventRecord(P.ev[2], st), "event");
  // two dependent alignment launches: batch 0 (or a speculative whole walk), then the rest of every
  // unfinished walk together with the relevant in-window peers (their relevance is taken from the walk
  // state after round 0, which only widens it: a superset of what the final state needs)
  const uint32_t peer_out0 = (uint32_t)nqs * kWalk;
  // small passes (deep clusters cut blocks small) spread every pair over a lane group
  align_round(sg0, kWalk, segc, "align 0");
  c->hip(launch_walk(0, q0, nqs, both, kSpecThr, P.d_top_seqno.p, P.d_top_count.p, P.d_ntop.p, c->d_lens.p,
                     P.d_res.p, c->d_acc.p, c->d_rank.p, P.d_ws.p, P.d_pq.p, P.d_pt.p, P.d_outidx.p, sg1, segc + kSegLens,
                     cells_w, st),
         "walk 0");
  // the previous block's pass (its walk states are final and stay until that buffer set's next walk, which is
  // queued after this one on the align stream): peers there whose device walk accepted are certain members
  // (relevant peers certain to become members are not aligned speculatively: config 2 4.02 -> 4.14 M, round 4)
  const Pass* prev = nullptr;
  for (const Pass& Q : c->pass)
    if (&Q != &P && Q.nq > 0 && Q.q0 + Q.nq == q0) prev = &Q;
  c->hip(launch_peer_pairs(q0, w0, nqs, both, c->d_lens.p, P.d_ws.p, P.d_peer_id.p, P.d_peer_count.p, P.d_npeer.p,
                           P.d_pq.p, P.d_pt.p, P.d_outidx.p, sg1, segc + kSegLens, cells_p, P.d_counters.p + 8,
                           peer_out0, P.d_paligned.p, lazy_peers ? 0 : 1,
                           prev ? prev->d_ws.p : nullptr, prev ? prev->d_npeer.p : nullptr, prev ? prev->q0 : 0,
                           prev ? prev->nq : 0, st),
         "peer pairs");
  align_round(sg1, kWalk + kPeerCap, segc + kSegLens, "align 1");
  c->hip(launch_walk(1, q0, nqs, both, kSpecThr, P.d_top_seqno.p, P.d_top_count.p, P.d_ntop.p, c->d_lens.p,
                     P.d_res.p, c->d_acc.p, c->d_rank.p, P.d_ws.p, P.d_pq.p, P.d_pt.p, P.d_outidx.p, sg1,
                     segc + 2 * kSegLens, cells_w, st),
         "walk 1");
  c->hip(hipEventRecord(P.ev[3], st), "event");
  // what the host needs goes straight to pinned host memory; the pass that next reuses these
  // buffers is enqueued only after the host has waited for ev[4]
  // blocks of at most kDirectRecQ queries write directly too
  P.rec_direct = c->rec_direct || nq <= kDirectRecQ;
  // rec_direct: k_pack writes the outcomes and records straight into the pinned host buffers (no DMA copies on the
  // chain the host waits for: a 3 MB record copy was 0.14 ms per config-2 block); otherwise device buffers + copies
  c->hip(launch_pack(nqs, w0, c->d_lens.p, P.d_ws.p, P.d_ntop.p, P.d_top_seqno.p, P.d_top_count.p, P.d_res.p,
                     P.d_npeer.p, P.d_peer_id.p, P.d_peer_count.p, P.d_res.p + peer_out0, P.d_paligned.p, P.d_reccount.p,
                     P.rec_direct ? P.h_hq.p : P.d_hq.p,
                     P.rec_direct ? P.h_rec.p : P.d_rec.p, P.d_counters.p, P.h_counters.p, P.h_reccount.p, st),
         "pack");
  P.ctr_zeroed = nqs > 0;
  if (!P.rec_direct) {
    c->hip(hipMemcpyAsync(P.h_hq.p, P.d_hq.p, (size_t)nqs * sizeof(HostQs), hipMemcpyDeviceToHost, st), "d2h outcomes");
    const size_t est = std::min<size_t>(P.rec_est, P.d_rec.n);
    c->hip(hipMemcpyAsync(P.h_rec.p, P.d_rec.p, est * 4, hipMemcpyDeviceToHost, st), "d2h records");
  }
  c->hip(hipEventRecord(P.ev[4], st), "event");
}

// The counting half of a split pass (block [q0, q0+nq), launch_prefilter mode 1): the lean kernel against
// the index as it stands and the window's peer tiles `wins` (oldest first, the block's own -- built -- last);
// the hits of wins[flag] (a block not yet resolved) become flagged candidates.  The second half is
// enqueue_pass(..., after_count = true) once that block is resolved and appended.  Bins past one counter
// segment are not split (a_live stays false and the second half runs the whole prefilter).
void enqueue_count(umiclust_ctx* c, Pass& P, int32_t q0, int32_t nq, const Tile* const* wins, int nwin, int flag,
                   int32_t slot, PfCapture* cap) {
  P.a_live = false;
  if (c->ix.nseg() > 1) return;
  // on its own stream, gated by the main stream's work so far (index append, peer tiles, this buffer set's
  // last merge): the main stream's next append and second half do not queue behind it
  hipStream_t st = c->st;
  wait_index_and_tiles(c, st);
  // this buffer set's last second half (full kernel + merge on the align stream) has read what
  // the counting half overwrites
  if (c->ix_st) c->hip(hipStreamWaitEvent(st, P.ev[1], 0), "wait");
  c->hip(hipEventSynchronize(P.ev_a), "sync");  // the last upload from h_tiles_a is done
  const int32_t nv = c->ix.stage_views(P.h_tiles_a, P.d_tiles_a, st);
  c->hip(hipEventRecord(P.ev_a, st), "event");
  PrefilterArgs a = prefilter_args(c, P, P.h_tiles_a.p, P.d_tiles_a.p, nv, q0, nq);
  a.seg_tile[0] = 0;
  a.seg_tile[1] = nv;
  uint64_t lo = UINT64_MAX;
  for (int i = 0; i < nwin; i++) lo = std::min(lo, wins[i]->post_base);
  for (int v = 0; v < nv; v++) lo = std::min(lo, P.h_tiles_a.p[v].post_base);
  a.seg_base[0] = lo;
  fill_peer_slots(a, wins, nwin, nullptr);
  a.flag_tile = flag >= 0 ? (kPeerTiles - nwin) + flag : -1;
  a.peer_base = a.cand_base = wins[0]->base;
  a.nlist_cap = nlist_cap(c, q0, nq, nv);
  if (cap) {
    cap->ntiles_count = nv;
    cap->one_wave = prefilter_one_wave(a) ? 1 : 0;
  }
  c->hip(hipEventRecord(c->a_ev[slot][0].get(c), st), "event");
  c->hip(launch_prefilter(a, st, 1), "prefilter (count)");
  c->hip(hipEventRecord(c->a_ev[slot][1].get(c), st), "event");
  c->stats.counter_cells += (int64_t)nq * c->both * a.ncent;
  if (c->tun.pf_probe) launch_pf_probe(c, a, st);
  c->last_a_slot = slot;
  P.a_live = true;
  P.a_q0 = q0;
  P.a_base = wins[0]->base;
  P.a_slot = slot;
}

namespace {

// One resolve_block call, replayable without a GPU (format read by tools/resolve_tsan_main.cpp): little-endian,
// "UCRD" v1, the parameters, hlen of the bin up to the block's end, the acceptance / rank tables, the window's states
// before, the pass's HostQs and records, round B's pairs and results, then the outputs (the block's states, targets
// and strands, the new centroids, alignments and cells).
void write_resolve_dump(const umiclust_ctx* c, const ResolveEnv& env, int32_t q0, int32_t nq, int32_t w0,
                        const StateView& state, const std::vector<uint8_t>& state_in, const HostQs* hq,
                        const uint32_t* recs, uint32_t nrec, const std::vector<uint32_t>& bpq,
                        const std::vector<uint32_t>& bpt, const std::vector<uint32_t>& bres,
                        const std::vector<int32_t>& new_cents, const ResolveStats& rs) {
  const std::string path = std::string(c->tun.resolve_dump, strcspn(c->tun.resolve_dump, ":")) + "." +
                           std::to_string(c->n_resolved - 1) + ".bin";
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return;
  auto w = [&](const void* p, size_t n) { fwrite(p, 1, n, f); };
  auto wi = [&](int64_t v) { w(&v, 8); };
  w("UCRD", 4);
  const int32_t s0 = state.s0;
  const int32_t hdr[12] = {1, q0, nq, w0, env.both, env.o4_T, env.maxaccepts, env.maxrejects, env.pre_resolve ? 1 : 0,
                           env.pre_spec ? 1 : 0, s0, 0};
  w(hdr, sizeof hdr);
  wi(q0 + nq - s0);
  w(env.hlen + s0, (size_t)(q0 + nq - s0));
  w(env.acc, (size_t)kTabL * kTabM);
  w(env.rank, (size_t)kTabL * kTabM * 2);
  wi((int64_t)state_in.size());
  w(state_in.data(), state_in.size());
  const int64_t nqs = (int64_t)nq * env.both;
  wi(nqs);
  w(hq, (size_t)nqs * sizeof(HostQs));
  wi(nrec);
  w(recs, (size_t)nrec * 4);
  wi((int64_t)bpq.size());
  w(bpq.data(), bpq.size() * 4);
  w(bpt.data(), bpt.size() * 4);
  w(bres.data(), bres.size() * 4);
  w(&state[q0], (size_t)nq);
  w(env.target + q0, (size_t)nq * 4);
  w(env.strand + q0, (size_t)nq);
  wi((int64_t)new_cents.size());
  w(new_cents.data(), new_cents.size() * 4);
  wi(rs.n_alignments);
  wi(rs.cells);
  fclose(f);
}

// Round B: the alignments deferred queries need (pairs bpq / bpt, in query order), synchronously; the scores go to
// bres and the device time between the first and last launch to t_al.
// On the copy stream (a hardware queue of its own, otherwise idle): on st_b it queued behind the split passes' index
// appends and peer-tile builds, which wait for the next counting half -- about one counting launch of latency on the
// host's critical path per block with deferred queries
void round_b(umiclust_ctx* c, const std::vector<uint32_t>& bpq, const std::vector<uint32_t>& bpt,
             std::vector<uint32_t>& bres, double& t_al) {
  const int32_t nb = (int32_t)bpq.size();
  hipStream_t sb = c->st_copy;
  alloc_each(c, nb, c->h_bpq, c->h_bpt, c->h_bres);
  memcpy(c->h_bpq.p, bpq.data(), (size_t)nb * 4);
  memcpy(c->h_bpt.p, bpt.data(), (size_t)nb * 4);
  // small rounds (the usual: tens of pairs) read their pairs from and write their scores to the pinned buffers
  // directly: one dispatch per query length and no copies on the host's critical path (two uploads and a download
  // were ~70 us of dispatch latency per block with deferred queries); large ones go through device buffers
  const bool direct = nb <= kRbDirect;
  const uint32_t *pq = c->h_bpq.p, *pt = c->h_bpt.p;
  uint32_t* pres = c->h_bres.p;
  if (!direct) {
    alloc_each(c, nb, c->d_bpq, c->d_bpt, c->d_bres);
    c->hip(hipMemcpyAsync(c->d_bpq.p, c->h_bpq.p, (size_t)nb * 4, hipMemcpyHostToDevice, sb), "h2d");
    c->hip(hipMemcpyAsync(c->d_bpt.p, c->h_bpt.p, (size_t)nb * 4, hipMemcpyHostToDevice, sb), "h2d");
    pq = c->d_bpq.p;
    pt = c->d_bpt.p;
    pres = c->d_bres.p;
  }
  c->hip(hipEventRecord(c->evb[0], sb), "event");
  // the pairs are in query order: one launch per run of one query length
  int nl = 0;
  for (int32_t x0 = 0; x0 < nb; nl++) {
    const int32_t L = c->hlen[bpq[x0] >> 1];
    int32_t x1 = x0 + 1;
    while (x1 < nb && c->hlen[bpq[x1] >> 1] == L) x1++;
    c->hip(launch_align(dev_seqs(c), L, c->ambig, pq + x0, pt + x0, x1 - x0, nullptr, nullptr, c->sc, pres + x0, sb,
                        c->tun.band_pairs),
           "align B");
    x0 = x1;
  }
  c->hip(hipEventRecord(c->evb[1], sb), "event");
  if (!direct)
    c->hip(hipMemcpyAsync(c->h_bres.p, c->d_bres.p, (size_t)nb * 4, hipMemcpyDeviceToHost, sb), "d2h");
  c->hip(hipStreamSynchronize(sb), "sync");
  memcpy(bres.data(), c->h_bres.p, (size_t)nb * 4);
  const double dev_s = elapsed_s(c, c->evb[0], c->evb[1]);
  t_al += dev_s;
  c->dbg.rb.dev_s += dev_s;
  c->dbg.rb.trips += 1;
  c->dbg.rb.launches += nl;
  c->dbg.rb.pairs += nb;
  c->dbg.rb.staged += direct ? 0 : 1;
}

}  // namespace

// Wait for a pass and resolve its block on the host in sorted order (resolve.cpp resolve_block).  Returns false if a
// peer list overflowed (the caller re-runs the block in smaller pieces).
bool resolve_pass(umiclust_ctx* c, Pass& P, const StateView& state, std::vector<int32_t>& new_cents,
                  double& t_pf, double& t_al, double& t_host, int32_t* resolved) {
  const int both = c->both;
  const int32_t q0 = P.q0, w0 = P.w0;
  int32_t nq = P.nq;
  int32_t nqs = nq * both;
  if (resolved) *resolved = 0;
  const double tsync0 = now_s();
  c->hip(hipEventSynchronize(P.ev[4]), "sync");
  c->stats.t_sync_s += now_s() - tsync0;
  c->dbg.t.wait += now_s() - tsync0;
  struct DAcc { double* p; double t0; ~DAcc() { *p += now_s() - t0; } } dtot{&c->dbg.t.total, tsync0};
  P.live = false;
  t_pf += elapsed_s(c, P.ev[0], P.ev[1]);
  if (P.a_timed) {
    const double s = elapsed_s(c, c->a_ev[P.t_slot][0], c->a_ev[P.t_slot][1]);
    t_pf += s;
    c->stats.t_count_s += s;
    c->stats.n_count_launches++;
    tl_add(c->dev, 0, c->a_ev[P.t_slot][0], c->a_ev[P.t_slot][1]);
  } else if (P.c_timed) {
    c->stats.t_count_s += elapsed_s(c, P.ev_c[0], P.ev_c[1]);
    c->stats.n_count_launches++;
    tl_add(c->dev, 0, P.ev_c[0], P.ev_c[1]);
  }
  t_al += elapsed_s(c, P.ev[2], P.ev[3]);
  tl_add(c->dev, 1, P.ev[2], P.ev[3]);
  {
    // records past the DMA'd prefix (a pass that used more than the estimate): fetch the rest now
    const size_t used = *P.h_reccount.p, est = std::min<size_t>(P.rec_est, P.d_rec.n);
    if (used > est && !P.rec_direct) {
      c->hip(hipMemcpyAsync(P.h_rec.p + est, P.d_rec.p + est, (used - est) * 4, hipMemcpyDeviceToHost, c->st_copy),
             "d2h records");
      c->hip(hipStreamSynchronize(c->st_copy), "sync");
    }
    P.rec_est = (uint32_t)std::max<size_t>(1u << 16, used + used / 2 + 4096);
  }
  c->stats.kmer_postings += P.h_counters.p[0];
  c->stats.pairs_peer += P.h_counters.p[8];
  // every alignment the device computed for this pass (walk rounds + speculative peers)
  {
    unsigned long long cw = 0, cp = 0;  // u64 cells of the walk pairs / the peer pairs (counters 12-13 / 14-15)
    memcpy(&cw, P.h_counters.p + 12, 8);
    memcpy(&cp, P.h_counters.p + 14, 8);
    c->stats.cells_computed += (int64_t)(cw + cp);
  }
  // a pageable copy of the per-query-strand outcomes (sequential, revisited below); the records
  // are read in place, only for the query-strands whose relevant peers include a centroid
  const double tc0 = now_s();
  P.hq_copy.assign(P.h_hq.p, P.h_hq.p + nqs);
  {
    uint32_t mx = 0;  // the block's deepest peer list (regrowth: a window far from the cap may double)
    for (int32_t qs = 0; qs < nqs; qs++) mx = std::max<uint32_t>(mx, P.hq_copy[qs].npeer);
    c->last_max_npeer = (int32_t)mx;
  }
  c->stats.t_sync_s += now_s() - tc0;
  c->dbg.t.hq_copy += now_s() - tc0;
  const HostQs* hq = P.hq_copy.data();
  if (!c->pool) c->pool.reset(new WorkPool(pool_threads(c)));
  // the records are copied into pageable memory first (one streaming read; scattered reads of the DMA'd
  // pinned buffer are slow): config 2 +2-3 %
  const uint32_t* recs = P.h_rec.p;
  {
    const double tc1 = now_s();
    // on the resolve threads: one core's streaming read of pinned memory is the limit (0.05 s per config-2 step)
    const size_t nw = *P.h_reccount.p;
    if (P.rec_copy.size() < nw) P.rec_copy.resize(nw + nw / 4);
    const int TC = nw < (1u << 18) ? 1 : c->pool->size();
    if (TC == 1) {
      memcpy(P.rec_copy.data(), P.h_rec.p, nw * 4);
    } else {
      c->pool->run([&](int t) {
        const size_t lo = nw * (size_t)t / (size_t)TC, hi = nw * (size_t)(t + 1) / (size_t)TC;
        memcpy(P.rec_copy.data() + lo, P.h_rec.p + lo, (hi - lo) * 4);
      });
    }
    recs = P.rec_copy.data();
    c->stats.t_sync_s += now_s() - tc1;
    c->dbg.t.rec_copy += now_s() - tc1;
  }
  ResolveEnv env;
  env.hlen = c->hlen.data();
  env.acc = c->h_acc.data();
  env.rank = c->h_rank.data();
  env.both = both;
  env.o4_T = c->o4_T;
  env.maxaccepts = c->p.maxaccepts;
  env.maxrejects = c->p.maxrejects;
  env.hqbin = c->pack_on ? c->hqbin.data() : nullptr;
  env.bin_s = c->bin_s.data();

  // (one context only: several lanes' pools already share the host's cores, config 3 7.59 -> 7.40 M UMIs/s with it)
  // (and only when every pool thread has a CPU of its own under the caller's current mask, L3Pin's included: its
  // workers spin-wait on each other)
  env.par_inorder = g_live_ctx.load() <= 1 && c->pool->size() <= affinity_cpus();
  env.par_min = c->tun.par_min;
  env.debug = c->tun.debug == 1;
  env.target = c->target.data();
  env.strand = c->strand.data();
  env.walk_dump = c->wd.empty() ? nullptr : c->wd.data();
  auto rb = [&](const std::vector<uint32_t>& bpq, const std::vector<uint32_t>& bpt, std::vector<uint32_t>& bres) {
    round_b(c, bpq, bpt, bres, t_al);
  };
  // UMICLUST_RESOLVE_DUMP: the pass's inputs, round-B pairs / results and outputs, for the host-only replay
  // (tools/resolve_tsan_main.cpp: the ThreadSanitizer harness of the CPU suite)
  const bool dump = c->tun.resolve_dump && !c->pack_on && c->dump_want(c->n_resolved);
  c->n_resolved++;
  std::vector<uint32_t> dpq, dpt, dres;
  std::vector<uint8_t> state_in;
  if (dump) state_in.assign(&state[w0], &state[w0] + (q0 + nq - w0));
  RoundB round_b_rec = [&](const std::vector<uint32_t>& bpq, const std::vector<uint32_t>& bpt, std::vector<uint32_t>& bres) {
    rb(bpq, bpt, bres);
    dpq.insert(dpq.end(), bpq.begin(), bpq.end());
    dpt.insert(dpt.end(), bpt.begin(), bpt.end());
    dres.insert(dres.end(), bres.begin(), bres.end());
  };
  ResolveStats rs;
  const double th0 = now_s();
  // partial resolution (resolved != nullptr): the queries before the block's first overflowing one depend on earlier
  // queries only, so they are resolved now and only the rest is re-run
  bool partial = false;
  if (resolved)
    for (int32_t qs = 0; qs < nqs; qs++)
      if (hq[qs].flags & 2u) {
        if (qs / both == 0) return false;
        nq = qs / both;
        nqs = nq * both;
        partial = true;
        break;
      }
  const int r = resolve_block(env, q0, nq, w0, hq, recs, state, P.rsx, *c->pool, new_cents, rs,
                              dump ? round_b_rec : RoundB(rb));
  const double th = now_s() - th0;
  if (r == kResolveOverflow) return false;
  if (r == kResolveStuck) c->fail(UMICLUST_EDEVICE, "internal: a deferred query of block %d is still unresolved", q0);
  if (r == kResolveBadPeer) c->fail(UMICLUST_EDEVICE, "internal: a peer of block %d is not an earlier query", q0);
  if (dump)
    write_resolve_dump(c, env, q0, nq, w0, state, state_in, hq, recs, *P.h_reccount.p, dpq, dpt, dres, new_cents, rs);
  t_host += th - rs.t_round_b_s;
  // UMICLUST_DEBUG: one line per resolved block (where the host's time goes, block by block)
  if (c->tun.debug == 1)
    fprintf(stderr, "blk q0 %d nq %d new %zu wait %.3f classify %.3f inorder %.3f roundB %.3f (%lld pairs) merged %lld "
            "deferred %lld ms-since-wait %.3f\n", q0, nq, new_cents.size(), 1e3 * (tc0 - tsync0), 1e3 * rs.t_classify_s,
            1e3 * rs.t_inorder_s, 1e3 * rs.t_round_b_s, (long long)rs.pairs_round_b, (long long)rs.n_merged_walks,
            (long long)rs.n_deferred, 1e3 * (now_s() - tsync0));
  c->stats.t_host_pass1_s += rs.t_classify_s + rs.t_inorder_s;
  c->dbg.t.classify += rs.t_classify_s;
  c->dbg.t.inorder += rs.t_inorder_s;
  c->dbg.t.round_b += rs.t_round_b_s;
  c->dbg.t.resolve_block += th;
  c->stats.n_alignments += rs.n_alignments;
  c->stats.cells += rs.cells;
  c->stats.n_merged_walks += rs.n_merged_walks;
  c->stats.t_merged_s += rs.t_merged_s;
  c->stats.n_deferred += rs.n_deferred;
  c->stats.pairs_round_b += rs.pairs_round_b;
  c->stats.cells_computed += rs.cells_round_b;
  DebugSums& d = c->dbg;  // (ResolveStats keeps arrays: resolve.cpp indexes them by the class it computes)
  d.mispredicted += rs.dbg[0], d.saved += rs.dbg[1], d.blocked += rs.dbg[2];
  d.q_no_record += rs.dbg_q[0], d.q_earlier_only += rs.dbg_q[1], d.q_in_block += rs.dbg_q[2], d.q_host_ns += rs.dbg_q[3];
  d.s_inline += rs.dbg_p[0], d.s_many_relevant += rs.dbg_p[1], d.s_record_read += rs.dbg_p[2];
  d.s_peers_scanned += rs.dbg_p[3];
  if (resolved) *resolved = nq;
  return !partial;
}

}  // namespace uc
