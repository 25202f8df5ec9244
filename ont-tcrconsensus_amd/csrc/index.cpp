// index.cpp -- the LSM centroid index of the bin being clustered (cluster_ctx.h Index): tile builds, the postings
// arena's layout, appends and the views a prefilter launch reads.  Every writer of the index's fields is here.
#include "cluster_ctx.h"

namespace uc {

// postings vbase + ((xoff + c) % seg_mod) / kParts (umiclust_internal.h), in the tile's arena slot
void build_tile(umiclust_ctx* c, Tile& t, const int32_t* map, int32_t first, int32_t n, int32_t xoff, int32_t vbase,
                int32_t seg_mod, hipStream_t st) {
  if (!st) st = c->st;
  if (!t.hist.p) {
    c->hip(t.hist.ensure(kBins), "tile alloc");
    c->hip(hipMemsetAsync(t.hist.p, 0, (size_t)kBins * 4, st), "tile memset");
  }
  c->hip(t.off.ensure(kBins + 1), "tile alloc");
  c->hip(t.cursor.ensure(kBins), "tile alloc");
  c->hip(t.partial.ensure(kScanBlocks), "tile alloc");
  if (tile_cap(n) > t.post_cap) c->fail(UMICLUST_EDEVICE, "internal: index tile slot too small");
  uint16_t* post = c->ix.arena.p + t.post_base;
  c->hip(launch_index_count(c->d_kmers.p, c->d_nk.p, map, first, n, xoff, t.hist.p, st), "index count");
  c->hip(launch_index_scan(t.hist.p, t.partial.p, t.off.p, t.cursor.p, post, st), "index scan");
  c->hip(launch_index_fill(c->d_kmers.p, c->d_nk.p, map, first, n, xoff, vbase, seg_mod, t.cursor.p, post, st),
         "index fill");
  // bank-aware posting order (kernels.hip k_list_arrange): large tiles (the base tile and sealed tiles, built
  // once per fold / seal); the small ones (delta, peer and round tiles, rebuilt every block) keep the fill's order
  if (n >= 2 * kDelta)
    c->hip(launch_index_arrange(t.off.p, post, st), "index arrange");
  t.n = n;
  t.built_n = n;
}

void Index::reset(int32_t n) {
  cent.clear();
  cent.reserve((size_t)n + 1);
  cent_len.clear();
  std::fill(cnt_ge, cnt_ge + kMaxLen + 1, 0);
  cent_len.reserve((size_t)n + 1);
  c->hip(hipStreamSynchronize(c->st), "sync");  // no queued work may still read the old tiles
  tiles.clear();
  base_tile.n = delta_tile[0].n = delta_tile[1].n = 0;
  c->last_a_slot = -1;  // (the base tile's latest reader: no counting half is queued)
  sealed_end = base_end = 0;
  index_end = 0;
  nix = 0;
  c->hip(d_cent.ensure((size_t)n + 1), "alloc cent");
  c->hip(d_cent_len.ensure((size_t)n + 1), "alloc cent");
  c->hip(h_cent.ensure((size_t)n + 1), "pin cent");
  c->hip(h_cent_len.ensure((size_t)n + 1), "pin cent");
  c->hip(d_seq2ord.ensure((size_t)n + 1), "alloc seq2ord");
  c->hip(h_seq2ord.ensure((size_t)n + 1), "pin seq2ord");
  std::fill(h_seq2ord.p, h_seq2ord.p + n, -1);
  c->hip(hipMemsetAsync(d_seq2ord.p, 0xff, (size_t)n * 4, c->st), "memset");
}

// postings arena: the base, delta, peer-ring and solo slots, then the sealed tile slots in creation
// order (n / kTile of them at most); a prefilter pass reads the slots of one counter segment (plus
// the unsealed ones in its last pass), which keeps its 32-bit buffer offsets in range
void Index::layout(int32_t n, int32_t T4) {
  uint64_t off = 0;
  auto slot = [&](Tile& t, int64_t nseq) {
    t.post_base = off;
    t.post_cap = tile_cap(nseq);
    off += t.post_cap;
  };
  slot(base_tile, kTile);
  slot(delta_tile[0], kDelta);
  slot(delta_tile[1], kDelta);
  for (Tile& t : c->blk_tile) slot(t, kMaxBlock);
  slot(c->solo_tile, kMaxBlock);
  if (T4)
    for (Tile& t : c->round_tile) slot(t, T4);
  sealed_slot0 = off;
  off += (uint64_t)(n / kTile) * tile_cap(kTile);
  c->hip(arena.ensure((size_t)off + 64), "alloc arena");
}

int32_t Index::stage_views(PinBuf<TileView>& h, DevBuf<TileView>& d, hipStream_t st) {
  int32_t nv = 0;
  const size_t need = tiles.size() + 2;
  if (need > h.n) {
    c->hip(hipStreamSynchronize(st), "sync");  // rare: the views array grows
    c->hip(h.ensure(need * 2), "pin");
    c->hip(d.ensure(need * 2), "alloc");
  }
  for (const auto& t : tiles)
    if (t->n > 0) h.p[nv++] = view_of(*t);
  if (base_tile.n > 0) h.p[nv++] = view_of(base_tile);
  if (delta_tile[delta_cur].n > 0) h.p[nv++] = view_of(delta_tile[delta_cur]);
  if (nv > kArgTiles)
    c->hip(hipMemcpyAsync(d.p, h.p, (size_t)nv * sizeof(TileView), hipMemcpyHostToDevice, st), "tiles");
  return nv;
}

// Enqueued on the main stream (split passes: the side stream) behind any queued pass, which keeps reading the tiles
// as they were when it was enqueued.
void Index::append(const std::vector<int32_t>& new_cents) {
  if (new_cents.empty()) return;
  hipStream_t st = c->ix_st ? c->ix_st : c->st;
  if (c->ix_st && c->last_r_ev) c->hip(hipStreamWaitEvent(st, c->last_r_ev, 0), "wait");
  const int32_t ord0 = (int32_t)cent.size();
  int32_t s2o_lo = 0, s2o_n = 0, bo_lo = 0, bo_n = 0;
  for (int32_t q : new_cents) {  // capacity reserved: no reallocation
    cent.push_back(q);
    cent_len.push_back(c->hlen[q]);
    for (int L = 0; L <= c->hlen[q]; L++) cnt_ge[L]++;
  }
  {
    // seqno -> ordinal for the merge's flagged hits (the new centroids are in sorted order)
    const int32_t s0 = c->bin_s[c->cur_bin];
    for (size_t i = 0; i < new_cents.size(); i++) h_seq2ord.p[new_cents[i] - s0] = ord0 + (int32_t)i;
    s2o_lo = new_cents.front() - s0;
    s2o_n = std::max(0, new_cents.back() - s0 - s2o_lo + 1);
  }
  if (c->pack_on) {
    // a bin's first query is always a centroid (nothing of its bin precedes it): its ordinal opens the bin's range
    // (the bins starting inside this append are consecutive: one copy)
    int32_t blo = INT32_MAX, bhi = -1;
    for (size_t i = 0; i < new_cents.size(); i++) {
      const int32_t q = new_cents[i], b = c->hqbin[q];
      if (q == c->bin_s[b]) {
        c->h_bin_ord0.p[b] = ord0 + (int32_t)i;
        blo = std::min(blo, b);
        bhi = std::max(bhi, b);
      }
    }
    if (bhi >= blo) {
      bo_lo = blo;
      bo_n = bhi - blo + 1;
    }
  }
  memcpy(h_cent.p + ord0, cent.data() + ord0, new_cents.size() * 4);
  memcpy(h_cent_len.p + ord0, cent_len.data() + ord0, new_cents.size());
  // one dispatch reads the pinned ranges (as the copies it replaces, at its execution time)
  c->hip(launch_append_stage(h_cent.p + ord0, h_cent_len.p + ord0, (int32_t)new_cents.size(), d_cent.p + ord0,
                             d_cent_len.p + ord0, h_seq2ord.p + s2o_lo, d_seq2ord.p + s2o_lo, s2o_n,
                             bo_n ? c->h_bin_ord0.p + bo_lo : nullptr, bo_n ? c->d_bin_ord0.p + bo_lo : nullptr, bo_n,
                             st),
         "append stage");
  const int32_t ordend = (int32_t)cent.size();
  if (nix >= ix_events.size()) ix_events.emplace_back();
  auto& ev = ix_events[nix++];
  c->hip(hipEventRecord(ev.first.get(c), st), "event");
  while (ordend - sealed_end >= kTile) {  // seal a full tile
    auto t = std::make_unique<Tile>();
    t->base = sealed_end;
    t->seg = t->base / kSegCentroids;
    t->post_cap = tile_cap(kTile);
    t->post_base = sealed_slot0 + (uint64_t)tiles.size() * t->post_cap;
    build_tile(c, *t, d_cent.p, t->base, kTile, t->base, kCentBase, kSegCentroids, st);
    tiles.push_back(std::move(t));
    sealed_end += kTile;
    base_end = std::max(base_end, sealed_end);
    base_tile.n = 0;
  }
  if (ordend - base_end > kDelta) {  // fold the delta into the base tile
    // the base is rebuilt in place: the latest counting half may still read it
    if (c->last_a_slot >= 0) c->hip(hipStreamWaitEvent(st, c->a_ev[c->last_a_slot][1], 0), "wait");
    base_tile.base = sealed_end;
    base_tile.seg = sealed_end / kSegCentroids;
    build_tile(c, base_tile, d_cent.p, sealed_end, ordend - sealed_end, sealed_end, kCentBase, kSegCentroids, st);
    base_end = ordend;
  }
  // the other delta slot was last read by a counting half the main stream has already waited for (the
  // second half of its pass precedes this append)
  delta_cur ^= 1;
  Tile& dt = delta_tile[delta_cur];
  dt.base = base_end;
  dt.seg = base_end / kSegCentroids;
  if (ordend > base_end)
    build_tile(c, dt, d_cent.p, base_end, ordend - base_end, base_end, kCentBase, kSegCentroids, st);
  else
    dt.n = 0;
  index_end = ordend;
  c->hip(hipEventRecord(ev.second.get(c), st), "event");
  if (c->ix_st) c->hip(hipEventRecord(c->ix_done.get(c), st), "event");
}

void Index::add_unindexed(const std::vector<int32_t>& cents) { cent.insert(cent.end(), cents.begin(), cents.end()); }

double Index::t_index_s() {
  double t = 0;
  for (size_t i = 0; i < nix; i++) t += elapsed_s(c, ix_events[i].first, ix_events[i].second);
  return t;
}

}  // namespace uc
