// plan.cpp -- block planning and cluster numbering (plan.h): integer policy only, no HIP.
#include "plan.h"

#include <algorithm>

#include "resolve.h"

namespace uc {

void BlockPlan::start(int32_t b_hint) {
  b_eff = hqbin ? B : (int32_t)std::min<int64_t>(B, std::max<int64_t>(kMinBlock, (int64_t)b_hint * 2));
  eff_bin = -1;
  clean = 0;
  blocks.clear();
  split_blocks(s0, b_eff);
}

void BlockPlan::split_blocks(int32_t from, int32_t bmax) {
  if (from >= s1) return;
  // packs: bmax (a deep cluster's halved size) holds until the end of `from`'s bin, the next bins start at B
  const int32_t until = hqbin ? bin_s[hqbin[from] + 1] : s1;
  for (int32_t q0 = from; q0 < s1;) {
    int32_t same = 1;
    const int32_t bcap = q0 < until ? bmax : B;
    if (mix) {  // across length changes, at most kSegLens lengths (one pair segment each)
      const int32_t lim = std::min<int32_t>(bcap, s1 - q0);
      int32_t lo = hlen[q0], hi = lo;  // (a pack's lengths restart at every bin)
      while (same < lim && std::max<int32_t>(hi, hlen[q0 + same]) - std::min<int32_t>(lo, hlen[q0 + same]) < kSegLens) {
        lo = std::min<int32_t>(lo, hlen[q0 + same]);
        hi = std::max<int32_t>(hi, hlen[q0 + same]);
        same++;
      }
    } else {
      while (q0 + same < s1 && same < bcap && hlen[q0 + same] == hlen[q0]) same++;
    }
    // O4: a block cut by the size cap ends at a round start (trimmed by < 1 round), so the next block's window needs
    // no round tile: only blocks starting at a length change (or a bin start in a pack) still begin mid-round
    // (same-box A/B: config 3 +2.2 %, config 5 +1.8 %, config 2 unchanged; profiles/r05/round_align_ab/)
    if (o4_T && same == bcap && q0 + same < s1) {
      const int32_t r = o4_round_start(o4_T, hqbin, bin_s, s0, q0 + same);
      if (r > q0 + same / 2) same = r - q0;
    }
    blocks.push_back({q0, same});
    q0 += same;
  }
}

bool BlockPlan::halve(int32_t q) {
  if (hqbin && hqbin[q] != eff_bin) {
    eff_bin = hqbin[q];
    b_eff = B;
  }
  if (b_eff <= kMinBlock) return false;
  b_eff = std::max(kMinBlock, b_eff / 2);
  return true;
}

void BlockPlan::overflowed(int32_t k) {
  clean = 0;
  if (k + 1 < nb() && halve(blocks[k].first)) {
    const int32_t from = blocks[k].first + blocks[k].second;
    blocks.resize((size_t)k + 1);
    split_blocks(from, b_eff);
  }
}

bool BlockPlan::resolved(int32_t k, int D, int32_t max_npeer) {
  if (max_npeer >= kRegrowDepth) {
    clean = 0;  // a deep window: no regrowth yet, and it does not count as a clean block
    return false;
  }
  if (!(regrow > 0 && b_eff < B && ++clean >= regrow && k + D < nb())) return false;
  b_eff = std::min<int32_t>(B, b_eff * 2);
  clean = 0;
  const int32_t from = blocks[k + D].first;
  blocks.resize((size_t)k + D);
  split_blocks(from, b_eff);
  return true;
}

void number_clusters(int32_t s0, int32_t s1, const std::vector<int32_t>& cent, const int32_t* target,
                     bool clusterout_sort, const int32_t* hqbin, int32_t bin0, int32_t nbins, int32_t* cno, int32_t* ocl,
                     ClusterNumbers& out) {
  // creation numbers: centroids in creation (= sorted seqno) order, members inherit their centroid's
  const int32_t K = (int32_t)cent.size();
  for (int32_t k = 0; k < K; k++) cno[cent[k]] = k;
  for (int32_t s = s0; s < s1; s++)
    if (target[s] >= 0) cno[s] = cno[target[s]];
  // output numbering: --clusterout_sort orders clusters by size desc, creation order
  std::vector<int32_t> size(K, 0);
  for (int32_t s = s0; s < s1; s++) size[cno[s]]++;
  std::vector<int32_t> order(K);
  for (int32_t k = 0; k < K; k++) order[k] = k;
  auto cbin = [&](int32_t k) { return hqbin ? hqbin[cent[k]] : bin0; };
  if (clusterout_sort)
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
      const int32_t ba = cbin(a), bb = cbin(b);
      return ba != bb ? ba < bb : size[a] > size[b];
    });
  out.rank_of.assign(K, 0);
  for (int32_t k = 0; k < K; k++) out.rank_of[order[k]] = k;
  out.ostart.assign((size_t)K + 1, 0);
  for (int32_t s = s0; s < s1; s++) {
    ocl[s] = out.rank_of[cno[s]];
    out.ostart[ocl[s] + 1]++;
  }
  for (int32_t k = 0; k < K; k++) out.ostart[k + 1] += out.ostart[k];
  out.omemb.assign(s1 - s0, 0);
  {
    std::vector<int32_t> fill(out.ostart.begin(), out.ostart.end() - 1);
    for (int32_t s = s0; s < s1; s++) out.omemb[fill[ocl[s]]++] = s;
  }
  // per bin: its output clusters are the consecutive output numbers [k0, k1); numbers within the bin
  out.bin_k.assign((size_t)nbins + 1, 0);
  for (int32_t b = 0, k1 = 0; b < nbins; b++) {
    while (k1 < K && cbin(order[k1]) == bin0 + b) k1++;
    out.bin_k[b + 1] = k1;
  }
  if (hqbin)
    for (int32_t s = s0; s < s1; s++) ocl[s] -= out.bin_k[hqbin[s] - bin0];
}

TracePlan plan_traceback(const uint8_t* hlen, const int32_t* target, const uint8_t* strand, int32_t lo, int32_t hi,
                         int32_t x0, int32_t* slot, uint32_t* pq, uint32_t* pt) {
  TracePlan tp;
  tp.x0 = x0;
  int32_t x = x0;
  for (int pass = 0; pass < 2; pass++) {
    int32_t& maxq = pass ? tp.maxq2 : tp.maxq1;
    for (int32_t s = lo; s < hi; s++)
      if (target[s] >= 0 && (((int32_t)hlen[s] <= kTwSplit) == (pass == 0))) {
        slot[s - lo] = x;
        pq[x] = ((uint32_t)s << 1) | strand[s];
        pt[x] = (uint32_t)target[s];
        maxq = std::max(maxq, (int32_t)hlen[s]);
        x++;
      }
    if (pass == 0) tp.n1 = x - x0;
  }
  tp.n2 = x - x0 - tp.n1;
  return tp;
}

int32_t traceback_maxl(const uint8_t* hlen, int32_t s0, int32_t s1) {
  return s1 > s0 ? *std::max_element(hlen + s0, hlen + s1) : kMaxLen;
}

}  // namespace uc
