// plan.h -- the integer policy of one clustering call, host-only C++ (no HIP): how a bin's sorted queries are cut
// into greedy blocks and re-cut after peer overflows and clean stretches (BlockPlan), and how the finished clusters
// are numbered for the output (number_clusters), and which member traceback goes to which launch and slot
// (plan_traceback).  driver.cpp's cluster_all drives them through ClusterRun (umiclust_consensus the last); tools/plan_check_main.cpp
// (tests/test_plan_cpu.py) exercises them under ASan + UBSan without a GPU.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#include "umiclust_consts.h"

namespace uc {

// Halving stops at 256 queries (a floor of kPeerCap / 4 = 32, at which no window can overflow, ran config 4's
// giant-molecule bin 200 in 8,578 blocks: 1.44 s alone against 0.6 s at 256; a peer-load feedback that re-cut the
// queued blocks from each block's largest peer list lost on config 5: profiles/r04/block_policy)
constexpr int32_t kMinBlock = 256;
// a block whose deepest peer list reaches this is not clean (regrowth)
constexpr int32_t kRegrowDepth = kPeerCap / 4;

// The blocks of the sorted seqnos [s0, s1): at most B queries each, of one length (the aligner is compiled per query
// length) or, mixed, of fewer than kSegLens lengths (one pair segment each).
struct BlockPlan {
  // what the plan reads (set by the caller before start)
  const uint8_t* hlen = nullptr;   // sorted lengths, absolute seqno
  int32_t s0 = 0, s1 = 0;
  int32_t B = 1;                   // the full block size
  bool mix = false;                // blocks across length changes
  int32_t o4_T = 0;                // policy O4: rounds of o4_T queries; 0 = sequential
  const int32_t* hqbin = nullptr;  // packs: sorted seqno -> load bin (nullptr: one bin)
  const int32_t* bin_s = nullptr;  // packs: each load bin's first sorted seqno
  int32_t regrow = 0;              // clean blocks after which the size doubles (0: never)
  // the plan
  std::vector<std::pair<int32_t, int32_t>> blocks;  // (first seqno, queries)
  int32_t b_eff = 1;     // the size blocks are cut at now
  int32_t eff_bin = -1;  // packs: the bin b_eff was last halved in (a deep cluster of one bin does not shrink the next)
  int32_t clean = 0;     // blocks resolved since the last overflow or deep window

  int32_t nb() const { return (int32_t)blocks.size(); }
  // Cut [s0, s1).  A bin starts at the block size the previous one ended with (b_hint), doubled: deep bins tend to
  // follow deep bins.  A pack starts at B.
  void start(int32_t b_hint);
  // append the blocks from query `from` on, of at most `bmax` queries
  void split_blocks(int32_t from, int32_t bmax);
  // halve the block size for q's bin; false: already at the smallest block
  bool halve(int32_t q);
  // Block k overflowed a peer list.  Deep clusters flood the peer window: the blocks after k are cut at half the size
  // (a smaller window holds fewer same-molecule peers), so the overflow re-runs do not repeat block after block.
  void overflowed(int32_t k);
  // Block k resolved without an overflow, its deepest peer list max_npeer; passes up to block k + D - 1 are queued.
  // Regrowth: after `regrow` consecutive clean blocks whose deepest peer list stayed below kRegrowDepth, the blocks not
  // yet queued (from block k + D) are cut at twice the size.  True: re-cut, and block k + D's prebuilt peer tile is
  // stale.  With overflowing blocks resolved up to their first overflowing query, a giant molecule's stretch no longer
  // pins a bin at 256-query blocks: config 4's bin 200 7.0 -> 1.6 s among 8 lanes, config 4 6.51 -> 7.59 M UMIs/s;
  // config 5's windows stay deep, so its blocks do not grow (3.33 / 3.36 M; ungated regrowth after 4 clean blocks:
  // 2.47 M) -- profiles/r05/regrow_ab/.
  bool resolved(int32_t k, int D, int32_t max_npeer);
};

// Cluster numbers of the sorted seqnos [s0, s1) once every target is final.  cent: the centroids' seqnos in creation
// (= sorted seqno) order; target[s]: the centroid seqno member s joined, -1 for a centroid.  cno, target and ocl are
// indexed by absolute seqno.  hqbin (packs: seqno -> load bin, bins [bin0, bin0 + nbins); nullptr: one bin).
struct ClusterNumbers {
  std::vector<int32_t> rank_of;        // creation number -> output number
  std::vector<int32_t> ostart, omemb;  // members per output cluster (centroid first), over the whole range
  std::vector<int32_t> bin_k;          // [nbins + 1] bin b's output clusters are the numbers [bin_k[b], bin_k[b + 1])
};
// cno[s]: the creation number (members inherit their centroid's); ocl[s]: the output number -- creation order, or with
// clusterout_sort by size descending, stable.  A pack's clusters stay grouped by bin (creation order already is), are
// sorted within their bin, and ocl counts from the bin's first cluster.
void number_clusters(int32_t s0, int32_t s1, const std::vector<int32_t>& cent, const int32_t* target,
                     bool clusterout_sort, const int32_t* hqbin, int32_t bin0, int32_t nbins, int32_t* cno, int32_t* ocl,
                     ClusterNumbers& out);

// The member tracebacks of the sorted seqnos [lo, hi) once every target is final (k_trace_wave, one wave per member):
// queries of at most kTwSplit nt go to a launch of their own, whose one-stripe direction store lets more waves share
// a CU, the longer ones to a second launch.  Members take consecutive traceback slots from x0 on, the first launch's
// before the second's, each in seqno order.
constexpr int32_t kTwSplit = 64;
struct TracePlan {
  int32_t x0 = 0;                // the first launch's first slot
  int32_t n1 = 0, n2 = 0;        // members of the first launch (slots [x0, x0 + n1)) and of the second (the next n2)
  int32_t maxq1 = 0, maxq2 = 0;  // each launch's longest query (0: no member)
};
// hlen, target and strand are indexed by absolute seqno (target[s] < 0: a centroid, not traced).  slot[s - lo] = the
// member's slot (a centroid's entry is left alone), pq[x] = (member seqno << 1) | strand and pt[x] = its centroid's
// seqno for every slot x given out; pq and pt are indexed by slot and hold x0 + (members of [lo, hi)) entries.
TracePlan plan_traceback(const uint8_t* hlen, const int32_t* target, const uint8_t* strand, int32_t lo, int32_t hi,
                         int32_t x0, int32_t* slot, uint32_t* pq, uint32_t* pt);
// the longest sequence among the seqnos [s0, s1), which sizes a traceback wave's LDS (kMaxLen for an empty range)
int32_t traceback_maxl(const uint8_t* hlen, int32_t s0, int32_t s1);

}  // namespace uc
