// cluster_ctx.h -- clustering's context and what its host files share: the index (index.cpp), the passes (pass.cpp),
// load and prepare (load.cpp), the file path (file_path.cpp), the kernel-level probes (probes.cpp), the timeline
// (timeline.cpp) and the pipeline, the context's life cycle and the session ABI (driver.cpp).  Included by those
// files only; the drop-ins see the core of ctx.h.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <utility>
#include <vector>

#include "ctx.h"
#include "plan.h"
#include "resolve.h"

struct umiclust_ctx;

namespace uc {

// Policy constants of the host side, with what they were measured against (the block planner's are in plan.h)
constexpr int32_t kDelta = 8192;  // centroids in the per-block delta tile before folding into base
// passes in flight: 2; 3 (window of three blocks) hides more host time but its extra peers cost more than that
// on configs 2/3/5 (profiles/r02/pipeline_depth_sweep.json)
constexpr int32_t kDepth = 2;
constexpr int32_t kBlockMin = 2048;  // the smallest default block (Tunables::block_div)
// small blocks (deep clusters: config 5's ~2k-query blocks) write their outcomes and records straight into pinned host
// memory: their copies are dispatch-bound (`profiles/r05/recdirect_small_ab/`: config 5 3.52 -> 3.64 M UMIs/s, config
// 2's 8k-query blocks lose with it)
constexpr int32_t kDirectRecQ = 4096;
// speculative walk below this best k-mer count (20 and 30 equal, 45 slower: profiles/r03/spec_ab)
constexpr int32_t kSpecThr = 30;
// lazy peers below this new-centroid rate (per mille; higher rates lose: profiles/r02/lazy_peer_sweep.json)
constexpr int32_t kLazyPermille = 5;
constexpr int32_t kRbDirect = 4096;  // round B: at most this many pairs read / written in pinned memory

// UMICLUST_DEBUG: what the per-bin summary reports, summed over the bin's passes
struct DebugSums {
  struct {  // resolve_pass phases and the pipeline's host side (s)
    double wait = 0, hq_copy = 0, rec_copy = 0, classify = 0, inorder = 0, enqueue = 0, total = 0, appends = 0,
           round_b = 0, resolve_block = 0;
  } t;
  struct {  // round B: device time between its first and last launch's events (s), round trips, launches, pairs,
            // trips of more than kRbDirect pairs
    double dev_s = 0, trips = 0, launches = 0, pairs = 0, staged = 0;
  } rb;
  int64_t mispredicted = 0, saved = 0, blocked = 0;  // relevant peers predicted members that were not / were / undetermined
  // queries without records / records with only earlier-block relevant peers / with an in-block relevant peer / host ns
  // in pass 1
  int64_t q_no_record = 0, q_earlier_only = 0, q_in_block = 0, q_host_ns = 0;
  // strands on the inline path / with > kInlineRel relevant peers / reading their record / peers scanned there
  int64_t s_inline = 0, s_many_relevant = 0, s_record_read = 0, s_peers_scanned = 0;
};

struct Tile {
  DevBuf<uint32_t> hist;      // [kBins], all zero between builds (the scan re-zeroes it)
  DevBuf<uint32_t> off;       // [kBins + 1] padded list offsets, tile-relative
  DevBuf<uint32_t> cursor;    // [kBins]
  DevBuf<uint32_t> partial;   // [kScanBlocks]
  uint64_t post_base = 0;     // the tile's slot in the postings arena
  size_t post_cap = 0;        // slot capacity (postings)
  int32_t n = 0;              // sequences
  int32_t base = 0;           // first centroid ordinal / first seqno (peer tiles)
  int32_t seg = 0;            // counter segment / peer region
  int32_t len = 0;            // peer tiles: the block's query length
  int32_t built_n = -1;       // n at last build
  bool prebuilt = false;      // peer tile built ahead of its pass (for the block [base, base + n))
};

// One greedy block in flight: its own peer tile, device outputs and pinned mirrors, so the device
// runs block k+1 while the host resolves block k.
struct Pass {
  int32_t q0 = 0, nq = 0, w0 = 0;  // block [q0, q0+nq), peer window [w0, q0+nq)
  bool live = false;
  bool rec_direct = false;  // this pass's outcomes and records written by k_pack into pinned host memory
  PinBuf<TileView> h_tiles;
  DevBuf<TileView> d_tiles;
  DevBuf<uint32_t> d_top_seqno;
  DevBuf<uint8_t> d_top_count, d_ntop;
  DevBuf<uint32_t> d_pcand, d_units;  // per-(query-strand, part) prefilter candidates, overflowed units
  DevBuf<uint8_t> d_pncand, d_ppeer_count, d_pnpeer;
  DevBuf<uint32_t> d_ppost;  // postings touched per (query-strand, part), summed by k_pf_merge
  DevBuf<uint16_t> d_ppeer_id;
  DevBuf<uint16_t> d_peer_id;
  DevBuf<uint8_t> d_peer_count, d_npeer;
  bool ctr_zeroed = false;      // d_counters re-zeroed by the last k_pack on this buffer set
  DevBuf<uint32_t> d_counters;  // [0] postings, [1..5] npairs per walk round, [8] peer pairs,
                                // [9] target residues of walk pairs, [10] of peer pairs
  DevBuf<uint32_t> d_pq, d_pt, d_outidx, d_res;
  DevBuf<WalkState> d_ws;
  DevBuf<HostQs> d_hq;              // k_pack's per query-strand outcomes, copied to h_hq by DMA
  DevBuf<unsigned long long> d_paligned;  // per query-strand: the peers k_peer_pairs aligned
  DevBuf<uint32_t> d_reccount;
  DevBuf<uint32_t> d_rec;           // k_pack's records, copied to h_rec by DMA (a prefix of rec_est words;
                                    // the host fetches the rest in the rare pass that used more)
  uint32_t rec_est = 1u << 16;
  // host side: per query-strand outcomes and records (DMA), counters (written by k_pack), record words used
  PinBuf<HostQs> h_hq;
  PinBuf<uint32_t> h_rec, h_counters, h_reccount;
  std::vector<HostQs> hq_copy;
  std::vector<uint32_t> rec_copy;
  ResolveScratch rsx;  // resolve_block's classification scratch (resolve.h)
  Event ev[5];         // prefilter begin/end, align begin/end, results in host memory
  // split passes: the counting half (enqueue_count) of the block this buffer set serves next
  PinBuf<TileView> h_tiles_a;
  DevBuf<TileView> d_tiles_a;
  DevBuf<uint32_t> d_anunits;  // overflowed units of the lean kernel (the merge resets it)
  Event ev_a;                  // after the counting half's view upload (h_tiles_a may be rewritten)
  Event ev_c[2];               // whole passes: the counting kernel alone
  bool c_timed = false;
  bool a_live = false, a_timed = false;
  int32_t a_q0 = -1, a_base = 0, a_slot = 0, t_slot = 0;
};

// What a pass's prefilter ran, for umiclust_prefilter and its siblings (the kernel-level parity entries)
struct PfCapture {
  uint32_t* h_nunits = nullptr;  // pinned: *nunits between the lean kernel and the full kernel over its units
  int32_t ntiles = 0, nseg = 0, one_wave = 0;  // centroid tiles read, counter segments, k_pf_count<0, 1> launched
  int32_t ntiles_count = 0;      // split passes: centroid tiles the counting half read (ntiles: the second half)
};

// The centroid index of the bin being clustered (index.cpp): sealed tiles (kTile centroids each, built once) + an
// open base tile (rebuilt every kDelta new centroids) + a delta tile (rebuilt every block) -- an LSM layout, so a
// block only rebuilds postings of at most kDelta centroids -- with the centroid tables the kernels read beside them.
// index.cpp holds every writer of these fields; the passes and the probes read them.
struct Index {
  umiclust_ctx* const c;
  std::vector<std::unique_ptr<Tile>> tiles;  // sealed
  Tile base_tile, delta_tile[2];  // the delta alternates: a counting half may still read the previous one
  int32_t delta_cur = 0;
  int32_t sealed_end = 0, base_end = 0;
  int32_t index_end = 0;          // centroid ordinals [0, index_end) are indexed
  DevBuf<uint16_t> arena;         // postings of every tile (one buffer, one descriptor per pass)
  uint64_t sealed_slot0 = 0;      // arena index of sealed tile 0's slot
  std::vector<int32_t> cent;      // ordinal -> seqno (current bin)
  std::vector<uint8_t> cent_len;
  DevBuf<int32_t> d_cent;         // ordinal -> seqno
  DevBuf<uint8_t> d_cent_len;     // ordinal -> length
  // pinned mirrors of cent / cent_len: every ordinal is uploaded once per bin from here (asynchronous DMA)
  PinBuf<int32_t> h_cent;
  PinBuf<uint8_t> h_cent_len;
  int32_t cnt_ge[kMaxLen + 1] = {};  // centroids of length >= L
  DevBuf<int32_t> d_seq2ord;      // [seqno - bin start] centroid ordinal or -1 (the merge's flagged hits)
  PinBuf<int32_t> h_seq2ord;
  std::vector<std::pair<Event, Event>> ix_events;  // index rebuild timing
  size_t nix = 0;

  explicit Index(umiclust_ctx* ctx) : c(ctx) {}
  // an empty index for a bin of n sequences, once the main stream has run what still reads the old tiles
  void reset(int32_t n);
  // the postings arena's slots: the index's own and the pipeline's peer tiles (T4: the O4 round tiles too)
  void layout(int32_t n, int32_t T4);
  // a block's new centroids (sorted seqnos) join the index, enqueued behind any queued pass
  void append(const std::vector<int32_t>& new_cents);
  // centroids that got creation numbers but never reach the index (O4: still pending when the bin ends)
  void add_unindexed(const std::vector<int32_t>& cents);
  // The tile views (sealed tiles, then base and current delta: segment order) in the pinned array h, uploaded to its
  // device mirror d on st when they are too many for the kernel arguments.  Returns their number.
  int32_t stage_views(PinBuf<TileView>& h, DevBuf<TileView>& d, hipStream_t st);
  // counter segments the indexed centroids span
  int32_t nseg() const { return (index_end + kSegCentroids - 1) / kSegCentroids; }
  // device time of the bin's appends so far (s); the streams are drained
  double t_index_s();
};

}  // namespace uc

// Clustering's state, on the core every entry point shares (ctx.h: device, main stream, error text, tunables, stats
// and the drop-ins' own state).
struct umiclust_ctx : uc::Ctx {
  template <typename T>
  using DevBuf = uc::DevBuf<T>;
  template <typename T>
  using PinBuf = uc::PinBuf<T>;
  umiclust_params p{};
  uc::Scoring sc{};
  int both = 2;
  bool ambig = false;             // some kept sequence holds a non-ACGT (IUPAC) symbol
  bool loaded = false;
  bool clustered = false;
  bool counted = false;           // this context is one of g_live_ctx
  DevBuf<unsigned long long> pf_prof;  // prefilter phase clocks (UMICLUST_PFPROF)

  // input (host copies kept only for the file path outputs).  A load holds one or more independent
  // region bins (umiclust_load_bins): bin b is input records [bin_in[b], bin_in[b+1]) and sorted
  // seqnos [bin_s[b], bin_s[b+1]) -- every bin is length-sorted on its own and clustered on its own,
  // with absolute seqnos on the device.
  int64_t n_input = 0;
  int32_t n = 0;                  // kept sequences (all bins)
  std::vector<int32_t> perm;      // sorted -> input index
  std::vector<uint8_t> hlen;      // sorted lengths
  std::vector<int64_t> bin_in;    // [nbins + 1] input record boundaries
  std::vector<int32_t> bin_s;     // [nbins + 1] sorted seqno boundaries
  int32_t cur_bin = -1;           // bin of the last umiclust_cluster* call

  // device: sequences
  DevBuf<char> d_ascii;
  DevBuf<int64_t> d_offs;
  DevBuf<int32_t> d_perm;
  DevBuf<uint32_t> d_codes;
  DevBuf<uint8_t> d_lens;
  DevBuf<uint16_t> d_kmers;
  DevBuf<uint8_t> d_nk;
  DevBuf<char> d_masked;
  DevBuf<int32_t> d_iota;
  size_t iota_n = 0;               // d_iota holds 0 .. iota_n - 1
  // staged raw records (umiclust_stage): ASCII + offsets in HBM (d_ascii, d_offs), lengths on the host
  bool staged = false;
  std::vector<uint32_t> rec_len;
  PinBuf<int32_t> h_perm;          // the sorted order's pinned mirror (perm upload)
  DevBuf<uint32_t> d_amb;    // [0] an ambiguous code was seen, [1] sequences whose masked output differs from the input
  PinBuf<uint32_t> h_amb;
  int64_t n_changed = 0;     // h_amb[1] of the last prepare: 0 -> the cluster files print the input bytes
  DevBuf<uint8_t> d_mchg;    // [sorted seqno] 1: its masked output differs from its input (the writer needs that row)
  PinBuf<uint16_t> h_xm;
  DevBuf<uint16_t> d_xm;
  // packs (umiclust_cluster_pack, multi-bin loads): sorted seqno -> load bin, each bin's first seqno and its first
  // centroid ordinal in the pack being clustered (INT32_MAX until indexed), the per-bin k-mer XOR masks
  std::vector<int32_t> hqbin;
  DevBuf<int32_t> d_qbin, d_bin_seq0, d_bin_ord0;
  PinBuf<int32_t> h_bin_ord0;
  bool pack_on = false;            // the current cluster_all call clusters a pack of several bins
  // device: tables
  DevBuf<uint8_t> d_acc;
  DevBuf<uint16_t> d_rank;
  std::vector<uint8_t> h_acc;
  std::vector<uint16_t> h_rank;
  uc::Index ix{this};             // device: the centroid index
  // two passes in flight (software pipeline over blocks) + round B on a side stream
  uc::Pass pass[uc::kPeerTiles];  // passes in flight (kDepth of them, <= kPeerTiles)
  uc::Tile blk_tile[uc::kPeerTiles + 1], solo_tile;  // per-block peer tiles (ring of depth + 1), overflow re-runs
  uc::Tile round_tile[2];         // O4 batched rounds: a pass's window from its first query's round start
  uc::Event a_ev[4][2];           // counting halves, ring by block: begin / end
  // split passes: index appends and peer-tile builds run on st_b beside the counting on the main stream;
  // they start after the latest second half (every earlier reader of the slots they rebuild precedes it)
  // and the main stream's next pass waits for ix_done
  hipStream_t ix_st = nullptr;     // null: the main stream; else st_b
  uc::Event ix_done;
  hipEvent_t last_r_ev = nullptr;  // the latest second half's ev[1] (its pass owns it)
  std::unique_ptr<uc::WorkPool> pool;  // host threads of resolve_pass (UMICLUST_RESOLVE_THREADS)
  // the file path's input (a multi-GB mapping: ~0.11 s of page-table teardown for config 2's 3.5 GB FASTA) is released
  // on this thread after the call has written its outputs; joined by the context's next file-path call and by
  // umiclust_destroy
  std::thread in_release;
  void join_release() {
    if (in_release.joinable()) in_release.join();
  }
  int32_t pass_B = 0;
  uc::Stream st_b, st_copy;
  PinBuf<uint32_t> h_bpq, h_bpt, h_bres;  // round B's pairs and results (pinned: no staged copies on the host's path)
  uc::Stream st_al;               // walk / alignment rounds / packing of the passes
  int32_t last_a_slot = -1;       // a_ev slot of the latest counting half
  uc::Event evb[2];
  DevBuf<uint32_t> d_bpq, d_bpt, d_bres;

  // results (sorted order, absolute seqnos; each bin's range is rewritten when it is clustered)
  std::vector<int32_t> cno;       // creation cluster number (within the bin)
  std::vector<uint8_t> strand;
  std::vector<int32_t> target;    // centroid seqno a member aligned to (-1 for centroids)
  std::vector<int32_t> ocl;       // output cluster number (within the bin)
  int32_t nclusters = 0;          // current bin
  // outputs of the current bin (output-cluster numbering)
  uc::ClusterNumbers num;         // creation -> output numbers, members per output cluster, clusters per bin (plan.h)
  std::vector<char> cons;
  std::vector<int64_t> cons_off;
  // per-bin results kept for umiclust_fetch_bin
  struct BinOut {
    bool done = false;
    int32_t K = 0;
    std::vector<char> cons;
    std::vector<int64_t> cons_off;
  };
  std::vector<BinOut> bout;
  // k_pack writes the outcomes and records straight into pinned host memory (true) or into device buffers copied by
  // DMA (false).  Set per clustering call: DMA with one context in the process (config 2: 4.33-4.36 vs 4.21-4.22 M
  // UMIs/s, the direct PCIe writes held k_pack at 133 us on the pass chain), direct with several (config 3, 8 lanes:
  // 7.56-7.60 vs 6.42-6.47 M: the lanes' copy dispatches contend for the hardware queues).
  bool rec_direct = false;
  uc::Event pt_ev;             // whole passes of single-bin loads: the next peer tile is built on st_b
  bool pt_pending = false;     // pt_ev recorded since the main stream last waited for it
  int32_t last_max_npeer = 0;
  DevBuf<uint32_t> d_probe;
  PinBuf<uint32_t> h_pf_nunits;   // umiclust_prefilter: the lean kernel's overflowed-unit count (PfCapture)
  int32_t o4_T = 0;               // policy O4 (umiclust_params.policy_threads): rounds of o4_T queries; 0 = sequential
  int32_t b_hint = 1 << 30;       // block size the last bin ended with (peer overflows halve it)
  int al_level = 0;                 // the alignment stream: 0 prioritised (al_priority), -1 plain (set_priority -1)
  int st_level = 0, prio_user = 0;  // the main stream's priority now / as umiclust_set_priority left it
  uc::DebugSums dbg;
  int64_t n_resolved = 0;
  bool dump_want(int64_t k) const {  // UMICLUST_RESOLVE_DUMP's pass list
    const char* c = strchr(tun.resolve_dump, ':');
    if (!c) return k == 10 || k == 40 || k == 80;
    for (const char* p = c + 1; *p;) {
      char* e;
      const long v = strtol(p, &e, 10);
      if (e == p) break;
      if (v == k) return true;
      p = *e == ',' ? e + 1 : e;
    }
    return false;
  }
  std::vector<int16_t> wd;
  // traceback / consensus buffers, kept across calls (a bin set clusters hundreds of small bins)
  DevBuf<uint32_t> t_mpq, t_mpt, t_mout;
  PinBuf<uint32_t> h_mpq, h_mpt;     // the member pairs' pinned staging (traceback launch)
  PinBuf<int32_t> h_mseq, h_mops, h_cstart;
  PinBuf<uint8_t> h_mstr;
  PinBuf<uint16_t> h_clen;           // consensus lengths / sequences / overflow flag (pinned downloads)
  PinBuf<char> h_craw;
  PinBuf<int32_t> h_over;
  std::vector<int32_t> t_opsidx;
  DevBuf<uint8_t> t_ops, t_mstrand;
  DevBuf<uint16_t> t_nops, t_conslen;
  DevBuf<int32_t> t_cstart, t_mseq, t_mops, t_over;
  DevBuf<char> t_cons;
  uc::Event tev[2];
  // umiclust_destroy, and every failure of umiclust_create.  The body joins the release thread, selects the device and
  // gives the context's count back; the members (buffers, events, streams) go after it.
  ~umiclust_ctx();
};

namespace uc {

extern std::atomic<int> g_live_ctx;  // contexts alive in this process (driver.cpp; L3Pin)

// ---- driver.cpp
// CPUs the calling thread may run on, and the resolve pool's size under them
int affinity_cpus();
int pool_threads(const umiclust_ctx* c);
// The main (counting) stream re-created at the greatest priority (level 1) or as a plain stream (0)
hipError_t main_stream_priority(umiclust_ctx* c, int level);
// member tracebacks and consensus: the launches ClusterRun and umiclust_consensus share
void ensure_traceback_buffers(umiclust_ctx* c, int32_t n);
void launch_tracebacks(umiclust_ctx* c, const DevSeqs& ds, const Scoring& sc, const TracePlan& tp, int32_t maxl,
                       hipStream_t stq);
void ensure_consensus_inputs(umiclust_ctx* c, int32_t n, int32_t K);
constexpr const char* kConsOverMsg = "consensus: %d clusters exceed the MSA column budget";
int32_t run_consensus(umiclust_ctx* c, const DevSeqs& ds, int32_t n, int32_t K, hipEvent_t ev);
// cluster_all under the call's host placement (L3Pin)
void cluster_pinned(umiclust_ctx* c, int32_t bin, bool multi_bin = false, int32_t npk = 1);

// One cluster_all call: what its steps share (per call, not part of the context).  Seqnos stay absolute everywhere.
// The steps are described where they are defined (driver.cpp); the probes drive the first ones and single passes.
struct ClusterRun {
  umiclust_ctx* const c;
  const int32_t bin, npk;  // the bins [bin, bin + npk)
  const bool multi_bin;
  const double t0 = now_s();
  const int32_t s0, s1, n;  // one bin (or pack) = the sorted seqnos [s0, s1)
  std::vector<uint8_t> state_buf;
  StateView state;
  BlockPlan plan;
  std::vector<int32_t> pending;    // O4: resolved centroids the index does not hold yet (sync_index)
  std::vector<int32_t> new_cents;  // the centroids of the block resolved last
  // Lazy peers: once new centroids have become rare (the last resolved block created fewer than kLazyPermille per
  // mille), in-window peers are not aligned speculatively; a query whose relevant peer turns out to be a centroid is
  // deferred and round B aligns what it needs (deep clusters: config 5)
  bool lazy = false;
  double t_pf = 0, t_al = 0, t_host = 0, t_cons = 0;
  int32_t tw_n = 0;            // member pairs handed to the traceback so far (tw_launch)
  int32_t tw_maxl = kMaxLen;   // the bin's longest sequence
  DevSeqs ds{};
  const int32_t T4;  // policy O4: queries per round (0: sequential)
  const int D;       // passes in flight

  ClusterRun(umiclust_ctx* ctx, int32_t bin_, int32_t npk_, bool multi)
      : c(ctx), bin(bin_), npk(npk_), multi_bin(multi), s0(ctx->bin_s[bin_]), s1(ctx->bin_s[bin_ + npk_]), n(s1 - s0),
        T4(ctx->o4_T), D(T4 ? 2 : kDepth) {}

  void reset_bin();
  void plan_blocks();
  void alloc_traceback();
  int32_t rstart(int32_t q) const;
  void sync_index(int32_t X);
  void round_window(int32_t q, const Tile** prevs, int& nprev, int slot);
  void keep_new_cents();
  void count_lazy(int32_t k, int32_t ahead);
  void run_alone(int32_t q0, int32_t nq);
  Tile& tile_of(int32_t k) { return c->blk_tile[k % (D + 1)]; }
  void enqueue(int32_t k, int nprev);
  void prebuild_peer(int32_t k);
  void run_whole();
  Tile& stile(int32_t j) { return c->blk_tile[j % (kPeerTiles + 1)]; }
  void build_peer(int32_t j, bool side);
  void second_half(int32_t j, int32_t first, bool after_count, PfCapture* cap = nullptr);
  void count_half(int32_t j, int32_t first, int flag, PfCapture* cap = nullptr);
  void prime(int32_t r);
  void run_split();
  void run_pipeline();
  void drain();
  void tw_launch(int32_t lo, int32_t hi, hipStream_t stq);
  void trace_members();
  void number();
  void consensus();
  void store_outputs();
  void report_pf_prof();
  void report_debug() const;
  void report();
};

// ---- index.cpp
// postings a tile slot of nseq sequences can need: every k-mer plus up to 7 padding postings per
// non-empty list
inline size_t tile_cap(int64_t nseq) {
  const int64_t raw = nseq * kMaxKmers;
  return (size_t)((raw + 7 * std::min<int64_t>(kBins, raw) + 64) & ~int64_t(7));
}
// (re)build one index or peer tile over sequences map[first .. first+n) with ordinals xoff + c
void build_tile(umiclust_ctx* c, Tile& t, const int32_t* map, int32_t first, int32_t n, int32_t xoff, int32_t vbase,
                int32_t seg_mod, hipStream_t st = nullptr);
inline TileView view_of(const Tile& t) {  // (several per prefilter launch, in index.cpp and pass.cpp)
  TileView v;
  v.off = t.off.p;
  v.post_base = t.post_base;
  v.n = t.n;
  v.base = t.base;
  v.seg = t.seg;
  v.len = t.len;
  return v;
}

inline DevSeqs dev_seqs(umiclust_ctx* c) {
  DevSeqs s;
  s.codes = c->d_codes.p;
  s.lens = c->d_lens.p;
  s.kmers = c->d_kmers.p;
  s.nk = c->d_nk.p;
  return s;
}

inline int32_t round_start(const umiclust_ctx* c, int32_t s0, int32_t q) {
  return o4_round_start(c->o4_T, c->pack_on ? c->hqbin.data() : nullptr, c->bin_s.data(), s0, q);
}

// the longest / shortest query of a block (sorted within a bin, but a pack's lengths restart at every bin)
inline int32_t block_maxlen(const umiclust_ctx* c, int32_t q0, int32_t nq) {
  int32_t m = 0;
  for (int32_t q = q0; q < q0 + nq; q++) m = std::max<int32_t>(m, c->hlen[q]);
  return m;
}
inline int32_t block_minlen(const umiclust_ctx* c, int32_t q0, int32_t nq) {
  int32_t m = kMaxLen;
  for (int32_t q = q0; q < q0 + nq; q++) m = std::min<int32_t>(m, c->hlen[q]);
  return m;
}

// ---- pass.cpp
void ensure_pass_buffers(umiclust_ctx* c, Pass& P, int32_t B);
void enqueue_pass(umiclust_ctx* c, Pass& P, int32_t q0, int32_t nq, const Tile* const* prevs, int nprev, Tile& own,
                  int32_t region, bool lazy_peers = false, bool after_count = false, PfCapture* cap = nullptr);
void enqueue_count(umiclust_ctx* c, Pass& P, int32_t q0, int32_t nq, const Tile* const* wins, int nwin, int flag,
                   int32_t slot, PfCapture* cap = nullptr);
bool resolve_pass(umiclust_ctx* c, Pass& P, const StateView& state, std::vector<int32_t>& new_cents, double& t_pf,
                  double& t_al, double& t_host, int32_t* resolved);

// ---- load.cpp
Scoring to_scoring(const umiclust_params& p);
void validate(umiclust_ctx* c, const umiclust_params& p);
void stage_impl(umiclust_ctx* c, const char* seqs, const int64_t* offs, int64_t n, const int64_t* bin_in = nullptr,
                int32_t nbins = 1);
void prepare_impl(umiclust_ctx* c, const umiclust_params* p);
void load_impl(umiclust_ctx* c, const umiclust_params* p, const char* seqs, const int64_t* offs, int64_t n,
               const int64_t* bin_in = nullptr, int32_t nbins = 1);

// ---- timeline.cpp
// the interval between two completed events of device dev joins the process-wide timeline (kind 0: counting
// launches, 1: alignment chains; umiclust_timeline)
void tl_add(int dev, int kind, hipEvent_t a, hipEvent_t b);

}  // namespace uc
