// Internal declarations shared by the HIP kernels (kernels.hip) and the host side (clustering: driver.cpp,
// index.cpp, pass.cpp, load.cpp, probes.cpp through cluster_ctx.h; dropin_*.cpp through ctx.h).  Not part of the C
// ABI (see include/umiclust.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "umiclust_consts.h"

namespace uc {

struct Scoring {
  int32_t match, mismatch;
  int32_t go[6], ge[6];  // QL TL QI TI QR TR
  int32_t boundary_open;
};

// One index tile: CSR over bins (part << 16 | k-mer); postings live in one arena shared by all tiles.
struct TileView {
  const uint32_t* off;     // [kBins + 1] tile-relative, each list a multiple of 8 postings
  uint64_t post_base;      // arena index of the tile's first posting
  int32_t n;               // sequences in the tile
  int32_t base;            // first centroid ordinal / first seqno (peer tiles)
  int32_t seg;             // counter segment (centroid tiles) / peer region 0|1 (peer tiles)
  int32_t len;             // peer tiles: the block's query length (one length per block)
};

struct DevSeqs {
  const uint32_t* codes;   // [(s*2+strand)*kCodeWords] 4-bit codes, sorted order
  const uint8_t* lens;     // [s]
  const uint16_t* kmers;   // [(s*2+strand)*kKmerStride]
  const uint8_t* nk;       // [s*2+strand]
};

// ---- kernel launchers (kernels.hip) ----
hipError_t launch_iota(int32_t* out, int32_t n, hipStream_t st);
hipError_t launch_prep(const char* ascii, const int64_t* offs, const int32_t* perm, int32_t n,
                       int dust, uint32_t* codes, uint8_t* lens, uint16_t* kmers, uint8_t* nk,
                       char* masked, uint32_t* ambig, hipStream_t st,
                       uint8_t* mchg = nullptr);
// XOR every k-mer of sequence s (both strands) with xmask[bin[s]] (packs: a bijection per bin)
hipError_t launch_kmer_xor(uint16_t* kmers, const uint8_t* nk, int32_t n, const int32_t* bin, const uint16_t* xmask,
                           hipStream_t st);
// index tile build over sequences c in [0, count) with seqno map[first + c] and ordinal
// x = xoff + c (centroid tiles: the centroid ordinal; peer tiles: c): count (hist[kBins], all zero
// on entry), scan (padded offsets off[kBins+1], fill cursors, padding postings written into post,
// hist re-zeroed), fill (posting = vbase + (x % seg_mod) / kParts)
constexpr int kScanPer = 1024;
constexpr int kScanBlocks = kBins / kScanPer;
hipError_t launch_index_count(const uint16_t* kmers, const uint8_t* nk, const int32_t* map, int32_t first,
                              int32_t count, int32_t xoff, uint32_t* hist, hipStream_t st);
hipError_t launch_index_scan(uint32_t* hist, uint32_t* partial, uint32_t* off, uint32_t* cursor, uint16_t* post,
                             hipStream_t st);
hipError_t launch_index_fill(const uint16_t* kmers, const uint8_t* nk, const int32_t* map, int32_t first,
                             int32_t count, int32_t xoff, int32_t vbase, int32_t seg_mod, uint32_t* cursor,
                             uint16_t* post, hipStream_t st);
// bank-aware posting order within every list of a tile (after the fill; kernels.hip k_list_arrange)
hipError_t launch_index_arrange(const uint32_t* off, uint16_t* post, hipStream_t st);
// the host-to-device half of an index append in one dispatch: n centroid seqnos / lengths, ns seq -> ordinal entries
// and nb bin-start ordinals, each read from pinned host memory and written to its device array
hipError_t launch_append_stage(const int32_t* hc, const uint8_t* hl, int32_t n, int32_t* dc, uint8_t* dl,
                               const int32_t* hs, int32_t* ds, int32_t ns, const int32_t* hb, int32_t* db, int32_t nb,
                               hipStream_t st);
// prefilter: for query-strands qs in [0, nqs): query seqno = q0 + qs/2 (or qs if !both), strand.
// postings-touched partial sums: slots counters[16 + 32 s], s < kPostSpread (separate L2 lines)
constexpr int kPostSpread = 32;
constexpr int kPartCand = 64;  // candidates a (query-strand, part) passes to the merge
// pass counters: [0..15] stats and pair counts, the postings partial sums, the overflowed-unit count
constexpr int kUnitsSlot = 16 + kPostSpread * 32;
// per-length pair counters of the three walk rounds (SegTab), kSegLens each
constexpr int kSegSlot = kUnitsSlot + 32;
constexpr int kCountersLen = kSegSlot + 3 * kSegLens;
constexpr int kPfWinBase = 128;   // k_pf_count: windows whose base list and start mask are tabulated (the rest: search)
// centroid tile views passed in the kernel arguments (a pass reads them by scalar loads either way; in the arguments
// they need no host-to-device copy, a blit dispatch between every two counting launches)
constexpr int kArgTiles = 32;
struct PrefilterArgs {
  DevSeqs seqs;
  const uint16_t* arena;   // postings of every tile
  const TileView* tiles;   // device array, centroid tiles in segment order (used when ntiles > kArgTiles)
  int32_t ntiles;
  TileView tv[kArgTiles];  // the same views when ntiles <= kArgTiles
  int32_t nseg;            // counter segments holding centroids (0 if none)
  int32_t seg_tile[kMaxSegs + 1];  // tiles of segment s: [seg_tile[s], seg_tile[s+1])
  uint64_t seg_base[kMaxSegs];     // lowest arena index a pass of segment s reads (peers: last pass)
  int32_t ncent;           // centroid ordinals [0, ncent) are indexed
  const int32_t* cent_seqno;  // centroid ordinal -> sorted seqno
  // centroids of length >= L, for L = 0..kMaxLen: lengths never increase with the ordinal (queries
  // are length-sorted, centroids appended in query order), so ordinal o has the largest L with
  // cnt_ge[L] > o
  int32_t cnt_ge[kMaxLen + 1];
  int32_t q0, nq;          // block of queries (sorted seqnos)
  int32_t both;            // strands per query (1 or 2)
  int32_t minwordmatches;
  // peer tiles: mini indexes over the + strand k-mers of the previous block and of this block
  // (base = first seqno, n = 0 if absent); together they cover the peer window [peer_base, q0+nq),
  // and a query sees the window entries before it
  TileView peer[kPeerTiles];  // oldest first, the block's own tile last (absent ones: n = 0)
  int32_t peer_base;
  int32_t nlist_cap;       // list-table capacity of the lean counting kernel (>= k-mers x tiles)
  int32_t pf1_lds;         // the lean counting kernel runs one-wave units when its LDS is at most this (bytes)
  // per-(query-strand, part) outputs, merged by launch_prefilter's last kernel: candidates (count >= the
  // threshold) as count << 24 | ordinal, unsorted, at most kPartCand (255 in pncand: overflow, re-run by
  // the full kernel, which writes its exact part top-41 in the same form)
  uint32_t* pcand;           // [nqs*kParts*kPartCand]
  uint8_t* pncand;           // [nqs*kParts]
  uint32_t* units;           // [nqs*kParts] overflowed (query-strand, part) units, *nunits of them
  uint32_t* nunits;  // (the merge resets *nunits to 0)
  // split passes (the counting of a block runs before the block two ahead of it is resolved): peer tile
  // flag_tile (>= 0) is that unresolved block; its hits become flagged candidates count << 24 | 1 << 23 |
  // (seqno - cand_base), kept by the merge if seq2ord[seqno] >= 0 (a centroid by then).  Stored peer ids
  // are relative to cand_base; the merge writes them relative to peer_base (id - peer_shift), and the full
  // kernel stores its own (peer_base-relative) ids + peer_id_add.
  int32_t flag_tile;
  int32_t cand_base;
  int32_t peer_shift;
  int32_t peer_id_add;
  const int32_t* seq2ord;  // [seqno] centroid ordinal or -1 (absolute seqnos)
  uint16_t* ppeer_id;        // [nqs*kParts*kPeerCap]
  uint8_t* ppeer_count;      // [nqs*kParts*kPeerCap]
  uint8_t* pnpeer;           // [nqs*kParts] (255 = overflow)
  uint32_t* ppost;           // [nqs*kParts] postings touched (stats; one atomic per merge workgroup)
  // outputs
  uint32_t* top_seqno;     // [nqs*kTopHits]
  uint8_t* top_count;      // [nqs*kTopHits]
  uint8_t* ntop;           // [nqs]
  uint16_t* peer_id;       // [nqs*kPeerCap] window-local (seqno - peer_base)
  uint8_t* peer_count;     // [nqs*kPeerCap]
  uint8_t* npeer;          // [nqs] (255 = overflow)
  uint32_t* postings_touched;  // counters[0]; the merge adds into kPostSpread slots 128 B apart after
                               // counters[16], which k_pack sums into the host copy of counters[0]
  unsigned long long* prof;    // [9] optional phase clocks of sampled workgroups (see k_prefilter), then their count
  // Packs (umiclust_cluster_pack: several bins in one greedy order, their k-mers XOR-scrambled per bin so other
  // bins' postings are sparse noise): query q of load bin qbin[q] takes centroid candidates only from ordinals >=
  // bin_ord0[bin] (INT32_MAX until the bin's first centroid is indexed) and peers / flagged hits only from
  // seqnos >= bin_seq0[bin]; k_pf_full keys centroids by cent_len (lengths are not monotone in the ordinal across
  // bins).  qbin == nullptr: one bin.
  const int32_t* qbin;
  const int32_t* bin_seq0;
  const int32_t* bin_ord0;
  const uint8_t* cent_len;
};
// two kernels: the per-part counting/selection (grid nqs*kParts) and the per-query-strand merge
// mode 0: the whole prefilter (lean counting + the full kernel over its overflowed units, or the full
// kernel alone for multi-segment bins, then the merge); mode 1: only the lean counting (a split pass's
// first half); mode 2: the full kernel over the units mode 1 left + the merge (a whole pass's second launch);
// mode 4: the same as a split pass's second half, where a query-strand with only some parts overflowed hands the
// full kernel its other parts too (k_pf_expand_units)
hipError_t launch_prefilter(const PrefilterArgs& a, hipStream_t st, int mode = 0);
// whether launch_prefilter's lean counting runs one-wave units (k_pf_count<0, 1>) for these arguments
bool prefilter_one_wave(const PrefilterArgs& a);

// alignment of pairs whose queries all have length qlen; pq = (query seqno << 1) | strand, pt = target seqno (plus strand)
// out[outidx ? outidx[k] : k] = matches | internal << 8 | (score & 0xffff) << 16.
// If dev_npairs != NULL only pairs k < *dev_npairs run (npairs is the launch bound).  Launches of at most
// band_max pairs (one-hot codes) spread each pair over a lane group (k_align_band) instead of one lane.
hipError_t launch_align(const DevSeqs& s, int32_t qlen, bool ambig, const uint32_t* pq, const uint32_t* pt, int32_t npairs,
                        const uint32_t* dev_npairs, const uint32_t* outidx, const Scoring& sc,
                        uint32_t* out, hipStream_t st, int32_t band_max = 0);

struct WalkState {
  unsigned long long lastkey;  // key of the last walked candidate
  uint32_t best_t;             // best accepted target seqno
  uint32_t cells;              // sum of qlen*tlen over walked candidates
  uint16_t best_rank;          // id rank of the best accepted hit
  uint8_t w;                   // candidates walked (aligned)
  uint8_t done;
  uint8_t acc;                 // an accepted hit exists
  uint8_t e;                   // candidates emitted for alignment so far (results exist for [0, e))
  uint8_t pad[2];
};
// round -1 initialises and emits batch 0 -- or, speculatively, every candidate up to kWalk when the best
// candidate's k-mer count is below spec_thr (junk-like lists walk to the end);
// round r >= 0 evaluates every batch whose results exist and, if the walk goes on, emits all of its
// remaining candidates (up to kWalk): a pass has two dependent alignment launches, not five.
// Speculation changes which alignments are computed, never the walk: batches are evaluated in order.
// A block may hold several query lengths (the aligner is compiled per length): the walk and the peer pairs append
// their pairs to per-length segments, segment i = query length lmax - i at pair index base[i] (its capacity is the
// block's query-strands of that length x the pairs one can emit), counted in seg_cnt[i]; one alignment launch per
// segment.  Blocks span at most kSegLens lengths.
struct SegTab {
  int32_t lmax;
  int32_t nseg;
  uint32_t base[kSegLens];
};
hipError_t launch_walk(int32_t round, int32_t q0, int32_t nqs, int32_t both, int32_t spec_thr,
                       const uint32_t* top_seqno, const uint8_t* top_count, const uint8_t* ntop,
                       const uint8_t* lens, const uint32_t* res, const uint8_t* acc_tab,
                       const uint16_t* rank_tab, WalkState* ws, uint32_t* pq, uint32_t* pt,
                       uint32_t* outidx, const SegTab& sg, uint32_t* seg_cnt, unsigned long long* cells,
                       hipStream_t st);
// cells accumulates qlen x tlen of the pairs emitted (the cells the device computes for them)
hipError_t launch_peer_pairs(int32_t q0, int32_t w0, int32_t nqs, int32_t both, const uint8_t* lens,
                             const WalkState* ws, const uint16_t* peer_id, const uint8_t* peer_count,
                             const uint8_t* npeer, uint32_t* pq, uint32_t* pt, uint32_t* outidx, const SegTab& sg,
                             uint32_t* seg_cnt, unsigned long long* cells, uint32_t* nstat, uint32_t out0,
                             unsigned long long* aligned, int32_t emit, const WalkState* ws_prev,
                             const uint8_t* npeer_prev, int32_t q0_prev, int32_t nq_prev, hipStream_t st);
hipError_t launch_pack(int32_t nqs, int32_t w0, const uint8_t* lens, const WalkState* ws, const uint8_t* ntop,
                       const uint32_t* top_seqno, const uint8_t* top_count, const uint32_t* res,
                       const uint8_t* npeer, const uint16_t* peer_id, const uint8_t* peer_count,
                       const uint32_t* peer_res, const unsigned long long* aligned, uint32_t* reccount, HostQs* hq,
                       uint32_t* rec, uint32_t* counters, uint32_t* hcounters, uint32_t* hreccount, hipStream_t st);
// traceback (one wave per pair, any query length): ops[k*kOpsStride...] ('M','D','I' in alignment order,
// right-aligned in the slot), nops[k], out[k] as launch_align's
// maxl: the longest query or target length among the pairs (sizes the kernel's LDS)
// maxl: the launch's longest sequence; maxq: its longest query (0: maxl) -- every pair's query must fit it
hipError_t launch_traceback(const DevSeqs& s, const uint32_t* pq, const uint32_t* pt, int32_t npairs,
                            const Scoring& sc, uint8_t* ops, uint16_t* nops, uint32_t* out, hipStream_t st,
                            int32_t maxl, int32_t maxq = 0);
// consensus: cluster c members member_seqno[cstart[c] .. cstart[c+1]) (centroid first),
// member_ops index per member (-1 for centroid), member strand.
hipError_t launch_consensus(const DevSeqs& s, const int32_t* cstart, int32_t nclusters,
                            const int32_t* member_seqno, const int32_t* member_opsidx,
                            const uint8_t* member_strand, const uint8_t* ops,
                            const uint16_t* nops, char* cons, uint16_t* conslen,
                            int32_t* overflow, hipStream_t st);

// ---- region-vs-region UMI overlap (overlap.hip) ----
struct OvBuffers {
  uint64_t* hash;                 // [n]
  int32_t* region;                // [n]
  unsigned long long* keys;       // [m] slot hash (~0 = empty)
  unsigned long long* rep;        // [m] lowest member index
  int64_t* slot;                  // [n]
  uint32_t* cnt;                  // [m]
  uint32_t* start;                // [m + 1]
  uint32_t* cursor;               // [m]
  uint32_t* bsum;                 // [m / 1024 + 1]
  uint32_t* members;              // [n]
  uint32_t* collision;            // [1]
  uint32_t* big;                  // [n / (kOvSmallBucket + 1) + 1] slots whose buckets k_ov_pairs hands on
  uint32_t* nbig;                 // [1]
};
constexpr int kOvSmallBucket = 32;  // larger buckets (a UMI in many regions): one workgroup each, region histogram
// one hash-table pass over n sequences of nreg regions (region r = [rstart[r], rstart[r+1])), table of
// mask + 1 slots; csr also buckets the members by slot.  Synchronous; *collided != 0 means two different
// sequences shared a 64-bit hash (re-run with another seed).
hipError_t launch_overlap_table(const char* seqs, const int64_t* offs, int64_t n, const int64_t* rstart, int32_t nreg,
                                uint64_t seed, uint64_t hmask, uint64_t mask, const OvBuffers& B, bool csr,
                                uint32_t* collided, hipStream_t st);
// total[a * nreg + b] += c_a(s) c_b(s), maxc[a * nreg + b] = max c_b(s) over sequences s held by a and b (a < b)
hipError_t launch_overlap_pairs(const OvBuffers& B, uint64_t mask, int32_t nreg, unsigned long long* total,
                                uint32_t* maxc, hipStream_t st);
// two sets (region 0 = the first n1 sequences, region 1 = the rest): counts[i] = equal sequences in set 2
hipError_t launch_overlap_two(const OvBuffers& B, uint64_t mask, int64_t n, int64_t n1, int64_t* counts,
                              hipStream_t st);

// ---- UMI extraction (extract.hip) ----
struct ExtractPatterns {
  uint64_t peq[2][256];   // [fwd | rev pattern][byte]: bit i = pattern[i] equals the byte
  uint64_t peqr[2][256];  // same for the reversed pattern
  int32_t m[2];           // pattern lengths (1..64)
  int32_t pad[2];
};
// out[(i * 2 + w) * 3 ...] = (edit distance or -1, start, end) of edlib HW locations[0] in window w of read i
hipError_t launch_extract(const char* seqs, const int64_t* offs, int64_t n, int32_t a5, int32_t a3, int32_t k,
                          const ExtractPatterns* P, int32_t* out, hipStream_t st);
// the same on host-gathered windows (read i's at win[i * S ...], 5' window first, 3' at a5; lengths wlen[2i + w])
constexpr int kExMaxSlot = 252;  // S <= this: 128 slots fit the LDS staging of k_extract_win
hipError_t launch_extract_win(const char* win, const uint8_t* wlen, int64_t n, int32_t S, int32_t a5, int32_t k,
                              const ExtractPatterns* P, int32_t* out, hipStream_t st);

// ---- per-record fixed-point expected error of FASTQ qualities (fastq_filter.hip; row f5) ----
// qual = the concatenated quality bytes, 16-byte aligned, with 16 readable bytes before and after them; record i =
// [offs[i], offs[i + 1]); table[256] indexed by the raw byte.  ee[i] = sum of table[b], qlo[i] / qhi[i] = min / max b
// (255 / 0 for an empty record).
hipError_t launch_fastq_ee(const uint8_t* qual, const int64_t* offs, int64_t n, const uint64_t* table, int64_t* ee,
                           uint8_t* qlo, uint8_t* qhi, hipStream_t st);
// The same with the counts of seqkit's `stat -a` table (row f5b): seq = the concatenated sequence bytes, laid out as
// qual is (the same offs, the same padding).  ee / qlo / qhi as above; counts[5 i ..] = record i's quality bytes with
// b - ascii >= 20, with b - ascii >= 30, its sequence bytes in "GCgc", in "Nn" and in "-. ".
hipError_t launch_fastq_stats(const uint8_t* qual, const uint8_t* seq, const int64_t* offs, int64_t n,
                              const uint64_t* table, int ascii, int64_t* ee, uint8_t* qlo, uint8_t* qhi,
                              uint32_t* counts, hipStream_t st);

// ---- region binning of BAM records (regionsplit.hip) ----
enum : int8_t { kBamUnmapped = 0, kBamSecondary = 1, kBamShort = 2, kBamLong = 3, kBamKept = 4, kBamNoRegion = 5,
                kBamNoCluster = 6 };
// raw: uncompressed BAM, roff[r]: offset of record r's block_size field; ref_len / ref_cluster per BAM reference
// (-1: not in the reference FASTA / not in the cluster dict)
hipError_t launch_bam_classify(const uint8_t* raw, const int64_t* roff, int64_t n, int32_t nref, const int64_t* ref_len,
                               const int32_t* ref_cluster, double minov, int32_t s5, int32_t s3, int8_t* cls,
                               int32_t* cluster, int64_t* outlen, hipStream_t st);
hipError_t launch_bam_emit(const uint8_t* raw, const int64_t* roff, int64_t n, const int8_t* cls, const int64_t* pos,
                           char* out, hipStream_t st);

// ---- UMI extraction from the kept BAM records (bamextract.hip; row f4+f1) ----
// res[r * 6 ...] = umiclust_extract_umis' six values for every record r < n with cls[r] == kBamKept, found in the two
// windows of the read as launch_bam_emit would write it; len[r] = bytes of the record's detected-UMI text (0: a UMI
// is missing, or the record is not kept), or one of the two marks below
constexpr int64_t kUmiHostName = -1;  // both UMIs found, the name holds "strand=": the host formats the record
constexpr int64_t kUmiBadName = -2;   // the name holds white space: the call refuses the file
hipError_t launch_bam_umi_search(const uint8_t* raw, const int64_t* roff, int64_t n, const int8_t* cls, int32_t a5,
                                 int32_t a3, int32_t k, const ExtractPatterns* P, int32_t* res, int64_t* len,
                                 hipStream_t st);
// the text of every record with len[r] > 0 at out + pos[r]
hipError_t launch_bam_emit_umi(const uint8_t* raw, const int64_t* roff, int64_t n, const int64_t* len,
                               const int32_t* res, const int64_t* pos, int32_t a3, char* out, hipStream_t st);

// ---- BAM record scan with tags and the cs:Z group-by (bamscan.hip) ----
struct BamScanCols {  // one entry per record
  int8_t* cls;        // bam::kScanUnmapped / kScanSecondary / kScanPrimary
  int32_t* ref;
  int32_t* l_seq;
  int64_t* reflen;    // M/D/N/=/X lengths, 0 -> 1
  int64_t* cols;      // M/I/D lengths
  int64_t* nm;
  uint8_t* nm_present;
  int64_t* cs_off;    // offset of the cs:Z bytes in raw
  int32_t* cs_len;    // -1: no cs tag
  uint64_t* cs_hash;
  int8_t* bad;        // malformed layout or aux field (aux fields are walked on primary records only)
};
hipError_t launch_bam_scan(const uint8_t* raw, int64_t raw_len, const int64_t* roff, int64_t n, uint64_t seed,
                           uint64_t hmask, const BamScanCols& o, hipStream_t st);
// table of mask + 1 slots (at least twice the records): slot[r] (-1: not grouped), per slot the lowest record and the
// count; *collision != 0 when two different strings shared a hash
hipError_t launch_cs_group(const uint8_t* raw, const BamScanCols& o, int64_t n, uint64_t mask, unsigned long long* keys,
                           unsigned long long* rep, uint32_t* cnt, int64_t* slot, uint32_t* collision,
                           hipStream_t st);

// ---- region split and name suffix on the session's columns (bamsplit.hip; rows f4b / f6b) ----
constexpr int8_t kBamAbsent = 7;  // keep[r] == 0: the record is not in the file that is being split
// classes of launch_bam_classify (+ kBamAbsent) from o.cls / o.ref / o.l_seq / o.reflen alone (the other columns are
// not read); keep may be null; ref_len / ref_bucket per BAM reference (-1: not a region / no bucket)
hipError_t launch_split_cols(const BamScanCols& o, const uint8_t* raw, const int64_t* roff, const uint8_t* keep,
                             int64_t n, int32_t nref, const int64_t* ref_len, const int32_t* ref_bucket, double minov,
                             int32_t s5, int32_t s3, int8_t* cls, int32_t* bucket, int64_t* outlen, hipStream_t st);
// value / status of the query name's last "_" field: status 1 = 1..18 ASCII digits, 0 = anything else
hipError_t launch_name_suffix(const uint8_t* raw, const int64_t* roff, int64_t n, int64_t* value, uint8_t* status,
                              hipStream_t st);

// ---- BGZF blocks inflated on the device (bgzf.hip) ----
struct BgzfBlock {   // one entry per block with ISIZE > 0, built by the host from the framing walk
  int64_t in_off;    // the DEFLATE payload in the compressed buffer
  int64_t out_off;   // the block's first byte in the inflated buffer (the sum of the ISIZEs before it)
  uint32_t in_len;
  uint32_t isize;
};
// One wave per block: out[out_off, + isize) and status[b] = an inf:: status of inflate.h (0 = ok).  comp: 4-byte
// aligned, comp_bytes a multiple of 4 that covers every payload (the bit reader reads whole words below it, none at or
// past it); the statuses say which blocks' bytes are good.
hipError_t launch_bgzf_inflate(const uint8_t* comp, int64_t comp_bytes, const BgzfBlock* blk, int64_t n, uint8_t* out,
                               int32_t* status, hipStream_t st);

// ---- BGZF blocks deflated on the device (bgzf.hip on deflate.h) ----
struct DeflateBlock {  // one entry per block, in file order
  int64_t in_off;      // the block's first byte in the input buffer
  uint32_t n;          // its bytes, 1..0xff00
  uint32_t pad;
};
constexpr int64_t kDeflateSlot = 0xff00 + 8;  // bytes between two blocks' output slots (n + 5 are used; a multiple of 4)
constexpr int64_t kDeflateGrid = 2048;        // workgroups of k_bgzf_deflate at most; tok holds 0xff00 words for each
// One wave per block, persistent: slots[b * kDeflateSlot, + payload) = the block's DEFLATE stream (dfl::run of
// deflate.h), meta[4 b ..] = kind (0 stored, 1 fixed, 2 dynamic), payload bytes, status (0 = ok), flags, fsize[b] =
// 26 + payload bytes (0 with a status).  tok: min(n, kDeflateGrid) * 0xff00 words of scratch; slots 4-byte aligned.
hipError_t launch_bgzf_deflate(const uint8_t* in, const DeflateBlock* blk, int64_t n, uint8_t* slots, uint32_t* tok,
                               int32_t* meta, int64_t* fsize, hipStream_t st);
// out[foff[b], + fsize[b]) = block b framed: header with BSIZE, payload, crc[b], ISIZE (foff = the scan of fsize)
hipError_t launch_bgzf_frame(const uint8_t* slots, const DeflateBlock* blk, const int32_t* meta, const int64_t* foff,
                             const uint32_t* crc, int64_t n, uint8_t* out, hipStream_t st);

// ---- SAM text to the session's raw and roff (samsort.hip on sam_text.h) ----
// body = the text after the header, n bytes.  Every pointer is device memory.
namespace sam {
struct Names;
struct Fields;
struct FSlot;
}  // namespace sam
// out[i] = base + in[0] + .. + in[i - 1]; *total (may be null) = base + the sum; in may be out
hipError_t launch_scan_i64(const int64_t* in, int64_t* out, int64_t n, int64_t base, int64_t* total, hipStream_t st);
// the chunks the line kernels split n bytes into: count[] and first[] have one entry per chunk
int64_t sam_line_chunks(int64_t n);
// *total = lines - 1 (a line starts at 0 and after every '\n' but the text's last byte); n > 0
hipError_t launch_sam_count_lines(const uint8_t* body, int64_t n, int64_t* count, int64_t* first, int64_t* total,
                                  hipStream_t st);
// start[nlines + 1]: line l = body[start[l], start[l + 1] - 1)
hipError_t launch_sam_scatter_lines(const uint8_t* body, int64_t n, const int64_t* first, int64_t nlines,
                                    int64_t* start, hipStream_t st);
// per line: fields, size, key, status (sam::measure); acc[0] = first refused line (start it at ~0), acc[1] = OR of the
// accepted keys, acc[2] = aux f values
hipError_t launch_sam_measure(const uint8_t* body, const int64_t* start, int64_t n, const sam::Names& N,
                              sam::Fields* fields, int64_t* size, uint64_t* key, int32_t* status, uint64_t* acc,
                              hipStream_t st);
// stable sort of (key, line) by key: key_a holds the keys (both key arrays are scratch afterwards), key_bits = the OR
// of all keys, hist = 256 * ceil(n / 256) entries; *sorted_idx = idx_a or idx_b, whichever holds the order
hipError_t launch_sam_sort(uint64_t* key_a, uint32_t* idx_a, uint64_t* key_b, uint32_t* idx_b, int64_t n,
                           uint64_t key_bits, int64_t* hist, const uint32_t** sorted_idx, hipStream_t st);
// roff[r] = base + the sizes of the records before r in sorted order; *total = one past the last record
hipError_t launch_sam_roff(const int64_t* size, const uint32_t* idx, int64_t n, int64_t base, int64_t* roff,
                           int64_t* total, hipStream_t st);
// the records at raw + roff[r] (sam::encode); the aux f values appended to slots[0, cap) through *nslots
hipError_t launch_sam_encode(const uint8_t* body, const int64_t* start, const uint32_t* idx, const int64_t* roff,
                             int64_t n, const sam::Names& N, const sam::Fields* fields, const int64_t* size,
                             uint8_t* raw, sam::FSlot* slots, uint64_t* nslots, int64_t cap, hipStream_t st);
// raw[at[i] .. + 4) = bits[i], little-endian
hipError_t launch_sam_put_f(uint8_t* raw, const int64_t* at, const uint32_t* bits, int64_t n, hipStream_t st);

// ---- the .bai index and flagstat of the session's kept records (bamindex.hip on bam_index.h) ----
// Every pointer is device memory.  keep may be null (every record); the block table (bam_index.h) may be empty
// (nblocks = 0: no virtual offsets, as flagstat alone needs it).
struct BaiIn {
  const uint8_t* raw;
  const int64_t* roff;
  const uint8_t* keep;
  int64_t n, header_end;
  const int64_t *coff, *ustart;
  int64_t nblocks;
  int32_t nref;
};
struct BaiCols {  // per kept record, in order: entry j = the j-th kept record
  uint32_t* rec;  // its index among all records
  int32_t *tid, *beg, *bin, *w0, *w1, *status;
  uint64_t *u, *v;  // the virtual offsets of its start and its end
};
struct BaiAcc {  // zeroed by the caller, first_bad set to ~0
  uint64_t* first_bad;   // min over the refused records of rec << 2 | status
  uint64_t* counters;    // the 32 of flagstat
  uint64_t *mapped, *unmapped, *n_intv;  // per reference
  uint64_t* n_no_coor;
};
namespace bai {
struct Run;  // bam_index.h: one run of kept records in one bin (reference, bin, start, end)
}  // namespace bai
// scratch: 4 arrays of n + 1 int64 (kept flag and size, their scans); nk[0] = kept records.  Fills the columns (status:
// the record's own) and the accumulators.
hipError_t launch_bai_keys(const BaiIn& I, int64_t* scratch, int64_t* nk, const BaiCols& o, const BaiAcc& A,
                           hipStream_t st);
// The order test against the kept record before (status, first_bad), the run heads and their scan (head, hx: n + 1
// int64 each; nruns[0] = runs), and the runs in file order with their sort keys (tid << 16 | bin).
hipError_t launch_bai_runs(const BaiCols& o, int64_t n, const int64_t* nk, int64_t* head, int64_t* hx, int64_t* nruns,
                           uint64_t* first_bad, bai::Run* runs, uint64_t* key, hipStream_t st);
// sorted[s] = runs[idx[s]]
hipError_t launch_bai_gather(const bai::Run* runs, const uint32_t* idx, int64_t nruns, bai::Run* sorted, hipStream_t st);
// win[base[tid] + w] = the smallest u of a record over window w (win starts as all-ones, nwin entries), then every
// untouched window takes the next touched one's value, reference by reference
hipError_t launch_bai_linear(const BaiCols& o, int64_t n, const int64_t* nk, const int64_t* base, const uint64_t* n_intv,
                             int32_t nref, uint64_t* win, int64_t nwin, hipStream_t st);

}  // namespace uc
