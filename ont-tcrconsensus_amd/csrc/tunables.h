// tunables.h -- every UMICLUST_* environment variable the C side reads.  Host-only, no HIP:
// g++ builds tunables.cpp, for the library and for the CPU suite's sanitizer programs.
#pragma once
#include "resolve.h"

namespace uc {

// A context's switches, read once by umiclust_create.
struct Tunables {
  // split passes (depth 2, UMICLUST_SPLIT=0 turns them off): a block's counting runs against the index
  // before the block two ahead is resolved, that block's hits flagged; only the merge and the alignment
  // wait for its resolution, so the counting leaves the host <-> device critical cycle
  int32_t split_env = -1;          // UMICLUST_SPLIT (-1: single-bin loads split, multi-bin sets do not)
  bool pin = true;                 // UMICLUST_PIN=0: host resolve threads not kept in the caller's L3 domain (L3Pin;
                                   // config 2 on two boxes: 3.41-3.90 M unpinned, 3.84-3.93 M pinned, profiles/r02/pin_ab.json);
                                   // off by default when LOCAL_WORLD_SIZE > 1
  bool pin_forced = false;         // UMICLUST_PIN=1: pinned even beside other contexts / ranks
  int par_min = kParInorderMin;    // UMICLUST_PAR_MIN: open queries from which the in-order phase runs on the pool
  int32_t band_pairs = 140000;     // UMICLUST_BAND: alignment launches of at most this many pairs run banded
                                   // (launch bound: a few one-lane waves per SIMD); 70,000 before the faster
                                   // k_align_pk (profiles/r03/band_ab.json)
  // UMICLUST_RESOLVE_THREADS: host threads of resolve_pass (caller included); 0: 8 while this is the process's only
  // context (config 2: host resolve 0.22 -> 0.14 s per step, profiles/r03/resolve_threads_ab.json), 4 beside others
  int32_t resolve_threads = 0;
  // UMICLUST_BLOCK; unset: a bin of n queries uses blocks of about n / block_div (>= kBlockMin): a small bin's
  // window then holds fewer same-molecule peers (fewer speculative peer alignments and overflows)
  int32_t block_size = 8192, block_div = 16;
  // UMICLUST_MIXLEN=0: blocks end at every query-length change (one alignment launch per round); =1: a block spans
  // up to kSegLens lengths (one launch per length and round): a small bin is then a few passes, not one per length
  int32_t mix_len = -1;  // -1: bins whose default block is below kMaxBlock (the bin has < 16 x kMaxBlock queries)
  int32_t pf1_lds = 10240;         // UMICLUST_PF1: one-wave counting units up to this LDS per unit (0: never)
  int32_t regrow = 8;              // UMICLUST_REGROW: clean shallow blocks before a halved block size doubles (0: never)
  // UMICLUST_FQ_CHUNK: quality bytes per chunk of the fastq_filter drop-in (its memory use: two pinned staging buffers
  // of this size plus one on the device; the file is never held whole), within [1 KiB, 2 GiB]
  int64_t fq_chunk = 64ll << 20;
  // UMICLUST_BGZF_WRITE=device|host: where umiclust_bam_write deflates its blocks; UMICLUST_BGZF_BATCH:
  // blocks per batch of the device writer within [1, 65536] (its memory use: two pinned staging buffers of
  // 0xff00 bytes a block, and on the device the input, one output slot a block and the framed bytes)
  bool bgzf_device = true;
  int32_t bgzf_batch = 1024;
  bool pf_prof = false, pf_probe = false;  // UMICLUST_PFPROF, UMICLUST_PFPROBE: the counting kernel's two instruments
  int debug = 0;  // UMICLUST_DEBUG: 1 per-block lines and sequential in-order resolution; 2 the per-bin summary only
  // UMICLUST_WALK_DUMP=<file>: per sorted seqno of the bin, the alignments each strand's walk counted and the
  // path that resolved it (0 device, 1 classify thread, 2 in order, 3 round B) -- a parity-debugging aid
  const char* walk_dump = nullptr;
  // UMICLUST_RESOLVE_DUMP=<prefix>[:i,j,...]: record resolve_block's inputs and outputs of the i-th, j-th, ... passes
  // of the context (default 10, 40, 80) to <prefix>.<i>.bin (single-bin clustering only)
  const char* resolve_dump = nullptr;
};
Tunables read_tunables();
// the switches that are no context's, each read when it is called
int env_debug();                  // UMICLUST_DEBUG's level (as Tunables::debug)
int env_io_threads();             // UMICLUST_IO_THREADS within [1, 16]; 0: unset
const char* env_o4();             // UMICLUST_O4's value, nullptr: unset
bool env_overlap_test_collide();  // UMICLUST_OVERLAP_TEST_COLLIDE is set
void warn_unknown_env();          // names retired or misspelled UMICLUST_* variables on stderr, once per process

}  // namespace uc
