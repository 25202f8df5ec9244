/*
 * umiclust.h -- C ABI of the MI355X-native UMI clustering hot path.
 *
 * Drop-in for the `vsearch --cluster_fast ... --consout ... --clusters ...` subprocess that
 * the reference runs per region bin:
 *   - round 1: /root/reference/ont_tcr_consensus/vsearch_umi_cluster.py:8-56  (vsearch_cluster)
 *   - round 2: /root/reference/ont_tcr_consensus/vsearch_umi_cluster.py:59-99 (vsearch_cluster_consensus)
 * The reference's boundary is `subprocess.run(argv)` (vsearch_umi_cluster.py:21,71) with files
 * as the only data exchange; `umiclust_run_argv` accepts that exact argv, `umiclust_run_fasta`
 * the decoded parameters, and the session API (`umiclust_load` / `umiclust_cluster` /
 * `umiclust_fetch`) the in-memory form used by the benchmark (inputs resident in HBM).
 *
 * Conventions: plain C types only; every function returns 0 (or a count) on success and a
 * negative UMICLUST_E* code on failure, never throws across the ABI; one umiclust_ctx per
 * (process, GPU); a context is not thread-safe, distinct contexts are.
 */
#ifndef UMICLUST_H
#define UMICLUST_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UMICLUST_ABI_VERSION 9

/* error codes (negative returns) */
#define UMICLUST_OK 0
#define UMICLUST_EINVAL (-22)   /* bad argument / parameters / argv */
#define UMICLUST_EIO (-5)       /* file read/write failure */
#define UMICLUST_ENOMEM (-12)   /* host or device allocation failed */
#define UMICLUST_EDEVICE (-19)  /* no HIP device / HIP runtime error */
#define UMICLUST_ESTATE (-77)   /* call out of order (e.g. cluster before load) */
#define UMICLUST_ERANGE (-34)   /* a sequence exceeds the supported length (UMICLUST_MAX_LEN) */

#define UMICLUST_MAX_LEN 112    /* longest sequence the kernels are compiled for */

/* gap slots (vsearch --gapopen/--gapext letters): Q = gap in the query (CIGAR I, consumes the
 * target), T = gap in the target (CIGAR D, consumes the query); L/I/R = left end, interior,
 * right end. */
enum { UMICLUST_QL = 0, UMICLUST_TL = 1, UMICLUST_QI = 2, UMICLUST_TI = 3, UMICLUST_QR = 4,
       UMICLUST_TR = 5 };

typedef struct umiclust_params {
  double id;              /* --id */
  double weak_id;         /* vsearch --weak_id (fraction); only classifies rejects */
  int32_t minseqlength;   /* --minseqlength */
  int32_t maxseqlength;   /* --maxseqlength */
  int32_t wordlength;     /* --wordlength (8; the kernels require 8) */
  int32_t minwordmatches; /* --minwordmatches (12 for wordlength 8) */
  int32_t maxaccepts;     /* --maxaccepts (1) */
  int32_t maxrejects;     /* --maxrejects (32) */
  int32_t match;          /* --match */
  int32_t mismatch;       /* --mismatch */
  int32_t gap_open[6];    /* --gapopen, indexed by UMICLUST_QL..UMICLUST_TR */
  int32_t gap_ext[6];     /* --gapext.  The 16-bit aligners take |match| + |mismatch| <= 66 and, per index,
                             gap_open >= 0, gap_ext >= 0, gap_open + gap_ext <= 66; anything else is
                             UMICLUST_EINVAL (DESIGN.md section 6 has the full condition) */
  int32_t strand_both;    /* --strand both */
  int32_t qmask_dust;     /* --qmask dust (vsearch default) */
  int32_t clusterout_sort;/* --clusterout_sort */
  int32_t clusterout_id;  /* --clusterout_id */
  int32_t fasta_width;    /* --fasta_width (80) */
  int32_t policy_boundary_open; /* E(i,0)/F(0,j) opened from the DP
                                   boundary (1, default) or -inf (0) */
  int32_t threads;        /* --threads n (vsearch_umi_cluster.py:33-34,83-84; n >= 25 in the pipeline,
                             utils.py:56-63).  Only read under policy_threads = 1. */
  int32_t policy_threads; /* SURVEY Appendix C O4 [L]: 0 (default) = the sequential definition (vsearch
                             --threads 1, cluster_core_serial); 1 = vsearch's multithreaded cluster_fast
                             restated (cluster_core_parallel): rounds of `threads` queries, each searched
                             against the index frozen at the round's start, then re-checked in order against
                             the round's new centroids (inserted into its hit list by k-mer count and
                             re-walked one alignment at a time).  umiclust_params_from_argv sets 1 whenever
                             the argv's --threads is > 1 (the reference's --threads 25: since round 5, ABI 8),
                             unless the environment has UMICLUST_O4=sequential. */
} umiclust_params;

/* presets */
#define UMICLUST_PRESET_ROUND1 1          /* --gapopen 0E/40I --mismatch -40 --match 10 */
#define UMICLUST_PRESET_VSEARCH_DEFAULT 2 /* --match 2 --mismatch -4 --gapopen 20I/2E */

typedef struct umiclust_stats {
  int64_t n_input;        /* records read */
  int64_t n_kept;         /* records within [minseqlength, maxseqlength] */
  int64_t n_clusters;
  int64_t n_alignments;   /* alignments vsearch's procedure performs (GCUPS numerator set) */
  int64_t cells;          /* sum of Lq*Lt over those alignments */
  int64_t cells_computed; /* cells the GPU computed (incl. speculative work) */
  int64_t kmer_postings;  /* prefilter postings touched */
  int64_t n_blocks;       /* greedy blocks */
  double t_total_s;       /* wall time of umiclust_cluster */
  double t_prefilter_s;   /* kernel time, prefilter (HIP events) */
  double t_align_s;       /* kernel time, alignment */
  double t_consensus_s;   /* kernel time, traceback + consensus */
  double t_host_s;        /* host greedy resolve */
  int64_t n_deferred;     /* queries resolved by the host's exact merged walk (in-block peers) */
  int64_t pairs_round_b;  /* alignments issued for deferred queries */
  int64_t pairs_peer;     /* speculative in-block peer alignments */
  double t_index_s;       /* kernel time, index tile rebuilds */
  double t_sync_s;        /* host wall time blocked on device->host result copies */
  double t_host_pass1_s;  /* host first in-order pass of every block */
  int64_t n_merged_walks; /* (query, strand) walks the host re-ran with in-block centroids */
  double t_merged_s;      /* host time inside those merged walks */
  double t_read_s;        /* file path: FASTA read + parse (umiclust_run_fasta*) */
  double t_write_s;       /* file path: cluster<N> / consout (+ in-process parse) writing */
  double t_run_s;         /* file path: the whole call, read to files written */
  int64_t n_reruns;       /* block pieces re-run alone after an in-window peer list overflowed */
  int64_t n_overlap_passes; /* overlap hash-table passes (1 + re-seeds after 64-bit hash collisions) */
  int64_t n_lazy_passes;  /* passes whose in-window peers were aligned on demand (round B) only */
  double t_count_s;       /* kernel time, the prefilter's counting kernel alone (k_pf_count, HIP events) */
  int64_t n_count_launches; /* its launches (one per pass over one counter segment) */
  int64_t kmer_postings_deferred; /* postings of the lists the counting kernel deferred (frequent k-mers whose
                                     matches it adds per surviving target instead; x 8 chunks, incl. padding;
                                     0 since round 5: the deferral was removed) */
  int64_t counter_cells;  /* ABI 8: sum over the counting launches of query-strands x centroids indexed (the C of
                             SURVEY 8d's prefilter bytes, postings x 4 B + C x 2 B counter traffic) */
  int64_t n_regrows;      /* ABI 9: times a block size halved by a peer-list overflow doubled again (after `regrow`
                             clean, shallow blocks; UMICLUST_REGROW) */
} umiclust_stats;

typedef struct umiclust_ctx umiclust_ctx;

/* ---- versioning / parameters ---- */
int32_t umiclust_abi_version(void);
/* fill p with a preset (UMICLUST_PRESET_*) and the given identity / length window */
int32_t umiclust_params_init(umiclust_params *p, int32_t preset, double identity,
                             int32_t minseqlength, int32_t maxseqlength);
/* parse a vsearch argv (argv[0] may be "vsearch"); fills p and the path outputs (each
 * buffer of pathcap bytes, may be NULL).  Unknown options -> UMICLUST_EINVAL. */
int32_t umiclust_params_from_argv(umiclust_params *p, int32_t argc, const char *const *argv,
                                  char *in_fasta, char *clusters_prefix, char *consout,
                                  char *log_path, int32_t pathcap);

/* ---- context ---- */
/* device_id >= 0 selects a HIP device; there is no CPU backend (a missing device returns NULL
 * and sets *err = UMICLUST_EDEVICE). */
umiclust_ctx *umiclust_create(int32_t device_id, int32_t *err);
void umiclust_destroy(umiclust_ctx *ctx);
/* ABI 7: the context's main (counting) stream at the device's greatest stream priority (level 1) or a plain
 * stream (level 0, the default); its alignment stream is prioritised at both levels.  Level -1 (background):
 * every stream plain, the alignment stream included.  Lets a caller running several bins at once on one GPU
 * (BinRunner lanes; tcr_consensus.py:231-245 runs one vsearch per bin) put the bins that set the makespan ahead
 * of the others.  Synchronises the context first.  Results do not depend on it. */
int32_t umiclust_set_priority(umiclust_ctx *ctx, int32_t level);
/* Waits for the host work a file-path call (umiclust_run_fasta / _run_argv / _run_fasta_parse) leaves running after
 * it returns: the release of its input (unmapping a multi-GB FASTA, ~0.11 s for config 2's 3.5 GB) and of the fused
 * path's smolecule_clusters.fa mapping (RAM-backed outputs; the file's contents are in place before the call returns),
 * done on a thread of the context once every output is written.  The context's next file-path call and umiclust_destroy wait
 * for it too.  Returns UMICLUST_OK.  (Round 6; an added function, the struct layouts are unchanged.) */
int32_t umiclust_wait_host(umiclust_ctx *ctx);
/* human-readable message for the last error on this context */
const char *umiclust_last_error(const umiclust_ctx *ctx);

/* ---- whole-file drop-in (vsearch CLI semantics) ---- */
/* Reads in_fasta, clusters, writes <clusters_prefix><N> per cluster, the consout FASTA and a
 * text log.  Any output path may be NULL. Returns number of clusters (>=0) or an error. */
int64_t umiclust_run_fasta(umiclust_ctx *ctx, const umiclust_params *p, const char *in_fasta,
                           const char *clusters_prefix, const char *consout, const char *log_path,
                           umiclust_stats *stats);
/* same, from the exact vsearch argv the reference builds (vsearch_umi_cluster.py:22-53). */
int64_t umiclust_run_argv(umiclust_ctx *ctx, int32_t argc, const char *const *argv,
                          umiclust_stats *stats);

/* ---- in-process consumer ---- */
/* Parameters of the reference's parse_umi_clusters / polish_cluster
 * (/root/reference/ont_tcr_consensus/parse_umi_clusters.py:10-21, :143-151). */
typedef struct umiclust_parse_params {
  int32_t min_reads_per_cluster;  /* min_reads_per_cluster (20) */
  int32_t max_reads_per_cluster;  /* max_reads_per_cluster (60) */
  int32_t balance_strands;        /* balance_strands (0) */
  int32_t max_clusters;           /* max_clusters; 0 = no limit (the reference's None); any other value
                                     stops once n_written > max_clusters, as Python's truthiness does */
} umiclust_parse_params;

typedef struct umiclust_parse_result {
  int64_t n_clusters;     /* consout records */
  int64_t n_written;      /* clusters written to clusters_fa/ */
  int64_t reads_found;    /* the reference's running total as it computes it (last cluster's count x 2) */
  int64_t reads_written;  /* likewise */
  int32_t empty_region;   /* 1: n_written == 0 or reads_found == 0 -- the caller appends the region to
                             regions_wo_clusters_txt (parse_umi_clusters.py:222-231) and no log is written */
  int32_t pad;
} umiclust_parse_result;

/* Replaces the vsearch_cluster -> parse_umi_clusters task pair (tcr_consensus.py:237-265 round 1,
 * :419-444 round 2; consumer parse_umi_clusters.py:10-242).
 * umiclust_run_fasta followed by parse_umi_clusters' outputs straight from the in-memory clusters:
 * <work_dir>/clusters_fa/cluster<N>.fasta, <work_dir>/smolecule_clusters.fa,
 * <work_dir>/vsearch_cluster_stats.tsv and <work_dir>/parse_cluster.log, byte-identical to running
 * the reference's parse_umi_clusters on the files umiclust_run_fasta writes (work_dir = the consout's
 * directory; clusterout_sort and clusterout_id must be set).  clusters_prefix may be NULL: the
 * per-cluster vsearch files, which the consumer only re-reads, are then not written at all.
 * <work_dir>/clusters_fa must not exist (UMICLUST_EEXIST).  A record header without the 7
 * `;`-separated fields or a strand other than + / - is UMICLUST_EFORMAT (the reference raises). */
#define UMICLUST_EEXIST (-17)   /* output directory already exists */
#define UMICLUST_EFORMAT (-74)  /* a record header does not follow the extract_umis format */
int64_t umiclust_run_fasta_parse(umiclust_ctx *ctx, const umiclust_params *p, const char *in_fasta,
                                 const char *clusters_prefix, const char *consout, const char *log_path,
                                 const umiclust_parse_params *pp, const char *work_dir,
                                 umiclust_parse_result *result, umiclust_stats *stats);

/* ---- session API (in-memory, inputs resident in HBM) ---- */
/* Stage n sequences (concatenated ASCII `seqs`, record i at [offsets[i], offsets[i+1])) into
 * device memory, then prepare them (umiclust_prepare).  = umiclust_stage + umiclust_prepare. */
int32_t umiclust_load(umiclust_ctx *ctx, const umiclust_params *p, const char *seqs,
                      const int64_t *offsets, int64_t n);
/* The two halves of umiclust_load (ABI 6).  umiclust_stage copies the raw records into HBM (bin_start as in
 * umiclust_load_bins; NULL = one bin) and keeps them resident.  umiclust_prepare does vsearch's load-time work on
 * the staged records (the length filter, DUST soft-masking and the stable length sort that
 * `vsearch --cluster_fast` runs before clustering; vsearch_umi_cluster.py:21-54 starts it): the length
 * filter and sort on the host, DUST, 4-bit codes and unique 8-mers on the device.  It may be called again with
 * other parameters (or the same, benchmarking: the headline times umiclust_prepare + umiclust_cluster). */
int32_t umiclust_stage(umiclust_ctx *ctx, const char *seqs, const int64_t *offsets, int64_t n,
                       const int64_t *bin_start, int32_t nbins);
int32_t umiclust_prepare(umiclust_ctx *ctx, const umiclust_params *p);
/* Run the hot path on the loaded sequences (prefilter, alignment, greedy, consensus).
 * Returns number of clusters. May be called repeatedly (benchmarking). */
int64_t umiclust_cluster(umiclust_ctx *ctx, umiclust_stats *stats);
/* Fetch results for the input records (input order):
 *   cluster[i]  output cluster number (clusterout_sort numbering), -1 if length-filtered
 *   strand[i]   0 '+', 1 '-' (orientation of record i relative to its centroid)
 *   centroid[i] 1 if record i is its cluster's centroid
 * and the consensus sequences: cluster c is cons[cons_off[c] .. cons_off[c+1]) (cons_off has
 * n_clusters+1 entries; cons capacity cons_cap bytes). Any pointer may be NULL. */
int64_t umiclust_fetch(umiclust_ctx *ctx, int32_t *cluster, uint8_t *strand, uint8_t *centroid,
                       char *cons, int64_t cons_cap, int64_t *cons_off);

/* ---- many region bins per load (BASELINE configs 3 and 4) ---- */
/* The reference runs one vsearch process per (library x region bin) (tcr_consensus.py:231-245 round 1,
 * :411-427 round 2).  A load may hold many such bins resident in HBM at once: bin b is input records
 * [bin_start[b], bin_start[b+1]) (bin_start has nbins+1 entries, bin_start[0] = 0, bin_start[nbins] = n).
 * Every bin is length-filtered, sorted and clustered on its own, exactly as its own vsearch run would
 * be; umiclust_load / umiclust_cluster / umiclust_fetch are the nbins = 1 case. */
int32_t umiclust_load_bins(umiclust_ctx *ctx, const umiclust_params *p, const char *seqs,
                           const int64_t *offsets, int64_t n, const int64_t *bin_start, int32_t nbins);
/* cluster one bin of the load; returns its number of clusters */
int64_t umiclust_cluster_bin(umiclust_ctx *ctx, int32_t bin, umiclust_stats *stats);
/* cluster the bins [first, first + nbins) of the load as one pack: the bins' queries in one greedy order (each bin
 * sorted on its own, the bins one after another), so small bins share the GPU passes of the bins around them.  Every
 * bin's result is exactly its own vsearch run's (tcr_consensus.py:231-245 runs one vsearch per bin); fetch each with
 * umiclust_fetch_bin.  Stats cover the whole pack; returns the pack's number of clusters.  Under the batched O4
 * policy every bin's rounds are counted from its own first sorted query. */
int64_t umiclust_cluster_pack(umiclust_ctx *ctx, int32_t first, int32_t nbins, umiclust_stats *stats);
/* umiclust_fetch for one clustered bin: arrays over the bin's input records (bin-local index) */
int64_t umiclust_fetch_bin(umiclust_ctx *ctx, int32_t bin, int32_t *cluster, uint8_t *strand,
                           uint8_t *centroid, char *cons, int64_t cons_cap, int64_t *cons_off);

/* ---- region-vs-region UMI overlap ---- */
/* Replaces the Python string scans of /root/reference/ont_tcr_consensus/extract_umis.py.
 * umiclust_overlap_counts: count_single_umi_overlaps (:270-290) for every UMI of set 1 at once:
 *   counts[i] = number of set-2 sequences byte-equal to set-1 sequence i.
 * umiclust_overlap_regions: count_overlapping_umis_between_2_regions (:293-342) for every region pair of
 *   count_overlapping_umis_between_all_regions (:345-369): region r = sequences [region_start[r],
 *   region_start[r+1]); for a < b, total[a * nregions + b] = the pair's summed count (the TSV value) and
 *   maxcount[a * nregions + b] = the largest count of one region-a UMI (> 1 = the warning).  Entries with
 *   a >= b are 0.  A GPU hash join: exact (byte comparison; a 64-bit hash collision re-runs with another
 *   seed). */
#define UMICLUST_OVERLAP_MAX_REGIONS 4096
int32_t umiclust_overlap_counts(umiclust_ctx *ctx, const char *seqs1, const int64_t *offsets1, int64_t n1,
                                const char *seqs2, const int64_t *offsets2, int64_t n2, int64_t *counts);
int32_t umiclust_overlap_regions(umiclust_ctx *ctx, const char *seqs, const int64_t *offsets, int64_t n,
                                 const int64_t *region_start, int32_t nregions, int64_t *total,
                                 int32_t *maxcount);

/* ---- UMI extraction ---- */
/* Replaces extract_umis (/root/reference/ont_tcr_consensus/extract_umis.py:189-267): per read, the first
 * adapter_length_5_end and the last adapter_length_3_end bases (:110-126) are searched for umi_fwd / umi_rev
 * as edlib does (:89-107: mode "HW", task "path", k = max_pattern_dist, the IUPAC additionalEqualities of
 * :26-87).  umiclust_extract_umis: out[i*6 + 0..2] = (edit distance or -1, start, end) of the 5' UMI in
 * its window, out[i*6 + 3..5] of the 3' UMI.  umiclust_extract_umis_file: FASTA or FASTQ in, the
 * <region>_detected_umis.fasta records of write_fasta (:154-186) out, in input order; returns the number
 * of reads with both UMIs (the reference's n_both_umi).  Patterns of 1..64 symbols.  A record name
 * without "strand=" is UMICLUST_EFORMAT ("Read strand not annotated!"). */
int32_t umiclust_extract_umis(umiclust_ctx *ctx, const char *seqs, const int64_t *offsets, int64_t n,
                              int32_t adapter_length_5_end, int32_t adapter_length_3_end,
                              int32_t max_pattern_dist, const char *umi_fwd, const char *umi_rev, int32_t *out);
int64_t umiclust_extract_umis_file(umiclust_ctx *ctx, const char *fastx_file, const char *out_fasta,
                                   int32_t adapter_length_5_end, int32_t adapter_length_3_end,
                                   int32_t max_pattern_dist, const char *umi_fwd, const char *umi_rev);

/* ---- region binning ---- */
/* Replaces the record loop of filter_and_split_reads_by_region_cluster
 * (/root/reference/ont_tcr_consensus/region_split.py:219-333): BAM in (BGZF inflated on the device, DESIGN.md §9e,
 * records classified and FASTA records built on the device), every kept primary alignment appended to
 * <out_dir>/region_cluster<k>.fasta as `>{query_name};strand={+|-}` + its forward sequence, in BAM order.
 * Regions come from the reference FASTA (names, lengths) and the cluster JSON (region_clusters[r], -1 if the
 * region is not in it).  counts = {n_unmapped, n_primary_mapped, n_short, n_long} of the records the
 * reference's loop reaches; reads_per_cluster[k] (ncluster_cap entries); region_detected[r] = 1 if a kept
 * record aligned to region r.  Returns the number of cluster files appended to.  A record aligned to a
 * reference missing from the regions (or from the cluster JSON once it passes the filters) stops the loop
 * as the reference's KeyError does: the records before it are written and UMICLUST_EFORMAT is returned with
 * the name in missing_name.  A record whose l_read_name, n_cigar_op or l_seq do not fit its block_size is
 * refused before anything runs on the device: UMICLUST_EFORMAT naming the record, missing_name not written,
 * nothing written. */
int64_t umiclust_region_split(umiclust_ctx *ctx, const char *bam_file, int32_t nregions,
                              const char *const *region_names, const int64_t *region_lengths,
                              const int32_t *region_clusters, double minimal_region_overlap,
                              int32_t max_softclip_5_end, int32_t max_softclip_3_end, const char *out_dir,
                              int64_t *counts, int64_t *reads_per_cluster, int32_t ncluster_cap,
                              uint8_t *region_detected, char *missing_name, int32_t missing_cap);

/* ---- region binning fused with UMI extraction (row f4+f1) ---- */
/* umiclust_region_split followed by umiclust_extract_umis_file on every file it wrote, in one pass over the BAM and
 * without the region FASTA files: for every cluster k with a kept record, <umi_out_dir>/region_cluster<k>_detected_umis.fasta
 * is created (truncated, as the reference opens it with "w") and holds, in BAM order, one write_fasta record
 * (extract_umis.py:154-186) per kept record in whose two windows both UMIs were found -- the bytes the two calls
 * produce one after the other; a cluster whose reads yield no UMI gets an empty file.  The UMI search runs on the
 * device on the record's 4-bit sequence: the read is the text umiclust_region_split would have written (the forward
 * sequence, `None` for a record without one), the windows are seq[:adapter_length_5_end] and
 * seq[-adapter_length_3_end:] (any lengths >= 0), the patterns umiclust_extract_umis' (1..64 symbols).  The header
 * fields are those of the text `{query_name};strand={+|-}`: read name = that text up to its first ';', strand = what
 * follows its first "strand=" up to the next one, so a query name holding ';' or "strand=" comes out as from the
 * two calls.  counts, reads_per_cluster, region_detected, missing_name and the refusal of malformed records are
 * umiclust_region_split's; umis_per_cluster[k] (ncluster_cap entries) = records written for cluster k (the
 * reference's n_both_umi).  Returns the number of clusters with a kept record = files created.
 * The reference's KeyError (see umiclust_region_split): counts and missing_name are filled, UMICLUST_EFORMAT is
 * returned and no file is created, since the exception ends the pipeline before extract_umis starts.
 * Differences: a kept record whose query name holds a byte in "\t\n\v\f\r " (SAM forbids them) is refused with
 * UMICLUST_EFORMAT naming the record, nothing written; and the read keeps a '=' base code, which the FASTA parser of
 * umiclust_extract_umis_file drops (it keeps letters only) and the reference's reader keeps. */
int64_t umiclust_region_split_extract(umiclust_ctx *ctx, const char *bam_file, int32_t nregions,
                                      const char *const *region_names, const int64_t *region_lengths,
                                      const int32_t *region_clusters, double minimal_region_overlap,
                                      int32_t max_softclip_5_end, int32_t max_softclip_3_end,
                                      int32_t adapter_length_5_end, int32_t adapter_length_3_end,
                                      int32_t max_pattern_dist, const char *umi_fwd, const char *umi_rev,
                                      const char *umi_out_dir, int64_t *counts, int64_t *reads_per_cluster,
                                      int64_t *umis_per_cluster, int32_t ncluster_cap, uint8_t *region_detected,
                                      char *missing_name, int32_t missing_cap);

/* ---- quality filtering (row f5) ---- */
/* Replaces the `vsearch --fastq_filter` subprocess of vsearch_fastq_filtering
 * (/root/reference/ont_tcr_consensus/preprocessing.py:104-159, argv :129-148; run once per library between
 * dorado_trim and minimap2_ont_align, tcr_consensus.py:156-169).  vsearch runs it on one thread (:104); here the
 * host threads index the mapped FASTQ in chunks and gather the quality bytes, the device sums each record's
 * expected error in fixed point (ee_fx = sum of llrint(10^(-q/10) * 2^40), order-independent), and the host decides,
 * recomputing in double exactly as vsearch states it whatever falls within a guard band of a threshold.  Policies
 * O7a-O7f (record form, quality range, expected error, decision order, options, log) are in DESIGN.md §9a.
 * The reference's own seqkit calls (:126-127, :156-157) are served by the same pass when it is asked for them:
 * umiclust_fastq_filter_stats below (row f5b). */
typedef struct umiclust_fastq_filter_params {
  int32_t fastq_ascii;      /* --fastq_ascii: 33 (default) or 64 */
  int32_t fastq_qmin;       /* --fastq_qmin (0) */
  int32_t fastq_qmax;       /* --fastq_qmax (41; the reference passes 93, :136-137) */
  int32_t fastq_minlen;     /* --fastq_minlen (1; the reference passes minimal_length, :140-141) */
  int32_t fastq_maxlen;     /* --fastq_maxlen; -1 = no limit */
  int32_t pad;
  double fastq_maxee;       /* --fastq_maxee; < 0 = not given */
  double fastq_maxee_rate;  /* --fastq_maxee_rate; < 0 = not given (the reference passes max_ee_rate_base, :138-139) */
} umiclust_fastq_filter_params;

typedef struct umiclust_fastq_filter_result {
  int64_t n_input, n_kept, n_discarded, bases_in, bases_kept;
  int64_t n_short, n_long, n_maxee, n_maxee_rate; /* discarded records by their first failing criterion (O7d order) */
  int64_t n_host_rechecked; /* records inside the guard band, decided by the host's sequential double sum */
  int64_t n_chunks;
  double ee_in, ee_kept;    /* sums, in input order, of the records' ee_fx * 2^-40 */
  double t_read_s;          /* indexing + gathering, summed over the chunks (overlaps the rest) */
  double t_h2d_s;           /* host-to-device copies (HIP events), summed */
  double t_kernel_s;        /* the kernel (HIP events), summed */
  double t_write_s;         /* decision + writers, summed */
  double t_total_s;         /* wall time of the call */
} umiclust_fastq_filter_result;

/* Parse the argv of preprocessing.py:129-148 (argv[0] may be "vsearch"); every option in the `--opt` and the `-opt`
 * spelling.  Fills p and the paths (each buffer of pathcap bytes, may be NULL).  Needs no context and no device.
 * Options outside O7e, a missing --fastq_filter or no output file -> UMICLUST_EINVAL. */
int32_t umiclust_fastq_filter_params_from_argv(umiclust_fastq_filter_params *p, int32_t argc,
                                               const char *const *argv, char *in_fastq, char *fastqout,
                                               char *fastqout_discarded, char *log_path, int32_t pathcap);
/* Filter in_fastq: kept records to fastqout, the others to fastqout_discarded, each as `@label\nSEQ\n+\nQUAL\n` in
 * input order; a text log with vsearch's summary line.  Any output path may be NULL.  Returns the number of kept
 * records.  A quality byte outside [fastq_qmin, fastq_qmax] is UMICLUST_EFORMAT naming the first such record; the
 * records before it are written.  Malformed FASTQ is UMICLUST_EFORMAT, gzip input UMICLUST_EINVAL. */
int64_t umiclust_fastq_filter(umiclust_ctx *ctx, const umiclust_fastq_filter_params *p, const char *in_fastq,
                              const char *fastqout, const char *fastqout_discarded, const char *log_path,
                              umiclust_fastq_filter_result *result);
/* same, from the exact argv the reference builds */
int64_t umiclust_fastq_filter_argv(umiclust_ctx *ctx, int32_t argc, const char *const *argv,
                                   umiclust_fastq_filter_result *result);

/* ---- seqkit's `stat -a` tables from the same pass (row f5b; DESIGN.md §9a, policy O8) ---- */
/* vsearch_fastq_filtering also runs `seqkit stat -a` on the raw FASTQ before the filter
 * (ont_tcr_consensus/preprocessing.py:126-127) and on the filtered FASTQ after it (:156-157);
 * analysis.py:76-81 reads the AvgQual column of the text.  The numbers of one table: integers counted exactly, and
 * the doubles O8c-O8e derive from them alone, so they do not depend on chunk size, thread count or backend. */
typedef struct umiclust_fastq_stats {
  int64_t num_seqs, sum_len, min_len, max_len;
  int64_t n50, n50_num;          /* O8c: the length at which the descending cumulative sum reaches half, and L50 */
  int64_t n_q20, n_q30;          /* quality bytes with byte - fastq_ascii >= 20 / >= 30 */
  int64_t n_gc, sum_n, sum_gap;  /* sequence bytes in "GCgc", in "Nn", in "-. " */
  uint64_t ee_fx_lo, ee_fx_hi;   /* the 128-bit sum of the records' ee_fx (2^-40 units) */
  int32_t type;                  /* O8f: 0 DNA, 1 RNA, 2 Protein */
  int32_t pad;
  double avg_len, q1, q2, q3;    /* O8c */
  double q20_pct, q30_pct, avg_qual, gc_pct; /* O8d, O8e */
} umiclust_fastq_stats;

/* umiclust_fastq_filter, and the two tables of preprocessing.py:126-127,156-157 (read by analysis.py:76-81) from
 * the same pass: stats_before_txt describes every record the filter read (its `file` column is in_fastq),
 * stats_after_txt every record it kept (`file` is fastqout, "-" without one); the text is policy O8.  before / after
 * receive the tables' numbers.  Any of the last five arguments may be NULL; with fastqout, fastqout_discarded and
 * log_path all NULL it is a statistics-only pass.  The two texts are written only when the whole call succeeds: on an
 * error the filter outputs are what umiclust_fastq_filter leaves and no statistics file is written. */
int64_t umiclust_fastq_filter_stats(umiclust_ctx *ctx, const umiclust_fastq_filter_params *p, const char *in_fastq,
                                    const char *fastqout, const char *fastqout_discarded, const char *log_path,
                                    const char *stats_before_txt, const char *stats_after_txt,
                                    umiclust_fastq_filter_result *result, umiclust_fastq_stats *before,
                                    umiclust_fastq_stats *after);
/* same, from the exact argv the reference builds (:129-148) beside its two seqkit calls (:126-127, :156-157; the
 * AvgQual column is what analysis.py:76-81 reads) */
int64_t umiclust_fastq_filter_stats_argv(umiclust_ctx *ctx, int32_t argc, const char *const *argv,
                                         const char *stats_before_txt, const char *stats_after_txt,
                                         umiclust_fastq_filter_result *result, umiclust_fastq_stats *before,
                                         umiclust_fastq_stats *after);

/* ---- consensus alignment filter and cs-tag census (row f6) ---- */
/* Replaces the per-record loops of ont_tcr_consensus/minimap2_align.py: count_cs_tags (:21-37, called on every
 * library's raw-read BAM at :140 and on the filtered consensus BAM at :341), calculate_blast_id (:13-18) and the
 * record loop and BAM output of filter_consensus_alignments (:158-359, :209-245).  A BAM session on the context:
 * open inflates the file on the device, scans every record on the device (class, refID, l_seq,
 * reference_length, the M/I/D column sum of :14-16, the NM and cs:Z aux tags) and groups the primary records by
 * their cs string exactly (hashed on the device, every member compared with its group's first record, re-run with
 * another seed on a collision).  The columns, names and strings are then read back in bulk and the Python drop-in
 * (umiclust/minimap2_align.py) forms every float and every line of text from them.
 * Memory model: umiclust_region_split's.  The whole inflated file is held on the host for the session and on the
 * device during open; chunked streaming is out of scope.
 * Errors: UMICLUST_EIO (unreadable or not BGZF), UMICLUST_EFORMAT (not BAM, a truncated record, or a primary
 * record whose fields or aux tags do not fit it -- unknown type byte, a field past the record end, a Z/H string
 * without NUL, an NM that is no integer, a cs that is no Z; the message names the record), UMICLUST_ESTATE (no
 * open session), UMICLUST_ERANGE (buf too small: a call with cap = 0 returns the size needed). */
/* inflate, scan, group; returns the number of records.  State lives in ctx until umiclust_bam_close or the next
 * open.  hash_bits: 64 normally; a smaller value masks the hash on the FIRST pass only (test hook: forces the
 * collision re-run) */
int64_t umiclust_bam_open(umiclust_ctx *ctx, const char *bam_file, int32_t hash_bits);
/* out[0..4] = n_records, n_refs, n_cs_groups, n_hash_reruns, index of the first malformed record or -1.  In an
 * open session out[4] covers layout defects only (variable-length fields that overrun block_size) of a record that is
 * unmapped, secondary or supplementary: the aux fields of such records are not walked, because the reference never
 * reads them, and any defect of a primary record has already failed the open with UMICLUST_EFORMAT */
int32_t umiclust_bam_counts(umiclust_ctx *ctx, int64_t *out);
/* DIAGNOSTIC, not part of the drop-in: out[0..2] = seconds of the last open: wall time from mapping the file until the
 * inflated bytes are on the host (upload of the compressed bytes, k_bgzf_inflate, copy back), host-to-device copies of
 * the compressed bytes and the record offsets (HIP events), scan + group + verify kernels of every hashing pass (HIP
 * events).  tools/bam_scan_bench.py reads the
 * figures of DESIGN.md §9b through it */
int32_t umiclust_bam_times(umiclust_ctx *ctx, double *out);
/* DIAGNOSTIC (an added function, ABI version unchanged): out[0..2] of the last open = BGZF blocks in the file, blocks
 * inflated on the device (every block with ISIZE > 0), compressed bytes uploaded */
int32_t umiclust_bam_inflate_info(umiclust_ctx *ctx, int64_t *out);
/* n-sized arrays, each may be NULL.  cls: 0 unmapped (flag & 4, tested first as :28 does), 1 secondary or
 * supplementary (flag & 0x900), 2 primary mapped.  l_seq is pysam's query_length.  reference_length: M/D/N/=/X
 * lengths, a zero sum counted as 1 (htslib bam_endpos).  cols: M/I/D lengths only (:14-16).  nm / nm_present: the
 * NM tag of any integer type (primary records only, as cs_group).  cs_group: -1 = no cs tag */
int32_t umiclust_bam_columns(umiclust_ctx *ctx, int8_t *cls, int32_t *ref, int32_t *l_seq, int64_t *reference_length,
                             int64_t *cols, int64_t *nm, uint8_t *nm_present, int32_t *cs_group);
/* reference names and lengths of the header: names NUL-joined into buf, off[n_refs+1]; returns the bytes needed */
int32_t umiclust_bam_refs(umiclust_ctx *ctx, char *buf, int64_t cap, int64_t *off, int64_t *len);
/* bulk gather for m records: kind 0 = query_name, 1 = cs string; bytes into buf, off[m+1]; returns bytes needed */
int64_t umiclust_bam_strings(umiclust_ctx *ctx, int32_t kind, const int64_t *rec, int64_t m, char *buf, int64_t cap,
                             int64_t *off);
/* per group (n_cs_groups, first-seen order): count over primary records, representative (= first) record */
int32_t umiclust_bam_cs_groups(umiclust_ctx *ctx, int64_t *count, int64_t *rep);
/* header + the records with keep[r] != 0, as BGZF (blocks of at most 0xff00 payload bytes, EOF block last): the
 * file inflates to the input's header bytes and the kept records' bytes verbatim, in input order (what
 * pysam.AlignmentFile(..., "wb", template=bam_in).write(entry) leaves, :207/:245, up to the compressed form);
 * returns the number written.  The blocks are deflated on the device (batches of UMICLUST_BGZF_BATCH
 * blocks, gathered and CRC32'd by the I/O threads, deflated and framed by k_bgzf_deflate / k_bgzf_frame, written in
 * order); the compressed bytes are valid gzip members but not zlib's.  zlib on the host writes the file instead with
 * UMICLUST_BGZF_WRITE=host, where the memory for a batch cannot be had, and for a single block the encoder refuses */
int64_t umiclust_bam_write(umiclust_ctx *ctx, const uint8_t *keep, const char *out_bam);
/* DIAGNOSTIC (an added function, ABI version unchanged): the session's last umiclust_bam_write.  out[0..7] = blocks
 * (EOF block not counted), blocks deflated on the device, of those stored / fixed / dynamic, blocks redone on the host,
 * batches, compressed bytes (the file's size); times[0..3] = seconds of upload, kernels, copy back (HIP events) and of
 * the host's gather + CRC32.  Either may be NULL.  A file the host wrote reports its blocks and bytes, zero elsewhere.
 * UMICLUST_ESTATE before the first write */
int32_t umiclust_bam_write_info(umiclust_ctx *ctx, int64_t *out, double *times);

/* ---- round-2 region split and precision census on the session (rows f4b / f6b) ---- */
/* Replaces the record loops of filter_and_split_reads_by_region (ont_tcr_consensus/region_split.py:336-435) and of
 * estimate_precision_at_num_subreads (minimap2_align.py:362-435), which the reference runs on the filtered consensus
 * BAM: the session that filtered it is split under the filter's keep mask, so one inflate and one scan serve the
 * filter, the filtered BAM, the cs census and the split.
 * Memory model: the session keeps the inflated file, the record offsets and the columns on the host only.  Each of
 * the two calls uploads what its kernel reads (the raw bytes and offsets; for the split also class, refID, l_seq,
 * reference_length and keep) and frees it on return. */
/* Split the open session's records (keep == NULL: all; else those with keep[r] != 0, the others being "not in the
 * file": skipped and counted nowhere) into FASTA buckets.  Region r of the reference FASTA goes to bucket
 * region_buckets[r] (in [0, nbuckets), or -1: the lookup raises, as a region missing from the cluster JSON does);
 * bucket b is appended to bucket_paths[b] as `>{query_name};strand={+|-}` + the forward sequence (`None` without
 * one), in BAM order.  A record is classified from the session's columns with umiclust_region_split's comparisons
 * (reference_length < L * overlap; l_seq > L * (2 - overlap) + (s5 + s3), the product rounded before the add).
 * counts = {n_unmapped, n_primary_mapped, n_short, n_long}; reads_per_bucket[nbuckets]; region_detected[nregions]
 * (may be NULL).  Returns the number of files appended to.
 * A primary record whose reference is not among the regions, whose refID is -1 (name `None`) or whose bucket is -1
 * stops the loop as umiclust_region_split's does: the records before it are written, the counters cover it as a
 * primary alignment, and UMICLUST_EFORMAT is returned with the name in missing_name.  Only kept primary records are
 * emitted and the open has checked their fields, so none is checked again (an empty name field: UMICLUST_EFORMAT).
 * UMICLUST_ESTATE without an open session, UMICLUST_EIO for a bucket path that cannot be appended to. */
int64_t umiclust_bam_split(umiclust_ctx *ctx, const uint8_t *keep, int32_t nregions, const char *const *region_names,
                           const int64_t *region_lengths, const int32_t *region_buckets, int32_t nbuckets,
                           const char *const *bucket_paths, double minimal_region_overlap, int32_t max_softclip_5_end,
                           int32_t max_softclip_3_end, int64_t *counts, int64_t *reads_per_bucket,
                           uint8_t *region_detected, char *missing_name, int32_t missing_cap);
/* umiclust_bam_split fused with the UMI extraction, as umiclust_region_split_extract fuses umiclust_region_split
 * (row f4+f1): the same arguments, classes, counters and KeyError, but bucket b's kept records go to
 * bucket_umi_paths[b] as detected-UMI records (the file is truncated; one is created for every bucket with a kept
 * record, empty if none of them holds both UMIs) and no region FASTA is written.  umis_per_bucket[nbuckets] = records
 * written.  On the KeyError no file is created.  Returns the number of buckets with a kept record. */
int64_t umiclust_bam_split_extract(umiclust_ctx *ctx, const uint8_t *keep, int32_t nregions,
                                   const char *const *region_names, const int64_t *region_lengths,
                                   const int32_t *region_buckets, int32_t nbuckets,
                                   const char *const *bucket_umi_paths, double minimal_region_overlap,
                                   int32_t max_softclip_5_end, int32_t max_softclip_3_end,
                                   int32_t adapter_length_5_end, int32_t adapter_length_3_end,
                                   int32_t max_pattern_dist, const char *umi_fwd, const char *umi_rev,
                                   int64_t *counts, int64_t *reads_per_bucket, int64_t *umis_per_bucket,
                                   uint8_t *region_detected, char *missing_name, int32_t missing_cap);
/* Per record (n-sized arrays, either may be NULL) the query name's tail: what follows its last "_", or the whole name
 * without one.  A tail of 1 to 18 ASCII digits (leading zeros included): value[r] = its decimal value, status[r] = 1.
 * Any other tail (empty, signed, a non-digit, 19 digits or more): status[r] = 0, value[r] = 0, and the caller applies
 * int(name.split("_")[-1]) itself so that the value or the ValueError is Python's own. */
int32_t umiclust_bam_name_suffix(umiclust_ctx *ctx, int64_t *value, uint8_t *status);
int32_t umiclust_bam_close(umiclust_ctx *ctx);

/* ---- a BAM session straight from SAM text, sorted on the device (added functions, ABI version
 * unchanged) ---- */
/* Replaces `samtools sort` and the read-back of its file in minimap2_ont_align (ont_tcr_consensus/minimap2_align.py
 * :133-137, and the count_cs_tags open of :140): sam_file is what `minimap2 -a` writes (:88-132).  A regular file is
 * mapped; any other readable path (a FIFO, /dev/fd/N) is read to its end, so minimap2 can stream into the call.  The
 * device splits the text into lines, parses every field, encodes the BAM records and sorts them stably by (refID as
 * unsigned, pos + 1, flag & 0x10) -- samtools' coordinate order, ties in input order; the host edits the header (@HD
 * SO:coordinate, GO: dropped, an @HD line added where there is none, no @PG) and parses the aux f values.  The session
 * is then exactly the one umiclust_bam_open builds from the sorted BAM: every umiclust_bam_* call works on it, and
 * umiclust_bam_write with every record kept is the drop-in for `samtools sort -o`.  `samtools index` (:138) and
 * `samtools flagstat` (:152-153) are umiclust_bam_write_index and umiclust_bam_flagstat on the same session (below).
 * The rules (csrc/sam_text.h, policy O9) restate htslib's sam_parse1; every refusal names the 1-based line and the
 * field, and leaves no session: UMICLUST_EFORMAT for a malformed header or line (fewer than 11 fields, an empty line,
 * a name over 254 bytes, an unknown RNAME / RNEXT -- named --, a malformed number or CIGAR, QUAL and SEQ of different
 * lengths, an aux type outside A i f Z H), UMICLUST_ERANGE for more than 65535 CIGAR operations, UMICLUST_EIO for a
 * path that cannot be read, UMICLUST_ENOMEM when the text and the records do not fit the device together.
 * Memory model: umiclust_bam_open's, with the text in place of the compressed file.  hash_bits: as umiclust_bam_open.
 * Returns the number of records. */
int64_t umiclust_sam_open(umiclust_ctx *ctx, const char *sam_file, int32_t hash_bits);
/* DIAGNOSTIC of a session that umiclust_sam_open made (UMICLUST_ESTATE for any other): out[0..3] = lines (header
 * included), records, text bytes uploaded, aux f values parsed on the host; times[0..4] = seconds by HIP events of the
 * upload, lines + measure, sort, encode, copy back.  Either may be NULL.  umiclust_bam_inflate_info reports 0, 0, 0
 * for such a session.  tools/sam_sort_bench.py reads the figures of DESIGN.md §9f through it */
int32_t umiclust_sam_info(umiclust_ctx *ctx, int64_t *out, double *times);
/* umiclust_region_split and umiclust_region_split_extract on the open session instead of a file (replacing the second
 * open of the raw-read BAM by filter_and_split_reads_by_region_cluster, region_split.py:219-333, after
 * minimap2_align.py:140 has read it once): no bam_file argument; the other arguments, the counters, the files, the
 * KeyError with its name, the white-space refusal and the error codes are theirs.  The session's raw bytes are
 * uploaded for the call, as umiclust_bam_split does, and the session stays open.  UMICLUST_ESTATE without one. */
int64_t umiclust_bam_region_split(umiclust_ctx *ctx, int32_t nregions, const char *const *region_names,
                                  const int64_t *region_lengths, const int32_t *region_clusters,
                                  double minimal_region_overlap, int32_t max_softclip_5_end, int32_t max_softclip_3_end,
                                  const char *out_dir, int64_t *counts, int64_t *reads_per_cluster,
                                  int32_t ncluster_cap, uint8_t *region_detected, char *missing_name,
                                  int32_t missing_cap);
int64_t umiclust_bam_region_split_extract(umiclust_ctx *ctx, int32_t nregions, const char *const *region_names,
                                          const int64_t *region_lengths, const int32_t *region_clusters,
                                          double minimal_region_overlap, int32_t max_softclip_5_end,
                                          int32_t max_softclip_3_end, int32_t adapter_length_5_end,
                                          int32_t adapter_length_3_end, int32_t max_pattern_dist, const char *umi_fwd,
                                          const char *umi_rev, const char *umi_out_dir, int64_t *counts,
                                          int64_t *reads_per_cluster, int64_t *umis_per_cluster, int32_t ncluster_cap,
                                          uint8_t *region_detected, char *missing_name, int32_t missing_cap);

/* ---- the .bai index and flagstat of the session, on the device (added functions, ABI version
 * unchanged) ---- */
/* Replaces `samtools index` (minimap2_align.py:138, :247).  umiclust_bam_write(keep, out_bam), then the index of
 * exactly that file at out_bai (NULL: out_bam + ".bai"): both writers record the compressed offset of every block
 * they frame, the device computes per kept record its bin, its windows and the virtual offsets of its start and end,
 * detects the runs of one bin, sorts them and fills the linear index; the host finishes (small bins move to their
 * parent, neighbouring chunks merge) and writes the file.  The rules are policy O10 (csrc/bam_index.h): the SAM
 * specification's §5.1.1 and §5.2 and htslib's finish, restated; bins are written in ascending number with the
 * pseudo-bin 37450 last, and n_no_coor always.  Returns the records written.  The kept records must be
 * coordinate-sorted (a session from umiclust_sam_open is): UMICLUST_EFORMAT "unsorted" names the first record that is
 * not; UMICLUST_ERANGE names a placed record with pos < 0 or an end past 2^29, which a .bai cannot address;
 * UMICLUST_EIO the index path.  On any of them the BAM stays and no file is left at out_bai. */
int64_t umiclust_bam_write_index(umiclust_ctx *ctx, const uint8_t *keep, const char *out_bam, const char *out_bai);
/* `samtools index bam_file`: the file's blocks are walked and inflated on the device as umiclust_bam_open does it, the
 * header and the record offsets parsed (no aux scan, no cs grouping), and the index written to out_bai (NULL: bam_file +
 * ".bai").  An open session is not touched, and none is needed.  Returns the number of records; the error codes are
 * umiclust_bam_open's and umiclust_bam_write_index's. */
int64_t umiclust_bam_index_file(umiclust_ctx *ctx, const char *bam_file, const char *out_bai);
/* Replaces `samtools flagstat` (:152-153) on the open session: the records with keep[r] != 0 (keep NULL: all).
 * out[32] (may be NULL): counter 2 k + w = row k of the text below, w = 0 QC-passed, 1 QC-failed (flag & 0x200).  text:
 * the 16 lines of samtools >= 1.13 (policy O11: total, primary, secondary, supplementary, duplicates, primary
 * duplicates, mapped, primary mapped, paired in sequencing, read1, read2, properly paired, with itself and mate mapped,
 * singletons, with mate mapped to a different chr, the same with mapQ>=5), NUL-terminated.  cap == 0: returns the bytes
 * text needs; otherwise fills it and returns them (UMICLUST_ERANGE when cap is smaller).  The records need no order. */
int32_t umiclust_bam_flagstat(umiclust_ctx *ctx, const uint8_t *keep, int64_t *out, char *text, int64_t cap);
/* DIAGNOSTIC of the context's last index, probe or flagstat call (UMICLUST_ESTATE before any): out[0..3] = kept
 * records, runs, chunks after the finish, linear-index windows; times[0..3] = seconds by HIP events of the upload, the
 * kernels and the copies back, and by the host's clock of the finish with the file.  Either may be NULL.
 * tools/bam_index_bench.py reads the figures of DESIGN.md §9h through it */
int32_t umiclust_bam_index_info(umiclust_ctx *ctx, int64_t *out, double *times);

/* ---- kernel-level entry points (parity tests) ---- */
/* The index kernels on the open session's kept records (keep NULL: all) under a block table the caller gives, with
 * everything they leave behind (csrc/bamindex.hip).  The table lists every block of the imagined file in order: block
 * b starts at compressed offset coff[b] and holds the stream bytes [ustart[b], ustart[b + 1]); the last entry is the
 * block after the data (the EOF block): ustart[nblocks - 1] = header bytes + kept record bytes.  UMICLUST_EINVAL for a
 * table that does not start at 0, decreases, holds more than 64 KiB in a block or ends elsewhere.  Each output may be
 * NULL:
 *   bin, u, v, status   per kept record, in order: its bin (0 without a reference), the virtual offsets of its start
 *                       and end, 0 or 1 = unsorted against the kept record before, 2 = outside 0 .. 2^29, 3 = a
 *                       reference the header does not hold
 *   runs, sorted_runs   4 int64 a run (reference, bin, start, end): in file order, and stably sorted by (reference, bin)
 *   n_intv, mapped, unmapped   per reference of the header
 *   linear              the linear indexes one after another, reference by reference
 *   counters[32]        as umiclust_bam_flagstat's
 *   info[0..5]          kept records, runs, windows, the first refused record (-1: none), its status, n_no_coor
 * A refused record is no error here: info names it, the per-record outputs, the counts and the counters are filled,
 * and runs, sorted_runs and linear are not.  UMICLUST_ERANGE: more runs than run_cap or more windows than linear_cap
 * (info is written). */
int32_t umiclust_bam_index_probe(umiclust_ctx *ctx, const uint8_t *keep, const int64_t *coff, const int64_t *ustart,
                                 int64_t nblocks, int32_t *bin, uint64_t *u, uint64_t *v, int32_t *status,
                                 int64_t *runs, int64_t *sorted_runs, int64_t run_cap, int64_t *n_intv,
                                 uint64_t *linear, int64_t linear_cap, int64_t *mapped, int64_t *unmapped,
                                 int64_t *counters, int64_t *info);
/* The quality kernel alone: record i = quals[offsets[i] .. offsets[i+1]); ee_fx[i] = sum over its bytes b with
 * 0 <= b - fastq_ascii <= 93 of llrint(10^(-(b - fastq_ascii)/10) * 2^40) (other bytes add 0), qlo[i] / qhi[i] = its
 * smallest / largest raw byte (255 / 0 for an empty record).  Records of more than 2^22 bytes: UMICLUST_ERANGE. */
int32_t umiclust_fastq_ee(umiclust_ctx *ctx, const uint8_t *quals, const int64_t *offsets, int64_t n,
                          int32_t fastq_ascii, int64_t *ee_fx, uint8_t *qlo, uint8_t *qhi);
/* The statistics kernel alone (row f5b: what the tables of preprocessing.py:126-127,156-157, read by
 * analysis.py:76-81, are summed from): record i's sequence is seqs[offsets[i] .. offsets[i+1]) and its quality the
 * same range of quals.  ee_fx, qlo, qhi as umiclust_fastq_ee's; counts[5 i ..] = the record's quality bytes with
 * b - fastq_ascii >= 20, those with b - fastq_ascii >= 30, its sequence bytes in "GCgc", in "Nn" and in "-. ".
 * Records of more than 2^22 bytes: UMICLUST_ERANGE. */
int32_t umiclust_fastq_record_stats(umiclust_ctx *ctx, const uint8_t *seqs, const uint8_t *quals,
                                    const int64_t *offsets, int64_t n, int32_t fastq_ascii, int64_t *ee_fx,
                                    uint8_t *qlo, uint8_t *qhi, uint32_t *counts);
/* Align npairs (query, target) pairs with the production alignment kernel.  Sequences are
 * ASCII; q/t record k at [q_off[k], q_off[k+1]).  Outputs per pair: score, matches,
 * internal alignment length (columns minus the terminal gap runs, vsearch align_trim) and,
 * if cigar_ops != NULL, the alignment ops ('M','D','I', alignment order) at
 * cigar_ops[k*ops_stride ...] with their count in ops_len[k]. */
int32_t umiclust_align_pairs(umiclust_ctx *ctx, const umiclust_params *p, const char *q,
                             const int64_t *q_off, const char *t, const int64_t *t_off,
                             int64_t npairs, int32_t *score, int32_t *matches,
                             int32_t *internal_len, char *cigar_ops, int32_t ops_stride,
                             int32_t *ops_len);
/* The member tracebacks and the consensus kernel (k_trace_wave, k_consensus) on clusters the caller names.  Records
 * are ASCII, record i at seqs[offsets[i] .. offsets[i+1]), 1..UMICLUST_MAX_LEN long, taken as they are (no length
 * filter, no sort, no DUST).  Cluster c is the member entries [cstart[c], cstart[c+1]) (cstart[0] = 0): member[x] is
 * a record index, the cluster's first entry its centroid; member_strand[x] = 1 reads the member as its reverse
 * complement (a centroid's is ignored).  A record may be in no cluster, never in two.
 *   ops_in == NULL (traced): every other member is aligned to its centroid exactly as a clustering call does it --
 *     queries of at most 64 nt in one launch, longer ones in a second, each sized by its longest query and by the
 *     call's longest record, members renumbered into traceback slots -- with p's scoring, then k_consensus reads
 *     those slots.  score / matches / internal_len[x] (each may be NULL) are the traceback's results as
 *     umiclust_align_pairs reports them; 0 for centroids.
 *   ops_in != NULL (given): member entry x's ops ('M' both, 'D' a member residue against a gap in the centroid, 'I' a
 *     centroid residue against a gap in the member; alignment order) are ops_in[x * ops_stride ...], ops_in_len[x] of
 *     them (centroid entries are not read).  They are checked on the host -- only M, D, I; at most 2 *
 *     UMICLUST_MAX_LEN; #M + #I = the centroid's length; #M + #D = the member's -- and uploaded into the slots; only
 *     k_consensus runs.  score / matches / internal_len are set to 0.
 * ops_out (may be NULL): the ops k_consensus read, downloaded from the slots, at ops_out[x * ops_stride ...] with
 * their count in ops_out_len[x] (0 for centroids).  ops_stride >= 2 * UMICLUST_MAX_LEN.  cons / cons_cap / cons_off
 * as umiclust_fetch: cons_off[nclusters + 1], cluster c's consensus at cons[cons_off[c] .. cons_off[c+1]).
 * UMICLUST_EINVAL: an empty cluster, a record index out of range, a record listed twice, a short ops_stride,
 * invalid given ops (nothing is launched).  UMICLUST_ERANGE: a record length outside 1..UMICLUST_MAX_LEN, or a
 * cluster whose alignment has more than 2048 columns (the per-member outputs are written, no consensus).  Works
 * beside the context's load: a loaded or clustered context stays as it was.
 * Not covered (each keeps its end-to-end tests): how clustering picks targets and strands, packs, policy O4. */
int32_t umiclust_consensus(umiclust_ctx *ctx, const umiclust_params *p, const char *seqs, const int64_t *offsets,
                           int64_t n, const int32_t *cstart, int32_t nclusters, const int32_t *member,
                           const uint8_t *member_strand, const char *ops_in, const int32_t *ops_in_len,
                           int32_t ops_stride, char *ops_out, int32_t *ops_out_len, int32_t *score,
                           int32_t *matches, int32_t *internal_len, char *cons, int64_t cons_cap,
                           int64_t *cons_off);
/* DUST-mask and extract unique 8-mers of n sequences on the device (K1). masked receives the
 * case-masked sequences (same layout as seqs); kmers[i*kstride ...] the sorted unique k-mer
 * codes of strand s (0 '+', 1 '-') at kmers[(2*i+s)*kstride], counts in nk[2*i+s]. */
int32_t umiclust_prep(umiclust_ctx *ctx, const umiclust_params *p, const char *seqs,
                      const int64_t *offsets, int64_t n, char *masked, uint16_t *kmers,
                      int32_t kstride, int32_t *nk);
/* Everything K1 (k_prep_wave) writes, copied out as the device holds it (an added function, ABI version unchanged).
 * Records are ASCII, record i at seqs[offsets[i] .. offsets[i+1]), 0..UMICLUST_MAX_LEN long, taken as they are (no
 * length filter); p->qmask_dust alone is read of p.  perm (n int32, or NULL: the identity) is a permutation of
 * 0..n-1: output row s is record perm[s], the way umiclust_prepare launches the kernel over its length sort.  Each
 * output may be NULL:
 *   masked[s * UMICLUST_MAX_LEN ...]   the output characters of row s (its length's worth; the rest is not written)
 *   codes[(s * 2 + strand) * 14 ...]   the 4-bit codes, 8 per u32, nibble t of word w = position 8 w + t, 0 past the
 *                                      record; strand 1 is the complemented reverse
 *   lens[s]                            the record's length
 *   kmers[(s * 2 + strand) * kstride ...], nk[s * 2 + strand]   the unique 8-mers in the order the device holds them
 *                                      (ascending), nk of them; kstride >= UMICLUST_MAX_LEN - 7, and kmers needs nk
 *   changed[s]                         1: the output characters of row s differ from its input (what the cluster-file
 *                                      writer reads to fetch single rows)
 *   flags[0], flags[1]                 bit 0: some output symbol is not A, C, G, T or U (selects the aligner family);
 *                                      the number of rows with changed = 1 (selects the writer's branch)
 * The flag words are allocated and zeroed by the call.  UMICLUST_EINVAL: perm is no permutation, decreasing offsets,
 * a short kstride; UMICLUST_ERANGE: a record longer than UMICLUST_MAX_LEN (nothing is launched).  Works beside the
 * context's load: a loaded or clustered context stays as it was. */
int32_t umiclust_prep_outputs(umiclust_ctx *ctx, const umiclust_params *p, const char *seqs,
                              const int64_t *offsets, int64_t n, const int32_t *perm, char *masked,
                              uint32_t *codes, uint8_t *lens, uint16_t *kmers, int32_t kstride, int32_t *nk,
                              uint8_t *changed, uint32_t *flags);
/* The region join of umiclust_overlap_regions with every array its kernels leave behind copied out (an added
 * function, ABI version unchanged).  seqs, offsets, n, region_start, nregions, total and maxcount are that function's,
 * and the kernels run in its order: the table passes with the member lists, then the region pairs.  The table has
 * m slots, m = the smallest power of two that is >= 1024 and >= 2 n, which the caller computes to size its buffers.
 * Each output may be NULL:
 *   hash[n]      the 64-bit hash of each sequence under the accepted seed
 *   region[n]    its region
 *   slot[n]      its slot in the table: equal for byte-equal sequences only
 *   rep_of[n]    the representative of its slot: the lowest index of an equal sequence
 *   cnt[m]       sequences per slot
 *   start[m+1]   the exclusive prefix sum of cnt (all 0 for n = 0, where no kernel runs)
 *   members[n]   the sequence indices bucketed by slot: slot s holds members[start[s] .. start[s+1]), ascending where
 *                it holds 2..32 of them
 *   big[*nbig]   the slots with more than 32 members, which a workgroup each takes over, in any order
 *   info[0..2]   m, the table passes that ran, the seed of the accepted pass
 * hash_bits (1..64): the hashes of the first table pass keep that many low bits, so different sequences collide and
 * the pass is repeated under the next seed with all 64 (64: the production run; 8: what the environment variable
 * UMICLUST_OVERLAP_TEST_COLLIDE sets for every call).  n_cap, m_cap and big_cap are the caller's capacities: of the
 * arrays over sequences, of cnt (start has one more) and of big.  UMICLUST_ERANGE: n_cap < n, m_cap < m, or more
 * than big_cap large buckets (info is written, in the last case *nbig too).  UMICLUST_EINVAL: what umiclust_overlap_regions refuses
 * (region boundaries that do not span [0, n] or decrease, nregions outside 1..UMICLUST_OVERLAP_MAX_REGIONS), hash_bits
 * outside 1..64, a negative capacity. */
int32_t umiclust_overlap_probe(umiclust_ctx *ctx, const char *seqs, const int64_t *offsets, int64_t n,
                               const int64_t *region_start, int32_t nregions, int32_t hash_bits, int64_t n_cap,
                               int64_t m_cap, int64_t big_cap, uint64_t *hash, int32_t *region, int64_t *slot,
                               int64_t *rep_of, uint32_t *cnt, uint32_t *start, uint32_t *members, uint32_t *big,
                               int64_t *nbig, int64_t *total, int32_t *maxcount, uint64_t *info);

/* The k-mer prefilter alone (k_pf_count, k_pf_full, k_pf_merge), launched as a whole pass of the pipeline launches
 * it, on the sequences of the current single-bin load (umiclust_load / umiclust_prepare; sequences given longest
 * first keep their input index as sorted seqno).  cent[ncent]: increasing sorted seqnos, appended to a fresh index
 * append_step at a time (which decides the tiles the kernels read: delta only, base + delta after folds, sealed
 * tiles).  The block is the queries [q0, q0 + nq), its peer window [w0, q0 + nq) with w0 = q0 - nprev * nq (nprev
 * = 0..2 earlier blocks of nq queries); every centroid seqno is < w0.  Per query-strand qs = (q - q0) * both +
 * strand (both = 2 under strand_both, else 1), what k_pf_merge wrote:
 *   top_seqno[qs * 41 ...], top_count[qs * 41 ...], ntop[qs]   the top hits, best first
 *   peer_id[qs * 128 ...] (seqno - w0), peer_count[qs * 128 ...], npeer[qs]   the in-window peers (255 = overflow)
 * and info[0..4]: (query-strand, part) units the lean kernel handed to the full kernel, centroid tiles the pass
 * read, counter segments, 1 if the one-wave layout of k_pf_count was launched, both.  Any output may be NULL.
 * More than 458,752 centroids (one counter segment) take the pipeline's multi-segment branch, up to its limit of 16
 * segments: the lean kernel does not run there -- k_pf_full counts every (query-strand, part) unit segment by segment
 * and merges a running top-41 -- so info[0] = 0 (nothing was handed over) and info[3] = 0, and info[2] > 1 tells.
 * Not covered (each keeps its end-to-end tests): policy O4 rounds; split passes and packs are the two siblings'
 * below.  nq > 8192, centroids in the window, a block spanning more than 32 lengths, policy_threads or several
 * bins: UMICLUST_EINVAL; no load: UMICLUST_ESTATE.  Leaves the context loaded and not clustered. */
int32_t umiclust_prefilter(umiclust_ctx *ctx, const int32_t *cent, int32_t ncent, int32_t q0, int32_t nq,
                           int32_t nprev, int32_t append_step, uint32_t *top_seqno, uint8_t *top_count,
                           uint8_t *ntop, uint16_t *peer_id, uint8_t *peer_count, uint8_t *npeer, int64_t *info);
/* umiclust_prefilter on a pack of a umiclust_load_bins load (an added function, ABI version unchanged): the bins
 * [first_bin, first_bin + nbins) in one greedy order, as umiclust_cluster_pack clusters them -- per-bin scrambled
 * k-mers, the earlier bins' centroids and peers cut out of the counter sweeps, the full kernel keyed by the centroid
 * length table.  cent, the window and the block lie in the pack's sorted seqno range, a block may cross a bin
 * boundary; the pass is a whole pass.  Outputs and info[0..4] as umiclust_prefilter's (seqnos absolute in the load).
 * UMICLUST_EINVAL besides umiclust_prefilter's: a pack outside the load, seqnos outside the pack, more than one
 * counter segment, and a cent that holds a seqno of some bin without that bin's first sequence (a bin's first
 * sequence is always its first centroid; the bin's ordinal range opens with it). */
int32_t umiclust_prefilter_pack(umiclust_ctx *ctx, int32_t first_bin, int32_t nbins, const int32_t *cent,
                                int32_t ncent, int32_t q0, int32_t nq, int32_t nprev, int32_t append_step,
                                uint32_t *top_seqno, uint8_t *top_count, uint8_t *ntop, uint16_t *peer_id,
                                uint8_t *peer_count, uint8_t *npeer, int64_t *info);
/* One split pass in the steady state of the single-bin pipeline (an added function, ABI version unchanged).  The
 * blocks are j-2 = [w0, w0 + nq), j-1 and j = [w0 + 2 nq, w0 + 3 nq); cent (all before w0) is appended append_step at
 * a time on the side stream; then, with no host synchronisation in between: the three peer tiles, the counting half
 * of block j (k_pf_count over the index and the three-block window, block j-2 flagged), the append of newcent[nnew]
 * (increasing seqnos inside block j-2: the centroids its resolution found), and the second half of block j (k_pf_full
 * over the overflowed units, k_pf_merge keeping the flagged hits that became centroids) with the window j-1 .. j.
 * The lists are those of block j against cent and newcent together with the window [w0 + nq, w0 + 3 nq): peer ids
 * are relative to w0 + nq.  info[0..4] as umiclust_prefilter's, info[0] counting the counting half's units (flagged
 * hits included) and info[1] the tiles the second half read; info[5] the tiles the counting half read; info[6] the
 * centroids in the sealed and base tiles after the append (ncent + nnew exactly when that append folded the delta).
 * UMICLUST_EINVAL besides umiclust_prefilter's: newcent outside block j-2 or not increasing, ncent + nnew past one
 * counter segment (the pipeline does not split there). */
int32_t umiclust_prefilter_split(umiclust_ctx *ctx, const int32_t *cent, int32_t ncent, const int32_t *newcent,
                                 int32_t nnew, int32_t w0, int32_t nq, int32_t append_step, uint32_t *top_seqno,
                                 uint8_t *top_count, uint8_t *ntop, uint16_t *peer_id, uint8_t *peer_count,
                                 uint8_t *npeer, int64_t *info);

/* One whole device pass (the prefilter, then k_walk, the per-length alignment rounds, k_peer_rel / k_peer_pairs and
 * k_pack), launched as the pipeline launches it, with everything the host's resolve step reads of it.  cent, ncent,
 * q0, nq, nprev, append_step, the load it needs, what it refuses and its error codes are umiclust_prefilter's.
 * flags bit 0: lazy peers (no peer is aligned speculatively; the masks are zero, the records still written).
 * flags bit 1 (needs nprev >= 1, else UMICLUST_EINVAL): the pass of the block before, [q0 - nq, q0), is enqueued
 *   first on the other buffer set, with the window's earlier blocks as its peers and no resolve in between, as the
 *   pipeline queues consecutive passes; the pass under test then reads that pass's final walk states to tell which
 *   of its peers there are expected to become members.  Without bit 1 every other buffer set is marked unused
 *   first, so that no pass an earlier umiclust_cluster left on the context is taken for the block before: the
 *   outputs depend on the arguments alone.
 * Outputs, each optional (NULL), per query-strand qs = (q - q0) * both + strand:
 *   top_seqno .. npeer   the prefilter's lists, as umiclust_prefilter returns them
 *   hostqs[nqs]          k_pack's outcomes (umiclust_pass_qs)
 *   rec[rec_cap]         k_pack's record words; *rec_total = the words the pass used.  More than rec_cap:
 *                        the first rec_cap words and every other output are filled, then UMICLUST_ERANGE
 *   res[nqs * 160]       the raw result words (matches | internal_len << 8 | (score & 0xffff) << 16): walk candidate
 *                        x of qs at [qs * 32 + x] (valid for x < e), peer y at [nqs * 32 + qs * 128 + y] (valid where
 *                        its aligned bit is set)
 *   aligned[nqs * 2]     bit y % 64 of word qs * 2 + y / 64: peer y was aligned in this pass
 *   walk[nqs]            the final walk states (umiclust_pass_walk)
 *   counters[16]         the pass counters as the host receives them: [8] peer pairs, [12..13] / [14..15] (64 bits
 *                        each, low word first) the cells of the emitted walk pairs / of the peer pairs
 *   info[0..4]           as umiclust_prefilter's
 * Not covered (each keeps its end-to-end tests): split passes, packs, policy O4 rounds, more than one counter
 * segment, and -- on a lone context -- blocks of more than 4096 queries, whose outcomes and records go through device
 * buffers and copies instead of straight into host memory (the entry point returns them all the same).  Leaves the
 * context loaded and not clustered.  (An added function: the struct layouts above and the ABI version are
 * unchanged.) */
typedef struct umiclust_pass_qs {
  uint32_t best_t;     /* best accepted target seqno (0xffffffff: none) */
  uint32_t cells;      /* sum of qlen * tlen over the walked candidates */
  uint32_t rec;        /* word offset of the record, 0xffffffff if none */
  uint16_t best_rank;  /* identity rank of the best accepted hit */
  uint8_t w;           /* candidates walked */
  uint8_t flags;       /* bit 0: an accepted hit; bit 1: peer list overflow */
  uint16_t nrel;       /* relevant peers */
  uint8_t e;           /* walk candidates with a result */
  uint8_t npeer;       /* peers in the window (255: overflow) */
  uint16_t rel[6];     /* window ids of the first 6 relevant peers, peer order */
} umiclust_pass_qs;
typedef struct umiclust_pass_walk {
  uint64_t lastkey;    /* (127 - count) << 56 | length << 48 | seqno of the last walked candidate; 0 before any */
  uint32_t best_t;
  uint32_t cells;
  uint16_t best_rank;
  uint8_t w, done, acc, e;
  uint8_t pad[2];
} umiclust_pass_walk;
#define UMICLUST_PASS_LAZY 1u
#define UMICLUST_PASS_PREV 2u
int32_t umiclust_pass(umiclust_ctx *ctx, const int32_t *cent, int32_t ncent, int32_t q0, int32_t nq, int32_t nprev,
                      int32_t append_step, uint32_t flags, uint32_t *top_seqno, uint8_t *top_count, uint8_t *ntop,
                      uint16_t *peer_id, uint8_t *peer_count, uint8_t *npeer, umiclust_pass_qs *hostqs, uint32_t *rec,
                      int64_t rec_cap, int64_t *rec_total, uint32_t *res, uint64_t *aligned, umiclust_pass_walk *walk,
                      uint32_t *counters, int64_t *info);

/* The same pass, queued and then resolved on the host by the pipeline's own resolve step, round B on the device
 * included: which queries of the block become centroids and which centroid each member joins.  The block arguments,
 * flags bits 0 and 1, the load it needs, what it refuses and its error codes are umiclust_pass's.
 * win_state[q0 - w0]: the states of the window's queries before the block, 1 = centroid, 2 = member (anything else:
 *   UMICLUST_EINVAL); cent and the window's centroids together are the centroids the block is clustered against.
 * flags bit 2 (UMICLUST_RESOLVE_PARTIAL): when a peer list of the block overflowed, the queries before the first
 *   overflowing one are resolved, as the pipeline does before it re-runs the rest; without it such a block resolves
 *   nothing.
 * Outputs, each optional (NULL):
 *   state[nq], target[nq], strand[nq]   per query 0 = not resolved, 1 = centroid, 2 = member; the centroid seqno a
 *                        member joins (-1 otherwise) and the strand of that hit
 *   new_cents[nq]        the block's new centroids, increasing; info[2] of them
 *   info[0..12]          queries resolved; 1 if that is the whole block; new centroids; the resolve step's alignments,
 *                        cells, merged walks, deferred queries and round-B pairs; round B's trips to the device, its
 *                        launches and its pairs as the device side counted them; strands per query; the trips that
 *                        went through device buffers (more than 4096 pairs)
 * Leaves the context loaded and not clustered.  (An added function: the struct layouts and the ABI version are
 * unchanged.) */
#define UMICLUST_RESOLVE_PARTIAL 4u
int32_t umiclust_resolve(umiclust_ctx *ctx, const int32_t *cent, int32_t ncent, int32_t q0, int32_t nq, int32_t nprev,
                         int32_t append_step, uint32_t flags, const uint8_t *win_state, uint8_t *state,
                         int32_t *target, uint8_t *strand, int32_t *new_cents, int64_t *info);

/* The BGZF inflate kernel alone (an added function, ABI version unchanged).
 * file = a whole BGZF byte string in host memory.  cap == 0: returns the inflated size (sum of ISIZE) without a
 * launch.  Otherwise inflates on the device into out and returns the size.  block_status (may be NULL): one int32 per
 * block, 0 = ok, > 0 = the decoder's error class (csrc/inflate.h).  If any block fails: UMICLUST_EFORMAT, the message
 * names the first bad block and its class, out holds the bytes of every good block at its offset.  A malformed
 * gzip/BC framing is UMICLUST_EFORMAT before any launch.  n_blocks (may be NULL): the number of blocks, set by every
 * call that passes the framing.  times (may be NULL): seconds of upload, kernel, download by HIP events.  CRC32 is
 * not checked. */
int64_t umiclust_bgzf_inflate(umiclust_ctx *ctx, const uint8_t *file, int64_t n, uint8_t *out, int64_t cap,
                              int32_t *block_status, int64_t *n_blocks, double *times);

/* The BGZF deflate kernels alone (an added function, ABI version unchanged).
 * data = n bytes in host memory, cut into blocks of 0xff00 bytes (the last one shorter).  cap == 0: returns an upper
 * bound on the output size without a launch.  Otherwise (cap at least that bound) deflates and frames every block on
 * the device and returns the size of the BGZF written to out, the 28-byte EOF block included; empty input gives the
 * EOF block alone.  Each block is one gzip member that inflates to its input bytes, and is byte for byte what
 * uc::deflate_block (csrc/deflate.h, the host restatement) produces; the CRC32s are computed on the host.
 * block_kind (may be NULL): per block 0 = stored, 1 = fixed, 2 = dynamic.  n_blocks (may be NULL): ceil(n / 0xff00),
 * set by every call.  times (may be NULL): seconds of upload, kernels, download by HIP events. */
int64_t umiclust_bgzf_deflate(umiclust_ctx *ctx, const uint8_t *data, int64_t n, uint8_t *out, int64_t cap,
                              int32_t *block_kind, int64_t *n_blocks, double *times);

/* ---- measurement (bench.py; no reference counterpart) ---- */
/* Process-wide device timeline of the counting launches (kind 0) and the alignment chains
 * (kind 1) of every context: busy_s = the union of their HIP-event brackets since the last
 * reset, launches = the number of brackets.  reset != 0 clears it and records a new
 * reference event on device_id first.  Several contexts (lanes) on one device overlap their
 * brackets, so the union is the time the kernel held the device, and the sum is not. */
int32_t umiclust_timeline(int32_t device_id, int32_t kind, int32_t reset, double *busy_s,
                          int64_t *launches);

#ifdef __cplusplus
}
#endif
#endif
