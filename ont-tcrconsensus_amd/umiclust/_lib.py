"""ctypes binding of the C ABI declared in include/umiclust.h (libumiclust.so, built in-tree).

There is no CPU fallback: if the library or a HIP device is missing every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libumiclust.so")

QL, TL, QI, TI, QR, TR = range(6)
PRESET_ROUND1 = 1
PRESET_VSEARCH_DEFAULT = 2
MAX_LEN = 112

ERRORS = {-22: "EINVAL", -5: "EIO", -12: "ENOMEM", -19: "EDEVICE", -77: "ESTATE", -34: "ERANGE", -17: "EEXIST",
          -74: "EFORMAT"}


class UmiclustError(RuntimeError):
    def __init__(self, code: int, msg: str = ""):
        super().__init__(f"umiclust error {code} ({ERRORS.get(code, '?')}): {msg}")
        self.code = code


class Params(C.Structure):
    _fields_ = [
        ("id", C.c_double),
        ("weak_id", C.c_double),
        ("minseqlength", C.c_int32),
        ("maxseqlength", C.c_int32),
        ("wordlength", C.c_int32),
        ("minwordmatches", C.c_int32),
        ("maxaccepts", C.c_int32),
        ("maxrejects", C.c_int32),
        ("match", C.c_int32),
        ("mismatch", C.c_int32),
        ("gap_open", C.c_int32 * 6),
        ("gap_ext", C.c_int32 * 6),
        ("strand_both", C.c_int32),
        ("qmask_dust", C.c_int32),
        ("clusterout_sort", C.c_int32),
        ("clusterout_id", C.c_int32),
        ("fasta_width", C.c_int32),
        ("policy_boundary_open", C.c_int32),
        ("threads", C.c_int32),
        ("policy_threads", C.c_int32),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("n_input", C.c_int64),
        ("n_kept", C.c_int64),
        ("n_clusters", C.c_int64),
        ("n_alignments", C.c_int64),
        ("cells", C.c_int64),
        ("cells_computed", C.c_int64),
        ("kmer_postings", C.c_int64),
        ("n_blocks", C.c_int64),
        ("t_total_s", C.c_double),
        ("t_prefilter_s", C.c_double),
        ("t_align_s", C.c_double),
        ("t_consensus_s", C.c_double),
        ("t_host_s", C.c_double),
        ("n_deferred", C.c_int64),
        ("pairs_round_b", C.c_int64),
        ("pairs_peer", C.c_int64),
        ("t_index_s", C.c_double),
        ("t_sync_s", C.c_double),
        ("t_host_pass1_s", C.c_double),
        ("n_merged_walks", C.c_int64),
        ("t_merged_s", C.c_double),
        ("t_read_s", C.c_double),
        ("t_write_s", C.c_double),
        ("t_run_s", C.c_double),
        ("n_reruns", C.c_int64),
        ("n_overlap_passes", C.c_int64),
        ("n_lazy_passes", C.c_int64),
        ("t_count_s", C.c_double),
        ("n_count_launches", C.c_int64),
        ("kmer_postings_deferred", C.c_int64),
        ("counter_cells", C.c_int64),
        ("n_regrows", C.c_int64),
    ]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class ParseParams(C.Structure):
    _fields_ = [("min_reads_per_cluster", C.c_int32), ("max_reads_per_cluster", C.c_int32),
                ("balance_strands", C.c_int32), ("max_clusters", C.c_int32)]


class ParseResult(C.Structure):
    _fields_ = [("n_clusters", C.c_int64), ("n_written", C.c_int64), ("reads_found", C.c_int64),
                ("reads_written", C.c_int64), ("empty_region", C.c_int32), ("pad", C.c_int32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class FastqFilterParams(C.Structure):
    """umiclust_fastq_filter_params (vsearch --fastq_filter options; negative maxlen / maxee / maxee_rate: not given)"""
    _fields_ = [("fastq_ascii", C.c_int32), ("fastq_qmin", C.c_int32), ("fastq_qmax", C.c_int32),
                ("fastq_minlen", C.c_int32), ("fastq_maxlen", C.c_int32), ("pad", C.c_int32),
                ("fastq_maxee", C.c_double), ("fastq_maxee_rate", C.c_double)]


class FastqFilterResult(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("n_input", "n_kept", "n_discarded", "bases_in", "bases_kept", "n_short",
                                         "n_long", "n_maxee", "n_maxee_rate", "n_host_rechecked", "n_chunks")] + \
               [(k, C.c_double) for k in ("ee_in", "ee_kept", "t_read_s", "t_h2d_s", "t_kernel_s", "t_write_s",
                                          "t_total_s")]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class FastqStats(C.Structure):
    """umiclust_fastq_stats: the numbers of one `seqkit stat -a` table (policy O8)"""
    _fields_ = [(k, C.c_int64) for k in ("num_seqs", "sum_len", "min_len", "max_len", "n50", "n50_num", "n_q20",
                                         "n_q30", "n_gc", "sum_n", "sum_gap")] + \
               [("ee_fx_lo", C.c_uint64), ("ee_fx_hi", C.c_uint64), ("type", C.c_int32), ("pad", C.c_int32)] + \
               [(k, C.c_double) for k in ("avg_len", "q1", "q2", "q3", "q20_pct", "q30_pct", "avg_qual", "gc_pct")]

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("pad", "ee_fx_lo", "ee_fx_hi", "type")}
        d["ee_fx"] = (self.ee_fx_hi << 64) | self.ee_fx_lo
        d["type"] = ("DNA", "RNA", "Protein")[self.type]
        return d


# every symbol include/umiclust.h declares
EXPORTS = [
    "umiclust_abi_version", "umiclust_params_init", "umiclust_params_from_argv", "umiclust_create",
    "umiclust_destroy", "umiclust_last_error", "umiclust_run_fasta", "umiclust_run_argv", "umiclust_run_fasta_parse",
    "umiclust_load", "umiclust_stage", "umiclust_prepare", "umiclust_set_priority", "umiclust_cluster", "umiclust_fetch", "umiclust_load_bins", "umiclust_cluster_bin", "umiclust_cluster_pack",
    "umiclust_fetch_bin", "umiclust_overlap_counts", "umiclust_overlap_regions", "umiclust_extract_umis",
    "umiclust_extract_umis_file", "umiclust_region_split", "umiclust_align_pairs", "umiclust_prep",
    "umiclust_prep_outputs", "umiclust_overlap_probe",
    "umiclust_timeline", "umiclust_wait_host", "umiclust_fastq_filter_params_from_argv", "umiclust_fastq_filter",
    "umiclust_fastq_filter_argv", "umiclust_fastq_filter_stats", "umiclust_fastq_filter_stats_argv",
    "umiclust_fastq_ee", "umiclust_fastq_record_stats", "umiclust_prefilter", "umiclust_consensus", "umiclust_pass",
    "umiclust_prefilter_pack", "umiclust_prefilter_split", "umiclust_resolve",
    "umiclust_bam_open", "umiclust_bam_counts", "umiclust_bam_times", "umiclust_bam_columns", "umiclust_bam_refs",
    "umiclust_bam_strings", "umiclust_bam_cs_groups", "umiclust_bam_write", "umiclust_bam_split",
    "umiclust_bam_name_suffix", "umiclust_bam_close", "umiclust_region_split_extract", "umiclust_bam_split_extract",
    "umiclust_bgzf_inflate", "umiclust_bam_inflate_info", "umiclust_sam_open", "umiclust_sam_info",
    "umiclust_bam_region_split", "umiclust_bam_region_split_extract", "umiclust_bgzf_deflate",
    "umiclust_bam_write_info", "umiclust_bam_write_index", "umiclust_bam_index_file", "umiclust_bam_flagstat",
    "umiclust_bam_index_probe", "umiclust_bam_index_info",
]
OVERLAP_MAX_REGIONS = 4096
# umiclust_pass_qs / umiclust_pass_walk (include/umiclust.h) and the largest record k_pack writes, in words
PASS_QS = np.dtype([("best_t", "<u4"), ("cells", "<u4"), ("rec", "<u4"), ("best_rank", "<u2"), ("w", "u1"),
                    ("flags", "u1"), ("nrel", "<u2"), ("e", "u1"), ("npeer", "u1"), ("rel", "<u2", (6,))])
PASS_WALK = np.dtype([("lastkey", "<u8"), ("best_t", "<u4"), ("cells", "<u4"), ("best_rank", "<u2"), ("w", "u1"),
                      ("done", "u1"), ("acc", "u1"), ("e", "u1"), ("pad", "u1", (2,))])
PASS_REC_WORDS = 1 + 2 * 32 + 8 + 2 * 128
ABI_VERSION = 9  # include/umiclust.h UMICLUST_ABI_VERSION: the struct layouts below

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise UmiclustError(-19, f"{LIB_PATH} not built (run `make -C ont-tcrconsensus_amd` or "
                                 "__graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    P = C.POINTER
    L.umiclust_abi_version.restype = C.c_int32
    if L.umiclust_abi_version() != ABI_VERSION:  # a stale build would read the structs with the wrong layout
        raise UmiclustError(-22, f"{LIB_PATH} has ABI {L.umiclust_abi_version()}, this binding expects "
                                 f"{ABI_VERSION}: rebuild (make -C ont-tcrconsensus_amd)")
    L.umiclust_params_init.restype = C.c_int32
    L.umiclust_params_init.argtypes = [P(Params), C.c_int32, C.c_double, C.c_int32, C.c_int32]
    L.umiclust_params_from_argv.restype = C.c_int32
    L.umiclust_params_from_argv.argtypes = [P(Params), C.c_int32, P(C.c_char_p), C.c_char_p, C.c_char_p,
                                            C.c_char_p, C.c_char_p, C.c_int32]
    L.umiclust_create.restype = C.c_void_p
    L.umiclust_create.argtypes = [C.c_int32, P(C.c_int32)]
    L.umiclust_destroy.restype = None
    L.umiclust_destroy.argtypes = [C.c_void_p]
    L.umiclust_wait_host.restype = C.c_int32
    L.umiclust_wait_host.argtypes = [C.c_void_p]
    L.umiclust_last_error.restype = C.c_char_p
    L.umiclust_last_error.argtypes = [C.c_void_p]
    L.umiclust_run_fasta.restype = C.c_int64
    L.umiclust_run_fasta.argtypes = [C.c_void_p, P(Params), C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                     P(Stats)]
    L.umiclust_run_fasta_parse.restype = C.c_int64
    L.umiclust_run_fasta_parse.argtypes = [C.c_void_p, P(Params), C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                           P(ParseParams), C.c_char_p, P(ParseResult), P(Stats)]
    L.umiclust_run_argv.restype = C.c_int64
    L.umiclust_run_argv.argtypes = [C.c_void_p, C.c_int32, P(C.c_char_p), P(Stats)]
    L.umiclust_load.restype = C.c_int32
    L.umiclust_load.argtypes = [C.c_void_p, P(Params), C.c_void_p, P(C.c_int64), C.c_int64]
    L.umiclust_stage.restype = C.c_int32
    L.umiclust_stage.argtypes = [C.c_void_p, C.c_void_p, P(C.c_int64), C.c_int64, P(C.c_int64), C.c_int32]
    L.umiclust_prepare.restype = C.c_int32
    L.umiclust_prepare.argtypes = [C.c_void_p, P(Params)]
    L.umiclust_set_priority.restype = C.c_int32
    L.umiclust_set_priority.argtypes = [C.c_void_p, C.c_int32]
    L.umiclust_cluster.restype = C.c_int64
    L.umiclust_cluster.argtypes = [C.c_void_p, P(Stats)]
    L.umiclust_fetch.restype = C.c_int64
    L.umiclust_fetch.argtypes = [C.c_void_p, P(C.c_int32), P(C.c_uint8), P(C.c_uint8), C.c_void_p, C.c_int64,
                                 P(C.c_int64)]
    L.umiclust_load_bins.restype = C.c_int32
    L.umiclust_load_bins.argtypes = [C.c_void_p, P(Params), C.c_void_p, P(C.c_int64), C.c_int64, P(C.c_int64),
                                     C.c_int32]
    L.umiclust_cluster_bin.restype = C.c_int64
    L.umiclust_cluster_bin.argtypes = [C.c_void_p, C.c_int32, P(Stats)]
    L.umiclust_cluster_pack.restype = C.c_int64
    L.umiclust_cluster_pack.argtypes = [C.c_void_p, C.c_int32, C.c_int32, P(Stats)]
    L.umiclust_fetch_bin.restype = C.c_int64
    L.umiclust_fetch_bin.argtypes = [C.c_void_p, C.c_int32, P(C.c_int32), P(C.c_uint8), P(C.c_uint8), C.c_void_p,
                                     C.c_int64, P(C.c_int64)]
    L.umiclust_overlap_counts.restype = C.c_int32
    L.umiclust_overlap_counts.argtypes = [C.c_void_p, C.c_void_p, P(C.c_int64), C.c_int64, C.c_void_p, P(C.c_int64),
                                          C.c_int64, P(C.c_int64)]
    L.umiclust_overlap_regions.restype = C.c_int32
    L.umiclust_overlap_regions.argtypes = [C.c_void_p, C.c_void_p, P(C.c_int64), C.c_int64, P(C.c_int64), C.c_int32,
                                           P(C.c_int64), P(C.c_int32)]
    L.umiclust_extract_umis.restype = C.c_int32
    L.umiclust_extract_umis.argtypes = [C.c_void_p, C.c_void_p, P(C.c_int64), C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_char_p, C.c_char_p, P(C.c_int32)]
    L.umiclust_extract_umis_file.restype = C.c_int64
    L.umiclust_extract_umis_file.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_char_p, C.c_char_p]
    L.umiclust_region_split.restype = C.c_int64
    L.umiclust_region_split.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, P(C.c_char_p), P(C.c_int64), P(C.c_int32),
                                        C.c_double, C.c_int32, C.c_int32, C.c_char_p, P(C.c_int64), P(C.c_int64),
                                        C.c_int32, P(C.c_uint8), C.c_char_p, C.c_int32]
    L.umiclust_region_split_extract.restype = C.c_int64
    L.umiclust_region_split_extract.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, P(C.c_char_p), P(C.c_int64),
                                                P(C.c_int32), C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                C.c_int32, C.c_char_p, C.c_char_p, C.c_char_p, P(C.c_int64),
                                                P(C.c_int64), P(C.c_int64), C.c_int32, P(C.c_uint8), C.c_char_p,
                                                C.c_int32]
    L.umiclust_align_pairs.restype = C.c_int32
    L.umiclust_align_pairs.argtypes = [C.c_void_p, P(Params), C.c_void_p, P(C.c_int64), C.c_void_p, P(C.c_int64),
                                       C.c_int64, P(C.c_int32), P(C.c_int32), P(C.c_int32), C.c_void_p, C.c_int32,
                                       P(C.c_int32)]
    L.umiclust_consensus.restype = C.c_int32
    L.umiclust_consensus.argtypes = [C.c_void_p, P(Params), C.c_void_p, P(C.c_int64), C.c_int64, P(C.c_int32), C.c_int32,
                                     P(C.c_int32), P(C.c_uint8), C.c_void_p, P(C.c_int32), C.c_int32, C.c_void_p,
                                     P(C.c_int32), P(C.c_int32), P(C.c_int32), P(C.c_int32), C.c_void_p, C.c_int64,
                                     P(C.c_int64)]
    L.umiclust_prep_outputs.restype = C.c_int32
    L.umiclust_prep_outputs.argtypes = [C.c_void_p, P(Params), C.c_void_p, P(C.c_int64), C.c_int64] + \
        [C.c_void_p] * 5 + [C.c_int32] + [C.c_void_p] * 3
    L.umiclust_overlap_probe.restype = C.c_int32
    L.umiclust_overlap_probe.argtypes = [C.c_void_p, C.c_void_p, P(C.c_int64), C.c_int64, P(C.c_int64), C.c_int32,
                                         C.c_int32, C.c_int64, C.c_int64, C.c_int64] + [C.c_void_p] * 12
    L.umiclust_prep.restype = C.c_int32
    L.umiclust_prep.argtypes = [C.c_void_p, P(Params), C.c_void_p, P(C.c_int64), C.c_int64, C.c_void_p,
                                P(C.c_uint16), C.c_int32, P(C.c_int32)]
    L.umiclust_timeline.restype = C.c_int32
    L.umiclust_timeline.argtypes = [C.c_int32, C.c_int32, C.c_int32, P(C.c_double), P(C.c_int64)]
    L.umiclust_fastq_filter_params_from_argv.restype = C.c_int32
    L.umiclust_fastq_filter_params_from_argv.argtypes = [P(FastqFilterParams), C.c_int32, P(C.c_char_p), C.c_char_p,
                                                         C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32]
    L.umiclust_fastq_filter.restype = C.c_int64
    L.umiclust_fastq_filter.argtypes = [C.c_void_p, P(FastqFilterParams), C.c_char_p, C.c_char_p, C.c_char_p,
                                        C.c_char_p, P(FastqFilterResult)]
    L.umiclust_fastq_filter_argv.restype = C.c_int64
    L.umiclust_fastq_filter_argv.argtypes = [C.c_void_p, C.c_int32, P(C.c_char_p), P(FastqFilterResult)]
    L.umiclust_fastq_ee.restype = C.c_int32
    L.umiclust_fastq_ee.argtypes = [C.c_void_p, C.c_void_p, P(C.c_int64), C.c_int64, C.c_int32, P(C.c_int64),
                                    P(C.c_uint8), P(C.c_uint8)]
    L.umiclust_fastq_filter_stats.restype = C.c_int64
    L.umiclust_fastq_filter_stats.argtypes = [C.c_void_p, P(FastqFilterParams), C.c_char_p, C.c_char_p, C.c_char_p,
                                              C.c_char_p, C.c_char_p, C.c_char_p, P(FastqFilterResult), P(FastqStats),
                                              P(FastqStats)]
    L.umiclust_fastq_filter_stats_argv.restype = C.c_int64
    L.umiclust_fastq_filter_stats_argv.argtypes = [C.c_void_p, C.c_int32, P(C.c_char_p), C.c_char_p, C.c_char_p,
                                                   P(FastqFilterResult), P(FastqStats), P(FastqStats)]
    L.umiclust_fastq_record_stats.restype = C.c_int32
    L.umiclust_fastq_record_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_int64), C.c_int64, C.c_int32,
                                              P(C.c_int64), P(C.c_uint8), P(C.c_uint8), P(C.c_uint32)]
    L.umiclust_prefilter.restype = C.c_int32
    L.umiclust_prefilter.argtypes = [C.c_void_p, P(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     P(C.c_uint32), P(C.c_uint8), P(C.c_uint8), P(C.c_uint16), P(C.c_uint8),
                                     P(C.c_uint8), P(C.c_int64)]
    lists = [P(C.c_uint32), P(C.c_uint8), P(C.c_uint8), P(C.c_uint16), P(C.c_uint8), P(C.c_uint8), P(C.c_int64)]
    L.umiclust_prefilter_pack.restype = C.c_int32
    L.umiclust_prefilter_pack.argtypes = [C.c_void_p, C.c_int32, C.c_int32, P(C.c_int32)] + [C.c_int32] * 5 + lists
    L.umiclust_prefilter_split.restype = C.c_int32
    L.umiclust_prefilter_split.argtypes = [C.c_void_p, P(C.c_int32), C.c_int32, P(C.c_int32)] + [C.c_int32] * 4 + lists
    L.umiclust_resolve.restype = C.c_int32
    L.umiclust_resolve.argtypes = [C.c_void_p, P(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                   C.c_uint32, P(C.c_uint8), P(C.c_uint8), P(C.c_int32), P(C.c_uint8), P(C.c_int32),
                                   P(C.c_int64)]
    L.umiclust_pass.restype = C.c_int32
    L.umiclust_pass.argtypes = [C.c_void_p, P(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                C.c_uint32, P(C.c_uint32), P(C.c_uint8), P(C.c_uint8), P(C.c_uint16), P(C.c_uint8),
                                P(C.c_uint8), C.c_void_p, P(C.c_uint32), C.c_int64, P(C.c_int64), P(C.c_uint32),
                                P(C.c_uint64), C.c_void_p, P(C.c_uint32), P(C.c_int64)]
    L.umiclust_bam_open.restype = C.c_int64
    L.umiclust_bam_open.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
    L.umiclust_bam_counts.restype = C.c_int32
    L.umiclust_bam_counts.argtypes = [C.c_void_p, P(C.c_int64)]
    L.umiclust_bam_times.restype = C.c_int32
    L.umiclust_bam_times.argtypes = [C.c_void_p, P(C.c_double)]
    L.umiclust_bam_inflate_info.restype = C.c_int32
    L.umiclust_bam_inflate_info.argtypes = [C.c_void_p, P(C.c_int64)]
    L.umiclust_bam_columns.restype = C.c_int32
    L.umiclust_bam_columns.argtypes = [C.c_void_p, P(C.c_int8), P(C.c_int32), P(C.c_int32), P(C.c_int64), P(C.c_int64),
                                       P(C.c_int64), P(C.c_uint8), P(C.c_int32)]
    L.umiclust_bam_refs.restype = C.c_int32
    L.umiclust_bam_refs.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, P(C.c_int64), P(C.c_int64)]
    L.umiclust_bam_strings.restype = C.c_int64
    L.umiclust_bam_strings.argtypes = [C.c_void_p, C.c_int32, P(C.c_int64), C.c_int64, C.c_void_p, C.c_int64,
                                       P(C.c_int64)]
    L.umiclust_bam_cs_groups.restype = C.c_int32
    L.umiclust_bam_cs_groups.argtypes = [C.c_void_p, P(C.c_int64), P(C.c_int64)]
    L.umiclust_bam_write.restype = C.c_int64
    L.umiclust_bam_write.argtypes = [C.c_void_p, P(C.c_uint8), C.c_char_p]
    L.umiclust_bam_split.restype = C.c_int64
    L.umiclust_bam_split.argtypes = [C.c_void_p, P(C.c_uint8), C.c_int32, P(C.c_char_p), P(C.c_int64), P(C.c_int32),
                                     C.c_int32, P(C.c_char_p), C.c_double, C.c_int32, C.c_int32, P(C.c_int64),
                                     P(C.c_int64), P(C.c_uint8), C.c_char_p, C.c_int32]
    L.umiclust_bam_split_extract.restype = C.c_int64
    L.umiclust_bam_split_extract.argtypes = [C.c_void_p, P(C.c_uint8), C.c_int32, P(C.c_char_p), P(C.c_int64),
                                             P(C.c_int32), C.c_int32, P(C.c_char_p), C.c_double, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_char_p, P(C.c_int64),
                                             P(C.c_int64), P(C.c_int64), P(C.c_uint8), C.c_char_p, C.c_int32]
    L.umiclust_bam_name_suffix.restype = C.c_int32
    L.umiclust_bam_name_suffix.argtypes = [C.c_void_p, P(C.c_int64), P(C.c_uint8)]
    L.umiclust_bgzf_inflate.restype = C.c_int64
    L.umiclust_bgzf_inflate.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, P(C.c_int32),
                                        P(C.c_int64), P(C.c_double)]
    L.umiclust_bgzf_deflate.restype = C.c_int64
    L.umiclust_bgzf_deflate.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, P(C.c_int32),
                                        P(C.c_int64), P(C.c_double)]
    L.umiclust_bam_write_info.restype = C.c_int32
    L.umiclust_bam_write_info.argtypes = [C.c_void_p, P(C.c_int64), P(C.c_double)]
    L.umiclust_bam_close.restype = C.c_int32
    L.umiclust_bam_close.argtypes = [C.c_void_p]
    L.umiclust_sam_open.restype = C.c_int64
    L.umiclust_sam_open.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
    L.umiclust_sam_info.restype = C.c_int32
    L.umiclust_sam_info.argtypes = [C.c_void_p, P(C.c_int64), P(C.c_double)]
    L.umiclust_bam_write_index.restype = C.c_int64
    L.umiclust_bam_write_index.argtypes = [C.c_void_p, P(C.c_uint8), C.c_char_p, C.c_char_p]
    L.umiclust_bam_index_file.restype = C.c_int64
    L.umiclust_bam_index_file.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    L.umiclust_bam_flagstat.restype = C.c_int32
    L.umiclust_bam_flagstat.argtypes = [C.c_void_p, P(C.c_uint8), P(C.c_int64), C.c_void_p, C.c_int64]
    L.umiclust_bam_index_probe.restype = C.c_int32
    L.umiclust_bam_index_probe.argtypes = [C.c_void_p, P(C.c_uint8), P(C.c_int64), P(C.c_int64), C.c_int64] + \
        [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4
    L.umiclust_bam_index_info.restype = C.c_int32
    L.umiclust_bam_index_info.argtypes = [C.c_void_p, P(C.c_int64), P(C.c_double)]
    # the path-based calls without their bam_file argument
    L.umiclust_bam_region_split.restype = C.c_int64
    L.umiclust_bam_region_split.argtypes = [a for k, a in enumerate(L.umiclust_region_split.argtypes) if k != 1]
    L.umiclust_bam_region_split_extract.restype = C.c_int64
    L.umiclust_bam_region_split_extract.argtypes = [a for k, a in enumerate(L.umiclust_region_split_extract.argtypes)
                                                    if k != 1]
    _lib = L
    return L


def timeline(kind: int, reset: bool = False, device: int = 0) -> tuple[float, int]:
    """umiclust_timeline: (union of the kind's HIP-event brackets in seconds, brackets) since the last reset;
    kind 0 = counting launches, 1 = alignment chains."""
    s, n = C.c_double(0.0), C.c_int64(0)
    rc = lib().umiclust_timeline(device, kind, 1 if reset else 0, C.byref(s), C.byref(n))
    if rc != 0:
        raise UmiclustError(rc, "timeline")
    return s.value, n.value


def params(preset: int = PRESET_ROUND1, identity: float = 0.93, minlen: int = 58, maxlen: int = 68,
           threads: int = 1) -> Params:
    """A preset's parameters; threads > 1 selects vsearch's --threads mode (policy O4, rounds of `threads` queries:
    umiclust_params.policy_threads = 1), threads = 1 the sequential definition."""
    p = Params()
    rc = lib().umiclust_params_init(C.byref(p), preset, identity, minlen, maxlen)
    if rc != 0:
        raise UmiclustError(rc, "params_init")
    if threads > 1:
        p.threads, p.policy_threads = int(threads), 1
    return p


def params_from_argv(argv: list[str]) -> tuple[Params, dict]:
    p = Params()
    bufs = [C.create_string_buffer(4096) for _ in range(4)]
    arr = (C.c_char_p * len(argv))(*[str(a).encode() for a in argv])
    rc = lib().umiclust_params_from_argv(C.byref(p), len(argv), arr, *bufs, 4096)
    if rc != 0:
        raise UmiclustError(rc, f"cannot parse argv {argv!r}")
    keys = ["in_fasta", "clusters_prefix", "consout", "log"]
    return p, {k: (b.value.decode() or None) for k, b in zip(keys, bufs)}


def fastq_filter_params(fastq_ascii: int = 33, fastq_qmin: int = 0, fastq_qmax: int = 41, fastq_minlen: int = 1,
                        fastq_maxlen: int = -1, fastq_maxee: float = -1.0,
                        fastq_maxee_rate: float = -1.0) -> FastqFilterParams:
    """vsearch's defaults; a negative fastq_maxlen / fastq_maxee / fastq_maxee_rate means the option is not given."""
    return FastqFilterParams(fastq_ascii, fastq_qmin, fastq_qmax, fastq_minlen, fastq_maxlen, 0, fastq_maxee,
                             fastq_maxee_rate)


def fastq_filter_params_from_argv(argv: list[str]) -> tuple[FastqFilterParams, dict]:
    """umiclust_fastq_filter_params_from_argv: the decoded options and the in / fastqout / fastqout_discarded / log
    paths (None where not given).  Needs no device."""
    p = FastqFilterParams()
    bufs = [C.create_string_buffer(4096) for _ in range(4)]
    arr = (C.c_char_p * len(argv))(*[str(a).encode() for a in argv])
    rc = lib().umiclust_fastq_filter_params_from_argv(C.byref(p), len(argv), arr, *bufs, 4096)
    if rc != 0:
        raise UmiclustError(rc, f"cannot parse argv {argv!r}")
    keys = ["in_fastq", "fastqout", "fastqout_discarded", "log"]
    return p, {k: (b.value.decode() or None) for k, b in zip(keys, bufs)}


def _i64(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _pack(seqs) -> tuple[np.ndarray, np.ndarray]:
    """list of str/bytes -> (uint8 buffer, int64 offsets)."""
    bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    off = np.zeros(len(bs) + 1, np.int64)
    if bs:
        np.cumsum([len(b) for b in bs], out=off[1:])
    buf = np.frombuffer(b"".join(bs) + b"\0", np.uint8).copy()
    return buf, off


class Context:
    """One device context (one per process and GPU)."""

    def __init__(self, device: int = 0):
        err = C.c_int32(0)
        self._h = lib().umiclust_create(device, C.byref(err))
        if not self._h:
            raise UmiclustError(err.value, f"no HIP device {device} (there is no CPU backend)")

    def close(self):
        if self._h:
            lib().umiclust_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int, what: str) -> int:
        if rc < 0:
            msg = lib().umiclust_last_error(self._h)
            raise UmiclustError(int(rc), f"{what}: {msg.decode() if msg else ''}")
        return rc

    def wait_host(self) -> None:
        """Waits for the host work the last file-path call left running (its input's release)."""
        self._check(lib().umiclust_wait_host(self._h), "wait_host")

    def run_fasta(self, p: Params, in_fasta: str, clusters_prefix: str | None, consout: str | None,
                  log: str | None) -> dict:
        st = Stats()
        enc = lambda x: x.encode() if x else None  # noqa: E731
        k = lib().umiclust_run_fasta(self._h, C.byref(p), enc(in_fasta), enc(clusters_prefix), enc(consout),
                                     enc(log), C.byref(st))
        self._check(k, "run_fasta")
        return st.as_dict()

    def run_fasta_parse(self, p: Params, in_fasta: str, clusters_prefix: str | None, consout: str | None,
                        log: str | None, pp: ParseParams, work_dir: str) -> tuple[dict, dict]:
        """Clustering + parse_umi_clusters' outputs from memory (include/umiclust.h)."""
        st, pr = Stats(), ParseResult()
        enc = lambda x: x.encode() if x else None  # noqa: E731
        k = lib().umiclust_run_fasta_parse(self._h, C.byref(p), enc(in_fasta), enc(clusters_prefix), enc(consout),
                                           enc(log), C.byref(pp), work_dir.encode(), C.byref(pr), C.byref(st))
        self._check(k, "run_fasta_parse")
        return st.as_dict(), pr.as_dict()

    def run_argv(self, argv: list[str]) -> dict:
        st = Stats()
        arr = (C.c_char_p * len(argv))(*[str(a).encode() for a in argv])
        k = lib().umiclust_run_argv(self._h, len(argv), arr, C.byref(st))
        self._check(k, "run_argv")
        return st.as_dict()

    def load(self, p: Params, seqs=None, buf: np.ndarray | None = None, off: np.ndarray | None = None) -> None:
        if seqs is not None:
            buf, off = _pack(seqs)
        n = len(off) - 1
        self._check(lib().umiclust_load(self._h, C.byref(p), buf.ctypes.data, _i64(off), n), "load")
        self._n = n
        self._bins = None

    def stage(self, buf: np.ndarray, off: np.ndarray, bin_start=None) -> None:
        """umiclust_stage: the raw records into HBM (one bin, or bins [bin_start[b], bin_start[b+1]))."""
        n = len(off) - 1
        bs = None if bin_start is None else np.ascontiguousarray(bin_start, np.int64)
        self._check(lib().umiclust_stage(self._h, buf.ctypes.data, _i64(off), n, None if bs is None else _i64(bs),
                                         0 if bs is None else len(bs) - 1), "stage")
        self._n = n
        self._bins = bs

    def prepare(self, p: Params) -> None:
        """umiclust_prepare: length filter, sort, DUST, codes and k-mers of the staged records."""
        self._check(lib().umiclust_prepare(self._h, C.byref(p)), "prepare")

    def set_priority(self, level: int) -> None:
        """umiclust_set_priority: 1 = this context's counting stream at the greatest priority, 0 = plain (the
        alignment stream prioritised at both), -1 = every stream plain (background)."""
        self._check(lib().umiclust_set_priority(self._h, int(level)), "set_priority")

    def cluster(self) -> dict:
        st = Stats()
        self._check(lib().umiclust_cluster(self._h, C.byref(st)), "cluster")
        return st.as_dict()

    def fetch(self) -> dict:
        return self.fetch_bin(0) if getattr(self, "_bins", None) is not None else self._fetch(None, self._n)

    def load_bins(self, p: Params, buf: np.ndarray, off: np.ndarray, bin_start) -> None:
        """Many region bins resident at once: bin b = records [bin_start[b], bin_start[b+1])."""
        bs = np.ascontiguousarray(bin_start, np.int64)
        n = len(off) - 1
        self._check(lib().umiclust_load_bins(self._h, C.byref(p), buf.ctypes.data, _i64(off), n, _i64(bs),
                                             len(bs) - 1), "load_bins")
        self._n = n
        self._bins = bs

    def cluster_pack(self, first: int, nbins: int) -> dict:
        """Bins [first, first + nbins) of the load in one greedy order (umiclust_cluster_pack); stats of the pack."""
        st = Stats()
        self._check(lib().umiclust_cluster_pack(self._h, first, nbins, C.byref(st)), "cluster_pack")
        return st.as_dict()

    def cluster_bin(self, b: int) -> dict:
        st = Stats()
        self._check(lib().umiclust_cluster_bin(self._h, b, C.byref(st)), "cluster_bin")
        return st.as_dict()

    def fetch_bin(self, b: int) -> dict:
        bs = getattr(self, "_bins", None)
        n = int(bs[b + 1] - bs[b]) if bs is not None else self._n
        return self._fetch(b, n)

    def _fetch(self, b, n: int) -> dict:
        cl = np.empty(max(n, 1), np.int32)
        sd = np.empty(max(n, 1), np.uint8)
        ce = np.empty(max(n, 1), np.uint8)
        P = C.POINTER
        if b is None:
            f = lambda *a: lib().umiclust_fetch(self._h, *a)  # noqa: E731
        else:
            f = lambda *a: lib().umiclust_fetch_bin(self._h, b, *a)  # noqa: E731
        k = self._check(f(None, None, None, None, 0, None), "fetch")
        off = np.zeros(k + 1, np.int64)
        self._check(f(None, None, None, None, 0, _i64(off)), "fetch")
        cons = np.zeros(int(off[-1]) + 1, np.uint8)
        self._check(f(cl.ctypes.data_as(P(C.c_int32)), sd.ctypes.data_as(P(C.c_uint8)),
                      ce.ctypes.data_as(P(C.c_uint8)), cons.ctypes.data, len(cons), _i64(off)), "fetch")
        raw = cons.tobytes()
        return dict(n_clusters=int(k), cluster=cl[:n], strand=sd[:n], centroid=ce[:n],
                    consensus=[raw[off[c]:off[c + 1]].decode() for c in range(k)])

    def overlap_counts(self, seqs1, seqs2) -> np.ndarray:
        """Per set-1 sequence, the number of byte-equal set-2 sequences (umiclust_overlap_counts)."""
        b1, o1 = _pack(seqs1)
        b2, o2 = _pack(seqs2)
        n1 = len(o1) - 1
        out = np.zeros(max(n1, 1), np.int64)
        self._check(lib().umiclust_overlap_counts(self._h, b1.ctypes.data, _i64(o1), n1, b2.ctypes.data, _i64(o2),
                                                  len(o2) - 1, _i64(out)), "overlap_counts")
        return out[:n1]

    def overlap_regions(self, regions) -> tuple[np.ndarray, np.ndarray]:
        """regions: list of sequence lists.  (total, maxcount) R x R matrices, entries [a, b] for a < b."""
        flat = [s for r in regions for s in r]
        buf, off = _pack(flat)
        rs = np.zeros(len(regions) + 1, np.int64)
        np.cumsum([len(r) for r in regions], out=rs[1:])
        R = len(regions)
        tot = np.zeros(R * R, np.int64)
        mx = np.zeros(R * R, np.int32)
        self._check(lib().umiclust_overlap_regions(self._h, buf.ctypes.data, _i64(off), len(flat), _i64(rs), R,
                                                   _i64(tot), mx.ctypes.data_as(C.POINTER(C.c_int32))),
                    "overlap_regions")
        return tot.reshape(R, R), mx.reshape(R, R)

    def overlap_probe(self, regions, hash_bits: int = 64, caps=None) -> dict:
        """umiclust_overlap_probe: the region join of overlap_regions with the arrays its kernels leave behind -- hash,
        region, slot, rep_of, members [n]; cnt [m], start [m + 1]; big (the slots handed to the workgroup kernel);
        total, maxcount [R, R]; m, passes, seed.  caps = (n_cap, m_cap, big_cap) overrides the capacities passed."""
        flat = [s for r in regions for s in r]
        buf, off = _pack(flat)
        n, R = len(flat), len(regions)
        rs = np.zeros(R + 1, np.int64)
        np.cumsum([len(r) for r in regions], out=rs[1:])
        m = 1024
        while m < 2 * n:
            m *= 2
        nb = n // 33 + 1
        u64 = np.iinfo(np.uint64).max
        o = dict(hash=np.full(max(n, 1), u64, np.uint64), region=np.full(max(n, 1), -1, np.int32),
                 slot=np.full(max(n, 1), -1, np.int64), rep_of=np.full(max(n, 1), -1, np.int64),
                 cnt=np.full(m, 0xffffffff, np.uint32), start=np.full(m + 1, 0xffffffff, np.uint32),
                 members=np.full(max(n, 1), 0xffffffff, np.uint32), big=np.full(nb, 0xffffffff, np.uint32),
                 nbig=np.full(1, -1, np.int64), total=np.full(R * R, -1, np.int64),
                 maxcount=np.full(R * R, -1, np.int32), info=np.zeros(3, np.uint64))
        n_cap, m_cap, big_cap = caps if caps is not None else (n, m, nb)
        rc = lib().umiclust_overlap_probe(self._h, buf.ctypes.data, _i64(off), n, _i64(rs), R, hash_bits, n_cap, m_cap,
                                          big_cap, *(o[k].ctypes.data for k in (
                                              "hash", "region", "slot", "rep_of", "cnt", "start", "members", "big",
                                              "nbig", "total", "maxcount", "info")))
        self._check(rc, "overlap_probe")
        nbig = int(o["nbig"][0])
        return dict(hash=o["hash"][:n], region=o["region"][:n], slot=o["slot"][:n], rep_of=o["rep_of"][:n],
                    cnt=o["cnt"], start=o["start"], members=o["members"][:n], big=o["big"][:nbig],
                    total=o["total"].reshape(R, R), maxcount=o["maxcount"].reshape(R, R), m=int(o["info"][0]),
                    passes=int(o["info"][1]), seed=int(o["info"][2]))

    def extract_umis(self, seqs, a5: int = 73, a3: int = 68, k: int = 3, fwd: str = "", rev: str = "") -> np.ndarray:
        """[n, 6] int32: (dist, start, end) of the 5' and 3' UMI per read (-1: none), window coordinates."""
        buf, off = _pack(seqs)
        n = len(off) - 1
        out = np.zeros(max(n, 1) * 6, np.int32)
        self._check(lib().umiclust_extract_umis(self._h, buf.ctypes.data, _i64(off), n, a5, a3, k, fwd.encode(),
                                                rev.encode(), out.ctypes.data_as(C.POINTER(C.c_int32))),
                    "extract_umis")
        return out[:n * 6].reshape(n, 6)

    def extract_umis_file(self, fastx: str, out_fasta: str, a5: int, a3: int, k: int, fwd: str, rev: str) -> int:
        return int(self._check(lib().umiclust_extract_umis_file(self._h, fastx.encode(), out_fasta.encode(), a5, a3, k,
                                                                fwd.encode(), rev.encode()), "extract_umis_file"))

    def fastq_filter(self, p: FastqFilterParams, in_fastq: str, fastqout: str | None,
                     fastqout_discarded: str | None = None, log: str | None = None) -> dict:
        """umiclust_fastq_filter (vsearch --fastq_filter): the result counters and phase times."""
        r = FastqFilterResult()
        enc = lambda x: os.fspath(x).encode() if x else None  # noqa: E731
        k = lib().umiclust_fastq_filter(self._h, C.byref(p), enc(in_fastq), enc(fastqout), enc(fastqout_discarded),
                                        enc(log), C.byref(r))
        self._check(k, "fastq_filter")
        return r.as_dict()

    def fastq_filter_argv(self, argv: list[str]) -> dict:
        """The same from the argv the reference builds (preprocessing.py:129-148)."""
        r = FastqFilterResult()
        arr = (C.c_char_p * len(argv))(*[str(a).encode() for a in argv])
        k = lib().umiclust_fastq_filter_argv(self._h, len(argv), arr, C.byref(r))
        self._check(k, "fastq_filter_argv")
        return r.as_dict()

    def fastq_filter_stats(self, p: FastqFilterParams, in_fastq: str, fastqout: str | None = None,
                           fastqout_discarded: str | None = None, log: str | None = None,
                           stats_before_txt: str | None = None, stats_after_txt: str | None = None) -> dict:
        """umiclust_fastq_filter_stats: the filter and, from the same pass, the two `seqkit stat -a` tables of the
        records read and of the records kept (policy O8).  Returns the result counters and phase times plus
        "before" / "after", the tables' numbers.  Without any filter output it is a statistics-only pass."""
        r, b, a = FastqFilterResult(), FastqStats(), FastqStats()
        enc = lambda x: os.fspath(x).encode() if x else None  # noqa: E731
        k = lib().umiclust_fastq_filter_stats(self._h, C.byref(p), enc(in_fastq), enc(fastqout),
                                              enc(fastqout_discarded), enc(log), enc(stats_before_txt),
                                              enc(stats_after_txt), C.byref(r), C.byref(b), C.byref(a))
        self._check(k, "fastq_filter_stats")
        return dict(r.as_dict(), before=b.as_dict(), after=a.as_dict())

    def fastq_filter_stats_argv(self, argv: list[str], stats_before_txt: str | None = None,
                                stats_after_txt: str | None = None) -> dict:
        """The same from the argv the reference builds (preprocessing.py:129-148)."""
        r, b, a = FastqFilterResult(), FastqStats(), FastqStats()
        enc = lambda x: os.fspath(x).encode() if x else None  # noqa: E731
        arr = (C.c_char_p * len(argv))(*[str(x).encode() for x in argv])
        k = lib().umiclust_fastq_filter_stats_argv(self._h, len(argv), arr, enc(stats_before_txt),
                                                   enc(stats_after_txt), C.byref(r), C.byref(b), C.byref(a))
        self._check(k, "fastq_filter_stats_argv")
        return dict(r.as_dict(), before=b.as_dict(), after=a.as_dict())

    def fastq_record_stats(self, seqs, quals, fastq_ascii: int = 33):
        """umiclust_fastq_record_stats: per record (`seqs[i]` and `quals[i]` are bytes objects of one length) the
        fixed-point expected error, the smallest / largest quality byte, and counts[i] = (n_q20, n_q30, n_gc, n_n,
        n_gap) as a uint32 array of shape (n, 5)."""
        if [len(x) for x in seqs] != [len(x) for x in quals]:
            raise ValueError("a record's sequence and quality differ in length")
        sbuf, off = _pack(seqs)
        qbuf, _ = _pack(quals)
        n = len(off) - 1
        ee = np.zeros(max(n, 1), np.int64)
        lo = np.zeros(max(n, 1), np.uint8)
        hi = np.zeros(max(n, 1), np.uint8)
        cnt = np.zeros((max(n, 1), 5), np.uint32)
        P = C.POINTER
        self._check(lib().umiclust_fastq_record_stats(self._h, sbuf.ctypes.data, qbuf.ctypes.data, _i64(off), n,
                                                      fastq_ascii, _i64(ee), lo.ctypes.data_as(P(C.c_uint8)),
                                                      hi.ctypes.data_as(P(C.c_uint8)),
                                                      cnt.ctypes.data_as(P(C.c_uint32))), "fastq_record_stats")
        return ee[:n], lo[:n], hi[:n], cnt[:n]

    def fastq_ee(self, quals, fastq_ascii: int = 33) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """umiclust_fastq_ee: per record of `quals` (bytes objects) the fixed-point expected error (int64, 2^-40
        units) and the smallest / largest raw byte (255 / 0 for an empty record)."""
        buf, off = _pack(quals)
        n = len(off) - 1
        ee = np.zeros(max(n, 1), np.int64)
        lo = np.zeros(max(n, 1), np.uint8)
        hi = np.zeros(max(n, 1), np.uint8)
        P = C.POINTER
        self._check(lib().umiclust_fastq_ee(self._h, buf.ctypes.data, _i64(off), n, fastq_ascii, _i64(ee),
                                            lo.ctypes.data_as(P(C.c_uint8)), hi.ctypes.data_as(P(C.c_uint8))),
                    "fastq_ee")
        return ee[:n], lo[:n], hi[:n]

    def region_split(self, bam_file: str, names, lengths, clusters, minov: float, s5: int, s3: int, out_dir: str):
        """umiclust_region_split: (counts[4], reads_per_cluster, region_detected); KeyError(name) as the
        reference raises it.  bam_file None: umiclust_bam_region_split, on the open session."""
        R = len(names)
        nm = (C.c_char_p * max(R, 1))(*[x.encode() for x in names])
        ln = np.asarray(lengths, np.int64)
        cl = np.asarray(clusters, np.int32)
        cap = int(max([0] + [k + 1 for k in clusters]))
        counts = np.zeros(4, np.int64)
        rpc = np.zeros(max(cap, 1), np.int64)
        det = np.zeros(max(R, 1), np.uint8)
        miss = C.create_string_buffer(4096)
        P = C.POINTER
        tail = (R, nm, _i64(ln), cl.ctypes.data_as(P(C.c_int32)), minov, s5, s3, os.fspath(out_dir).encode(),
                _i64(counts), _i64(rpc), cap, det.ctypes.data_as(P(C.c_uint8)), miss, 4096)
        if bam_file is None:
            rc = lib().umiclust_bam_region_split(self._h, *tail)
        else:
            rc = lib().umiclust_region_split(self._h, os.fspath(bam_file).encode(), *tail)
        if rc == -74 and miss.value:
            raise KeyError(miss.value.decode())
        if rc == -74 and (lib().umiclust_last_error(self._h) or b"").startswith(b"TypeError: "):
            raise TypeError(lib().umiclust_last_error(self._h).decode()[len("TypeError: "):])
        self._check(rc, "region_split")
        return counts, rpc[:cap], det[:R]

    def region_split_extract(self, bam_file: str, names, lengths, clusters, minov: float, s5: int, s3: int, a5: int,
                             a3: int, k: int, fwd: str, rev: str, umi_out_dir: str):
        """umiclust_region_split_extract (row f4+f1): region_split and extract_umis_file in one pass,
        region_cluster<k>_detected_umis.fasta in umi_out_dir and no region FASTA.  (counts[4], reads_per_cluster,
        umis_per_cluster, region_detected); KeyError(name) as region_split raises it, with no file written.  bam_file
        None: umiclust_bam_region_split_extract, on the open session."""
        R = len(names)
        nm = (C.c_char_p * max(R, 1))(*[x.encode() for x in names])
        ln = np.asarray(lengths, np.int64)
        cl = np.asarray(clusters, np.int32)
        cap = int(max([0] + [k_ + 1 for k_ in clusters]))
        counts = np.zeros(4, np.int64)
        rpc, upc = np.zeros(max(cap, 1), np.int64), np.zeros(max(cap, 1), np.int64)
        det = np.zeros(max(R, 1), np.uint8)
        miss = C.create_string_buffer(4096)
        P = C.POINTER
        tail = (R, nm, _i64(ln), cl.ctypes.data_as(P(C.c_int32)), minov, s5, s3, a5, a3, k, fwd.encode(), rev.encode(),
                os.fspath(umi_out_dir).encode(), _i64(counts), _i64(rpc), _i64(upc), cap,
                det.ctypes.data_as(P(C.c_uint8)), miss, 4096)
        if bam_file is None:
            rc = lib().umiclust_bam_region_split_extract(self._h, *tail)
        else:
            rc = lib().umiclust_region_split_extract(self._h, os.fspath(bam_file).encode(), *tail)
        if rc == -74 and miss.value:
            raise KeyError(miss.value.decode())
        self._check(rc, "region_split_extract")
        return counts, rpc[:cap], upc[:cap], det[:R]

    def bam_open(self, bam_file: str, hash_bits: int = 64) -> "BamSession":
        """umiclust_bam_open: the BAM session of this context (one at a time; row f6)."""
        self._check(lib().umiclust_bam_open(self._h, os.fspath(bam_file).encode(), hash_bits), "bam_open")
        return BamSession(self)

    def sam_open(self, sam_file, hash_bits: int = 64) -> "BamSession":
        """umiclust_sam_open: the BAM session of SAM text -- a file, a FIFO or /dev/fd/N -- parsed,
        encoded and coordinate-sorted on the device; the session umiclust_bam_open gives for `samtools sort`'s file."""
        self._check(lib().umiclust_sam_open(self._h, os.fspath(sam_file).encode(), hash_bits), "sam_open")
        return BamSession(self)

    def bam_index_file(self, bam_file, bai=None) -> int:
        """umiclust_bam_index_file: `samtools index bam_file` on the device, the index at `bai` (None:
        bam_file + ".bai").  Returns the number of records; an open session stays as it is."""
        return int(self._check(lib().umiclust_bam_index_file(
            self._h, os.fspath(bam_file).encode(), os.fspath(bai).encode() if bai is not None else None),
            "bam_index_file"))

    def bam_index_info(self) -> dict:
        """umiclust_bam_index_info: the counts and seconds of this context's last index, probe or flagstat call"""
        out, t = np.zeros(4, np.int64), np.zeros(4, np.float64)
        self._check(lib().umiclust_bam_index_info(self._h, _i64(out), t.ctypes.data_as(C.POINTER(C.c_double))),
                    "bam_index_info")
        d = dict(zip(("kept", "runs", "chunks", "windows"), (int(x) for x in out)))
        d.update(zip(("upload_s", "kernel_s", "copy_back_s", "finish_s"), (float(x) for x in t)))
        return d

    def bgzf_inflate(self, data, want_status: bool = False):
        """umiclust_bgzf_inflate: the BGZF byte string `data` inflated on the device, as a uint8 array.
        want_status: returns (bytes, status, error) instead -- one int32 per block (0 = ok, else the decoder's error
        class) and None or, where a block was refused, the UmiclustError (EFORMAT, naming the first such block) that
        the plain call raises; the bytes of every good block are in place either way.  Malformed framing raises."""
        L = lib()
        src = np.frombuffer(data, np.uint8)
        nblk = C.c_int64(-1)
        size = self._check(L.umiclust_bgzf_inflate(self._h, src.ctypes.data, len(src), None, 0, None, C.byref(nblk),
                                                   None), "bgzf_inflate")
        out, status, times = np.zeros(max(size, 1), np.uint8), np.zeros(max(nblk.value, 1), np.int32), np.zeros(3)
        rc = L.umiclust_bgzf_inflate(self._h, src.ctypes.data, len(src), out.ctypes.data, len(out),
                                     status.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nblk),
                                     times.ctypes.data_as(C.POINTER(C.c_double)))
        self.bgzf_times = {"h2d_s": float(times[0]), "kernel_s": float(times[1]), "d2h_s": float(times[2])}
        out, status = out[:size], status[:nblk.value]
        if not want_status:
            self._check(rc, "bgzf_inflate")
            return out
        err = None
        if rc < 0:
            try:
                self._check(rc, "bgzf_inflate")
            except UmiclustError as e:
                if e.code != -74 or not status.any():
                    raise
                err = e
        return out, status, err

    def bgzf_deflate(self, data, want_info: bool = False):
        """umiclust_bgzf_deflate: `data` cut into 0xff00-byte blocks, deflated and framed on the
        device, as the uint8 array of a BGZF file (EOF block included).  want_info: returns (bytes, kinds) instead --
        one int32 per block, 0 = stored, 1 = fixed, 2 = dynamic."""
        L = lib()
        src = np.frombuffer(data, np.uint8)
        nblk = C.c_int64(-1)
        cap = self._check(L.umiclust_bgzf_deflate(self._h, src.ctypes.data, len(src), None, 0, None, C.byref(nblk),
                                                  None), "bgzf_deflate")
        out, kinds, times = np.zeros(cap, np.uint8), np.zeros(max(nblk.value, 1), np.int32), np.zeros(3)
        size = self._check(L.umiclust_bgzf_deflate(self._h, src.ctypes.data, len(src), out.ctypes.data, len(out),
                                                   kinds.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nblk),
                                                   times.ctypes.data_as(C.POINTER(C.c_double))), "bgzf_deflate")
        self.bgzf_times = {"h2d_s": float(times[0]), "kernel_s": float(times[1]), "d2h_s": float(times[2])}
        return (out[:size], kinds[:nblk.value]) if want_info else out[:size]

    def align_pairs(self, p: Params, queries, targets, with_ops: bool = False) -> dict:
        qb, qo = _pack(queries)
        tb, to = _pack(targets)
        n = len(qo) - 1
        P = C.POINTER
        sc = np.zeros(max(n, 1), np.int32)
        m = np.zeros(max(n, 1), np.int32)
        il = np.zeros(max(n, 1), np.int32)
        stride = 2 * MAX_LEN
        ops = np.zeros(max(n, 1) * stride, np.uint8) if with_ops else None
        nops = np.zeros(max(n, 1), np.int32) if with_ops else None
        rc = lib().umiclust_align_pairs(self._h, C.byref(p), qb.ctypes.data, _i64(qo), tb.ctypes.data, _i64(to), n,
                                        sc.ctypes.data_as(P(C.c_int32)), m.ctypes.data_as(P(C.c_int32)),
                                        il.ctypes.data_as(P(C.c_int32)), ops.ctypes.data if with_ops else None,
                                        stride, nops.ctypes.data_as(P(C.c_int32)) if with_ops else None)
        self._check(rc, "align_pairs")
        out = dict(score=sc[:n], matches=m[:n], internal_len=il[:n])
        if with_ops:
            raw = ops.tobytes()
            out["ops"] = [raw[k * stride:k * stride + nops[k]].decode() for k in range(n)]
        return out

    def consensus(self, p: Params, seqs, clusters, strands=None, ops=None) -> dict:
        """umiclust_consensus: the member tracebacks (ops None) or the given ops, then the consensus kernel.
        clusters: lists of record indices into seqs, centroid first; strands: the same shape, 1 = the member is read
        as its reverse complement (default: all 0); ops: the same shape, an 'M' / 'D' / 'I' string per member (the
        centroid's entry is ignored).  Returns per cluster the consensus and, in the shape of clusters, the ops the
        consensus kernel read (strings, '' for centroids) and the traceback's score, matches and internal_len."""
        buf, off = _pack(seqs)
        n = len(off) - 1
        K = len(clusters)
        cstart = np.zeros(K + 1, np.int32)
        if K:
            np.cumsum([len(m) for m in clusters], out=cstart[1:])
        nm = int(cstart[-1])
        member = np.array([r for m in clusters for r in m] + [0], np.int32)
        mstr = np.zeros(nm + 1, np.uint8)
        if strands is not None:
            mstr[:nm] = [int(x) for m in strands for x in m]
        stride = 2 * MAX_LEN
        P = C.POINTER
        i32 = lambda a: a.ctypes.data_as(P(C.c_int32))  # noqa: E731
        ops_in = ops_in_len = None
        if ops is not None:
            flat = [(o if isinstance(o, bytes) else str(o or "").encode()) for m in ops for o in m]
            width = max([stride] + [len(o) for o in flat])  # an over-long member is the library's to reject
            ops_in = np.zeros((nm + 1) * width, np.uint8)
            ops_in_len = np.zeros(nm + 1, np.int32)
            for x, o in enumerate(flat):
                ops_in[x * width:x * width + len(o)] = np.frombuffer(o, np.uint8)
                ops_in_len[x] = len(o)
        else:
            width = stride
        ops_out = np.zeros((nm + 1) * width, np.uint8)
        ops_out_len = np.zeros(nm + 1, np.int32)
        sc, mt, il = (np.zeros(nm + 1, np.int32) for _ in range(3))
        cons = np.zeros(K * stride + 1, np.uint8)
        coff = np.zeros(K + 1, np.int64)
        rc = lib().umiclust_consensus(self._h, C.byref(p), buf.ctypes.data, _i64(off), n, i32(cstart), K, i32(member),
                                      mstr.ctypes.data_as(P(C.c_uint8)),
                                      None if ops_in is None else ops_in.ctypes.data,
                                      None if ops_in is None else i32(ops_in_len), width, ops_out.ctypes.data,
                                      i32(ops_out_len), i32(sc), i32(mt), i32(il), cons.ctypes.data, len(cons),
                                      _i64(coff))
        self._check(rc, "consensus")
        raw, oraw = cons.tobytes(), ops_out.tobytes()

        def shaped(a):
            return [list(a[cstart[k]:cstart[k + 1]]) for k in range(K)]
        out_ops = [oraw[x * width:x * width + ops_out_len[x]].decode() for x in range(nm)]
        return dict(consensus=[raw[coff[k]:coff[k + 1]].decode() for k in range(K)], ops=shaped(out_ops),
                    score=shaped(sc[:nm]), matches=shaped(mt[:nm]), internal_len=shaped(il[:nm]))

    def _prefilter_lists(self, what: str, nq: int, ninfo: int, call) -> dict:
        """the output buffers of the prefilter probes; call(*buffers) -> return code"""
        nqs = max(nq, 1) * 2
        top_seqno = np.zeros((nqs, 41), np.uint32)
        top_count = np.zeros((nqs, 41), np.uint8)
        ntop = np.zeros(nqs, np.uint8)
        peer_id = np.zeros((nqs, 128), np.uint16)
        peer_count = np.zeros((nqs, 128), np.uint8)
        npeer = np.zeros(nqs, np.uint8)
        info = np.zeros(8, np.int64)
        P = C.POINTER
        u8 = lambda a: a.ctypes.data_as(P(C.c_uint8))  # noqa: E731
        self._check(call(top_seqno.ctypes.data_as(P(C.c_uint32)), u8(top_count), u8(ntop),
                         peer_id.ctypes.data_as(P(C.c_uint16)), u8(peer_count), u8(npeer), _i64(info)), what)
        n = nq * int(info[4])
        return dict(top_seqno=top_seqno[:n], top_count=top_count[:n], ntop=ntop[:n], peer_id=peer_id[:n],
                    peer_count=peer_count[:n], npeer=npeer[:n], info=info[:ninfo], both=int(info[4]))

    def prefilter(self, cent, q0: int, nq: int, nprev: int = 0, append_step: int = 1 << 30) -> dict:
        """umiclust_prefilter on the current load: the top and peer lists of the block [q0, q0 + nq) against the
        centroids `cent` (increasing sorted seqnos before the window), per query-strand (rows), and info[0..3]."""
        ce = np.ascontiguousarray(cent, np.int32)
        return self._prefilter_lists("prefilter", nq, 4, lambda *out: lib().umiclust_prefilter(
            self._h, ce.ctypes.data_as(C.POINTER(C.c_int32)), len(ce), q0, nq, nprev, append_step, *out))

    def prefilter_pack(self, first: int, nbins: int, cent, q0: int, nq: int, nprev: int = 0,
                       append_step: int = 1 << 30) -> dict:
        """umiclust_prefilter_pack: prefilter() on the pack [first, first + nbins) of a load_bins load."""
        ce = np.ascontiguousarray(cent, np.int32)
        return self._prefilter_lists("prefilter_pack", nq, 4, lambda *out: lib().umiclust_prefilter_pack(
            self._h, first, nbins, ce.ctypes.data_as(C.POINTER(C.c_int32)), len(ce), q0, nq, nprev, append_step, *out))

    def prefilter_split(self, cent, newcent, w0: int, nq: int, append_step: int = 1 << 30) -> dict:
        """umiclust_prefilter_split: block [w0 + 2 nq, w0 + 3 nq) as a split pass -- the counting half with block
        [w0, w0 + nq) flagged, the append of `newcent` (seqnos of that block), the second half; info[0..6]."""
        ce = np.ascontiguousarray(cent, np.int32)
        nc = np.ascontiguousarray(newcent, np.int32)
        p32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
        return self._prefilter_lists("prefilter_split", nq, 7, lambda *out: lib().umiclust_prefilter_split(
            self._h, p32(ce), len(ce), p32(nc), len(nc), w0, nq, append_step, *out))

    def run_pass(self, cent, q0: int, nq: int, nprev: int = 0, append_step: int = 1 << 30, lazy: bool = False,
                 prev: bool = False, rec_cap: int | None = None) -> dict:
        """umiclust_pass on the current load: one whole device pass of the block [q0, q0 + nq) -- the prefilter's
        lists (as prefilter()), k_pack's outcomes `hostqs` (PASS_QS records), the record words `rec` (rec_total of
        them), the raw result words `res` (walk: [qs, x]) and `peer_res` ([qs, y]), the `aligned` masks ([qs, 2]), the
        final walk states `walk` (PASS_WALK records) and the 16 pass counters.  rec_cap: room for the records (default:
        the largest a pass can write); a pass that needs more raises UmiclustError(-34)."""
        ce = np.ascontiguousarray(cent, np.int32)
        nqs = max(nq, 1) * 2
        top_seqno = np.zeros((nqs, 41), np.uint32)
        top_count = np.zeros((nqs, 41), np.uint8)
        ntop = np.zeros(nqs, np.uint8)
        peer_id = np.zeros((nqs, 128), np.uint16)
        peer_count = np.zeros((nqs, 128), np.uint8)
        npeer = np.zeros(nqs, np.uint8)
        hostqs = np.zeros(nqs, PASS_QS)
        cap = nqs * PASS_REC_WORDS if rec_cap is None else rec_cap
        rec = np.zeros(max(cap, 1), np.uint32)
        total = np.zeros(1, np.int64)
        res = np.zeros(nqs * 160, np.uint32)
        aligned = np.zeros((nqs, 2), np.uint64)
        walk = np.zeros(nqs, PASS_WALK)
        counters = np.zeros(16, np.uint32)
        info = np.zeros(8, np.int64)
        P = C.POINTER
        u8 = lambda a: a.ctypes.data_as(P(C.c_uint8))  # noqa: E731
        u32 = lambda a: a.ctypes.data_as(P(C.c_uint32))  # noqa: E731
        rc = lib().umiclust_pass(self._h, ce.ctypes.data_as(P(C.c_int32)), len(ce), q0, nq, nprev, append_step,
                                 (1 if lazy else 0) | (2 if prev else 0), u32(top_seqno), u8(top_count), u8(ntop),
                                 peer_id.ctypes.data_as(P(C.c_uint16)), u8(peer_count), u8(npeer), hostqs.ctypes.data,
                                 u32(rec), cap, _i64(total), u32(res), aligned.ctypes.data_as(P(C.c_uint64)),
                                 walk.ctypes.data, u32(counters), _i64(info))
        self._check(rc, "pass")
        n = nq * int(info[4])
        return dict(top_seqno=top_seqno[:n], top_count=top_count[:n], ntop=ntop[:n], peer_id=peer_id[:n],
                    peer_count=peer_count[:n], npeer=npeer[:n], info=info[:4], both=int(info[4]), hostqs=hostqs[:n],
                    rec=rec[:min(int(total[0]), cap)], rec_total=int(total[0]), res=res[:n * 32].reshape(n, 32),
                    peer_res=res[n * 32:n * 160].reshape(n, 128), aligned=aligned[:n], walk=walk[:n],
                    counters=counters)

    def run_resolve(self, cent, q0: int, nq: int, nprev: int = 0, win_state=(), append_step: int = 1 << 30,
                    lazy: bool = False, prev: bool = False, partial: bool = False) -> dict:
        """umiclust_resolve on the current load: the pass of the block [q0, q0 + nq) queued as run_pass queues it, then
        resolved by the pipeline's own resolve step with the window's states `win_state` (1 centroid, 2 member per
        query of [q0 - nprev * nq, q0)), round B on the device.  state / target / strand per query, new_cents,
        resolved (queries), all (bool), the resolve step's n_alignments, cells, n_merged_walks, n_deferred,
        pairs_round_b, and round B's trips, launches, pairs and staged trips (rb_*) on the device side."""
        ce = np.ascontiguousarray(cent, np.int32)
        ws = np.ascontiguousarray(win_state, np.uint8)
        if len(ws) != nprev * nq:
            raise ValueError("win_state must hold nprev * nq states")
        n = max(nq, 1)
        state = np.zeros(n, np.uint8)
        target = np.full(n, -1, np.int32)
        strand = np.zeros(n, np.uint8)
        newc = np.zeros(n, np.int32)
        info = np.zeros(16, np.int64)
        P = C.POINTER
        u8 = lambda a: a.ctypes.data_as(P(C.c_uint8))  # noqa: E731
        i32 = lambda a: a.ctypes.data_as(P(C.c_int32))  # noqa: E731
        rc = lib().umiclust_resolve(self._h, i32(ce), len(ce), q0, nq, nprev, append_step,
                                    (1 if lazy else 0) | (2 if prev else 0) | (4 if partial else 0), u8(ws), u8(state),
                                    i32(target), u8(strand), i32(newc), _i64(info))
        self._check(rc, "resolve")
        keys = ("resolved", "all", "n_new", "n_alignments", "cells", "n_merged_walks", "n_deferred", "pairs_round_b",
                "rb_trips", "rb_launches", "rb_pairs", "both", "rb_staged")
        out = {k: int(v) for k, v in zip(keys, info)}
        out.update(state=state[:nq], target=target[:nq], strand=strand[:nq], new_cents=newc[:out["n_new"]],
                   all=bool(out["all"]))
        return out

    def prep(self, p: Params, seqs) -> dict:
        b, o = _pack(seqs)
        n = len(o) - 1
        masked = np.zeros(len(b), np.uint8)
        kst = MAX_LEN - 7  # >= unique 8-mers per strand
        km = np.zeros(max(n, 1) * 2 * kst, np.uint16)
        nk = np.zeros(max(n, 1) * 2, np.int32)
        P = C.POINTER
        rc = lib().umiclust_prep(self._h, C.byref(p), b.ctypes.data, _i64(o), n, masked.ctypes.data,
                                 km.ctypes.data_as(P(C.c_uint16)), kst, nk.ctypes.data_as(P(C.c_int32)))
        self._check(rc, "prep")
        mb = masked.tobytes()
        return dict(masked=[mb[o[i]:o[i + 1]].decode() for i in range(n)],
                    kmers=[[list(km[(2 * i + s) * kst:(2 * i + s) * kst + nk[2 * i + s]]) for s in range(2)]
                           for i in range(n)])

    def prep_outputs(self, p: Params, seqs, perm=None) -> dict:
        """umiclust_prep_outputs: everything K1 writes for the records (row s is record perm[s]), as the device holds
        it -- masked (bytes per row), codes [n, 2, 14], lens, kmers (per row and strand, device order), nk [n, 2],
        changed, ambig and n_changed (the two flag words)."""
        b, o = _pack(seqs)
        n = len(o) - 1
        pm = None if perm is None else np.ascontiguousarray(perm, np.int32)
        if pm is not None and len(pm) != n:
            raise ValueError("perm: one entry per record")
        kst = MAX_LEN - 7
        masked = np.zeros((max(n, 1), MAX_LEN), np.uint8)
        codes = np.full((max(n, 1), 2, MAX_LEN // 8), 0xffffffff, np.uint32)
        lens = np.full(max(n, 1), 255, np.uint8)
        km = np.zeros((max(n, 1), 2, kst), np.uint16)
        nk = np.full((max(n, 1), 2), -1, np.int32)
        changed = np.full(max(n, 1), 255, np.uint8)
        flags = np.full(2, 0xffffffff, np.uint32)
        rc = lib().umiclust_prep_outputs(self._h, C.byref(p), b.ctypes.data, _i64(o), n,
                                         None if pm is None else pm.ctypes.data, masked.ctypes.data, codes.ctypes.data,
                                         lens.ctypes.data, km.ctypes.data, kst, nk.ctypes.data, changed.ctypes.data,
                                         flags.ctypes.data)
        self._check(rc, "prep_outputs")
        lens, nk = lens[:n], nk[:n]
        return dict(masked=[masked[s, :lens[s]].tobytes().decode("latin-1") for s in range(n)], codes=codes[:n],
                    lens=lens, kmers=[[[int(x) for x in km[s, st, :nk[s, st]]] for st in range(2)] for s in range(n)],
                    nk=nk, changed=changed[:n], ambig=int(flags[0]), n_changed=int(flags[1]))


class BamSession:
    """The columns of an open BAM session (umiclust_bam_*), read once; names and cs strings are gathered in bulk on
    request.  The attributes are what umiclust.minimap2_align's formatting half takes from any source: n, cls, ref,
    l_seq, reference_length, cols, nm, nm_present, cs_group, ref_names, ref_lengths, query_names(idx),
    cs_strings(idx), write(keep, path), and -- for the round-2 split and the precision census --
    split(...) and name_suffix()."""

    def __init__(self, ctx: Context):
        self._ctx = ctx
        L, h, P = lib(), ctx._h, C.POINTER
        cnt = np.zeros(5, np.int64)
        ctx._check(L.umiclust_bam_counts(h, _i64(cnt)), "bam_counts")
        self.n, self.n_refs, self.n_cs_groups, self.n_hash_reruns, self.first_malformed = (int(x) for x in cnt)
        t = np.zeros(3, np.float64)
        ctx._check(L.umiclust_bam_times(h, t.ctypes.data_as(P(C.c_double))), "bam_times")
        self.times = {"inflate_s": float(t[0]), "h2d_s": float(t[1]), "device_s": float(t[2])}
        n = self.n
        self.cls, self.ref, self.l_seq = np.zeros(n, np.int8), np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.reference_length, self.cols, self.nm = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.nm_present, self.cs_group = np.zeros(n, np.uint8), np.zeros(n, np.int32)
        ctx._check(L.umiclust_bam_columns(
            h, self.cls.ctypes.data_as(P(C.c_int8)), self.ref.ctypes.data_as(P(C.c_int32)),
            self.l_seq.ctypes.data_as(P(C.c_int32)), _i64(self.reference_length), _i64(self.cols), _i64(self.nm),
            self.nm_present.ctypes.data_as(P(C.c_uint8)), self.cs_group.ctypes.data_as(P(C.c_int32))), "bam_columns")
        need = ctx._check(L.umiclust_bam_refs(h, None, 0, None, None), "bam_refs")
        buf, off = np.zeros(max(need, 1), np.uint8), np.zeros(self.n_refs + 1, np.int64)
        self.ref_lengths = np.zeros(self.n_refs, np.int64)
        if self.n_refs:
            ctx._check(L.umiclust_bam_refs(h, buf.ctypes.data, need, _i64(off), _i64(self.ref_lengths)), "bam_refs")
        raw = buf.tobytes()
        self.ref_names = [raw[off[r]:off[r + 1] - 1].decode("ascii") for r in range(self.n_refs)]
        self.group_count, self.group_rep = np.zeros(self.n_cs_groups, np.int64), np.zeros(self.n_cs_groups, np.int64)
        ctx._check(L.umiclust_bam_cs_groups(h, _i64(self.group_count), _i64(self.group_rep)), "bam_cs_groups")

    def _strings(self, kind: int, idx) -> list:
        idx = np.ascontiguousarray(idx, np.int64)
        m = len(idx)
        if m == 0:
            return []
        L, h = lib(), self._ctx._h
        need = self._ctx._check(L.umiclust_bam_strings(h, kind, _i64(idx), m, None, 0, None), "bam_strings")
        buf, off = np.zeros(max(need, 1), np.uint8), np.zeros(m + 1, np.int64)
        if need:
            self._ctx._check(L.umiclust_bam_strings(h, kind, _i64(idx), m, buf.ctypes.data, need, _i64(off)),
                             "bam_strings")
        raw = buf.tobytes()
        return [raw[off[x]:off[x + 1]].decode("ascii") for x in range(m)]

    def inflate_info(self) -> tuple:
        """umiclust_bam_inflate_info: (BGZF blocks, blocks inflated on the device, compressed bytes uploaded) of the
        open."""
        out = np.zeros(3, np.int64)
        self._ctx._check(lib().umiclust_bam_inflate_info(self._ctx._h, _i64(out)), "bam_inflate_info")
        return tuple(int(x) for x in out)

    def write_info(self) -> dict:
        """umiclust_bam_write_info: the counts and seconds of this session's last write"""
        out, t = np.zeros(8, np.int64), np.zeros(4, np.float64)
        self._ctx._check(lib().umiclust_bam_write_info(self._ctx._h, _i64(out), t.ctypes.data_as(C.POINTER(C.c_double))),
                         "bam_write_info")
        d = dict(zip(("blocks", "device_blocks", "stored", "fixed", "dynamic", "host_blocks", "batches",
                      "compressed_bytes"), (int(x) for x in out)))
        d.update(zip(("upload_s", "kernel_s", "copy_back_s", "gather_crc_s"), (float(x) for x in t)))
        return d

    def sam_info(self) -> dict:
        """umiclust_sam_info: the counts and HIP-event seconds of the umiclust_sam_open that made this session"""
        out, t = np.zeros(4, np.int64), np.zeros(5, np.float64)
        self._ctx._check(lib().umiclust_sam_info(self._ctx._h, _i64(out), t.ctypes.data_as(C.POINTER(C.c_double))),
                         "sam_info")
        d = dict(zip(("lines", "records", "text_bytes", "f_values"), (int(x) for x in out)))
        d.update(zip(("upload_s", "measure_s", "sort_s", "encode_s", "copy_back_s"), (float(x) for x in t)))
        return d

    def region_split(self, names, lengths, clusters, minov: float, s5: int, s3: int, out_dir):
        """umiclust_bam_region_split: Context.region_split on this session instead of a file"""
        return self._ctx.region_split(None, names, lengths, clusters, minov, s5, s3, out_dir)

    def region_split_extract(self, names, lengths, clusters, minov: float, s5: int, s3: int, a5: int, a3: int, k: int,
                             fwd: str, rev: str, umi_out_dir):
        """umiclust_bam_region_split_extract: Context.region_split_extract on this session instead of a file"""
        return self._ctx.region_split_extract(None, names, lengths, clusters, minov, s5, s3, a5, a3, k, fwd, rev,
                                              umi_out_dir)

    def query_names(self, idx) -> list:
        return self._strings(0, idx)

    def cs_strings(self, idx) -> list:
        return self._strings(1, idx)

    def _keep(self, keep):
        """(the array that owns the bytes, the pointer the ABI takes): None passes as NULL"""
        if keep is None:
            return None, None
        keep = np.ascontiguousarray(np.asarray(keep) != 0, np.uint8)
        if len(keep) != self.n:
            raise ValueError("keep needs one entry per record")
        return keep, keep.ctypes.data_as(C.POINTER(C.c_uint8))

    def write(self, keep, path, index=None) -> int:
        """umiclust_bam_write; with index=True (path + ".bai") or index=<a path>, umiclust_bam_write_index: the file
        and its .bai"""
        if keep is None:
            raise ValueError("keep needs one entry per record")  # (a write names what it keeps)
        keep, kp = self._keep(keep)
        if index is None or index is False:
            return int(self._ctx._check(lib().umiclust_bam_write(self._ctx._h, kp, os.fspath(path).encode()),
                                        "bam_write"))
        bai = None if index is True else os.fspath(index).encode()
        return int(self._ctx._check(lib().umiclust_bam_write_index(self._ctx._h, kp, os.fspath(path).encode(), bai),
                                    "bam_write_index"))

    FLAGSTAT_ROWS = ("total", "primary", "secondary", "supplementary", "duplicates", "primary_duplicates", "mapped",
                     "primary_mapped", "paired", "read1", "read2", "properly_paired", "both_mapped", "singletons",
                     "mate_other_chr", "mate_other_chr_mapq5")

    def flagstat(self, keep=None) -> tuple[dict, str]:
        """umiclust_bam_flagstat (policy O11): ({row: (QC-passed, QC-failed)}, the text `samtools
        flagstat` prints) over the records with keep[r] != 0 (None: all)"""
        keep, kp = self._keep(keep)
        L, h = lib(), self._ctx._h
        out = np.zeros(32, np.int64)
        need = self._ctx._check(L.umiclust_bam_flagstat(h, kp, _i64(out), None, 0), "bam_flagstat")
        buf = C.create_string_buffer(need)
        self._ctx._check(L.umiclust_bam_flagstat(h, kp, _i64(out), buf, need), "bam_flagstat")
        return ({k: (int(out[2 * x]), int(out[2 * x + 1])) for x, k in enumerate(self.FLAGSTAT_ROWS)},
                buf.value.decode("ascii"))

    def index_probe(self, keep, coff, ustart) -> dict:
        """umiclust_bam_index_probe: the index kernels on the kept records (None: all) under the block table (coff,
        ustart), with every array they leave.  A refused record is reported in first_bad / first_status."""
        keep, kp = self._keep(keep)
        coff, ustart = np.ascontiguousarray(coff, np.int64), np.ascontiguousarray(ustart, np.int64)
        if len(coff) != len(ustart):
            raise ValueError("coff and ustart need one entry per block")
        nk = self.n if keep is None else int(np.count_nonzero(keep))
        # a reference's windows: at most 2^29 >> 14 each, and every window of a reference but its last few holds a record
        wcap = 32768 * min(self.n_refs, nk) + 1
        a = dict(bin=np.zeros(nk, np.int32), u=np.zeros(nk, np.uint64), v=np.zeros(nk, np.uint64),
                 status=np.zeros(nk, np.int32), runs=np.zeros((nk, 4), np.int64), sorted_runs=np.zeros((nk, 4), np.int64),
                 n_intv=np.zeros(self.n_refs, np.int64), linear=np.zeros(wcap, np.uint64),
                 mapped=np.zeros(self.n_refs, np.int64), unmapped=np.zeros(self.n_refs, np.int64),
                 counters=np.zeros(32, np.int64), info=np.zeros(6, np.int64))
        p = {k: x.ctypes.data for k, x in a.items()}
        self._ctx._check(lib().umiclust_bam_index_probe(
            self._ctx._h, kp, _i64(coff), _i64(ustart), len(coff), p["bin"], p["u"], p["v"], p["status"], p["runs"],
            p["sorted_runs"], nk, p["n_intv"], p["linear"], wcap, p["mapped"], p["unmapped"], p["counters"], p["info"]),
            "bam_index_probe")
        nkept, nruns, nwin, first_bad, first_status, n_no_coor = (int(x) for x in a.pop("info"))
        a.update(runs=a["runs"][:nruns], sorted_runs=a["sorted_runs"][:nruns], linear=a["linear"][:nwin], n_kept=nkept,
                 first_bad=first_bad, first_status=first_status, n_no_coor=n_no_coor)
        return a

    def index_info(self) -> dict:
        """umiclust_bam_index_info: the counts and seconds of the context's last index, probe or flagstat call"""
        return self._ctx.bam_index_info()

    def split(self, keep, names, lengths, buckets, bucket_paths, overlap: float, s5: int, s3: int):
        """umiclust_bam_split: the records (keep None: all, else those with keep[r] != 0) appended as FASTA to
        bucket_paths[buckets[region]]; (counts[4], reads_per_bucket, region_detected).  KeyError(name) as
        Context.region_split raises it."""
        R, B = len(names), len(bucket_paths)
        P = C.POINTER
        kp = None
        if keep is not None:
            keep = np.ascontiguousarray(np.asarray(keep) != 0, np.uint8)
            if len(keep) != self.n:
                raise ValueError("keep needs one entry per record")
            kp = keep.ctypes.data_as(P(C.c_uint8))
        nm = (C.c_char_p * max(R, 1))(*[x.encode() for x in names])
        paths = (C.c_char_p * max(B, 1))(*[os.fspath(x).encode() for x in bucket_paths])
        ln = np.ascontiguousarray(lengths, np.int64)
        bk = np.ascontiguousarray(buckets, np.int32)
        counts = np.zeros(4, np.int64)
        per_bucket = np.zeros(max(B, 1), np.int64)
        det = np.zeros(max(R, 1), np.uint8)
        miss = C.create_string_buffer(4096)
        rc = lib().umiclust_bam_split(self._ctx._h, kp, R, nm, _i64(ln), bk.ctypes.data_as(P(C.c_int32)), B, paths,
                                      overlap, s5, s3, _i64(counts), _i64(per_bucket), det.ctypes.data_as(P(C.c_uint8)),
                                      miss, 4096)
        if rc == -74 and miss.value:
            raise KeyError(miss.value.decode())
        self._ctx._check(rc, "bam_split")
        return counts, per_bucket[:B], det[:R]

    def split_extract(self, keep, names, lengths, buckets, bucket_umi_paths, overlap: float, s5: int, s3: int, a5: int,
                      a3: int, k: int, fwd: str, rev: str):
        """umiclust_bam_split_extract (row f4+f1): split() and extract_umis_file in one pass, the
        detected-UMI records of bucket b in bucket_umi_paths[b] (truncated) and no region FASTA.  (counts[4],
        reads_per_bucket, umis_per_bucket, region_detected); KeyError(name) as split() raises it, no file written."""
        R, B = len(names), len(bucket_umi_paths)
        P = C.POINTER
        kp = None
        if keep is not None:
            keep = np.ascontiguousarray(np.asarray(keep) != 0, np.uint8)
            if len(keep) != self.n:
                raise ValueError("keep needs one entry per record")
            kp = keep.ctypes.data_as(P(C.c_uint8))
        nm = (C.c_char_p * max(R, 1))(*[x.encode() for x in names])
        paths = (C.c_char_p * max(B, 1))(*[os.fspath(x).encode() for x in bucket_umi_paths])
        ln = np.ascontiguousarray(lengths, np.int64)
        bk = np.ascontiguousarray(buckets, np.int32)
        counts = np.zeros(4, np.int64)
        per_bucket, umis = np.zeros(max(B, 1), np.int64), np.zeros(max(B, 1), np.int64)
        det = np.zeros(max(R, 1), np.uint8)
        miss = C.create_string_buffer(4096)
        rc = lib().umiclust_bam_split_extract(
            self._ctx._h, kp, R, nm, _i64(ln), bk.ctypes.data_as(P(C.c_int32)), B, paths, overlap, s5, s3, a5, a3, k,
            fwd.encode(), rev.encode(), _i64(counts), _i64(per_bucket), _i64(umis), det.ctypes.data_as(P(C.c_uint8)),
            miss, 4096)
        if rc == -74 and miss.value:
            raise KeyError(miss.value.decode())
        self._ctx._check(rc, "bam_split_extract")
        return counts, per_bucket[:B], umis[:B], det[:R]

    def name_suffix(self) -> tuple[np.ndarray, np.ndarray]:
        """umiclust_bam_name_suffix: per record (value, status) of the query name's last "_" field; status 0 where the
        field is not 1..18 ASCII digits and int() has to decide."""
        value, status = np.zeros(self.n, np.int64), np.zeros(self.n, np.uint8)
        self._ctx._check(lib().umiclust_bam_name_suffix(self._ctx._h, _i64(value),
                                                        status.ctypes.data_as(C.POINTER(C.c_uint8))), "bam_name_suffix")
        return value, status

    def close(self) -> None:
        if self._ctx is not None:
            self._ctx._check(lib().umiclust_bam_close(self._ctx._h), "bam_close")
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
