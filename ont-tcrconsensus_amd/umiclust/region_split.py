"""Drop-in for filter_and_split_reads_by_region_cluster of /root/reference/ont_tcr_consensus/region_split.py
(:219-333): the region binning that produces the hot path's shards.

Same signature, defaults, files (append-mode region_cluster<k>.fasta, the
<bam>_filter_and_split_reads_by_region_cluster.err log) and return value (the list of cluster FASTA paths, a
set's order).  The BAM record loop runs in the library (umiclust_region_split: BGZF inflated on the device, DESIGN.md
§9e, records classified and FASTA records built on the GPU); the log is formatted here with the same
Python expressions as the reference.  No CPU fallback.

Also the round-2 function of the same file, filter_and_split_reads_by_region (:336-435, row f4b): one
append-mode region_<name>.fasta per reference name, no cluster lookup, the
<bam>_filter_and_split_reads_by_region.err log.  It runs on a BAM session (umiclust_bam_open + umiclust_bam_split),
so that minimap2_align.filter_consensus_alignments_and_split can split the session that filtered the consensus BAM.

The round-1 functions have session forms too: filter_and_split_reads_by_region_cluster_from and
filter_split_and_extract_umis_from take an open session -- the one minimap2_align.minimap2_ont_align_session returns --
in place of the BAM path, so that the raw-read alignments are parsed and scanned once and no BAM is read back.
"""
from __future__ import annotations

import collections
import json
import os
from typing import Union

import numpy as np

from . import vsearch_umi_cluster as _v
from .extract_umis import UMI_FWD_DEFAULT, UMI_REV_DEFAULT

NEGATIVE_CONTROL_SUFFIXES = ("_v_n", "cdr3j_n", "full_n")  # region_split.py:305


def _fasta_entries(path):
    """(name, sequence) of a FASTA file as pysam.FastxFile yields them (name = header up to whitespace)."""
    name, parts = None, []
    with open(path) as fh:
        for line in fh:
            line = line.rstrip("\n")
            if line.startswith(">"):
                if name is not None:
                    yield name, "".join(parts)
                toks = line[1:].split()
                name, parts = (toks[0] if toks else ""), []
            elif name is not None:
                parts.append(line.strip())
    if name is not None:
        yield name, "".join(parts)


def generate_regions_set_from_ref_fa(reference, remove_negative_control_regions=False,
                                     negative_control_regions_suffix_str_tuple=None):
    """region_split.py:29-49."""
    if remove_negative_control_regions:
        return {n for n, _ in _fasta_entries(reference) if not n.endswith(negative_control_regions_suffix_str_tuple)}
    return {n for n, _ in _fasta_entries(reference)}


def generate_region_length_dict_from_ref_fa(reference):
    """region_split.py:52-58."""
    return {n: len(s) for n, s in _fasta_entries(reference)}


def filter_and_split_reads_by_region_cluster(bam_file: Union[str, os.PathLike[str]],
                                             region_cluster_dict_json: Union[str, os.PathLike[str]],
                                             reference: Union[str, os.PathLike[str]],
                                             logs_dir: Union[str, os.PathLike[str]],
                                             region_fasta_out_dir: Union[str, os.PathLike[str]],
                                             minimal_region_overlap: float = 0.95, max_softclip_5_end: int = 73,
                                             max_softclip_3_end: int = 68):
    log_file = os.path.join(logs_dir,
                            os.path.basename(bam_file).split(".")[0] + "_filter_and_split_reads_by_region_cluster.err")
    with open(region_cluster_dict_json, "r") as json_in:
        region_cluster_dict = json.load(json_in)
    region_length_dict = generate_region_length_dict_from_ref_fa(reference=reference)
    names = list(region_length_dict)
    counts, per_cluster, detected = _v.context().region_split(
        os.fspath(bam_file), names, [region_length_dict[n] for n in names],
        [int(region_cluster_dict[n]) if n in region_cluster_dict else -1 for n in names], minimal_region_overlap,
        max_softclip_5_end, max_softclip_3_end, os.fspath(region_fasta_out_dir))
    clusters = _write_region_cluster_log(log_file, reference, names, counts, per_cluster, detected)
    return list({os.path.join(region_fasta_out_dir, "region_cluster{}.fasta".format(k)) for k in clusters})


def _write_region_cluster_log(log_file, reference, names, counts, per_cluster, detected):
    """The <bam>_filter_and_split_reads_by_region_cluster.err log, as region_split.py:285-331 builds it from the loop's
    counters; returns the clusters that got a read, in the order of the reference's counter."""
    n_unmapped, n_primary_mapped, n_short, n_long = (int(x) for x in counts)
    n_reads_region_cluster_counter = collections.defaultdict(int)
    for k, v in enumerate(per_cluster):
        if v:
            n_reads_region_cluster_counter[k] = int(v)
    detected_regions_set = {names[r] for r, d in enumerate(detected) if d}

    logging_str = "Total # primary alignments in bam file: " + str(n_primary_mapped) + "\n"
    logging_str += (
        "median # of primary alignments in region clusters that have minimal region overlap and are not too long: "
        + str(round(np.median(list(n_reads_region_cluster_counter.values())), 3)) + "\n")
    logging_str += ("% of primary alignments that have shorter overlap than minimal region overlap: "
                    + str(round(100 * n_short / n_primary_mapped, 2)) + "\n")
    logging_str += "% of primary alignments that have too long reads: " + str(round(100 * n_long / n_primary_mapped, 2)) + "\n"
    regions_set = generate_regions_set_from_ref_fa(reference=reference, remove_negative_control_regions=True,
                                                   negative_control_regions_suffix_str_tuple=NEGATIVE_CONTROL_SUFFIXES)
    detected_regions_set = set([r for r in detected_regions_set if not r.endswith(NEGATIVE_CONTROL_SUFFIXES)])
    fraction_regions_detected = len(regions_set.intersection(detected_regions_set)) / len(regions_set)
    number_missing_regions = len(regions_set.difference(detected_regions_set))
    missing_regions = regions_set.difference(detected_regions_set)
    logging_str += ("fraction detected regions of total regions in reference in initial non-polished read alignments: "
                    + str(round(fraction_regions_detected, 4)) + "\n")
    logging_str += ("# of missing regions from reference in initial non-polished read alignments: "
                    + str(number_missing_regions) + "\n")
    logging_str += ("missing/non-detected regions from reference in initial non-polished read alignments: "
                    + str(missing_regions) + "\n")
    with open(log_file, "w") as ferr:
        ferr.write(logging_str)
    del n_unmapped
    return list(n_reads_region_cluster_counter)


def filter_split_and_extract_umis(bam_file: Union[str, os.PathLike[str]],
                                  region_cluster_dict_json: Union[str, os.PathLike[str]],
                                  reference: Union[str, os.PathLike[str]], logs_dir: Union[str, os.PathLike[str]],
                                  umi_fasta_out_dir: Union[str, os.PathLike[str]],
                                  minimal_region_overlap: float = 0.95, max_softclip_5_end: int = 73,
                                  max_softclip_3_end: int = 68, adapter_length_5_end: int = None,
                                  adapter_length_3_end: int = None, max_pattern_dist: int = 3,
                                  umi_fwd: str = UMI_FWD_DEFAULT, umi_rev: str = UMI_REV_DEFAULT):
    """filter_and_split_reads_by_region_cluster followed by extract_umis(write_region=True) on every file it returns
    (tcr_consensus.py:190-223; row f4+f1), in one pass over the BAM (umiclust_region_split_extract):
    the same .err log and the same region_cluster<k>_detected_umis.fasta files in umi_fasta_out_dir, but no region
    FASTA is written or read.  The adapter lengths default to the soft-clip lengths, as the pipeline passes them.
    Returns the UMI FASTA paths that hold a record -- the pipeline's filtered_umi_fasta_list -- in a set's order."""
    log_file = os.path.join(logs_dir,
                            os.path.basename(bam_file).split(".")[0] + "_filter_and_split_reads_by_region_cluster.err")
    with open(region_cluster_dict_json, "r") as json_in:
        region_cluster_dict = json.load(json_in)
    region_length_dict = generate_region_length_dict_from_ref_fa(reference=reference)
    names = list(region_length_dict)
    counts, per_cluster, umis, detected = _v.context().region_split_extract(
        os.fspath(bam_file), names, [region_length_dict[n] for n in names],
        [int(region_cluster_dict[n]) if n in region_cluster_dict else -1 for n in names], minimal_region_overlap,
        max_softclip_5_end, max_softclip_3_end,
        max_softclip_5_end if adapter_length_5_end is None else adapter_length_5_end,
        max_softclip_3_end if adapter_length_3_end is None else adapter_length_3_end, max_pattern_dist, umi_fwd,
        umi_rev, os.fspath(umi_fasta_out_dir))
    _write_region_cluster_log(log_file, reference, names, counts, per_cluster, detected)
    return list({os.path.join(umi_fasta_out_dir, "region_cluster{}_detected_umis.fasta".format(k))
                 for k, v in enumerate(umis) if v})


def _round1_inputs(bam_file, region_cluster_dict_json, reference, logs_dir):
    """log path, region names, lengths and clusters as the round-1 functions above hand them to the library"""
    log_file = os.path.join(logs_dir,
                            os.path.basename(bam_file).split(".")[0] + "_filter_and_split_reads_by_region_cluster.err")
    with open(region_cluster_dict_json, "r") as json_in:
        region_cluster_dict = json.load(json_in)
    region_length_dict = generate_region_length_dict_from_ref_fa(reference=reference)
    names = list(region_length_dict)
    return (log_file, names, [region_length_dict[n] for n in names],
            [int(region_cluster_dict[n]) if n in region_cluster_dict else -1 for n in names])


def filter_and_split_reads_by_region_cluster_from(src, bam_file, region_cluster_dict_json, reference, logs_dir,
                                                  region_fasta_out_dir, minimal_region_overlap: float = 0.95,
                                                  max_softclip_5_end: int = 73, max_softclip_3_end: int = 68):
    """filter_and_split_reads_by_region_cluster over an open BAM session `src` (a _lib.BamSession, from bam_open or
    sam_open) instead of the file: the same region_cluster<k>.fasta files, the same log -- named after `bam_file`, which
    need not exist -- and the same return value (umiclust_bam_region_split)."""
    log_file, names, lengths, clusters = _round1_inputs(bam_file, region_cluster_dict_json, reference, logs_dir)
    counts, per_cluster, detected = src.region_split(names, lengths, clusters, minimal_region_overlap,
                                                     max_softclip_5_end, max_softclip_3_end,
                                                     os.fspath(region_fasta_out_dir))
    kept = _write_region_cluster_log(log_file, reference, names, counts, per_cluster, detected)
    return list({os.path.join(region_fasta_out_dir, "region_cluster{}.fasta".format(k)) for k in kept})


def filter_split_and_extract_umis_from(src, bam_file, region_cluster_dict_json, reference, logs_dir, umi_fasta_out_dir,
                                       minimal_region_overlap: float = 0.95, max_softclip_5_end: int = 73,
                                       max_softclip_3_end: int = 68, adapter_length_5_end: int = None,
                                       adapter_length_3_end: int = None, max_pattern_dist: int = 3,
                                       umi_fwd: str = UMI_FWD_DEFAULT, umi_rev: str = UMI_REV_DEFAULT):
    """filter_split_and_extract_umis over an open BAM session `src` instead of the file: the same log, named after
    `bam_file`, the same region_cluster<k>_detected_umis.fasta files and the same return value
    (umiclust_bam_region_split_extract).  With the session of minimap2_ont_align_session this is the
    whole of tcr_consensus.py:170-223 on one parse and one scan, with no BAM in between."""
    log_file, names, lengths, clusters = _round1_inputs(bam_file, region_cluster_dict_json, reference, logs_dir)
    counts, per_cluster, umis, detected = src.region_split_extract(
        names, lengths, clusters, minimal_region_overlap, max_softclip_5_end, max_softclip_3_end,
        max_softclip_5_end if adapter_length_5_end is None else adapter_length_5_end,
        max_softclip_3_end if adapter_length_3_end is None else adapter_length_3_end, max_pattern_dist, umi_fwd,
        umi_rev, os.fspath(umi_fasta_out_dir))
    _write_region_cluster_log(log_file, reference, names, counts, per_cluster, detected)
    return list({os.path.join(umi_fasta_out_dir, "region_cluster{}_detected_umis.fasta".format(k))
                 for k, v in enumerate(umis) if v})


def filter_and_split_reads_by_region_from(src, keep, bam_file, reference, logs_dir, region_fasta_out_dir,
                                          minimal_region_overlap=0.95, max_softclip_5_end=73, max_softclip_3_end=68):
    """filter_and_split_reads_by_region (region_split.py:336-435) over an open BAM session `src` (a _lib.BamSession, or
    any object with its attributes and split()): the records with keep[r] != 0 (keep None: all) are the file.  One
    append-mode region_<name>.fasta per reference name, the <bam>_filter_and_split_reads_by_region.err log named after
    `bam_file`, and the list of the FASTA paths written, in a set's order.  Pinned by tests/golden/by_region, which
    the reference's own function produced."""
    log_file = os.path.join(logs_dir, os.path.basename(bam_file).split(".")[0] + "_filter_and_split_reads_by_region.err")
    region_length_dict = generate_region_length_dict_from_ref_fa(reference=reference)
    names = list(region_length_dict)
    paths = [os.path.join(region_fasta_out_dir, "region_{}.fasta".format(n)) for n in names]
    try:
        counts, per_region, detected = src.split(keep, names, [region_length_dict[n] for n in names],
                                                 list(range(len(names))), paths, minimal_region_overlap,
                                                 max_softclip_5_end, max_softclip_3_end)
    except KeyError:
        _split_key_error(src, keep, region_length_dict)
        raise
    _write_region_log(log_file, reference, names, counts, per_region, detected)
    return list({paths[r] for r, v in enumerate(per_region) if v})


def _split_key_error(src, keep, region_length_dict):
    """The KeyError of the reference's loop, after the library's: the reference looks the region up for every primary
    record, before either filter (:374), so the first one whose reference name the FASTA lacks raises, and a refID of
    -1 is the name None, not the string 'None'."""
    ref = np.asarray(src.ref)
    primary = np.asarray(src.cls) == 2
    if keep is not None:
        primary &= np.asarray(keep) != 0
    for r in np.flatnonzero(primary).tolist():
        name = src.ref_names[ref[r]] if 0 <= ref[r] < len(src.ref_names) else None
        if name not in region_length_dict:
            raise KeyError(name) from None


def _write_region_log(log_file, reference, names, counts, per_region, detected):
    """The <bam>_filter_and_split_reads_by_region.err log, as region_split.py:397-430 builds it."""
    n_unmapped, n_primary_mapped, n_short, n_long = (int(x) for x in counts)
    n_reads_region_counter = {names[r]: int(v) for r, v in enumerate(per_region) if v}
    detected_regions_set = {names[r] for r, d in enumerate(detected) if d}

    logging_str = "Total # primary alignments in bam file: " + str(n_primary_mapped) + "\n"
    logging_str += ("median # of primary alignments in regions that have minimal region overlap and are not too long: "
                    + str(round(np.median(list(n_reads_region_counter.values())), 3)) + "\n")
    logging_str += ("% of primary alignments that have shorter overlap than minimal region overlap: "
                    + str(round(100 * n_short / n_primary_mapped, 2)) + "\n")
    logging_str += "% of primary alignments that have too long reads: " + str(round(100 * n_long / n_primary_mapped, 2)) + "\n"
    regions_set = generate_regions_set_from_ref_fa(reference=reference, remove_negative_control_regions=True,
                                                   negative_control_regions_suffix_str_tuple=NEGATIVE_CONTROL_SUFFIXES)
    detected_regions_set = set([r for r in detected_regions_set if not r.endswith(NEGATIVE_CONTROL_SUFFIXES)])
    fraction_regions_detected = len(regions_set.intersection(detected_regions_set)) / len(regions_set)
    number_missing_regions = len(regions_set.difference(detected_regions_set))
    missing_regions = regions_set.difference(detected_regions_set)
    logging_str += "fraction detected regions of total regions in reference: " + str(round(fraction_regions_detected, 4)) + "\n"
    logging_str += "# of missing regions from reference: " + str(number_missing_regions) + "\n"
    logging_str += "missing/non-detected regions from reference: " + str(missing_regions) + "\n"
    with open(log_file, "w") as ferr:
        ferr.write(logging_str)
    del n_unmapped


def filter_split_and_extract_umis_by_region_from(src, keep, bam_file, reference, logs_dir, umi_fasta_out_dir,
                                                 minimal_region_overlap=0.95, max_softclip_5_end=73,
                                                 max_softclip_3_end=68, adapter_length_5_end=None,
                                                 adapter_length_3_end=None, max_pattern_dist=3,
                                                 umi_fwd=UMI_FWD_DEFAULT, umi_rev=UMI_REV_DEFAULT):
    """filter_and_split_reads_by_region_from followed by extract_umis(write_region=True) on every file it returns
    (tcr_consensus.py:376-403; row f4+f1), in one pass over the session (umiclust_bam_split_extract):
    the same .err log and the same detected-UMI files, no region FASTA.  A region's file is named as extract_umis names
    it after region_<name>.fasta: "region_<name>" up to its first ".", then "_detected_umis.fasta"; two regions whose
    names give one path are a ValueError (the reference lets one file overwrite the other).  Returns the UMI FASTA
    paths that hold a record, in a set's order."""
    log_file = os.path.join(logs_dir, os.path.basename(bam_file).split(".")[0] + "_filter_and_split_reads_by_region.err")
    region_length_dict = generate_region_length_dict_from_ref_fa(reference=reference)
    names = list(region_length_dict)
    paths = [os.path.join(umi_fasta_out_dir,
                          os.path.basename("region_{}.fasta".format(n)).split(".")[0] + "_detected_umis.fasta")
             for n in names]
    if len(set(paths)) != len(paths):
        raise ValueError("two regions share one detected-UMI file name")
    try:
        counts, per_region, umis, detected = src.split_extract(
            keep, names, [region_length_dict[n] for n in names], list(range(len(names))), paths,
            minimal_region_overlap, max_softclip_5_end, max_softclip_3_end,
            max_softclip_5_end if adapter_length_5_end is None else adapter_length_5_end,
            max_softclip_3_end if adapter_length_3_end is None else adapter_length_3_end, max_pattern_dist, umi_fwd,
            umi_rev)
    except KeyError:
        _split_key_error(src, keep, region_length_dict)
        raise
    _write_region_log(log_file, reference, names, counts, per_region, detected)
    return list({paths[r] for r, v in enumerate(umis) if v})


def filter_and_split_reads_by_region(bam_file: Union[str, os.PathLike[str]], reference: Union[str, os.PathLike[str]],
                                     logs_dir: Union[str, os.PathLike[str]],
                                     region_fasta_out_dir: Union[str, os.PathLike[str]],
                                     minimal_region_overlap: float = 0.95, max_softclip_5_end: int = 73,
                                     max_softclip_3_end: int = 68):
    """region_split.py:336-435 -- same signature, defaults, files and return value.  The file is read by a BAM session
    (umiclust_bam_open), which also walks the aux tags of its primary records and groups their cs strings; the split
    needs neither, but the reference calls this function on the filtered consensus BAM alone, a small file, and
    minimap2_align.filter_consensus_alignments_and_split splits the filter's own session without reading it again."""
    with _v.context().bam_open(os.fspath(bam_file)) as src:
        return filter_and_split_reads_by_region_from(src, None, bam_file, reference, logs_dir, region_fasta_out_dir,
                                                     minimal_region_overlap, max_softclip_5_end, max_softclip_3_end)
