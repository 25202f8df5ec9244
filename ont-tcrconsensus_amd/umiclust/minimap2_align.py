"""Drop-ins for the per-record loops of ont_tcr_consensus/minimap2_align.py:
count_cs_tags (:21-37), the cs-tag log blocks of minimap2_ont_align (:141-150), filter_consensus_alignments
(:158-359) and estimate_precision_at_num_subreads (:362-435, row f6b); and
filter_consensus_alignments_and_split, which runs the filter and the round-2 split of region_split.py:336-435 on one
session.

The BAM is read once by a session of the library (umiclust_bam_open: BGZF inflated on the device, DESIGN.md §9e,
every record scanned and the cs:Z strings grouped exactly on the GPU); this module only forms the reference's floats and
text from the integer columns, with the same Python and numpy expressions as the reference, so values and their
repr are equal by construction.  It needs numpy only (no pysam, no pandas).  No CPU fallback: the columns come from
the device, or -- in the CPU tests -- from any object with the attributes of _lib.BamSession.
"""
from __future__ import annotations

import collections
import csv
import os
import subprocess
from typing import Union

import numpy as np

from . import vsearch_umi_cluster as _v
from .extract_umis import UMI_FWD_DEFAULT, UMI_REV_DEFAULT
from .region_split import (filter_and_split_reads_by_region_from, filter_split_and_extract_umis_by_region_from,
                           generate_region_length_dict_from_ref_fa)

PRIMARY = 2  # the cls column: 0 unmapped, 1 secondary or supplementary, 2 primary mapped


def _blast_id(src, r: int) -> float:
    """calculate_blast_id (:13-18) of record r from its integer columns."""
    if not src.nm_present[r]:
        raise KeyError("tag 'NM' not present")  # pysam's get_tag message, restated
    cols = int(src.cols[r])  # Python ints: the quotient is Python's own true division, ZeroDivisionError included
    return (cols - int(src.nm[r])) / cols


def _reference_name(src, r: int):
    ref = int(src.ref[r])
    return src.ref_names[ref] if 0 <= ref < len(src.ref_names) else None


def _census(src, keep=None):
    """The primary records with a cs tag (among keep): their indices, and per distinct tag its group id, the
    position of its first record and its count -- first-seen order is the order of `first`."""
    mask = (np.asarray(src.cls) == PRIMARY) & (np.asarray(src.cs_group) >= 0)
    if keep is not None:
        mask &= np.asarray(keep) != 0
    sel = np.flatnonzero(mask)
    uniq, first, counts = np.unique(np.asarray(src.cs_group)[sel], return_index=True, return_counts=True)
    return sel, uniq, first, counts


class _Opened:
    """a path opens (and closes) a session on the process's device context; a session passes through"""

    def __init__(self, bam_file_or_session):
        self._own = isinstance(bam_file_or_session, (str, os.PathLike))
        self.src = _v.context().bam_open(os.fspath(bam_file_or_session)) if self._own else bam_file_or_session

    def __enter__(self):
        return self.src

    def __exit__(self, *a):
        if self._own:
            self.src.close()


def count_cs_tags(bam_file: Union[str, os.PathLike[str]]):
    """:21-37 -- the same three objects, keys inserted in first-seen order (Counter.most_common breaks ties by it)."""
    per_tag = collections.Counter()
    regions, identities = collections.defaultdict(collections.Counter), collections.defaultdict(collections.Counter)
    with _Opened(bam_file) as src:
        sel, uniq, first, counts = _census(src)
        order = np.argsort(first, kind="stable")
        tags = src.cs_strings(sel[first[order]])
        tag_of_group = {int(uniq[g]): tags[x] for x, g in enumerate(order)}
        # one pass in BAM order, as the reference's loop (:27-35): an exception leaves the counters as far as it got
        for r in sel.tolist():
            tag = tag_of_group[int(src.cs_group[r])]
            per_tag[tag] += 1
            regions[tag][_reference_name(src, r)] += 1
            identities[tag][_blast_id(src, r)] += 1
    return per_tag, regions, identities


def cs_tag_report(bam_file_or_session, keep=None, top: int = 40, sub: int = 4) -> str:
    """The three text blocks of :141-150 and :344-357 over the primary records (those with keep[r] != 0 when keep is
    given, i.e. the census of the file umiclust_bam_write(keep) leaves).  Only the top groups' strings are gathered
    and only their records are visited; the full dictionaries of count_cs_tags are never built."""
    with _Opened(bam_file_or_session) as src:
        sel, uniq, first, counts = _census(src, keep)
        # Counter.most_common(top): by count, ties in insertion (= first-seen) order
        order = sorted(range(len(uniq)), key=lambda x: (-int(counts[x]), int(first[x])))[:top]
        tags = src.cs_strings(sel[first[order]]) if order else []
        rank = {int(uniq[g]): x for x, g in enumerate(order)}
        region = [collections.Counter() for _ in order]
        blast = [collections.Counter() for _ in order]
        groups = np.asarray(src.cs_group)[sel]
        for r in sel[np.isin(groups, uniq[order])].tolist() if order else []:
            x = rank[int(src.cs_group[r])]
            region[x][_reference_name(src, r)] += 1
            blast[x][_blast_id(src, r)] += 1  # keyed on the Python float: (100, 50) and (200, 100) are one key
    out = ["\nTop %d most common cs tags:\n" % top]
    for x, g in enumerate(order):
        out.append(str((tags[x], int(counts[g]))) + "\n")
    out.append("\nTop %d most common regions counted for each of the top %d most common cs tags:\n" % (sub, top))
    for x in range(len(order)):
        out.append(str(tags[x]) + " " + str(region[x].most_common(sub)) + "\n")
    out.append("\nTop %d most common blast identities counted for each of the top %d most common cs tags:\n" % (sub, top))
    for x in range(len(order)):
        out.append(str(tags[x]) + " " + str(blast[x].most_common(sub)) + "\n")
    return "".join(out)


def write_cs_tag_report(fh, bam_file_or_session, keep=None, top: int = 40, sub: int = 4) -> None:
    """what a pipeline puts in place of :140-150: write_cs_tag_report(ferr, bam_file)"""
    fh.write(cs_tag_report(bam_file_or_session, keep=keep, top=top, sub=sub))


def _write(src, keep, path, index: bool) -> int:
    """src.write, asking for the .bai only where it is wanted: a source without one keeps working"""
    return src.write(keep, path, index=True) if index else src.write(keep, path)


def samtools_sort(sam_file: Union[str, os.PathLike[str]], bam_file: Union[str, os.PathLike[str]],
                  index: bool = False) -> int:
    """`samtools sort -o bam_file sam_file` (:133-137) on the device (umiclust_sam_open): the text --
    a file, a FIFO or /dev/fd/N -- parsed, encoded and coordinate-sorted, every record written.  Returns their number.
    index=True also writes bam_file + ".bai" from the same session (`samtools index`, :138)."""
    with _v.context().sam_open(os.fspath(sam_file)) as src:
        return _write(src, np.ones(src.n, np.uint8), bam_file, index)


def samtools_index(bam_file: Union[str, os.PathLike[str]]) -> int:
    """`samtools index bam_file` (:138, :247) on the device (umiclust_bam_index_file): bam_file +
    ".bai".  Returns the number of records."""
    return _v.context().bam_index_file(os.fspath(bam_file))


def samtools_flagstat(bam_file_or_session, out_path: Union[str, os.PathLike[str]]) -> dict:
    """`samtools flagstat bam_file > out_path` (:152-153) on the device (umiclust_bam_flagstat), from a
    file or from an open session.  Returns the counters, {row: (QC-passed, QC-failed)}."""
    with _Opened(bam_file_or_session) as src:
        counters, text = src.flagstat()
    with open(out_path, "w") as fh:
        fh.write(text)
    return counters


def minimap2_ont_align_session(fastx: Union[str, os.PathLike[str]], reference: Union[str, os.PathLike[str]],
                               logs_dir: Union[str, os.PathLike[str]], minimap2_threads: int,
                               minimap2_params: str = None, bam_file: Union[str, os.PathLike[str]] = None,
                               index: bool = False, flagstat: bool = False):
    """minimap2_ont_align (:76-155) without the BAM in the middle: minimap2 runs with the reference's argv and its
    stderr in the same <fastx>_minimap2.err log; its SAM output is read from the pipe by umiclust_sam_open, which
    parses, encodes and coordinate-sorts it on the device; the three cs-tag blocks of :140-150 are appended to the log
    from that session; and the open session is returned, for region_split.filter_split_and_extract_umis_from and its
    like.  The sorted BAM is written only when bam_file is given; index=True (which needs bam_file) writes its .bai
    with it (`samtools index`, :138).  flagstat=True writes <logs_dir>/<name>_flagstat.out (:152-153) from the session,
    <name> being the BAM's as :86 forms it -- bam_file's, or the FASTX's where none is written.  DESIGN.md §9h."""
    if index and bam_file is None:
        raise ValueError("index=True needs bam_file: a .bai indexes a file")
    log_file = os.path.join(logs_dir, os.path.basename(fastx).split(".")[0] + "_minimap2")
    with open(log_file + ".err", "w") as ferr:
        minimap2_process = subprocess.Popen(
            [
                "minimap2",
                "-ax",
                "map-ont",
                "-k19",
                "-w 19",
                "-U50,500",
                "-g10k",
                "--end-bonus=10",
                "-t",
                str(minimap2_threads),
                "--cap-kalloc",
                "500m",
                minimap2_params if minimap2_params else "--cs",
                reference,
                fastx,
            ],
            stdout=subprocess.PIPE,
            stderr=ferr,
        )
        try:
            src = _v.context().sam_open("/dev/fd/%d" % minimap2_process.stdout.fileno())
        finally:
            minimap2_process.stdout.close()
            minimap2_process.wait()
        try:
            write_cs_tag_report(ferr, src)
            if bam_file is not None:
                _write(src, np.ones(src.n, np.uint8), bam_file, index)
            if flagstat:
                stem = os.path.basename(bam_file if bam_file is not None else fastx).split(".")[0]
                samtools_flagstat(src, os.path.join(logs_dir, stem + "_flagstat.out"))
        except Exception:
            src.close()
            raise
    return src


def _to_csv(path, columns, rows) -> None:
    """pandas.DataFrame(rows, columns=columns).to_csv(path, index=False): minimal quoting, floats as repr"""
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh, lineterminator="\n")
        w.writerow(columns)
        for row in rows:
            w.writerow([repr(v) if isinstance(v, float) else v for v in (row if isinstance(row, tuple) else (row,))])


def _flat(lists_by_key) -> list:
    """the values of a dict of lists, key by key in insertion order"""
    return [v for values in lists_by_key.values() for v in values]


def _pairs(lists_by_key) -> list:
    """(key, value) for every value of a dict of lists: the rows of the two-column CSVs"""
    return [(key, v) for key, values in lists_by_key.items() for v in values]


def _write_lines(fh, lines) -> None:
    """lines of (label, value, digits): label + str(value()), rounded to `digits` unless None; value None: the label
    alone.  A value is computed when its line is written, so an exception leaves the lines before it in the file."""
    for label, value, digits in lines:
        if value is None:
            fh.write(label + "\n")
            continue
        v = value()
        fh.write(label + str(v if digits is None else round(v, digits)) + "\n")


def filter_consensus_alignments_from(src, consensus_bam_file, reference, logs_dir, blast_id_threshold,
                                     minimal_region_overlap=0.9975, max_softclip_5_end=73, max_softclip_3_end=68,
                                     index="samtools"):
    """filter_consensus_alignments (:158-359) over the columns of `src` (a _lib.BamSession, or any object with its
    attributes): the decisions, the seven CSVs, the log and -- through src.write -- the filtered BAM.  Values and
    texts are pinned by tests/golden/bam_filter, which the reference's own function produced.  index: "samtools" runs
    `samtools index` on the filtered BAM as the reference does (:247); "device" has the session write the .bai with
    the BAM instead, and no subprocess runs."""
    return _filter_consensus_alignments(src, consensus_bam_file, reference, logs_dir, blast_id_threshold,
                                        minimal_region_overlap, max_softclip_5_end, max_softclip_3_end, index)[0]


def _filter_consensus_alignments(src, consensus_bam_file, reference, logs_dir, blast_id_threshold,
                                 minimal_region_overlap, max_softclip_5_end, max_softclip_3_end, index="samtools"):
    """filter_consensus_alignments_from, returning (filtered BAM path, keep): keep[r] != 0 for the records written"""
    if index not in ("samtools", "device"):
        raise ValueError("index is 'samtools' or 'device'")
    stem = os.path.basename(consensus_bam_file).split(".")[0]
    filtered = os.path.splitext(consensus_bam_file)[0] + "_filtered.bam"
    lengths = generate_region_length_dict_from_ref_fa(reference=reference)
    overlap, threshold, clip = minimal_region_overlap, blast_id_threshold, max_softclip_5_end + max_softclip_3_end

    # the record loop (:209-245) over the primary alignments in BAM order.  Per region, in first-seen order: the
    # bases missing from a too short overlap, the bases a too long read has in excess, the blast identities; and the
    # identities again per number of subreads (the query name's last "_" field)
    missing, excess, identity, by_subreads = (collections.defaultdict(list) for _ in range(4))
    n = dict(primary=0, short=0, long=0, sized=0, written=0)
    primary = np.flatnonzero(np.asarray(src.cls) == PRIMARY)
    names = src.query_names(primary)
    spans = np.asarray(src.reference_length)[primary].tolist()  # Python ints, so that every comparison and difference
    reads = np.asarray(src.l_seq)[primary].tolist()             # below is Python's int-with-float arithmetic
    keep = np.zeros(src.n, np.uint8)
    raised = None
    try:
        for j, r in enumerate(primary.tolist()):
            n["primary"] += 1
            region = _reference_name(src, r)
            need = lengths[region] * overlap  # KeyError(region): a reference that the FASTA does not hold
            if spans[j] < need:
                n["short"] += 1
                missing[region].append(need - spans[j])
                continue
            most = lengths[region] * (2 - overlap) + clip
            if reads[j] > most:
                n["long"] += 1
                excess[region].append(reads[j] - most)
                continue
            n["sized"] += 1
            x = _blast_id(src, r)
            identity[region].append(x)
            by_subreads[names[j].split("_")[-1]].append(x)
            if x > threshold:
                n["written"] += 1
                keep[r] = 1
    except (KeyError, ZeroDivisionError) as e:
        raised = e
    # the reference's output file is closed with what was written before the exception, and nothing else follows
    try:
        _write(src, keep, filtered, index == "device" and raised is None)  # :247 on the device: the .bai with the BAM
    except Exception:
        if raised is None:
            raise
    if raised is not None:
        raise raised
    if index == "samtools":
        subprocess.run(["samtools", "index", filtered])  # :247, kept as it is

    # the seven CSVs (:253-279), as DataFrame.to_csv(index=False) writes them
    for suffix, columns, rows in (
            ("_number_of_subreads_blast_id.csv", ["number_of_subreads", "blast_id"], _pairs(by_subreads)),
            ("_region_nt_too_short.csv", ["region", "number_of_nt"], _pairs(missing)),
            ("_region_nt_too_long.csv", ["region", "number_of_nt"], _pairs(excess)),
            ("_region_blast_id.csv", ["region", "blast_id"], _pairs(identity)),
            ("_nt_too_short.csv", ["number_of_nt"], _flat(missing)),
            ("_nt_too_long.csv", ["number_of_nt"], _flat(excess)),
            ("_blast_id.csv", ["blast_id"], _flat(identity))):
        _to_csv(os.path.join(logs_dir, stem + suffix), columns, rows)

    # the log (:281-357): labels are the reference's output text; values use numpy's median / quantile / mean / log10
    sizes, ids = list(lengths.values()), _flat(identity)
    pct = lambda part, whole: (lambda: 100 * n[part] / n[whole])  # noqa: E731
    quantile = lambda q: (lambda: np.quantile(ids, q))  # noqa: E731
    lines = [
        ("Consensus alignment filtering performed with the following parameters:", None, None),
        ("- minimal region overlap: ", lambda: overlap, None),
        ("- minimal blast identity with reference: ", lambda: threshold, None),
        ("From these parameters follows:", None, None),
        ("- Minimal Phred Q = ", lambda: -10 * np.log10(1 - threshold), 2),
        ("- Median region nucleotide length: ", lambda: np.median(sizes), None),
        ("- Median allowed too few nucleotides/region: ", lambda: np.median([L - L * overlap for L in sizes]), 2),
        ("- Median allowed too many nucleotides/region: ", lambda: np.median([L * (2 - overlap) - L for L in sizes]), 2),
        ("- Median allowed variants (i.e., indels and mismatches)/region: ",
         lambda: np.median([L - L * threshold for L in sizes]), 2),
        ("", None, None),
        ("Total # primary alignments in bam file before filtering: ", lambda: n["primary"], None),
        ("% of primary alignments that have shorter overlap than minimal region overlap: ", pct("short", "primary"), 2),
        ("% of primary alignments that have too long reads: ", pct("long", "primary"), 2),
        ("Median # of too few nucleotides of alignments that have shorter than minimal region overlap: ",
         lambda: np.median(_flat(missing)), 2),
        ("Median # of too many nucleotides of alignments that have longer than minimal region overlap: ",
         lambda: np.median(_flat(excess)), 2),
        ("Median blast identity of alignments: ", lambda: np.median(ids), 6),
        ("15th percentile blast identity of alignments: ", quantile(0.15), 6),
        ("25th percentile blast identity of alignments: ", quantile(0.25), 6),
        ("75th percentile blast identity of alignments: ", quantile(0.75), 6),
        ("Average blast identity of alignments: ", lambda: np.mean(ids), 6),
        ("Total # primary alignments written to filtered bam file: ", lambda: n["written"], None),
        ("% of primary alignments written to filtered bam file: ", pct("written", "primary"), 2),
        ("% primary alignments of primary alignments with minimal overlap written to filtered bam file: ",
         pct("written", "sized"), 2),
    ]
    with open(os.path.join(logs_dir, stem + "_bam_filter.log"), "w") as fh:
        _write_lines(fh, lines)
        # :341-357 re-reads the file it just wrote; its records are the kept ones of this session
        fh.write(cs_tag_report(src, keep=keep))
    return filtered, keep


def filter_consensus_alignments(consensus_bam_file: Union[str, os.PathLike[str]],
                                reference: Union[str, os.PathLike[str]], logs_dir: Union[str, os.PathLike[str]],
                                blast_id_threshold: float, minimal_region_overlap: float = 0.9975,
                                max_softclip_5_end: int = 73, max_softclip_3_end: int = 68, index: str = "samtools"):
    """:158-359 -- same signature, defaults, files and return value; index="device" writes the .bai of :247 from the
    session instead of running samtools."""
    with _Opened(consensus_bam_file) as src:
        return filter_consensus_alignments_from(src, consensus_bam_file, reference, logs_dir, blast_id_threshold,
                                                minimal_region_overlap, max_softclip_5_end, max_softclip_3_end, index)


def filter_consensus_alignments_and_split(consensus_bam_file: Union[str, os.PathLike[str]],
                                          reference: Union[str, os.PathLike[str]],
                                          logs_dir: Union[str, os.PathLike[str]], blast_id_threshold: float,
                                          region_fasta_out_dir: Union[str, os.PathLike[str]],
                                          minimal_region_overlap: float = 0.9975, max_softclip_5_end: int = 73,
                                          max_softclip_3_end: int = 68, index: str = "samtools"):
    """tcr_consensus.py's filter_consensus_alignments (:366-374) and filter_and_split_reads_by_region (:376-384) on one
    session: the filter runs as above (it still writes and indexes the filtered BAM), then the session's records are
    split under the filter's keep mask instead of the filtered BAM being read back.  The split takes the filter's
    overlap and softclip arguments, as :376-384 passes them, and names its log after the filtered BAM, as the two-step
    call does.  Returns (filtered BAM path, list of region_<name>.fasta paths)."""
    with _Opened(consensus_bam_file) as src:
        filtered, keep = _filter_consensus_alignments(src, consensus_bam_file, reference, logs_dir, blast_id_threshold,
                                                      minimal_region_overlap, max_softclip_5_end, max_softclip_3_end,
                                                      index)
        fastas = filter_and_split_reads_by_region_from(src, keep, filtered, reference, logs_dir, region_fasta_out_dir,
                                                       minimal_region_overlap, max_softclip_5_end, max_softclip_3_end)
    return filtered, fastas


def filter_consensus_alignments_split_and_extract(consensus_bam_file: Union[str, os.PathLike[str]],
                                                  reference: Union[str, os.PathLike[str]],
                                                  logs_dir: Union[str, os.PathLike[str]], blast_id_threshold: float,
                                                  umi_fasta_out_dir: Union[str, os.PathLike[str]],
                                                  minimal_region_overlap: float = 0.9975, max_softclip_5_end: int = 73,
                                                  max_softclip_3_end: int = 68, adapter_length_5_end: int = None,
                                                  adapter_length_3_end: int = None, max_pattern_dist: int = 3,
                                                  umi_fwd: str = UMI_FWD_DEFAULT, umi_rev: str = UMI_REV_DEFAULT,
                                                  index: str = "samtools"):
    """filter_consensus_alignments_and_split with the UMI extraction of tcr_consensus.py:386-403 fused into the split
    (row f4+f1): the filter runs as above, then the session's records are split under its keep mask and
    searched for their UMIs in one pass, so that region_<name>_detected_umis.fasta is written and no region FASTA is.
    The adapter lengths default to the soft-clip lengths, as the pipeline passes them.  Returns (filtered BAM path, list
    of the detected-UMI FASTA paths that hold a record)."""
    with _Opened(consensus_bam_file) as src:
        filtered, keep = _filter_consensus_alignments(src, consensus_bam_file, reference, logs_dir, blast_id_threshold,
                                                      minimal_region_overlap, max_softclip_5_end, max_softclip_3_end,
                                                      index)
        umi_fastas = filter_split_and_extract_umis_by_region_from(
            src, keep, filtered, reference, logs_dir, umi_fasta_out_dir, minimal_region_overlap, max_softclip_5_end,
            max_softclip_3_end, adapter_length_5_end, adapter_length_3_end, max_pattern_dist, umi_fwd, umi_rev)
    return filtered, umi_fastas


def estimate_precision_at_num_subreads_from(src, consensus_bam_file, reference, logs_dir, minimal_region_overlap=1.0,
                                            blast_id_threshold=1.0, max_softclip_5_end=73, max_softclip_3_end=68,
                                            num_subreads_threshold=6):
    """estimate_precision_at_num_subreads (:362-435) over the columns and name_suffix() of `src`: the CSV and the five
    printed lines.  Pinned by tests/golden/precision, which the reference's own function produced."""
    path = os.path.join(logs_dir, os.path.basename(consensus_bam_file).split(".")[0]
                        + "_precision_at_different_num_subreads.csv")
    lengths = generate_region_length_dict_from_ref_fa(reference=reference)
    overlap, clip = minimal_region_overlap, max_softclip_5_end + max_softclip_3_end
    primary = np.flatnonzero(np.asarray(src.cls) == PRIMARY)
    value, status = src.name_suffix()
    # a tail the device does not read as 1..18 digits goes through int() itself: its value or its ValueError
    odd = primary[np.asarray(status)[primary] == 0]
    odd_name = dict(zip(odd.tolist(), src.query_names(odd)))
    spans = np.asarray(src.reference_length)[primary].tolist()  # Python ints, as in the filter above
    reads = np.asarray(src.l_seq)[primary].tolist()
    mapped, written = collections.defaultdict(int), collections.defaultdict(int)
    n_primary = n_mapped_above = n_written_above = 0
    for j, r in enumerate(primary.tolist()):
        n_primary += 1
        num_subreads = int(odd_name[r].split("_")[-1]) if r in odd_name else int(value[r])
        mapped[num_subreads] += 1
        if num_subreads >= num_subreads_threshold:
            n_mapped_above += 1
        region = _reference_name(src, r)
        if spans[j] < lengths[region] * overlap:  # KeyError(region): a reference that the FASTA does not hold
            continue
        if reads[j] > lengths[region] * (2 - overlap) + clip:
            continue
        if _blast_id(src, r) >= blast_id_threshold:
            written[num_subreads] += 1
            if num_subreads >= num_subreads_threshold:
                n_written_above += 1
    # (Series(written) / Series(mapped)).fillna(0).sort_index().to_csv(header=True, index_label="num_subreads")
    _to_csv(path, ["num_subreads", "precision"], [(k, written[k] / mapped[k] if k in written else 0.0)
                                                  for k in sorted(mapped)])
    expanded = [k for k, count in mapped.items() for _ in range(count)]
    print(n_written_above, n_mapped_above)
    print("median # of subreads:", np.median(expanded))
    print("mean # of subreads:", np.mean(expanded))
    print("n primary mapped:", n_primary)
    print("Overall precision above " + str(num_subreads_threshold) + " is:", n_written_above / n_mapped_above)


def estimate_precision_at_num_subreads(consensus_bam_file: Union[str, os.PathLike[str]],
                                       reference: Union[str, os.PathLike[str]], logs_dir: Union[str, os.PathLike[str]],
                                       minimal_region_overlap: float = 1.0, blast_id_threshold: float = 1.0,
                                       max_softclip_5_end: int = 73, max_softclip_3_end: int = 68,
                                       num_subreads_threshold: int = 6):
    """:362-435 -- same signature, defaults, CSV and printed lines; no pandas."""
    with _Opened(consensus_bam_file) as src:
        return estimate_precision_at_num_subreads_from(src, consensus_bam_file, reference, logs_dir,
                                                       minimal_region_overlap, blast_id_threshold, max_softclip_5_end,
                                                       max_softclip_3_end, num_subreads_threshold)
