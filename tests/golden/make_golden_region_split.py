"""Generate tests/golden/region_split/*.json from the REFERENCE itself (run here, not on the GPU box): inputs
and outputs of filter_and_split_reads_by_region_cluster (/root/reference/ont_tcr_consensus/region_split.py:
219-333).

pysam is not installed (ordinary ModuleNotFoundError): pysam.AlignmentFile is replaced by the
BAM reader of oracle/bam.py (SAM/BAM specification restated) and pysam.FastxFile by make_golden.py's FASTA
iterator.  The BAM inputs are written by oracle/bam.py from the records stored in the fixture, so the fixture
holds data only (records, reference regions, parameters, output files).

Six cases are draws of make_case; the rest are hand-built (hand_cases) for what those draws never hold: names past
one 64-lane trip, every CIGAR op, every sequence code, kept records without a sequence, a region without a cluster,
records at both thresholds (with the rows where a fused multiply-add of the `too long` bound decides differently
from the reference's rounded product, asserted here in exact arithmetic), and a file without primary records.

Usage: python tests/golden/make_golden_region_split.py  (requires /root/reference)
"""
from __future__ import annotations

import json
import os
import random
import shutil
import string
import sys
import tempfile
from fractions import Fraction

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "oracle")]
import bam  # noqa: E402
import make_golden  # noqa: E402


def make_case(rng, name, n_regions, n_reads, minimal_region_overlap=0.95, s5=73, s3=68, pre_existing=False,
              unknown_ref=False, no_cigar_at=None):
    regions = []
    for r in range(n_regions):
        suffix = rng.choice(["", "", "", "_v_n", "cdr3j_n", "full_n"]) if r > 1 else ""
        regions.append((f"TRBV{r}_{rng.randint(1, 99)}{suffix}", rng.randint(300, 700)))
    clusters = {}
    k = 0
    for nm, _ in regions:  # some regions share a cluster (the homology clustering's output)
        if clusters and rng.random() < 0.3:
            clusters[nm] = rng.choice(list(clusters.values()))
        else:
            clusters[nm] = k
            k += 1
    refs = list(regions)
    if unknown_ref:
        refs.append(("not_in_reference", 500))
    records = []
    for i in range(n_reads):
        ref = rng.randrange(len(refs))
        rlen = refs[ref][1]
        kind = rng.random()
        flag = 0
        if kind < 0.05:
            flag = 4
        elif kind < 0.1:
            flag = 256
        elif kind < 0.13:
            flag = 2048
        if rng.random() < 0.5:
            flag |= 16
        aln = int(rlen * rng.choice([1.0, 0.99, 0.97, 0.96, 0.9, 0.6])) if flag & 4 == 0 else 0
        clip5, clip3 = rng.randint(0, 90), rng.randint(0, 80)
        extra = rng.choice([0, 0, 0, 5, rlen])  # an occasional far-too-long read
        cigar = ([("S", clip5)] if clip5 else []) + [("M", aln + extra)] + ([("S", clip3)] if clip3 else []) \
            if aln else []
        if aln and rng.random() < 0.3:
            cigar = cigar[:-1] + [("D", 3), ("I", 2)] + cigar[-1:]
        qlen = sum(ln for op, ln in cigar if op in "MIS=X") if cigar else rng.randint(50, 300)
        alpha = "ACGTN" if rng.random() < 0.1 else "ACGT"
        seq = "".join(rng.choice(alpha) for _ in range(qlen))
        if flag & 256 and rng.random() < 0.5:
            seq = ""  # secondary without a stored sequence
        records.append(dict(name=f"read{i:05d}", flag=flag, ref=ref if not flag & 4 or rng.random() < 0.5 else -1,
                            pos=rng.randint(0, 20), cigar=cigar, seq=seq))
        if i == no_cigar_at:  # a mapped primary record without a CIGAR: reference_length 1 (htslib bam_endpos)
            records[-1].update(flag=16, ref=0, cigar=[])
    pre = {}
    if pre_existing:  # the reference appends to region_cluster<k>.fasta
        pre = {f"region_cluster{clusters[regions[0][0]]}.fasta": ">old;strand=+\nACGT\n"}
    return dict(name=name, regions=regions, refs=refs, clusters=clusters, records=records, pre_existing=pre,
                minimal_region_overlap=minimal_region_overlap, max_softclip_5_end=s5, max_softclip_3_end=s3)


# ---------------------------------------------------------------- hand-built cases: what make_case never draws
NAME_CHARS = string.ascii_letters + string.digits + "_-:/.#+|"
DEFAULT_REGIONS = [("TRBV1_1", 60), ("TRBV2_2", 60)]


def _seq(rng, n, alpha="ACGT"):
    return "".join(rng.choice(alpha) for _ in range(n))


def _cigar(span, qlen):
    """Reference span `span` and query length `qlen`: M for what they share, then D or S for the difference."""
    m = min(span, qlen)
    return ([("M", m)] if m else []) + ([("D", span - m)] if span > m else []) + ([("S", qlen - m)] if qlen > m else [])


def _rec(name, flag, ref, cigar, seq, pos=0):
    return dict(name=name, flag=flag, ref=ref, pos=pos, cigar=cigar, seq=seq)


def _case(name, regions, records, clusters=None, ov=0.95, s5=73, s3=68):
    if clusters is None:
        clusters = {nm: k for k, (nm, _) in enumerate(regions)}
    return dict(name=name, regions=list(regions), refs=list(regions), clusters=clusters, records=records,
                pre_existing={}, minimal_region_overlap=ov, max_softclip_5_end=s5, max_softclip_3_end=s3)


def long_bounds(length, ov, slack):
    """The `too long` bound as the reference evaluates it (product rounded to a double, then the add) and as one
    fused multiply-add would (the exact value, rounded once)."""
    return length * (2 - ov) + slack, float(Fraction(length) * Fraction(2 - ov) + slack)


def name_lengths_case(rng):
    """Kept reads on both strands whose names run to 1, 63, 64, 65, 128 and 254 bytes (l_read_name <= 255): the
    64-lane name loop of the emit kernel takes one to four trips."""
    records = []
    for ln in (1, 63, 64, 65, 128, 254):
        for flag in (0, 16):
            name = "".join(rng.choice(NAME_CHARS) for _ in range(ln))
            records.append(_rec(name, flag, len(records) % 2, _cigar(60, 60), _seq(rng, 60)))
    return _case("name_lengths", DEFAULT_REGIONS, records)


def cigar_ops_case(rng):
    """Every CIGAR op; region length 100, so a reference span of 95 passes.  The span comes from M D N = X alone."""
    regions = [("TRBV7_9", 100), ("TRBV5_1", 100)]
    every = [("H", 5), ("S", 3), ("M", 30), ("I", 2), ("D", 3), ("N", 10), ("P", 2), ("=", 30), ("X", 22), ("S", 4),
             ("H", 6)]  # span 30 + 3 + 10 + 30 + 22 = 95, query 3 + 30 + 2 + 30 + 22 + 4 = 91
    cigars = [("every_op", every, 91),
              ("span_from_N", [("S", 20), ("N", 96), ("S", 20)], 40),
              ("span_from_N_short", [("S", 20), ("N", 94), ("S", 20)], 40),
              ("span_from_eq", [("=", 97)], 97),
              ("span_from_X", [("X", 95)], 95),
              ("span_from_X_short", [("X", 94)], 94),
              ("span_from_D", [("I", 40), ("D", 95)], 40),
              ("hard_clips", [("H", 10), ("M", 96), ("H", 7)], 96),
              ("hard_and_soft", [("H", 1), ("S", 9), ("M", 100), ("S", 8), ("H", 2)], 117),
              ("only_I_S", [("S", 10), ("I", 30), ("S", 5)], 45),  # reference_length 1: short
              ("only_H_P", [("H", 5), ("P", 3), ("H", 5)], 30),  # the same
              ("pad_inside", [("M", 50), ("P", 4), ("M", 50)], 100)]
    records = []
    for nm, cg, qlen in cigars:
        for flag in (0, 16):
            records.append(_rec(f"{nm}_{'r' if flag else 'f'}", flag, len(records) % 2, cg, _seq(rng, qlen)))
    return _case("cigar_ops", regions, records)


def iupac_seq_case(rng):
    """All 16 sequence codes on both strands; l_seq 1, 2, 63, 64, 65, 127 (odd and even, either side of the emit
    kernel's 64-lane stride).  The stand-in's get_forward_sequence complements A C G T only (N, X and every other
    code unchanged): this pins pysam's table as oracle/bam.py restates it, not pysam itself."""
    records = []
    for ln in (1, 2, 63, 64, 65, 127):
        for flag in (0, 16):
            head = rng.sample(bam.SEQ_CODES, min(ln, 16))  # every code once where the read is long enough
            seq = "".join(head) + _seq(rng, ln - len(head), bam.SEQ_CODES)
            records.append(_rec(f"iupac{ln}_{'r' if flag else 'f'}", flag, len(records) % 2, _cigar(60, ln), seq))
    for flag in (0, 16):  # the short reads cannot hold all 16: one read per strand made of the codes in table order
        records.append(_rec(f"table_{'r' if flag else 'f'}", flag, 0, _cigar(60, 32), bam.SEQ_CODES * 2))
    return _case("iupac_seq", DEFAULT_REGIONS, records)


def kept_without_seq_case(rng):
    """Primary records that store no sequence (l_seq 0) and pass both filters: 0 > 60 * 1.05 + 141 is false, so the
    reference prints `None` for them."""
    records = [_rec("with_seq_f", 0, 0, _cigar(60, 60), _seq(rng, 60)),
               _rec("no_seq_f", 0, 0, _cigar(60, 0), ""),
               _rec("no_seq_r", 16, 1, _cigar(58, 0), ""),
               _rec("with_seq_r", 16, 1, _cigar(60, 60), _seq(rng, 60)),
               _rec("no_seq_short", 0, 0, _cigar(56, 0), ""),  # 56 < 57: short, nothing printed
               _rec("no_seq_last", 16, 0, _cigar(57, 0), "")]
    return _case("kept_without_seq", DEFAULT_REGIONS, records)


def no_cluster_case(rng):
    """A region of the reference FASTA that the cluster JSON lacks: its short and long records are counted (the
    cluster lookup comes after both filters), its first passing record raises KeyError after the files of the
    earlier records are written, and nothing after it is reached."""
    regions = [("TRBV1_1", 60), ("TRBV2_2", 60), ("TRBV3_unclustered", 60)]
    records = [_rec("a0", 0, 0, _cigar(60, 60), _seq(rng, 60)),
               _rec("b0", 16, 1, _cigar(59, 61), _seq(rng, 61)),
               _rec("c_short", 0, 2, _cigar(56, 60), _seq(rng, 60)),
               _rec("a1", 16, 0, _cigar(60, 60), _seq(rng, 60)),
               _rec("c_long", 16, 2, _cigar(60, 205), _seq(rng, 205)),  # bound 60 * 1.05 + 141 = 204
               _rec("b1", 0, 1, _cigar(57, 57), _seq(rng, 57)),
               _rec("c_passes", 0, 2, _cigar(60, 60), _seq(rng, 60)),
               _rec("a_never", 0, 0, _cigar(60, 60), _seq(rng, 60)),
               _rec("b_never", 16, 1, _cigar(60, 60), _seq(rng, 60)),
               _rec("c_never", 16, 2, _cigar(60, 60), _seq(rng, 60))]
    return _case("no_cluster", regions, records, clusters={"TRBV1_1": 0, "TRBV2_2": 3})


def threshold_edges_case(rng, name, ov, s5, s3, lengths):
    """Per region length L: reference spans at floor(L * ov) - 1 .. + 2 and, at full span, query lengths at the
    long bound - 1, + 0, + 1."""
    regions = [(f"TRBV{k + 1}_len{length}", length) for k, length in enumerate(lengths)]
    records = []
    for r, (nm, length) in enumerate(regions):
        lo = int(length * ov)
        hi = int(long_bounds(length, ov, s5 + s3)[0])
        for d in (-1, 0, 1, 2):
            records.append(_rec(f"{nm}_span{d:+d}", 16 * (len(records) & 1), r, _cigar(lo + d, 40), _seq(rng, 40)))
        for d in (-1, 0, 1):
            records.append(_rec(f"{nm}_query{d:+d}", 16 * (len(records) & 1), r, _cigar(length, hi + d),
                                _seq(rng, hi + d)))
    return _case(name, regions, records, ov=ov, s5=s5, s3=s3)


def fused_flips(case):
    """(region length, query length) of the primary records that the rounded and the fused bound decide differently."""
    slack = case["max_softclip_5_end"] + case["max_softclip_3_end"]
    out = []
    for r in case["records"]:
        rounded, fused = long_bounds(case["refs"][r["ref"]][1], case["minimal_region_overlap"], slack)
        if (len(r["seq"]) > rounded) != (len(r["seq"]) > fused):
            out.append((case["refs"][r["ref"]][1], len(r["seq"])))
    return out


def no_primary_case(rng):
    """Only unmapped, secondary and supplementary records: no file is written and the log arithmetic divides by the
    zero primary count."""
    records = [_rec(f"np{i}", flag, ref, _cigar(60, 60) if ref >= 0 else [], seq)
               for i, (flag, ref, seq) in enumerate([(4, -1, _seq(rng, 50)), (4 | 16, 0, _seq(rng, 60)),
                                                     (256, 0, _seq(rng, 60)), (256 | 16, 1, ""),
                                                     (2048, 1, _seq(rng, 60)), (2048 | 16, 0, _seq(rng, 60)),
                                                     (4, -1, "")])]
    return _case("no_primary", DEFAULT_REGIONS, records)


def hand_cases(rng):
    edges = [threshold_edges_case(rng, "threshold_edges_093", 0.93, 73, 68, [400, 100]),
             threshold_edges_case(rng, "threshold_edges_093_tight", 0.93, 10, 10, [1900]),
             threshold_edges_case(rng, "threshold_edges_095", 0.95, 73, 68, [500]),
             threshold_edges_case(rng, "threshold_edges_100", 1.0, 0, 0, [300]),
             threshold_edges_case(rng, "threshold_edges_050", 0.5, 10, 10, [640])]
    flips = [f for c in edges for f in fused_flips(c)]
    assert sorted(flips) == [(100, 248), (400, 569), (1900, 2053)], flips  # the rows a fused bound gets wrong
    return [name_lengths_case(rng), cigar_ops_case(rng), iupac_seq_case(rng), kept_without_seq_case(rng),
            no_cluster_case(rng)] + edges + [no_primary_case(rng)]


def write_inputs(case, d):
    """BAM, reference FASTA, cluster JSON, output dir (with any pre-existing files), logs dir."""
    os.makedirs(d, exist_ok=True)
    bam_path = os.path.join(d, "barcode07.sorted.bam")
    bam.write_bam(bam_path, [tuple(r) for r in case["refs"]], case["records"])
    ref_fa = os.path.join(d, "reference.fa")
    rng = random.Random(len(case["regions"]))
    with open(ref_fa, "w") as fh:
        for nm, ln in case["regions"]:
            s = "".join(rng.choice("ACGT") for _ in range(ln))
            fh.write(f">{nm}\n" + "\n".join(s[i:i + 60] for i in range(0, ln, 60)) + "\n")
    js = os.path.join(d, "region_cluster_dict.json")
    with open(js, "w") as fh:
        json.dump(case["clusters"], fh)
    out = os.path.join(d, "out")
    logs = os.path.join(d, "logs")
    os.makedirs(out)
    os.makedirs(logs)
    for fn, txt in case["pre_existing"].items():
        with open(os.path.join(out, fn), "w") as fh:
            fh.write(txt)
    return bam_path, ref_fa, js, out, logs


def run_reference(mod, case):
    tmp = tempfile.mkdtemp(prefix="rs_")
    try:
        bam_path, ref_fa, js, out, logs = write_inputs(case, tmp)
        res = dict(case)
        try:
            ret = mod.filter_and_split_reads_by_region_cluster(
                bam_file=bam_path, region_cluster_dict_json=js, reference=ref_fa, logs_dir=logs,
                region_fasta_out_dir=out, minimal_region_overlap=case["minimal_region_overlap"],
                max_softclip_5_end=case["max_softclip_5_end"], max_softclip_3_end=case["max_softclip_3_end"])
            res["result"] = sorted(os.path.relpath(p, tmp) for p in ret)
            res["error"] = None
        except Exception as e:  # KeyError: an unknown region; ZeroDivisionError: the log of a file without primaries
            res["result"] = None
            res["error"] = f"{type(e).__name__}: {e}"
        res["out_files"] = {fn: open(os.path.join(out, fn)).read() for fn in sorted(os.listdir(out))}
        res["log_files"] = {fn: open(os.path.join(logs, fn)).read() for fn in sorted(os.listdir(logs))}
        return res
    finally:
        shutil.rmtree(tmp)


def main():
    make_golden._stub_modules()
    sys.modules["pysam"].AlignmentFile = bam.AlignmentFile
    mod = make_golden._load("region_split")
    rng = random.Random(20261016)
    cases = [make_case(rng, "small", 6, 150), make_case(rng, "many_regions", 30, 500),
             make_case(rng, "loose_overlap", 8, 250, minimal_region_overlap=0.5, s5=10, s3=10),
             make_case(rng, "append_existing", 5, 150, pre_existing=True),
             make_case(rng, "unknown_reference", 5, 150, unknown_ref=True),
             make_case(rng, "no_cigar", 5, 150, no_cigar_at=97)]
    cases += hand_cases(random.Random(20261020))  # after the drawn six, with an rng of their own
    od = os.path.join(HERE, "region_split")
    os.makedirs(od, exist_ok=True)
    for c in cases:
        r = run_reference(mod, c)
        with open(os.path.join(od, c["name"] + ".json"), "w") as fh:
            json.dump(r, fh, indent=0, sort_keys=True)
        print(c["name"], r["result"], r["error"], list(r["log_files"]))


if __name__ == "__main__":
    main()
