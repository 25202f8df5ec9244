"""Row f4+f1 on the GPU: the region split fused with the UMI extraction.  Every test runs one BAM
through three paths and compares their files byte for byte: (a) the fused call, (b) gpu_ctx.region_split into a fresh
directory followed by gpu_ctx.extract_umis_file on every file it wrote, (c) the plain CPU composition of
tests/split_extract_ref.py (oracle/region_split.py feeding oracle/extract.py).  The reads carry planted UMIs and the
tests assert what they found, so that none can pass on files with nothing in them."""
import json
import os
import random
import re
import warnings

import numpy as np
import pytest
import split_extract_ref as ref
from make_golden_region_split import write_inputs
from test_gpu_region_split import _mixed_records, _norm_log
from test_region_split_cpu import cases
from test_round2_cpu import FUSED_CASES, GOLD, norm_log, read_dir
from umiclust import _lib, minimap2_align
from umiclust import extract_umis as eu
from umiclust import region_split as rs

import bam
import bam_ref

pytestmark = pytest.mark.gpu

EFORMAT = -74
UMI_FILE = "region_cluster%d_detected_umis.fasta"


def _rec(name, flag, ref_id, span, seq):
    return dict(name=name, flag=flag, ref=ref_id, pos=0, cigar=[("M", span)], seq=seq)


def _read_dir(d):
    return {fn: open(os.path.join(d, fn), "rb").read() for fn in sorted(os.listdir(d))}


def three_way(ctx, tmp_path, refs, regions, clusters, records, ov, s5, s3, a5, a3, k, fwd=ref.UMI_FWD, rev=ref.UMI_REV,
              block=60000, pre_existing=None):
    """One BAM through (a), (b) and (c).  The KeyError must be the same in all three, with no UMI file in (a); else the
    UMI files, umis_per_cluster against each extract_umis_file return, and counts, reads_per_cluster and
    region_detected against (b)'s.  Returns (c)'s files as text, its kept entries and its per-cluster UMI counts."""
    tmp_path.mkdir(exist_ok=True)
    path = str(tmp_path / "in.bam")
    bam.write_bam(path, [tuple(r) for r in refs], records, block=block)
    da, db, dfa = tmp_path / "a", tmp_path / "b", tmp_path / "fa"
    for d in (da, db, dfa):
        d.mkdir()
    for fn, text in (pre_existing or {}).items():
        (da / fn).write_text(text)
    names, lengths = [nm for nm, _ in regions], [ln for _, ln in regions]
    cl = [clusters.get(nm, -1) for nm in names]
    got_a = got_b = want = err_a = err_b = err_c = None
    try:
        want = ref.compose(refs, regions, clusters, records, ov, s5, s3, a5, a3, k, fwd, rev)
    except KeyError as e:
        err_c = str(e)
    try:
        got_b = ctx.region_split(path, names, lengths, cl, ov, s5, s3, str(dfa))
    except KeyError as e:
        err_b = str(e)
    try:
        got_a = ctx.region_split_extract(path, names, lengths, cl, ov, s5, s3, a5, a3, k, fwd, rev, str(da))
    except KeyError as e:
        err_a = str(e)
    assert err_a == err_b == err_c
    if err_a is not None:
        assert os.listdir(da) == []
        return None
    n_b = {}
    for fn in sorted(os.listdir(dfa)):
        c = int(re.fullmatch(r"region_cluster(\d+)\.fasta", fn).group(1))
        n_b[c] = ctx.extract_umis_file(str(dfa / fn), str(db / (UMI_FILE % c)), a5, a3, k, fwd, rev)
    files_a, files_b = _read_dir(da), _read_dir(db)
    files_c = {fn: t.encode() for fn, t in want[3].items()}
    assert sorted(files_a) == sorted(files_b) == sorted(files_c)
    for fn in files_a:
        assert files_a[fn] == files_b[fn], (fn, "fused vs two-step")
        assert files_a[fn] == files_c[fn], (fn, "fused vs CPU composition")
    counts, per_cluster, umis, detected = got_a
    assert {c: int(v) for c, v in enumerate(umis) if per_cluster[c]} == n_b == want[4]
    assert np.array_equal(counts, got_b[0]) and np.array_equal(per_cluster, got_b[1])
    assert np.array_equal(detected, got_b[2])
    assert dict(zip(("unmapped", "primary", "short", "long"), (int(x) for x in counts))) == want[0]
    return want[3], want[5], want[4]


# ---------------------------------------------------------------- mixed classes and clusters
def test_mixed_classes_and_clusters(gpu_ctx, tmp_path):
    """6,000 planted reads among 1,500 records of every other class (unmapped, secondary, short, long, no sequence),
    13 regions in 6 clusters, BGZF blocks of 4,096 bytes: many workgroups, records across blocks, odd and even l_seq,
    reverse reads stored reverse-complemented.  (The plain reference's two dynamic programs per read are most of this
    test's run time.)"""
    rng = random.Random(11)
    a5, a3, k = 40, 36, 3
    regions = [(f"TRBV{i}_{rng.randint(1, 9)}", rng.randint(30, 150)) for i in range(13)]
    clusters = {nm: i // 2 for i, (nm, _) in enumerate(regions[:12])}
    records = _mixed_records(rng, 1500, regions, 0.9, 220, never_passing={12})
    records += ref.planted_records(rng, 6000, regions[:12], a5, a3, k)
    rng.shuffle(records)
    files, kept, umis = three_way(gpu_ctx, tmp_path, regions, regions, clusters, records, 0.9, 120, 100, a5, a3, k,
                                  block=4096)
    assert len(files) == 6 and len(kept) > 5000
    assert {len(seq) % 2 for _, seq in kept} == {0, 1} and any(seq == "None" for _, seq in kept)
    ref.conditions(files, len(kept), k)


# ---------------------------------------------------------------- window edges
def _edge_records(rng, a5, a3, k, fwd, rev, per=3):
    """reads of every length on and next to the window bounds, on both strands, each starting with an instance of fwd
    and ending with one of rev as far as its length allows"""
    out = []
    lengths = sorted({x for x in (0, 1, 2, a5 - 1, a5, a5 + 1, a5 + a3 - 1, a5 + a3, a5 + a3 + 1,
                                  len(fwd) + len(rev) + 10) if x >= 0})  # the last one holds both UMIs in any window
    for length in lengths:
        for reverse in (False, True):
            for j in range(per if length else 1):
                head = ref._instance(rng, fwd, rng.randint(0, k + 1), "ACGT")
                tail = ref._instance(rng, rev, rng.randint(0, k + 1), "ACGT")
                fill = "".join(rng.choices("ACGT", k=max(0, length - len(head) - len(tail))))
                text = (head + fill + tail) if j else (head + tail + fill)
                text = text[:length] if j % 2 else text[len(text) - length:]
                out.append(_rec("e%d_%d_%d" % (length, reverse, j), 16 * reverse, 0, 100, ref.stored(text, reverse)))
    return out


@pytest.mark.parametrize("m,k", [(1, 0), (2, 1), (28, 3), (63, 12), (64, 12)])
def test_window_edges(gpu_ctx, tmp_path, m, k):
    """l_seq in {0, 1, 2, a5 - 1, a5, a5 + 1, a5 + a3 - 1, a5 + a3, a5 + a3 + 1} on both strands with patterns of m
    symbols; windows (40, 36), a5 = 0, a3 = 0 (the whole read), 255 (the kernels' stated range) and 256."""
    rng = random.Random(1000 + m)
    if m == 28:
        fwd, rev = ref.UMI_FWD, ref.UMI_REV
    else:
        fwd, rev = ("A", "T") if m == 1 else ("".join(rng.choices("ACGTVBN", k=m)), "".join(rng.choices("ACGTVBN", k=m)))
    regions = [("TRBV_e", 100)]
    found = 0
    for a5, a3 in ((40, 36), (0, 36), (40, 0), (255, 255), (256, 256)):
        if m >= 63 and a5 < 255:
            a5, a3 = a5 and a5 + 40, a3 and a3 + 40  # a window that can hold the pattern
        records = _edge_records(rng, a5, a3, k, fwd, rev, per=2 if a5 >= 255 else 3)
        files, kept, umis = three_way(gpu_ctx, tmp_path / f"w{a5}_{a3}", regions, regions, {"TRBV_e": 0}, records, 0.95,
                                      400, 400, a5, a3, k, fwd, rev, block=4096)
        assert len(kept) == len(records) and ("e0_0_0;strand=+", "None") in kept and ("e0_1_0;strand=-", "None") in kept
        text = files[UMI_FILE % 0]
        if a5 == 0:
            assert text == ""  # an empty 5' window holds no UMI
        else:
            found += umis[0]
            assert 0 < umis[0] < len(records)
        if m == 1 and a5:  # the sequence-less kept record: N equals A and T
            assert ">e0_0_0;strand=+;umi_fwd_dist=0;umi_rev_dist=0;umi_fwd_seq=N;umi_rev_seq=N;seq=None\nNN\n" in text
            assert ">e0_1_0;strand=-;umi_fwd_dist=0;umi_rev_dist=0;umi_fwd_seq=N;umi_rev_seq=N;seq=None\nNN\n" in text
    assert found > 20


def test_non_acgt_codes_inside_a_umi_on_a_reverse_read(gpu_ctx, tmp_path):
    """Y and K inside the UMIs as mismatches (a code equals plain bases only), R and S where the pattern has G and C: the forward
    sequence leaves the stored codes as they are (only A/C/G/T are complemented), and so does the combined UMI's
    reverse complement."""
    fwd, rev = "ACGGAC", "TTCCAA"
    text = "ACRYAC" + "GGMGG" + "TTKSAA"
    records = [_rec("iupac", 16, 0, 100, ref.stored(text, True)), _rec("plain", 0, 0, 100, "ACGGAC" + "CC" + "TTCCAA")]
    files, kept, umis = three_way(gpu_ctx, tmp_path, [("TRBV_e", 100)], [("TRBV_e", 100)], {"TRBV_e": 2}, records,
                                  0.95, 73, 68, 10, 9, 2, fwd, rev)
    assert kept[0] == ("iupac;strand=-", text) and umis == {2: 2}
    assert files[UMI_FILE % 2].startswith(
        f">iupac;strand=-;umi_fwd_dist=1;umi_rev_dist=1;umi_fwd_seq=ACRYAC;umi_rev_seq=TTKSAA;seq={text}\nTTSKAAGTYRGT\n")


# ---------------------------------------------------------------- names
def test_names(gpu_ctx, tmp_path):
    """Names of 1, 63, 64, 65 and 254 bytes (the emit kernel's ';' search runs 64 bytes a step) and names that hold ';',
    'strand=', ';strand=-' and '=': read name and strand come out as the two-step path prints them."""
    rng = random.Random(5)
    fwd, rev = "ACGTAC", "TTGGAA"
    names = ["n", "a" * 63, "b" * 64, "c" * 65, "d" * 254, "e" * 70 + ";" + "f" * 100, ";", "x;y;z", "a=b",
             "strand=", "q;strand=-", "strand=+strand=-", "s" * 200 + "strand=", "pstrand", "g" * 63 + ";", "h" * 64 + ";t"]
    records = []
    for i, nm in enumerate(names):
        for reverse in (False, True):
            text = "ACGTAC" + "".join(rng.choices("ACGT", k=7 + i)) + "TTGGAA"
            records.append(_rec(nm, 16 * reverse, 0, 100, ref.stored(text, reverse)))
    records.append(_rec("strand=none", 0, 0, 100, "C" * 30))  # a name for the host, without UMIs: no record
    files, kept, umis = three_way(gpu_ctx, tmp_path, [("TRBV_e", 100)], [("TRBV_e", 100)], {"TRBV_e": 0}, records,
                                  0.95, 73, 68, 12, 12, 0, fwd, rev)
    assert umis == {0: 2 * len(names)}
    text = files[UMI_FILE % 0]
    assert "\n>q;strand=-;;umi_fwd_dist=0" in text and "\n>;strand=+;umi_fwd_dist=0" in text
    assert "\n>strand=;strand=;;umi_fwd_dist=0" in text  # of "strand=": ';' between it and the appended "strand="
    assert "\n>strand=+strand=-;strand=+;umi_fwd_dist=0" in text  # '+' between the name's two "strand="


@pytest.mark.parametrize("bad", ["two words", "tab\there", "line\nfeed", "v\x0bt", "f\x0cf", "cr\r"])
def test_white_space_in_a_kept_name_is_refused(gpu_ctx, tmp_path, bad):
    records = [_rec("fine", 0, 0, 100, "ACGTAC" + "CCCC" + "TTGGAA"), _rec(bad, 0, 0, 100, "ACGTAC" + "CCCC" + "TTGGAA")]
    bam.write_bam(str(tmp_path / "in.bam"), [("TRBV_e", 100)], records)
    out = tmp_path / "umis"
    out.mkdir()
    with pytest.raises(_lib.UmiclustError) as e:
        gpu_ctx.region_split_extract(str(tmp_path / "in.bam"), ["TRBV_e"], [100], [0], 0.95, 73, 68, 12, 12, 0, "ACGTAC",
                                     "TTGGAA", str(out))
    assert e.value.code == EFORMAT and "record 1" in str(e.value) and os.listdir(out) == []
    # the same name on a record that is not kept is nobody's header
    records[1]["flag"] = 4
    bam.write_bam(str(tmp_path / "in.bam"), [("TRBV_e", 100)], records)
    got = gpu_ctx.region_split_extract(str(tmp_path / "in.bam"), ["TRBV_e"], [100], [0], 0.95, 73, 68, 12, 12, 0,
                                       "ACGTAC", "TTGGAA", str(out))
    assert [int(x) for x in got[2]] == [1] and os.listdir(out) == [UMI_FILE % 0]


# ---------------------------------------------------------------- the size pass's widths
def test_two_digit_distances(gpu_ctx, tmp_path):
    """64-symbol patterns with k = 12: umi_*_dist of 10, 11 and 12 take two bytes in the size pass and in the text."""
    rng = random.Random(64)
    fwd, rev = "".join(rng.choices("ACGT", k=64)), "".join(rng.choices("ACGT", k=64))
    regions = [("TRBV_e", 100), ("TRBV_f", 120)]
    records = ref.planted_records(rng, 160, regions, 100, 100, 12, fwd, rev)
    files, kept, umis = three_way(gpu_ctx, tmp_path, regions, regions, {"TRBV_e": 0, "TRBV_f": 1}, records, 0.95, 400,
                                  400, 100, 100, 12, fwd, rev)
    dists = [int(d) for t in files.values() for d in re.findall(r"umi_(?:fwd|rev)_dist=(\d+);", t)]
    assert {10, 11, 12} <= set(dists) and set(range(10)) & set(dists) and len(kept) == 160


# ---------------------------------------------------------------- files
def test_empty_file_truncation_and_no_records(gpu_ctx, tmp_path):
    """A cluster whose reads all lack a UMI gets an empty file in both paths; a pre-existing output file is replaced,
    not appended to; a BAM without records creates nothing."""
    fwd, rev = "ACGTAC", "TTGGAA"
    regions = [("TRBV_e", 100), ("TRBV_f", 80)]
    records = [_rec("has", 0, 0, 100, "ACGTAC" + "CCCC" + "TTGGAA"), _rec("none1", 0, 1, 80, "C" * 40),
               _rec("none2", 16, 1, 80, "G" * 41)]
    old = {UMI_FILE % 0: ">old;strand=+;umi_fwd_dist=0\nAAAA\n" * 50, UMI_FILE % 7: "old text\n" * 50}
    files, kept, umis = three_way(gpu_ctx, tmp_path / "some", regions, regions, {"TRBV_e": 0, "TRBV_f": 7}, records, 0.95,
                                  73, 68, 12, 12, 0, fwd, rev, pre_existing=old)
    assert files[UMI_FILE % 7] == "" and files[UMI_FILE % 0].count(">") == 1 and umis == {0: 1, 7: 0}
    assert three_way(gpu_ctx, tmp_path / "none", regions, regions, {"TRBV_e": 0, "TRBV_f": 7}, [], 0.95, 73, 68, 12, 12,
                     0, fwd, rev)[0] == {}


def test_key_error_in_the_middle(gpu_ctx, tmp_path):
    """A passing record of a region without a cluster in the middle: the same KeyError and counts as region_split, and
    no UMI file (the exception ends the pipeline before extract_umis starts)."""
    rng = random.Random(8)
    regions = [(f"TRBV{i}", 100 + i) for i in range(4)]
    clusters = {nm: i for i, (nm, _) in enumerate(regions[:3])}
    records = ref.planted_records(rng, 400, regions[:3], 40, 36, 3)
    records.insert(250, _rec("passes", 16, 3, 103, "A" * 103))
    assert three_way(gpu_ctx, tmp_path, regions, regions, clusters, records, 0.9, 200, 200, 40, 36, 3) is None
    names, lengths = [nm for nm, _ in regions], [ln for _, ln in regions]
    L, P, C = _lib.lib(), _lib.C.POINTER, _lib.C
    nm = (C.c_char_p * 4)(*[x.encode() for x in names])
    cl = np.array([0, 1, 2, -1], np.int32)
    res = []
    for fused in (False, True):
        counts, rpc, upc = np.zeros(4, np.int64), np.zeros(3, np.int64), np.zeros(3, np.int64)
        miss = C.create_string_buffer(64)
        out = tmp_path / ("raw%d" % fused)
        out.mkdir()
        head = (gpu_ctx._h, str(tmp_path / "in.bam").encode(), 4, nm, _lib._i64(np.array(lengths, np.int64)),
                cl.ctypes.data_as(P(C.c_int32)), 0.9, 200, 200)
        if fused:
            rc = L.umiclust_region_split_extract(*head, 40, 36, 3, ref.UMI_FWD.encode(), ref.UMI_REV.encode(),
                                                 str(out).encode(), _lib._i64(counts), _lib._i64(rpc), _lib._i64(upc), 3,
                                                 None, miss, 64)
        else:
            rc = L.umiclust_region_split(*head, str(out).encode(), _lib._i64(counts), _lib._i64(rpc), 3, None, miss, 64)
        res.append((rc, counts.tolist(), miss.value))
        assert bool(os.listdir(out)) == (not fused)
    assert res[0] == res[1] and res[0][0] == EFORMAT and res[0][2] == b"TRBV3" and res[0][1][1] == 251


# ---------------------------------------------------------------- the Python drop-in
def _two_step_python(bam_path, js, ref_fa, logs, fa_dir, umi_dir, **kw):
    split_kw = {x: kw[x] for x in ("minimal_region_overlap", "max_softclip_5_end", "max_softclip_3_end")}
    fastas = rs.filter_and_split_reads_by_region_cluster(bam_path, js, ref_fa, logs, fa_dir, **split_kw)
    umi_kw = dict(adapter_length_5_end=kw["max_softclip_5_end"], adapter_length_3_end=kw["max_softclip_3_end"])
    umi_kw.update({x: kw[x] for x in ("adapter_length_5_end", "adapter_length_3_end", "max_pattern_dist", "umi_fwd",
                                      "umi_rev") if x in kw})
    return [p for p in (eu.extract_umis(f, umi_dir, True, **umi_kw) for f in fastas) if p]


def _drop_in_both(case, tmp_path, **umi_kw):
    """filter_split_and_extract_umis against filter_and_split_reads_by_region_cluster + extract_umis per file: the
    exception, the log (its set line as a set), the UMI files and the returned set of paths"""
    got = []
    kw = dict(minimal_region_overlap=case["minimal_region_overlap"], max_softclip_5_end=case["max_softclip_5_end"],
              max_softclip_3_end=case["max_softclip_3_end"], **umi_kw)
    for tag in ("fused", "two_step"):
        bam_path, ref_fa, js, _, logs = write_inputs(case, str(tmp_path / tag))
        fa_dir, umi_dir = tmp_path / tag / "fa", tmp_path / tag / "umis"
        fa_dir.mkdir(), umi_dir.mkdir()
        ret = err = None
        try:
            if tag == "fused":
                ret = rs.filter_split_and_extract_umis(bam_path, js, ref_fa, logs, str(umi_dir), **kw)
            else:
                ret = _two_step_python(bam_path, js, ref_fa, logs, str(fa_dir), str(umi_dir), **kw)
        except (KeyError, ZeroDivisionError, TypeError) as e:
            err = f"{type(e).__name__}: {e}"
        got.append((err, sorted(os.path.relpath(p, str(umi_dir)) for p in ret) if ret is not None else None,
                    _read_dir(umi_dir), {fn: _norm_log(t.decode()) for fn, t in _read_dir(logs).items()}))
        if tag == "fused":
            assert os.listdir(fa_dir) == []
    # with an exception the pipeline never reaches extract_umis: no UMI file in either path
    assert got[0] == got[1]
    return got[0]


@pytest.mark.parametrize("case", cases(), ids=[c["name"] for c in cases()])
def test_python_drop_in_on_the_region_split_fixtures(tmp_path, case):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # numpy's median of an empty list, as in the reference
        err, ret, files, logs = _drop_in_both(case, tmp_path)
    assert err == case["error"]
    if err is None:
        kept = sum(t.count(">") for t in case["out_files"].values()) - sum(t.count(">") for t in case["pre_existing"].values())
        assert bool(files) == (kept > 0) and list(logs) == list(case["log_files"])


def test_python_drop_in_on_planted_reads(tmp_path):
    """the same through reads that hold UMIs: the returned paths are the files with a record, and an empty file of a
    cluster without one is written but not returned"""
    rng = random.Random(21)
    regions = [["TRBV%d" % i, 90 + i] for i in range(5)]
    records = ref.planted_records(rng, 300, regions[:4], 40, 36, 3)
    records.append(_rec("lonely", 0, 4, 94, "C" * 60))
    case = dict(refs=regions, regions=regions, records=records, clusters={nm: i // 2 for i, (nm, _) in enumerate(regions)},
                pre_existing={}, minimal_region_overlap=0.9, max_softclip_5_end=150, max_softclip_3_end=150)
    err, ret, files, logs = _drop_in_both(case, tmp_path, adapter_length_5_end=40, adapter_length_3_end=36,
                                          max_pattern_dist=3)
    assert err is None and ret == [UMI_FILE % 0, UMI_FILE % 1] and sorted(files) == [UMI_FILE % c for c in range(3)]
    assert files[UMI_FILE % 2] == b"" and sum(t.count(b">") for t in files.values()) > 90


# ---------------------------------------------------------------- round 2: the session
def test_session_split_extract_under_a_keep_mask(gpu_ctx, tmp_path):
    """BamSession.split_extract against BamSession.split + extract_umis_file per bucket, on 2,000 planted consensus-like
    records over 7 regions: no mask, a random mask and all zeros; then a region without a bucket."""
    rng = random.Random(32)
    a5, a3, k = 33, 30, 2
    regions = [("TRBV%d_%d" % (i, rng.randint(1, 9)), rng.randint(150, 300)) for i in range(7)]
    records = ref.planted_records(rng, 2000, regions, a5, a3, k, prefix="cons_")
    for r in records[::50]:
        r["flag"] |= rng.choice([4, 0x100, 0x800])
    bam.write_bam(str(tmp_path / "in.bam"), regions, records, block=4096)
    names, lengths = [nm for nm, _ in regions], [ln for _, ln in regions]
    buckets = [6, 0, 3, 3, 1, 5, 2]
    masks = {"none": None, "random": np.array([rng.random() < 0.5 for _ in records], np.uint8),
             "zeros": np.zeros(len(records), np.uint8)}
    with gpu_ctx.bam_open(tmp_path / "in.bam") as s:
        for tag, keep in masks.items():
            d = tmp_path / tag
            (d / "fa").mkdir(parents=True), (d / "two").mkdir(), (d / "one").mkdir()
            fa = [str(d / "fa" / ("b%d.fasta" % b)) for b in range(7)]
            one = [str(d / "one" / ("b%d_detected_umis.fasta" % b)) for b in range(7)]
            want = s.split(keep, names, lengths, buckets, fa, 0.9, 200, 200)
            n_two = {b: gpu_ctx.extract_umis_file(fa[b], str(d / "two" / ("b%d_detected_umis.fasta" % b)), a5, a3, k,
                                                  ref.UMI_FWD, ref.UMI_REV) for b in range(7) if os.path.exists(fa[b])}
            got = s.split_extract(keep, names, lengths, buckets, one, 0.9, 200, 200, a5, a3, k, ref.UMI_FWD, ref.UMI_REV)
            assert _read_dir(d / "one") == _read_dir(d / "two")
            assert {b: int(v) for b, v in enumerate(got[2]) if got[1][b]} == n_two
            assert all(np.array_equal(x, y) for x, y in zip((got[0], got[1], got[3]), want))
            if tag == "zeros":
                assert os.listdir(d / "one") == []
            else:
                files = {fn: t.decode() for fn, t in _read_dir(d / "one").items()}
                assert len(files) == 6
                ref.conditions(files, int(got[1].sum()), k)
        out = tmp_path / "no_bucket"
        out.mkdir()
        with pytest.raises(KeyError) as e:
            s.split_extract(None, names, lengths, [6, 0, -1, 3, 1, 5, 2], [str(out / ("b%d" % b)) for b in range(7)], 0.9,
                            200, 200, a5, a3, k, ref.UMI_FWD, ref.UMI_REV)
        assert e.value.args[0] == names[2] and os.listdir(out) == []


@pytest.mark.parametrize("name", FUSED_CASES)
def test_filter_split_and_extract_equals_its_steps(name, tmp_path, monkeypatch):
    """filter_consensus_alignments_split_and_extract against filter_consensus_alignments_and_split + extract_umis per
    region file: the filtered BAM's stream, the logs, the UMI files and the returned paths.  (The fixtures' reads are
    ACGT repeated, so the patterns are cut from that.)"""
    monkeypatch.setattr(minimap2_align.subprocess, "run", lambda *a, **k: None)  # samtools index
    case = json.load(open(os.path.join(GOLD, "bam_filter", name + ".json")))
    umi = dict(max_pattern_dist=1, umi_fwd="GTACNTAC", umi_rev="TACGNACG")
    got = []
    for tag in ("fused", "steps"):
        d = tmp_path / tag
        for sub in ("logs", "fa", "umis"):
            (d / sub).mkdir(parents=True)
        bam_ref.write_fasta(d / "ref.fa", case["regions"])
        bam_ref.write_bam(d / "cons.bam", case["refs"], case["records"])
        args = (str(d / "cons.bam"), str(d / "ref.fa"), str(d / "logs"), case["params"]["blast_id_threshold"])
        kw = dict(minimal_region_overlap=case["params"]["minimal_region_overlap"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if tag == "fused":
                filtered, paths = minimap2_align.filter_consensus_alignments_split_and_extract(*args, str(d / "umis"), **kw,
                                                                                               **umi)
            else:
                filtered, fastas = minimap2_align.filter_consensus_alignments_and_split(*args, str(d / "fa"), **kw)
                paths = [p for p in (eu.extract_umis(f, str(d / "umis"), True, 73, 68, **umi) for f in fastas) if p]
        got.append((sorted(os.path.relpath(p, str(d)) for p in paths), read_dir(d / "umis"),
                    {fn: norm_log(t) for fn, t in read_dir(d / "logs").items()}, bam_ref.check_bgzf(filtered)))
        assert (tag == "fused") == (os.listdir(d / "fa") == [])
    assert got[0] == got[1]
    assert got[0][0] and sum(t.count(">") for t in got[0][1].values()) == len(case["expect"]["kept"])
