"""§8f row f4 on the GPU: umiclust.region_split (BGZF on the host threads, record classification and FASTA
emission on the device) against the reference's own outputs on the same inputs (tests/golden/region_split,
made by running region_split.py here with a pysam stand-in, tests/golden/make_golden_region_split.py); then the
entry point itself (gpu_ctx.region_split) against oracle/region_split.py on seeded records that no fixture could
hold: many workgroups, records across BGZF blocks, a 70,001-nt read, sparse cluster ids, no records at all, and a
sweep of the `too long` bound."""
import ast
import os

import pytest
from make_golden_region_split import write_inputs
from test_region_split_cpu import cases, error_class
from umiclust import region_split as rs

pytestmark = pytest.mark.gpu

SET_LINE = "missing/non-detected regions from reference in initial non-polished read alignments: "


def _norm_log(text):
    """The last line prints a Python set, whose order depends on string hashing: compare it as a set."""
    out = []
    for line in text.splitlines():
        if line.startswith(SET_LINE):
            out.append((SET_LINE, frozenset(ast.literal_eval(line[len(SET_LINE):]) or ())))
        else:
            out.append(line)
    return out


@pytest.mark.parametrize("case", cases(), ids=[c["name"] for c in cases()])
def test_region_split_vs_reference_fixtures(tmp_path, case):
    bam_path, ref_fa, js, out, logs = write_inputs(case, str(tmp_path))
    kw = dict(minimal_region_overlap=case["minimal_region_overlap"], max_softclip_5_end=case["max_softclip_5_end"],
              max_softclip_3_end=case["max_softclip_3_end"])
    if case["error"]:
        exc = error_class(case)
        with pytest.raises(exc) as e:
            rs.filter_and_split_reads_by_region_cluster(bam_path, js, ref_fa, logs, out, **kw)
        assert f"{exc.__name__}: {e.value}" == case["error"]
    else:
        ret = rs.filter_and_split_reads_by_region_cluster(bam_path, js, ref_fa, logs, out, **kw)
        assert sorted(os.path.relpath(p, str(tmp_path)) for p in ret) == case["result"]
    got = {fn: open(os.path.join(out, fn)).read() for fn in sorted(os.listdir(out))}
    assert got == case["out_files"]
    gl = {fn: _norm_log(open(os.path.join(logs, fn)).read()) for fn in sorted(os.listdir(logs))}
    assert gl == {fn: _norm_log(t) for fn, t in case["log_files"].items()}


# ---------------------------------------------------------------- the entry point itself against oracle/region_split.py
import random  # noqa: E402

import bam  # noqa: E402
import region_split as ors  # noqa: E402

NAME_CHARS = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_-:/.#+|"


def _first_difference(got, want):
    """The name of the first record at which two FASTA texts differ."""
    g, w = got.split(">")[1:], want.split(">")[1:]
    for x in range(max(len(g), len(w))):
        if x >= len(g) or x >= len(w) or g[x] != w[x]:
            return (w[x] if x < len(w) else g[x]).split(";strand=")[0][:80]
    return None


def _both(ctx, tmp_path, regions, refs, clusters, records, ov, s5, s3, block=60000):
    """gpu_ctx.region_split and oracle split_records on the same records: counts, per-cluster counts, detected regions
    and every output file byte for byte; a KeyError must be the same KeyError after the same files.  Returns the
    oracle's counts and files."""
    path = str(tmp_path / "in.bam")
    bam.write_bam(path, [tuple(r) for r in refs], records, block=block)
    got_dir, want_dir = tmp_path / "got", tmp_path / "want"
    got_dir.mkdir()
    want_dir.mkdir()
    recs = [bam.AlignedSegment(refs, r["ref"], r["pos"], r["flag"], r["name"],
                               [(bam.CIGAR_OPS.index(op), ln) for op, ln in r["cigar"]], r["seq"] or None)
            for r in records]
    names, lengths = [nm for nm, _ in regions], [ln for _, ln in regions]
    want = want_err = got = got_err = None
    try:
        want = ors.split_records(recs, dict(regions), clusters, ov, s5, s3, out_dir=str(want_dir))
    except KeyError as e:
        want_err = str(e)
    try:
        got = ctx.region_split(path, names, lengths, [clusters.get(nm, -1) for nm in names], ov, s5, s3, str(got_dir))
    except KeyError as e:
        got_err = str(e)
    assert got_err == want_err
    files = {fn: open(want_dir / fn).read() for fn in sorted(os.listdir(want_dir))}
    got_files = {fn: open(got_dir / fn).read() for fn in sorted(os.listdir(got_dir))}
    assert sorted(got_files) == sorted(files)
    for fn in files:
        assert got_files[fn] == files[fn], (fn, "first differing record", _first_difference(got_files[fn], files[fn]))
    if want is None:
        return None, files
    counts, per_cluster, _, detected = want
    g_counts, g_per_cluster, g_detected = got
    assert dict(zip(("unmapped", "primary", "short", "long"), (int(x) for x in g_counts))) == counts
    assert {k: int(v) for k, v in enumerate(g_per_cluster) if v} == per_cluster
    assert {names[r] for r, d in enumerate(g_detected) if d} == detected
    return counts, files


def _rec(name, flag, ref, cigar, seq):
    return dict(name=name, flag=flag, ref=ref, pos=0, cigar=cigar, seq=seq)


def _mixed_records(rng, n, refs, ov, slack, never_passing=()):
    """Records of about 30..200 nt mixing what the fixtures hold one at a time: names of 1..254 bytes, every CIGAR op
    (spans from M, D, N, = or X), all 16 sequence codes, records without a sequence, a CIGAR or a reference, every
    flag, spans and query lengths on and next to both thresholds.  References listed in `never_passing` only get
    records that one of the two filters drops."""
    out = []
    for i in range(n):
        ref = rng.randrange(len(refs))
        length = refs[ref][1]
        lo, hi = int(length * ov), int(length * (2 - ov) + slack)
        u = rng.random()
        flag = 4 if u < 0.05 else 256 if u < 0.09 else 2048 if u < 0.12 else 0
        flag |= 16 * (rng.random() < 0.5)
        span = rng.choice([lo - 1, lo, lo + 1, lo + 2, length, rng.randint(1, length + 5)])
        if ref in never_passing and rng.random() < 0.5:
            span = rng.randint(1, max(1, lo - 1))
        span = max(span, 1)
        cigar = []
        left = span
        while left:  # the span split over the ops that consume the reference, I and P between them
            ln = min(left, rng.randint(1, 60))
            op = rng.choice("MMMM=XDN")
            cigar.append((op, ln))
            left -= ln
            if left and rng.random() < 0.3:
                cigar.append((rng.choice("IP"), rng.randint(1, 4)))
        qlen = sum(ln for op, ln in cigar if op in "MI=X")
        clip5, clip3 = rng.choice([0, 0, rng.randint(1, 40)]), rng.choice([0, 0, rng.randint(1, 40)])
        if rng.random() < 0.25 or (ref in never_passing and span >= lo):  # the query length on or next to the bound
            target = hi + (rng.choice([-1, 0, 1, 2]) if ref not in never_passing else rng.randint(1, 3))
            clip5, clip3 = 0, max(0, target - qlen)
        cigar = ([("S", clip5)] if clip5 else []) + cigar + ([("S", clip3)] if clip3 else [])
        qlen += clip5 + clip3
        if rng.random() < 0.1:
            cigar = [("H", rng.randint(1, 9))] + cigar + [("H", rng.randint(1, 9))]
        u = rng.random()
        if u < 0.02:
            cigar = []  # reference_length 1
        elif u < 0.04:
            cigar = [("S", 5), ("I", qlen), ("S", 3)]  # the same
            qlen += 8
        alpha = bam.SEQ_CODES if rng.random() < 0.15 else "ACGT"
        seq = "".join(rng.choices(alpha, k=qlen))
        if rng.random() < 0.03 and ref not in never_passing:
            seq = ""  # no stored sequence: a kept one prints None
        nl = rng.choice([1, 63, 64, 65, 128, 254]) if rng.random() < 0.06 else rng.randint(2, 20)
        name = "".join(rng.choices(NAME_CHARS, k=nl))
        if flag & 4 and rng.random() < 0.5:
            ref, cigar = -1, []
        out.append(_rec(name, flag, ref, cigar, seq))
    return out


def test_entry_point_vs_oracle_mixed_records(gpu_ctx, tmp_path):
    """20,000 records over many classify workgroups and emit blocks, in BGZF blocks of 4,096 bytes so that nearly every
    record straddles one.  One region has no cluster: its records are all short or too long, which the reference counts
    without looking the cluster up."""
    rng = random.Random(7)
    regions = [(f"TRBV{k}_{rng.randint(1, 9)}", rng.randint(30, 150)) for k in range(13)]
    clusters = {nm: k // 2 for k, (nm, _) in enumerate(regions[:12])}
    records = _mixed_records(rng, 20000, regions, 0.9, 35, never_passing={12})
    counts, files = _both(gpu_ctx, tmp_path, regions, regions, clusters, records, 0.9, 20, 15, block=4096)
    kept = sum(t.count(">") for t in files.values())
    assert counts["unmapped"] > 500 and counts["short"] > 2000 and counts["long"] > 1000 and kept > 3000
    assert sum(t.count("\nNone\n") for t in files.values()) > 20 and len(files) == 6


def test_entry_point_raises_at_the_first_passing_record_without_cluster(gpu_ctx, tmp_path):
    """The same stream with a passing record of the unclustered region late in it: KeyError after the files of the
    records before it."""
    rng = random.Random(8)
    regions = [(f"TRBV{k}_{rng.randint(1, 9)}", rng.randint(30, 150)) for k in range(5)]
    clusters = {nm: k for k, (nm, _) in enumerate(regions[:4])}
    records = _mixed_records(rng, 3000, regions, 0.9, 35, never_passing={4})
    records.insert(2500, _rec("passes", 16, 4, [("M", regions[4][1])], "A" * regions[4][1]))
    counts, files = _both(gpu_ctx, tmp_path, regions, regions, clusters, records, 0.9, 20, 15, block=4096)
    assert counts is None and files


def test_entry_point_record_larger_than_a_bgzf_block(gpu_ctx, tmp_path):
    """A kept reverse-strand read of 70,001 nt (l_seq odd) on a region of 70,000: the record spans two BGZF blocks and
    the emit kernel's lane loop runs over a thousand trips."""
    rng = random.Random(9)
    regions = [("TRBV_long", 70000), ("TRBV_b", 50)]
    seq = "".join(rng.choices("ACGT" * 8 + bam.SEQ_CODES, k=70001))
    records = [_rec("before", 0, 1, [("M", 50)], "".join(rng.choices("ACGT", k=50))),
               _rec("long_read", 16, 0, [("M", 70000), ("S", 1)], seq),
               _rec("after", 16, 1, [("M", 50)], "".join(rng.choices("ACGT", k=50)))]
    counts, files = _both(gpu_ctx, tmp_path, regions, regions, {"TRBV_long": 1, "TRBV_b": 0}, records, 0.95, 73, 68)
    assert counts == dict(unmapped=0, primary=3, short=0, long=0) and len(files["region_cluster1.fasta"]) > 70001


def test_entry_point_sparse_cluster_ids(gpu_ctx, tmp_path):
    """Cluster ids 0 and 4,999, every kept read in the second."""
    rng = random.Random(10)
    regions = [("TRBV_a", 80), ("TRBV_z", 90)]
    records = []
    for i in range(60):
        ref = i % 2
        span = 40 if ref == 0 else rng.randint(86, 90)  # every read of TRBV_a is short
        records.append(_rec(f"r{i}", 16 * (i % 3 == 0), ref, [("M", span)], "".join(rng.choices("ACGT", k=span))))
    counts, files = _both(gpu_ctx, tmp_path, regions, regions, {"TRBV_a": 0, "TRBV_z": 4999}, records, 0.95, 73, 68)
    assert list(files) == ["region_cluster4999.fasta"] and counts["short"] == 30


def test_entry_point_without_records(gpu_ctx, tmp_path):
    """A BAM that ends after its header: counts of zero and no file.  (The ZeroDivisionError of the reference belongs to
    the log arithmetic of the Python wrapper: fixture no_primary.)"""
    regions = [("TRBV_a", 80), ("TRBV_z", 90)]
    counts, files = _both(gpu_ctx, tmp_path, regions, regions, {"TRBV_a": 0, "TRBV_z": 1}, [], 0.95, 73, 68)
    assert counts == dict(unmapped=0, primary=0, short=0, long=0) and files == {}


@pytest.mark.parametrize("length", [100, 400, 900, 1900])
@pytest.mark.parametrize("ov", [0.5, 0.8, 0.9, 0.93, 0.95, 0.97, 1.0])
def test_entry_point_long_bound_sweep(gpu_ctx, tmp_path, ov, length):
    """Query lengths on the `too long` bound and one to either side, with the default slack (73 + 68) and with 10 + 10.
    The reference rounds length * (2 - ov) before it adds the slack; one fused multiply-add lands an ulp below the
    integer bound at overlap 0.93 for all four lengths with slack 141 and for 1900 with slack 20 (exact arithmetic:
    make_golden_region_split.long_bounds), and drops the read of exactly that length as long."""
    regions = [(f"TRBV_len{length}", length)]
    for s5, s3 in ((73, 68), (10, 10)):
        hi = int(length * (2 - ov) + (s5 + s3))
        records = [_rec(f"q{hi + d}", 16 * (d == 0), 0, [("M", length), ("S", hi + d - length)] if hi + d > length
                        else [("M", hi + d), ("D", length - hi - d)], "ACGT" * ((hi + d) // 4) + "ACGT"[:(hi + d) % 4])
                   for d in (-1, 0, 1)]
        d = tmp_path / f"slack{s5 + s3}"
        d.mkdir()
        counts, files = _both(gpu_ctx, d, regions, regions, {regions[0][0]: 0}, records, ov, s5, s3)
        assert counts == dict(unmapped=0, primary=3, short=0, long=1), (ov, length, s5 + s3)
