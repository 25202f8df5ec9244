"""Rows f4b / f6b on the GPU: the round-2 region split and the precision census on the real BAM
session.  Every by-region and precision fixture (the reference's own outputs, tests/golden/by_region and precision)
through the file forms and the session forms; BamSession.split and name_suffix against tests/split_ref.py on seeded
records that no fixture holds; the session split against umiclust_region_split (row f4) on one BAM; and the fused
filter + split against its two steps."""
import gzip
import json
import os
import random

import numpy as np
import pytest
from test_gpu_region_split import _mixed_records
from test_round2_cpu import (BY_REGION, FUSED_CASES, GOLD, PRECISION, check_by_region, check_precision,
                             fused_and_two_step)
from umiclust import _lib, minimap2_align
from umiclust import region_split as rs
from umiclust import vsearch_umi_cluster as _v

import bam
import bam_ref
import split_ref

pytestmark = pytest.mark.gpu

EIO, EINVAL, EFORMAT, ESTATE = -5, -22, -74, -77


# ---------------------------------------------------------------- the fixtures through the real session
@pytest.mark.parametrize("form", ["file", "session"])
@pytest.mark.parametrize("name", sorted(BY_REGION))
def test_by_region_equals_the_reference(name, form, tmp_path):
    def from_session(bam_path, ref_fa, logs, out, **kw):
        with _v.context().bam_open(bam_path) as s:
            return rs.filter_and_split_reads_by_region_from(s, np.ones(s.n, np.uint8), bam_path, ref_fa, logs, out, **kw)
    check_by_region(BY_REGION[name], tmp_path, rs.filter_and_split_reads_by_region if form == "file" else from_session)


@pytest.mark.parametrize("form", ["file", "session"])
@pytest.mark.parametrize("name", sorted(PRECISION))
def test_precision_equals_the_reference(name, form, tmp_path, capsys):
    def from_session(bam_path, fasta, logs, **params):
        with _v.context().bam_open(bam_path) as s:
            return minimap2_align.estimate_precision_at_num_subreads_from(s, bam_path, fasta, logs, **params)
    check_precision(PRECISION[name], name, tmp_path, capsys,
                    minimap2_align.estimate_precision_at_num_subreads if form == "file" else from_session)


# ---------------------------------------------------------------- BamSession.split against the plain reference
def compare_split(s, col, keep, names, lengths, buckets, nb, ov, s5, s3, d):
    """s.split and split_ref.split_texts on the same records: the KeyError, every bucket's bytes, the counts, the
    per-bucket counts and the detected regions"""
    d.mkdir()
    paths = [str(d / ("b%d.fa" % b)) for b in range(nb)]
    counts, per_bucket, detected, texts, missing = split_ref.split_texts(col, keep, names, lengths, buckets, nb, ov, s5, s3)
    got = err = None
    try:
        got = s.split(keep, names, lengths, buckets, paths, ov, s5, s3)
    except KeyError as e:
        err = e.args[0]
    assert err == missing
    files = {b: open(paths[b]).read() for b in range(nb) if os.path.exists(paths[b])}
    assert files == {b: t for b, t in enumerate(texts) if t}
    if err is None:
        assert [int(x) for x in got[0]] == counts and [int(x) for x in got[1]] == per_bucket
        assert [int(x) for x in got[2]] == detected
    return counts, texts, missing


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1000])
def test_session_split_vs_plain_reference(n, tmp_path):
    """Either side of the 256-thread classify block and the 4-record emit block; BGZF blocks of 4,096 bytes, so that
    records straddle them; buckets 39, 0 and 7 (shared by two regions) of 40; no mask, a random mask, all zeros and all
    ones; then the same with a region whose bucket is -1."""
    rng = random.Random(100 + n)
    regions = [("TRBV%d_%d" % (k, rng.randint(1, 9)), rng.randint(30, 150)) for k in range(5)]
    refs = regions + [("not_a_region", 80)]
    records = _mixed_records(rng, n, regions, 0.9, 35)
    path = str(tmp_path / "in.bam")
    bam.write_bam(path, refs, records, block=4096)
    col = split_ref.Session(gzip.decompress(open(path, "rb").read()))
    names, lengths = [nm for nm, _ in regions], [ln for _, ln in regions]
    buckets = [39, 0, 7, 7, 12]
    masks = {"none": None, "random": np.array([rng.random() < 0.5 for _ in range(n)], np.uint8),
             "zeros": np.zeros(n, np.uint8), "ones": np.ones(n, np.uint8)}
    with _v.context().bam_open(path) as s:
        assert s.n == n
        for tag, keep in masks.items():
            counts, texts, missing = compare_split(s, col, keep, names, lengths, buckets, 40, 0.9, 20, 15, tmp_path / tag)
            assert missing is None and (tag != "zeros" or (counts == [0, 0, 0, 0] and not any(texts)))
        if n >= 255:
            assert sum(t.count(">") for t in texts) > n // 10 and counts[2] and counts[3] and counts[0]
        _, _, missing = compare_split(s, col, masks["random"], names, lengths, [39, 0, -1, 7, 12], 40, 0.9, 20, 15,
                                      tmp_path / "no_bucket")
        assert (missing == names[2]) == (n >= 255)
        if n:  # a primary record on a reference that is no region: the lookup raises before either filter
            _, _, missing = compare_split(s, col, None, names[1:], lengths[1:], buckets[1:], 40, 0.9, 20, 15,
                                          tmp_path / "no_region")
            assert (missing == names[0]) == (n >= 255)


def test_session_split_agrees_with_region_split(gpu_ctx, tmp_path):
    """Bucket = cluster id, paths region_cluster<k>.fasta, no mask: the files and counters are those that
    Context.region_split (row f4, which classifies from the CIGAR itself) writes from the same BAM."""
    rng = random.Random(31)
    regions = [("TRBV%d_%d" % (k, rng.randint(1, 9)), rng.randint(30, 150)) for k in range(9)]
    clusters = [k // 2 for k in range(9)]
    bam.write_bam(str(tmp_path / "in.bam"), regions, _mixed_records(rng, 1500, regions, 0.93, 35), block=4096)
    names, lengths = [nm for nm, _ in regions], [ln for _, ln in regions]
    f4, f4b = tmp_path / "f4", tmp_path / "f4b"
    f4.mkdir(), f4b.mkdir()
    want = gpu_ctx.region_split(str(tmp_path / "in.bam"), names, lengths, clusters, 0.93, 20, 15, str(f4))
    with gpu_ctx.bam_open(tmp_path / "in.bam") as s:
        got = s.split(None, names, lengths, clusters, [f4b / ("region_cluster%d.fasta" % k) for k in range(5)], 0.93, 20, 15)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and int(got[1].min()) > 0
    assert sorted(os.listdir(f4b)) == sorted(os.listdir(f4)) and len(os.listdir(f4)) == 5
    for fn in os.listdir(f4):
        assert (f4b / fn).read_bytes() == (f4 / fn).read_bytes(), fn


@pytest.mark.parametrize("name", FUSED_CASES)
def test_filter_and_split_equals_the_two_steps(name, tmp_path, monkeypatch):
    case = json.load(open(os.path.join(GOLD, "bam_filter", name + ".json")))
    fused_and_two_step(case, tmp_path, monkeypatch)


# ---------------------------------------------------------------- name_suffix
def suffix_names(rng, n):
    """names of 1..254 bytes over the tail classes: digits of 1..20 places, leading zeros, empty, signed, a non-digit in
    any place, no "_" at all, and the "_" at byte 0, at the last byte and 19 bytes or more from the end"""
    body = "abcXYZ019_-+. "
    out = ["7", "_", "_7", "7_", "x", "0" * 18, "0" * 19, "9" * 18, "9" * 19, "_" + "9" * 18, "_" + "9" * 19,
           "a" * 253 + "_", "a" * 252 + "_1", "_" + "1" * 253, "1" * 254, "a_" + "0" * 17 + "1", "a_" + "0" * 18 + "1"]
    while len(out) < n:
        kind = rng.randrange(9)
        digits = "".join(rng.choices("0123456789", k=rng.choice([1, 2, 3, 17, 18, 19, 20, rng.randint(1, 20)])))
        tail = {0: digits, 1: "0" * rng.randint(1, 10) + digits[:8], 2: "", 3: rng.choice("+-") + digits[:17],
                4: digits[:rng.randint(0, len(digits))] + rng.choice("xX .-") + digits[:rng.randint(0, 5)],
                5: digits, 6: digits, 7: " " + digits[:5], 8: digits + "_"}[kind]
        room = 254 - len(tail)
        if room < 1 or kind == 5:
            name = tail[:254] or "1"  # no "_" at all: the whole name is the tail
        else:
            head = "".join(rng.choices(body, k=rng.choice([0, 0, 1, 5, rng.randint(0, room - 1)])))
            name = head + "_" + tail
        out.append(name)
    return out


def test_name_suffix_vs_plain_reference(tmp_path):
    rng = random.Random(77)
    names = suffix_names(rng, 1000)
    assert {len(x) for x in names} >= {1, 2, 19, 20, 254} and len(names) == 1000
    recs = [{"name": x, "flag": rng.choice([0, 16, 4, 0x100]), "cigar": "5M", "tags": []} for x in names]
    raw = bam_ref.write_bam(tmp_path / "in.bam", [["r", 10]], recs, block=4096)
    want_v, want_s = split_ref.Session(raw).name_suffix()
    for x, v, st in zip(names, want_v, want_s):  # the plain reference against Python's int() where it claims a value
        assert not st or int(x.split("_")[-1]) == v
    assert 300 < int(want_s.sum()) < 800
    with _v.context().bam_open(tmp_path / "in.bam") as s:
        assert s.query_names(np.arange(s.n)) == names
        got_v, got_s = s.name_suffix()
    assert got_v.dtype == np.int64 and got_s.dtype == np.uint8
    bad = np.flatnonzero((got_s != want_s) | (got_v != want_v))
    assert bad.size == 0, [(names[i], int(got_v[i]), int(got_s[i])) for i in bad[:5]]


# ---------------------------------------------------------------- errors
def test_split_and_suffix_errors(tmp_path):
    ctx = _v.context()
    case = BY_REGION["kept_without_seq"]
    bam.write_bam(str(tmp_path / "in.bam"), [tuple(r) for r in case["refs"]], case["records"])
    names, lengths = [nm for nm, _ in case["regions"]], [ln for _, ln in case["regions"]]
    L, h = _lib.lib(), ctx._h
    with ctx.bam_open(tmp_path / "in.bam") as s:
        with pytest.raises(ValueError):
            s.split(np.ones(s.n - 1, np.uint8), names, lengths, [0, 1], [tmp_path / "a", tmp_path / "b"], 0.95, 73, 68)
        with pytest.raises(_lib.UmiclustError) as e:  # a bucket that is none of the paths
            s.split(None, names, lengths, [0, 2], [tmp_path / "a", tmp_path / "b"], 0.95, 73, 68)
        assert e.value.code == EINVAL
        with pytest.raises(_lib.UmiclustError) as e:
            s.split(None, names, lengths, [0, 1], [tmp_path / "absent" / "a", tmp_path / "b"], 0.95, 73, 68)
        assert e.value.code == EIO
        assert not os.path.exists(tmp_path / "a")
    with ctx.bam_open(tmp_path / "in.bam") as s:
        pass
    with pytest.raises(_lib.UmiclustError) as e:
        ctx._check(L.umiclust_bam_name_suffix(h, None, None), "name_suffix")
    assert e.value.code == ESTATE
    counts = np.zeros(4, np.int64)
    assert L.umiclust_bam_split(h, None, 0, None, None, None, 0, None, 0.9, 0, 0, _lib._i64(counts), None, None, None,
                                0) == ESTATE


def test_refusal_order_of_the_six_split_entries(tmp_path):
    """What each of the six split entries refuses first, by raw ABI calls.  Round 2 (umiclust_bam_split[_extract]) asks
    for the session before it looks at an argument; the round-1 session entries check their arguments and the UMI
    patterns first and ask for the session afterwards; in all of them the umis_per_* check and the patterns come before
    the remaining arguments; and a counter capacity below the cluster ids is UMICLUST_ERANGE only after the files are
    written and the counters below the capacity are filled."""
    ERANGE = -34
    ctx = _v.context()
    case = BY_REGION["kept_without_seq"]
    bam.write_bam(str(tmp_path / "in.bam"), [tuple(r) for r in case["refs"]], case["records"])
    names, lengths = [nm for nm, _ in case["regions"]], [ln for _, ln in case["regions"]]
    L, h, P = _lib.lib(), ctx._h, _lib.C.POINTER
    c_i32, c_u8 = _lib.C.c_int32, _lib.C.c_uint8
    nm = (_lib.C.c_char_p * 2)(*[x.encode() for x in names])
    ln, cl = np.asarray(lengths, np.int64), np.asarray([0, 1], np.int32)
    counts, rpc, upc = np.zeros(4, np.int64), np.full(2, -1, np.int64), np.zeros(2, np.int64)
    regions = (2, nm, _lib._i64(ln), cl.ctypes.data_as(P(c_i32)))
    paths = (_lib.C.c_char_p * 2)(*[str(tmp_path / ("b%d.fasta" % k)).encode() for k in range(2)])
    out = str(tmp_path).encode()
    umi = (73, 68, 3, b"TTTVVVVTTVVVVTTVVVVTTVVVVTTT", b"AAABBBBAABBBBAABBBBAABBBBAAA")
    last = lambda: L.umiclust_last_error(h).decode()
    with ctx.bam_open(tmp_path / "in.bam"):
        # the umis_per_bucket check comes before the region arguments (nregions < 0 here)
        assert L.umiclust_bam_split_extract(h, None, -1, None, None, None, 2, paths, 0.95, 73, 68, *umi,
                                            _lib._i64(counts), _lib._i64(rpc), None, None, None, 0) == EINVAL
        # capacity 1, cluster ids 0 and 1: refused after the files and the counters
        assert L.umiclust_region_split(h, str(tmp_path / "in.bam").encode(), *regions, 0.95, 73, 68, out,
                                       _lib._i64(counts), _lib._i64(rpc), 1, None, None, 0) == ERANGE
        assert "cluster ids up to 1 exceed the counter capacity" in last()
        assert sorted(os.listdir(tmp_path)) == ["in.bam", "region_cluster0.fasta", "region_cluster1.fasta"]
        assert (tmp_path / "region_cluster0.fasta").read_text() == case["out_files"]["region_TRBV1_1.fasta"]
        assert (tmp_path / "region_cluster1.fasta").read_text() == case["out_files"]["region_TRBV2_2.fasta"]
        assert rpc.tolist() == [3, -1] and counts.tolist() == [0, 6, 1, 0]
    # no session
    assert L.umiclust_bam_split(h, None, 0, None, None, None, 0, None, 0.9, 0, 0, None, None, None, None, 0) == ESTATE
    assert L.umiclust_bam_split_extract(h, None, 0, None, None, None, 0, None, 0.9, 0, 0, *umi, None, None, None, None,
                                        None, 0) == ESTATE
    tail = (_lib._i64(counts), _lib._i64(rpc))
    assert L.umiclust_bam_region_split(h, *regions, 0.95, 73, 68, None, *tail, 2, None, None, 0) == EINVAL
    assert L.umiclust_bam_region_split_extract(h, *regions, 0.95, 73, 68, *umi, None, *tail, _lib._i64(upc), 2, None,
                                               None, 0) == EINVAL
    assert last() == "bad argument"
    assert L.umiclust_bam_region_split(h, *regions, 0.95, 73, 68, out, *tail, 2, None, None, 0) == ESTATE
    assert L.umiclust_bam_region_split_extract(h, *regions, 0.95, 73, 68, *umi, out, *tail, _lib._i64(upc), 2, None,
                                               None, 0) == ESTATE
    long_umi = umi[:3] + (b"N" * 65, umi[4])
    assert L.umiclust_bam_region_split_extract(h, *regions, 0.95, 73, 68, *long_umi, None, *tail, _lib._i64(upc), 2,
                                               None, None, 0) == EINVAL
    assert last() == "UMI patterns of 1..64 symbols are supported (got 65)"
    assert sorted(os.listdir(tmp_path)) == ["in.bam", "region_cluster0.fasta", "region_cluster1.fasta"]
