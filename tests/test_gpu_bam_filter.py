"""§8f row f6 on the GPU: the BAM session's device columns and cs groups against tests/bam_ref.py, and
both drop-ins of umiclust.minimap2_align end to end against what the reference's own functions left on the same inputs
(tests/golden/bam_filter, made by tests/golden/make_golden_bam_filter.py)."""
import os
import random

import numpy as np
import pytest
from test_bam_filter_cpu import CASES, MALFORMED, RUNNING, check_against_fixture, check_census, report_of, run_drop_in
from umiclust import _lib, minimap2_align, synth
from umiclust import vsearch_umi_cluster as _v

import bam_ref

pytestmark = pytest.mark.gpu

EIO, EINVAL, ERANGE, EFORMAT, ESTATE = -5, -22, -34, -74, -77


def check_columns(s, col):
    """the session's columns, groups, names and strings equal bam_ref's"""
    assert (s.n, s.n_refs, s.n_cs_groups) == (col.n, len(col.ref_names), len(col.group_strings))
    assert s.ref_names == col.ref_names and np.array_equal(s.ref_lengths, col.ref_lengths)
    for k in ("cls", "ref", "l_seq", "reference_length", "cols", "nm", "nm_present", "cs_group"):
        got, want = getattr(s, k), getattr(col, k)
        assert got.dtype == want.dtype and np.array_equal(got, want), (k, np.flatnonzero(got != want)[:5])
    assert np.array_equal(s.group_count, col.group_count) and np.array_equal(s.group_rep, col.group_rep)
    assert s.cs_strings(s.group_rep) == col.group_strings
    every = np.arange(s.n)
    assert s.query_names(every) == col.query_names(every)
    assert s.cs_strings(every) == col.cs_strings(every)


@pytest.mark.parametrize("name", RUNNING)
def test_device_columns_and_groups(name, tmp_path):
    case = CASES[name]
    raw = bam_ref.write_bam(tmp_path / "in.bam", case["refs"], case["records"], block=4000 if name == "aux_walk" else 60000)
    with _v.context().bam_open(tmp_path / "in.bam") as s:
        check_columns(s, bam_ref.Columns(raw))
        assert s.n_hash_reruns == 0
        assert s.first_malformed == -1  # the aux fields of a record the reference never reads are not walked


@pytest.mark.parametrize("name", RUNNING)
def test_drop_ins_equal_the_reference(name, tmp_path, monkeypatch):
    case = CASES[name]
    raw = bam_ref.write_bam(tmp_path / (name + ".bam"), case["refs"], case["records"])
    got = run_drop_in(None, case, tmp_path, monkeypatch, name)
    check_against_fixture(got, case, raw)
    check_census(str(tmp_path / (name + ".bam")), case)
    if case["expect"]["error"] is None:
        with open(tmp_path / "census.txt", "w") as fh:
            minimap2_align.write_cs_tag_report(fh, tmp_path / (name + ".bam"))
        if case["expect"]["cs_error"] is None:
            assert open(tmp_path / "census.txt").read() == report_of(case["expect"])
    if name == "big_output":
        assert len(got[4]) > 0x10000 and os.path.getsize(tmp_path / (name + "_filtered.bam")) > 28
    if name == "zero_kept":
        assert got[3] == [] and got[4] == raw[:bam_ref.decode(raw)[1]]


def test_last_record_cs_ends_the_buffer(tmp_path):
    case = CASES["last_record"]
    raw = bam_ref.write_bam(tmp_path / "in.bam", case["refs"], case["records"])
    assert raw.endswith(case["records"][-1]["tags"][-1][2].encode() + b"\0")  # the clamp: nothing to read after it
    with _v.context().bam_open(tmp_path / "in.bam") as s:
        check_columns(s, bam_ref.Columns(raw))


@pytest.mark.parametrize("name", MALFORMED)
def test_malformed_primary_record_is_eformat(name, tmp_path):
    case = CASES[name]
    bam_ref.write_bam(tmp_path / "in.bam", case["refs"], case["records"])
    ctx = _v.context()
    with pytest.raises(_lib.UmiclustError) as e:
        ctx.bam_open(tmp_path / "in.bam")
    r = case["eformat_record"]
    assert e.value.code == EFORMAT and "record %d (%s)" % (r, case["records"][r]["name"]) in str(e.value)
    with pytest.raises(_lib.UmiclustError) as e:  # no session was left open
        _lib.BamSession(ctx)
    assert e.value.code == ESTATE


def test_forced_collision_reruns_and_stays_exact(tmp_path):
    case = CASES["forced_collision"]
    raw = bam_ref.write_bam(tmp_path / "in.bam", case["refs"], case["records"])
    col = bam_ref.Columns(raw)
    assert len(col.group_strings) >= 300  # more strings than 8-bit hashes: the first pass must collide
    with _v.context().bam_open(tmp_path / "in.bam", hash_bits=case["hash_bits"]) as s:
        assert s.n_hash_reruns >= 1
        check_columns(s, col)
        masked = (s.cs_group.copy(), s.group_count.copy(), s.group_rep.copy())
    with _v.context().bam_open(tmp_path / "in.bam", hash_bits=64) as s:
        assert s.n_hash_reruns == 0
        assert all(np.array_equal(a, b) for a, b in zip(masked, (s.cs_group, s.group_count, s.group_rep)))


def random_records(rng, n, nrefs):
    pool = [":%d*%s:%d" % (rng.randrange(1, 200), rng.choice(["ag", "ct"]), rng.randrange(1, 200)) + "+acgt" * rng.randrange(0, 60)
            for _ in range(150)]
    fill = [("XA", "A", "q"), ("Xc", "c", -7), ("XS", "S", 513), ("Xi", "i", -9), ("Xf", "f", 0.25), ("XH", "H", "00FF"),
            ("XB", "B", ["s", [1, -2, 3]]), ("Xb", "B", ["I", []])]
    recs = []
    for i in range(n):
        nops = rng.choice([0, 1, 2, 5, 63, 64, 65, 140])
        cigar = [[rng.choice("MIDNSHP=X"), rng.randrange(1, 40)] for _ in range(nops)]
        tags = [list(rng.choice(fill)) for _ in range(rng.randrange(0, 4))]
        tags.append(["ZZ", "Z", "z" * rng.randrange(0, 200)])
        if rng.random() < 0.9:
            tags.append(["NM", rng.choice("cCsSiI"), rng.randrange(0, 100)])
        if rng.random() < 0.9:
            tags.append(["cs", "Z", rng.choice(pool) if rng.random() < 0.8 else ":%d" % i])
        rng.shuffle(tags)
        flag = rng.choice([0, 0, 0, 0, 16, 4, 0x100, 0x800])
        recs.append({"name": "r%d_%d" % (i, rng.randrange(1, 40)), "flag": flag, "ref": rng.randrange(-1, nrefs), "pos": i,
                     "cigar": cigar, "l_seq": rng.randrange(0, 300), "tags": tags})
    return recs


def test_random_2000_records_columns_and_writer(tmp_path):
    rng = random.Random(6)
    refs = [["ref%d" % r, 100 + r] for r in range(7)]
    raw = bam_ref.write_bam(tmp_path / "in.bam", refs, random_records(rng, 2000, len(refs)), block=0xff00)
    col = bam_ref.Columns(raw)
    keep = np.array([rng.random() < 0.5 for _ in range(col.n)], np.uint8)
    with _v.context().bam_open(tmp_path / "in.bam") as s:
        check_columns(s, col)
        assert s.times["device_s"] > 0 and s.times["inflate_s"] > 0
        for k, path in ((keep, "half.bam"), (np.ones(col.n, np.uint8), "all.bam"), (np.zeros(col.n, np.uint8), "none.bam")):
            assert s.write(k, tmp_path / path) == int(k.sum())
            assert bam_ref.check_bgzf(tmp_path / path) == col.expected_stream(k)
    assert len(col.expected_stream(keep)) > 2 * 0xff00  # several blocks


def test_session_errors(tmp_path):
    ctx = _v.context()
    with pytest.raises(_lib.UmiclustError) as e:
        ctx.bam_open(tmp_path / "absent.bam")
    assert e.value.code == EIO
    (tmp_path / "text.bam").write_bytes(b"@HD\tVN:1.6\n")
    with pytest.raises(_lib.UmiclustError) as e:
        ctx.bam_open(tmp_path / "text.bam")
    assert e.value.code == EIO
    bam_ref.write_bgzf(tmp_path / "notbam.bam", b"SAM\x01" + b"\0" * 40)
    with pytest.raises(_lib.UmiclustError) as e:
        ctx.bam_open(tmp_path / "notbam.bam")
    assert e.value.code == EFORMAT
    case = CASES["last_record"]
    raw = bam_ref.build_raw(case["refs"], case["records"])
    bam_ref.write_bgzf(tmp_path / "cut.bam", raw[:-5])
    with pytest.raises(_lib.UmiclustError) as e:
        ctx.bam_open(tmp_path / "cut.bam")
    assert e.value.code == EFORMAT and "truncated BAM record 2" in str(e.value)
    bam_ref.write_bgzf(tmp_path / "ok.bam", raw)
    s = ctx.bam_open(tmp_path / "ok.bam")
    L, h = _lib.lib(), ctx._h
    idx, off, buf = np.arange(3, dtype=np.int64), np.zeros(4, np.int64), np.zeros(4, np.uint8)
    assert L.umiclust_bam_strings(h, 1, _lib._i64(idx), 3, buf.ctypes.data, 4, _lib._i64(off)) == ERANGE
    assert L.umiclust_bam_strings(h, 1, _lib._i64(idx), 3, None, 0, None) == sum(len(x) for x in s.cs_strings(idx))
    assert L.umiclust_bam_strings(h, 2, _lib._i64(idx), 3, None, 0, None) == EINVAL
    idx[2] = 3
    assert L.umiclust_bam_strings(h, 0, _lib._i64(idx), 3, None, 0, None) == EINVAL
    s.close()
    for call in (lambda: _lib.BamSession(ctx), lambda: ctx._check(L.umiclust_bam_close(h), "close"),
                 lambda: ctx._check(L.umiclust_bam_write(h, None, b"x.bam"), "write")):
        with pytest.raises(_lib.UmiclustError) as e:
            call()
        assert e.value.code == ESTATE


def test_context_closed_while_every_drop_in_holds_state(tmp_path):
    """A context is torn down with the f5 events and staging slots, the f1 window buffers and an open BAM session
    still in it; a second context on the same device then computes the same."""
    name = min(RUNNING, key=lambda k: len(CASES[k]["records"]))
    raw = bam_ref.write_bam(tmp_path / "in.bam", CASES[name]["refs"], CASES[name]["records"])
    rng = random.Random(13)
    quals = [b"", b"!", bytes(rng.randrange(33, 75) for _ in range(70))]
    reads = ["".join(rng.choice("ACGT") for _ in range(200)) for _ in range(2)]
    umis = [["".join(rng.choice("ACGT") for _ in range(64)) for _ in range(2)] for _ in range(2)]
    umis[1][0] = umis[0][1]

    def every_drop_in(ctx):
        ee = ctx.fastq_ee(quals)
        ex = ctx.extract_umis(reads, fwd=synth.UMI_FWD, rev=synth.UMI_REV)
        ov = ctx.overlap_counts(umis[0], umis[1])
        return [np.array(a) for a in (*ee, ex, ov)], ctx.bam_open(tmp_path / "in.bam")

    ctx = _lib.Context(_v._device())
    first, s = every_drop_in(ctx)
    check_columns(s, bam_ref.Columns(raw))
    ctx.close()  # the session is still open
    with _lib.Context(_v._device()) as ctx:
        again, s = every_drop_in(ctx)
        assert len(first) == len(again) and all(np.array_equal(a, b) for a, b in zip(first, again))
        assert list(first[0][:2]) == [0, 1 << 40] and list(first[4]) == [0, 1]  # "!" is Q0, p = 1
        check_columns(s, bam_ref.Columns(raw))
        s.close()
