"""The .bai index and flagstat on the device: the kernels of bamindex.hip through
BamSession.index_probe on every case of tests/bai_cases.py, array by array against tests/bai_ref.py (the plain Python
restatement of policies O10 and O11); the indexed write under both batch sizes and the host writer, against bai_ref on
the block table of the file actually written, with the specification's reader contract on that file;
Context.bam_index_file against bai_ref, against the host restatement (tools/bai_check_main.cpp, built plain) and
against the indexed write; flagstat; the Python drop-ins; and the refusals."""
import os
import shutil
import stat
import subprocess
import warnings

import numpy as np
import pytest
from test_bam_filter_cpu import CASES as FILTER_CASES
from test_bam_filter_cpu import RUNNING
from umiclust import _lib, minimap2_align
from umiclust import vsearch_umi_cluster as _v

import bai_cases
import bai_ref
import bam_ref
import sam_cases
import sam_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIO, ESTATE, ERANGE, EFORMAT = -5, -77, -34, -74
BY_NAME = {c.name: c for c in bai_cases.CASES}
WRITTEN = ["empty", "nocoor_only", "refs_257", "boundaries", "cigars", "alternating_every_second", "keep_drop_first_of_ref",
           "keep_drop_whole_ref", "keep_none", "big_record", "multiple_of_block", "flags"]


def open_case(ctx, raw, tmp_path, block=60000):
    path = tmp_path / "in.bam"
    bam_ref.write_bgzf(path, raw, block)
    return ctx.bam_open(path)


def reader_contract(path, bai, ref):
    bai_ref.check_reader_contract(bai_ref.BgzfReader(path), bai, ref, bai_cases.query_grid(ref))


# ---------------------------------------------------------------- the kernels, array by array
@pytest.mark.parametrize("case", bai_cases.CASES, ids=repr)
def test_index_probe_equals_the_reference(case, tmp_path):
    ref = bai_ref.Index(case.raw, case.keep, case.coff, case.ustart)
    with open_case(_v.context(), case.raw, tmp_path) as s:
        got = s.index_probe(case.keep, case.coff, case.ustart)
        info = s.index_info()
    assert (got["n_kept"], got["first_bad"], got["first_status"], got["n_no_coor"]) == (ref.n_kept, -1, 0, ref.n_no_coor)
    for k in ("bin", "u", "v", "status", "n_intv", "mapped", "unmapped", "linear"):
        assert got[k].tolist() == getattr(ref, k), k
    assert got["runs"].tolist() == ref.runs and got["sorted_runs"].tolist() == ref.sorted_runs
    assert got["counters"].tolist() == bai_ref.flagstat(case.raw, case.keep)[0]
    assert (info["kept"], info["runs"], info["windows"]) == (ref.n_kept, len(ref.runs), len(ref.linear))


@pytest.mark.parametrize("name,raw,record,status,hide", bai_cases.REFUSALS, ids=[r[0] for r in bai_cases.REFUSALS])
def test_index_probe_names_the_refused_record(name, raw, record, status, hide, tmp_path):
    case, hidden = bai_cases.Case(name, raw), bai_cases.Case(name, raw, keep=hide)
    with open_case(_v.context(), raw, tmp_path) as s:
        got = s.index_probe(None, case.coff, case.ustart)
        assert (got["first_bad"], got["first_status"]) == (record, status)
        assert got["status"].tolist() == bai_ref.Index(raw, None, case.coff, case.ustart).status
        assert len(got["runs"]) == len(got["linear"]) == 0
        got = s.index_probe(hide, hidden.coff, hidden.ustart)
        assert got["first_bad"] == -1 and got["sorted_runs"].tolist() == bai_ref.Index(raw, hide, hidden.coff,
                                                                                       hidden.ustart).sorted_runs
        with pytest.raises(_lib.UmiclustError) as e:  # a table that ends elsewhere than the kept stream
            s.index_probe(hide, case.coff, case.ustart)
        assert e.value.code == -22


# ---------------------------------------------------------------- the indexed write
@pytest.mark.parametrize("mode", ["batch1", "batch2", "host"])
def test_write_index_indexes_the_file_it_wrote(mode, tmp_path, monkeypatch):
    monkeypatch.delenv("UMICLUST_BGZF_WRITE", raising=False)
    if mode == "host":
        monkeypatch.setenv("UMICLUST_BGZF_WRITE", "host")
    else:
        monkeypatch.setenv("UMICLUST_BGZF_BATCH", mode[-1])
    with _lib.Context(0) as ctx:
        for name in WRITTEN:
            case = BY_NAME[name]
            d = tmp_path / name
            d.mkdir()
            keep = case.keep if case.keep is not None else [1] * len(bai_cases.sizes_of(case.raw)[1])
            with open_case(ctx, case.raw, d) as s:
                out = d / "out.bam"
                assert s.write(keep, out, index=True) == sum(keep)
                info, winfo = s.index_info(), s.write_info()
            assert bam_ref.check_bgzf(out) == bam_ref.Columns(case.raw).expected_stream(keep), name
            assert (winfo["device_blocks"] == 0) == (mode == "host")
            coff, ustart = bai_ref.block_table(out)
            ref = bai_ref.Index(case.raw, keep, coff, ustart)
            bai = (d / "out.bam.bai").read_bytes()
            assert bai == ref.bytes, name
            assert (info["kept"], info["runs"], info["windows"]) == (ref.n_kept, len(ref.runs), len(ref.linear))
            assert info["chunks"] == sum(len(c) for b in ref.bins_of for c in b.values())
            reader_contract(out, bai, ref)


def test_write_index_path_and_plain_write_unchanged(tmp_path):
    case = BY_NAME["three_refs"]
    with open_case(_v.context(), case.raw, tmp_path) as s:
        keep = np.ones(s.n, np.uint8)
        assert s.write(keep, tmp_path / "plain.bam") == s.n and not (tmp_path / "plain.bam.bai").exists()
        assert s.write(keep, tmp_path / "named.bam", index=tmp_path / "elsewhere.bai") == s.n
        assert not (tmp_path / "named.bam.bai").exists()
        assert (tmp_path / "plain.bam").read_bytes() == (tmp_path / "named.bam").read_bytes()
        coff, ustart = bai_ref.block_table(tmp_path / "named.bam")
        assert (tmp_path / "elsewhere.bai").read_bytes() == bai_ref.Index(case.raw, None, coff, ustart).bytes
        with pytest.raises(_lib.UmiclustError) as e:
            s.write(keep, tmp_path / "again.bam", index=tmp_path / "no_such_dir" / "x.bai")
        assert e.value.code == EIO and (tmp_path / "again.bam").exists()


# ---------------------------------------------------------------- samtools index of a file
@pytest.fixture(scope="module")
def host_index(tmp_path_factory):
    """tools/bai_check_main.cpp built WITHOUT sanitizers (`make bai_check BAI_SAN=`): the host restatement as a plain
    program, or None without a compiler.  Its run under ASan + UBSan belongs to the CPU suite (tests/test_bai_cpu.py,
    the same cases)."""
    if shutil.which("g++") is None:
        return None  # the comparison with it is left out; the test itself needs no compiler
    out = tmp_path_factory.mktemp("bai_check_plain")
    b = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ont-tcrconsensus_amd"), "bai_check", "BAI_SAN=",
                        f"SAN_OUT={out}"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr

    def run(path):
        r = subprocess.run([str(out / "bai_check"), "file", str(path), str(out / "o.bai"), str(out / "o.txt")],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
        return (out / "o.bai").read_bytes()
    return run


@pytest.mark.parametrize("block", [60000, 300])
def test_bam_index_file(block, tmp_path, host_index):
    ctx = _v.context()
    for name in ("boundaries", "alternating", "cigars", "big_record", "many_refs", "refs_257", "refs_513", "empty"):
        raw, path = BY_NAME[name].raw, tmp_path / (name + ".bam")
        bam_ref.write_bgzf(path, raw, block)
        assert ctx.bam_index_file(path) == len(bai_cases.sizes_of(raw)[1])
        coff, ustart = bai_ref.block_table(path)
        ref = bai_ref.Index(raw, None, coff, ustart)
        bai = (tmp_path / (name + ".bam.bai")).read_bytes()
        assert bai == ref.bytes, name
        assert host_index is None or host_index(path) == bai, name
        reader_contract(path, bai, ref)


def test_bam_index_file_beside_a_session_and_on_the_written_file(tmp_path):
    case, ctx = BY_NAME["alternating"], _v.context()
    with open_case(ctx, case.raw, tmp_path) as s:
        keep = (np.arange(s.n) % 3 != 0).astype(np.uint8)
        s.write(keep, tmp_path / "out.bam", index=True)
        assert ctx.bam_index_file(tmp_path / "out.bam", tmp_path / "again.bai") == int(keep.sum())
        assert (tmp_path / "again.bai").read_bytes() == (tmp_path / "out.bam.bai").read_bytes()
        assert s.flagstat()[0]["total"] == (s.n, 0)  # the session is still the one that was opened
    with pytest.raises(_lib.UmiclustError) as e:
        ctx.bam_index_file(tmp_path / "absent.bam")
    assert e.value.code == EIO


# ---------------------------------------------------------------- flagstat
@pytest.mark.parametrize("name", ["flags", "flags_every_second", "cigars", "keep_none"])
def test_flagstat(name, tmp_path):
    case = BY_NAME[name]
    want, text = bai_ref.flagstat(case.raw, case.keep)
    with open_case(_v.context(), case.raw, tmp_path) as s:
        got, got_text = s.flagstat(case.keep)
    assert [x for k in s.FLAGSTAT_ROWS for x in got[k]] == want and got_text == text
    assert got_text.splitlines()[7].endswith(")") and " primary mapped (" in got_text.splitlines()[7]


def test_flagstat_needs_no_order(tmp_path):
    raw = bai_cases.REFUSALS[1][1]  # tid decreasing
    with open_case(_v.context(), raw, tmp_path) as s:
        assert s.flagstat()[1] == bai_ref.flagstat(raw)[1]


# ---------------------------------------------------------------- the Python drop-ins
def placed_text(n, seed=5) -> bytes:
    """sam_cases.order_text without its records at POS 0 of a reference: pos -1 in the BAM, which policy O10 refuses"""
    lines = sam_cases.order_text(n, seed=seed).splitlines(keepends=True)
    return "".join(ln for ln in lines if ln[0] == "@" or ln.split("\t")[2] == "*" or ln.split("\t")[3] != "0").encode("latin-1")


def test_samtools_sort_refuses_pos_0_of_a_reference(tmp_path):
    text = sam_cases.order_text(700).encode("latin-1")
    raw, roff = sam_ref.encode(text)
    (tmp_path / "in.sam").write_bytes(text)
    with pytest.raises(_lib.UmiclustError) as e:
        minimap2_align.samtools_sort(tmp_path / "in.sam", tmp_path / "sorted.bam", index=True)
    first = bam_ref.decode(raw)[2][0]
    assert (first.ref, first.pos) != (-1, -1) and first.pos == -1  # the sort puts them first
    assert e.value.code == ERANGE and "record 0 (%s)" % first.query_name in str(e.value)
    assert bam_ref.check_bgzf(tmp_path / "sorted.bam") == raw and not (tmp_path / "sorted.bam.bai").exists()


def test_samtools_sort_index_and_flagstat(tmp_path):
    text = placed_text(700)
    raw, roff = sam_ref.encode(text)
    (tmp_path / "in.sam").write_bytes(text)
    bam = tmp_path / "sorted.bam"
    assert minimap2_align.samtools_sort(tmp_path / "in.sam", bam, index=True) == len(roff)
    assert bam_ref.check_bgzf(bam) == raw
    coff, ustart = bai_ref.block_table(bam)
    ref = bai_ref.Index(raw, None, coff, ustart)
    bai = (tmp_path / "sorted.bam.bai").read_bytes()
    assert ref.first_bad < 0 and bai == ref.bytes
    reader_contract(bam, bai, ref)
    os.remove(tmp_path / "sorted.bam.bai")
    assert minimap2_align.samtools_index(bam) == len(roff) and (tmp_path / "sorted.bam.bai").read_bytes() == bai
    counters = minimap2_align.samtools_flagstat(bam, tmp_path / "flagstat.out")
    want, want_text = bai_ref.flagstat(raw)
    assert (tmp_path / "flagstat.out").read_text() == want_text and counters["total"] == (want[0], want[1])


@pytest.mark.parametrize("with_bam", [True, False])
def test_minimap2_ont_align_session_flagstat_and_index(tmp_path, monkeypatch, with_bam):
    text = placed_text(300)
    raw, roff = sam_ref.encode(text)
    (tmp_path / "prepared.sam").write_bytes(text)
    bindir, logs = tmp_path / "bin", tmp_path / "logs"
    bindir.mkdir(), logs.mkdir()
    stub = bindir / "minimap2"
    stub.write_text("#!/bin/sh\ncat %s\n" % (tmp_path / "prepared.sam"))
    stub.chmod(stub.stat().st_mode | stat.S_IXUSR)
    monkeypatch.setenv("PATH", str(bindir) + os.pathsep + os.environ["PATH"])
    bam = tmp_path / "lib7.sorted.bam" if with_bam else None
    src = minimap2_align.minimap2_ont_align_session("/data/lib1.fastq.gz", "/data/ref.fa", str(logs), 2, bam_file=bam,
                                                    index=with_bam, flagstat=True)
    try:
        stem = "lib7" if with_bam else "lib1"
        assert sorted(os.listdir(logs)) == sorted(["lib1_minimap2.err", stem + "_flagstat.out"])
        assert (logs / (stem + "_flagstat.out")).read_text() == bai_ref.flagstat(raw)[1]
        if with_bam:
            coff, ustart = bai_ref.block_table(bam)
            assert (tmp_path / "lib7.sorted.bam.bai").read_bytes() == bai_ref.Index(raw, None, coff, ustart).bytes
        else:
            assert not [f for f in os.listdir(tmp_path) if f.endswith((".bam", ".bai"))]
    finally:
        src.close()
    with pytest.raises(ValueError):
        minimap2_align.minimap2_ont_align_session("/data/lib1.fastq.gz", "/data/ref.fa", str(logs), 2, index=True)


def _sorted_filter_case():
    for name in RUNNING:
        case = FILTER_CASES[name]
        keys = [(r.get("ref", 0) & 0xffffffff, r.get("pos", 0)) for r in case["records"]]
        if case["expect"]["error"] is None and keys == sorted(keys) and len(case["expect"]["kept"]) > 1:
            return name
    raise AssertionError("no coordinate-sorted filter case")


def test_filter_consensus_alignments_indexes_on_the_device(tmp_path, monkeypatch):
    name = _sorted_filter_case()
    case = FILTER_CASES[name]
    bam_ref.write_bam(tmp_path / (name + ".bam"), case["refs"], case["records"])
    calls = []
    monkeypatch.setattr(minimap2_align.subprocess, "run", lambda *a, **k: calls.append(a[0]))
    logs, fasta = tmp_path / "logs", tmp_path / "ref.fa"
    logs.mkdir()
    bam_ref.write_fasta(fasta, case["regions"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = minimap2_align.filter_consensus_alignments(str(tmp_path / (name + ".bam")), str(fasta), str(logs),
                                                         index="device", **case["params"])
    assert calls == [] and out == str(tmp_path / (name + "_filtered.bam"))
    stream = bam_ref.check_bgzf(out)
    coff, ustart = bai_ref.block_table(out)
    ref = bai_ref.Index(stream, None, coff, ustart)
    assert ref.n_kept == len(case["expect"]["kept"]) and open(out + ".bai", "rb").read() == ref.bytes
    with pytest.raises(ValueError):
        minimap2_align.filter_consensus_alignments(str(tmp_path / (name + ".bam")), str(fasta), str(logs),
                                                   index="pysam", **case["params"])


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("name,raw,record,status,hide", bai_cases.REFUSALS, ids=[r[0] for r in bai_cases.REFUSALS])
def test_refusals_name_the_record_and_leave_no_index(name, raw, record, status, hide, tmp_path):
    ctx = _v.context()
    names = [r.query_name for r in bam_ref.decode(raw)[2]]
    code = {bai_ref.UNSORTED: EFORMAT, bai_ref.RANGE: ERANGE}[status]
    with open_case(ctx, raw, tmp_path) as s:
        out = tmp_path / "out.bam"
        (tmp_path / "out.bam.bai").write_bytes(b"stale")
        with pytest.raises(_lib.UmiclustError) as e:
            s.write(np.ones(s.n, np.uint8), out, index=True)
        assert e.value.code == code and "record %d (%s)" % (record, names[record]) in str(e.value)
        assert ("unsorted" in str(e.value)) == (status == bai_ref.UNSORTED)
        assert bam_ref.check_bgzf(out) == raw and not (tmp_path / "out.bam.bai").exists()
        with pytest.raises(_lib.UmiclustError) as e:  # the same file through samtools index
            ctx.bam_index_file(out)
        assert e.value.code == code and "record %d (%s)" % (record, names[record]) in str(e.value)
        assert not (tmp_path / "out.bam.bai").exists()
        assert s.write(hide, out, index=True) == sum(hide)  # the defect hidden by keep: accepted
        coff, ustart = bai_ref.block_table(out)
        assert (tmp_path / "out.bam.bai").read_bytes() == bai_ref.Index(raw, hide, coff, ustart).bytes


def test_no_open_session(tmp_path):
    with _lib.Context(0) as fresh:
        L, h = _lib.lib(), fresh._h
        assert L.umiclust_bam_write_index(h, None, str(tmp_path / "x.bam").encode(), None) == ESTATE
        assert L.umiclust_bam_flagstat(h, None, None, None, 0) == ESTATE
        assert L.umiclust_bam_index_info(h, None, None) == ESTATE
        one = np.zeros(1, np.int64)
        assert L.umiclust_bam_index_probe(h, None, _lib._i64(one), _lib._i64(one), 1, *([None] * 6), 0, None, None, 0,
                                          *([None] * 4)) == ESTATE
        assert not os.listdir(tmp_path)
