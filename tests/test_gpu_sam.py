"""The SAM-text open on the GPU: Context.sam_open -- lines, measure, sort and encode kernels of
csrc/samsort.hip on the rules of csrc/sam_text.h -- against the plain Python reference tests/sam_ref.py on every text
of tests/sam_cases.py.  For a text the library takes: the session's columns, names and strings equal bam_ref.Columns of
the reference's bytes, umiclust_bam_write with every record kept is well-formed BGZF that inflates to exactly those
bytes, and minimap2_align.samtools_sort leaves the same file.  For one it refuses: the code, the line, the field, and
no session."""
import os
import threading

import bam_ref
import numpy as np
import pytest
import sam_cases
import sam_ref
from umiclust import _lib, minimap2_align

pytestmark = pytest.mark.gpu

EIO, ERANGE, EFORMAT, ESTATE = -5, -34, -74, -77
CASES = sam_cases.cases()
TAKEN = [c for c in CASES if c[2] is None]
REFUSED = [c for c in CASES if c[2] is not None]


def check_columns(s, col):
    """the session's columns, groups, names and strings equal bam_ref's (as tests/test_gpu_bam_filter.py checks them)"""
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


def first_difference(got: bytes, want: bytes, roff):
    """the record and the byte at which two BAM streams part, for the assertion's message"""
    if got == want:
        return None
    x = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    rec = max([r for r, o in enumerate(roff) if o <= x], default=-1)
    return dict(byte=x, record=rec, in_record=x - roff[rec] if rec >= 0 else x, sizes=(len(got), len(want)))


@pytest.mark.parametrize("name,text,refusal", TAKEN, ids=[c[0] for c in TAKEN])
def test_open_write_and_sort_equal_the_reference(gpu_ctx, tmp_path, name, text, refusal):
    raw, roff = sam_ref.encode(text)
    path = tmp_path / "in.sam"
    path.write_bytes(text)
    with gpu_ctx.sam_open(path) as s:
        check_columns(s, bam_ref.Columns(raw))
        assert s.inflate_info() == (0, 0, 0) and s.first_malformed == -1
        info = s.sam_info()
        head, lines = sam_ref.split(text)
        assert (info["lines"], info["records"]) == (len(head) + len(lines), len(lines))
        assert info["f_values"] == sum(f[3:5] == b"f:" for ln in lines for f in ln.split(b"\t")[11:])
        assert s.write(np.ones(s.n, np.uint8), tmp_path / "out.bam") == len(roff)
    got = bam_ref.check_bgzf(tmp_path / "out.bam")
    assert got == raw, first_difference(got, raw, roff)
    assert minimap2_align.samtools_sort(path, tmp_path / "sorted.bam") == len(roff)
    assert (tmp_path / "sorted.bam").read_bytes() == (tmp_path / "out.bam").read_bytes()


@pytest.mark.parametrize("name,text,refusal", REFUSED, ids=[c[0] for c in REFUSED])
def test_refusals_name_the_line_and_leave_no_session(gpu_ctx, tmp_path, name, text, refusal):
    code, lineno, field, holds = refusal
    path = tmp_path / "in.sam"
    path.write_bytes(text)
    with pytest.raises(_lib.UmiclustError) as e:
        gpu_ctx.sam_open(path)
    assert e.value.code == dict(EFORMAT=EFORMAT, ERANGE=ERANGE)[code]
    assert "line %d: %s" % (lineno, field) in str(e.value) and (holds or "") in str(e.value)
    assert _lib.lib().umiclust_bam_counts(gpu_ctx._h, _lib._i64(np.zeros(5, np.int64))) == ESTATE


def test_text_from_a_fifo(gpu_ctx, tmp_path):
    """a path that is no regular file is read to its end: 5,000 records through a FIFO, far more than a pipe holds"""
    text = dict((c[0], c[1]) for c in CASES)["order_5000"]
    raw, roff = sam_ref.encode(text)
    fifo = tmp_path / "sam.fifo"
    os.mkfifo(fifo)

    def feed():
        with open(fifo, "wb") as fh:
            fh.write(text)

    t = threading.Thread(target=feed)
    t.start()
    try:
        with gpu_ctx.sam_open(fifo) as s:
            assert s.n == len(roff) and s.sam_info()["text_bytes"] == len(text) - text.index(b"q0\t")
            s.write(np.ones(s.n, np.uint8), tmp_path / "out.bam")
    finally:
        t.join()
    assert bam_ref.check_bgzf(tmp_path / "out.bam") == raw


def test_every_bam_call_works_on_the_session(gpu_ctx, tmp_path):
    """a keep mask on write, and a second open that replaces the first"""
    text = dict((c[0], c[1]) for c in CASES)["order_257"]
    raw, roff = sam_ref.encode(text)
    col = bam_ref.Columns(raw)
    (tmp_path / "in.sam").write_bytes(text)
    keep = (np.arange(len(roff)) % 3 == 0).astype(np.uint8)
    with gpu_ctx.sam_open(tmp_path / "in.sam") as s:
        assert s.write(keep, tmp_path / "third.bam") == int(keep.sum())
        assert s.name_suffix()[1].tolist() == [0] * s.n  # "q17" has no "_" field of digits alone
    assert bam_ref.check_bgzf(tmp_path / "third.bam") == col.expected_stream(keep)
    bam_ref.write_bgzf(tmp_path / "sorted.bam", raw)
    with gpu_ctx.bam_open(tmp_path / "sorted.bam") as s:
        check_columns(s, col)
        with pytest.raises(_lib.UmiclustError) as e:
            s.sam_info()
        assert e.value.code == ESTATE


def test_errors(gpu_ctx, tmp_path):
    with pytest.raises(_lib.UmiclustError) as e:
        gpu_ctx.sam_open(tmp_path / "missing.sam")
    assert e.value.code == EIO
