"""BGZF blocks deflated on the device: k_bgzf_deflate and k_bgzf_frame through Context.bgzf_deflate
on every input of tests/deflate_cases.py -- byte for byte the file the host restatement of the encoder writes
(tools/deflate_check_main.cpp, built plain), every member read back by Python's gzip and by the device's own inflate
-- and the BAM session's writer on it: batch seams, keep masks whose segments begin and end inside blocks, the host
switch, and samtools_sort's file."""
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from umiclust import _lib, minimap2_align

import bam_ref
import deflate_cases as dc
import sam_cases
import sam_ref
from test_gpu_bam_filter import check_columns

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_encoder(tmp_path_factory):
    """tools/deflate_check_main.cpp built WITHOUT sanitizers (`make deflate_check DEFLATE_SAN=`) over all cases: name ->
    (the BGZF bytes it wrote, the kinds of its blocks).  Its run under ASan + UBSan belongs to the CPU suite
    (tests/test_bgzf_deflate_cpu.py, the same inputs)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("deflate_check_plain")
    b = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ont-tcrconsensus_amd"), "deflate_check", "DEFLATE_SAN=",
                        f"SAN_OUT={out}"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    c = dc.cases()
    dc.write_case_file(out / "cases.bin", list(c.values()))
    r = subprocess.run([str(out / "deflate_check"), "cases", str(out / "cases.bin"), str(out / "out.bgzf")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"cases={len(c)} " in r.stdout and " bad=0" in r.stdout, r.stdout[-2000:]
    data, names, res = (out / "out.bgzf").read_bytes(), list(c), {}
    kinds = {k: [] for k in names}
    for i, kind in re.findall(r"block (\d+) \d+ kind=(\d)", r.stdout):
        kinds[names[int(i)]].append(int(kind))
    for i, off, size in re.findall(r"case (\d+) off=(\d+) size=(\d+)", r.stdout):
        res[names[int(i)]] = (data[int(off):int(off) + int(size)], kinds[names[int(i)]])
    assert len(res) == len(c)
    return res


def test_all_cases_equal_the_host_restatement(gpu_ctx, host_encoder):
    """one call per input (a call cuts its input every 0xff00 bytes, so inputs of other lengths cannot share one);
    `everything` is all of them in one call"""
    for name, data in dc.cases().items():
        want, want_kinds = host_encoder[name]
        out, kinds = gpu_ctx.bgzf_deflate(data, want_info=True)
        got = out.tobytes()
        mem = dc.members(got)
        assert len(mem) == dc.n_blocks(data) + 1 and mem[-1] == dc.EOF_BLOCK, name
        for k, m in enumerate(mem[:-1]):  # name the first block that differs
            assert gzip.decompress(m) == data[k * dc.BLOCK:(k + 1) * dc.BLOCK], (name, k)
            assert len(m) - 26 <= min(dc.BLOCK, len(data) - k * dc.BLOCK) + 5, (name, k)
        assert kinds.tolist() == want_kinds, name
        assert got == want, name
        assert gpu_ctx.bgzf_inflate(got).tobytes() == data, name
        if data:
            assert gpu_ctx.bgzf_times["kernel_s"] > 0
    assert gpu_ctx.bgzf_deflate(b"").tobytes() == dc.EOF_BLOCK
    L, nblk = _lib.lib(), _lib.C.c_int64(-1)
    src = np.frombuffer(dc.cases()["everything"], np.uint8)
    bound = L.umiclust_bgzf_deflate(gpu_ctx._h, src.ctypes.data, len(src), None, 0, None, _lib.C.byref(nblk), None)
    assert nblk.value == dc.n_blocks(dc.cases()["everything"]) and bound >= len(host_encoder["everything"][0])
    small = np.zeros(100, np.uint8)
    assert L.umiclust_bgzf_deflate(gpu_ctx._h, src.ctypes.data, len(src), small.ctypes.data, 100, None, None, None) == -34


# ---------------------------------------------------------------- the session's writer
def session_records():
    """the 320-record shape of tests/test_gpu_bgzf_inflate.py"""
    refs = [["regA", 760], ["regB", 720], ["regC", 700], ["other", 690]]
    recs = []
    for i in range(320):
        ref = i % 4
        ln = refs[ref][1] - (i % 7) * (i % 3)
        recs.append({"name": "read%d_%d" % (i, 1 + i % 9), "flag": (0, 0, 16, 0, 4, 0x100, 0, 0x800)[i % 8], "ref": ref, "pos": i % 5,
                     "cigar": "%dS%dM%dI%dM" % (i % 4 + 1, ln // 2, i % 3 + 1, ln - ln // 2),
                     "tags": [["NM", "i", i % 11], ["cs", "Z", ":%d*ag:%d" % (10 + i % 13, 20 + i % 5)]]})
    return refs, recs


@pytest.fixture(scope="module")
def session_bam(tmp_path_factory):
    d = tmp_path_factory.mktemp("deflate_session")
    refs, recs = session_records()
    raw = bam_ref.build_raw(refs, recs)
    assert 3 * 0xff00 < len(raw) < 7 * 0xff00
    bam_ref.write_bgzf(d / "in.bam", raw, block=0xff00)
    col = bam_ref.Columns(raw)
    r = np.arange(col.n)
    masks = {"all": np.ones(col.n, np.uint8), "none": np.zeros(col.n, np.uint8), "third": (r % 3 != 1).astype(np.uint8),
             "runs": ((r // 7) % 2 == 0).astype(np.uint8)}
    return d / "in.bam", col, masks


@pytest.mark.parametrize("batch", [1, 2])
def test_session_writer_across_batch_seams(session_bam, tmp_path, monkeypatch, batch):
    path, col, masks = session_bam
    monkeypatch.setenv("UMICLUST_BGZF_BATCH", str(batch))
    monkeypatch.delenv("UMICLUST_BGZF_WRITE", raising=False)
    with _lib.Context(0) as ctx:
        with ctx.bam_open(path) as s:
            for name, keep in masks.items():
                out = tmp_path / f"{name}.bam"
                want = col.expected_stream(keep)
                assert s.write(keep, out) == int(keep.sum())
                assert bam_ref.check_bgzf(out) == want, name
                info, nb = s.write_info(), -(-len(want) // 0xff00)
                assert (info["blocks"], info["device_blocks"], info["host_blocks"]) == (nb, nb, 0), name
                assert info["batches"] == -(-nb // batch), name
                assert info["stored"] + info["fixed"] + info["dynamic"] == nb and info["dynamic"] >= nb - 1
                assert info["compressed_bytes"] == os.path.getsize(out) and info["kernel_s"] > 0
        with ctx.bam_open(tmp_path / "third.bam") as s:  # the written file reopens to the same columns
            check_columns(s, bam_ref.Columns(col.expected_stream(masks["third"])))
    assert nb >= 2  # (the last mask's: more than one batch either way)


def test_host_switch(session_bam, tmp_path, monkeypatch):
    path, col, masks = session_bam
    monkeypatch.setenv("UMICLUST_BGZF_WRITE", "host")
    with _lib.Context(0) as ctx, ctx.bam_open(path) as s:
        with pytest.raises(_lib.UmiclustError):
            s.write_info()  # nothing written yet
        keep = masks["third"]
        assert s.write(keep, tmp_path / "host.bam") == int(keep.sum())
        info = s.write_info()
    want = col.expected_stream(keep)
    assert bam_ref.check_bgzf(tmp_path / "host.bam") == want
    assert info["device_blocks"] == 0 and info["batches"] == 0 and info["blocks"] == -(-len(want) // 0xff00)
    assert info["compressed_bytes"] == os.path.getsize(tmp_path / "host.bam")


def test_samtools_sort_writes_the_reference_stream(gpu_ctx, tmp_path):
    text = sam_cases.order_text(700).encode("latin-1")
    raw, roff = sam_ref.encode(text)
    (tmp_path / "in.sam").write_bytes(text)
    assert minimap2_align.samtools_sort(tmp_path / "in.sam", tmp_path / "sorted.bam") == len(roff)
    assert bam_ref.check_bgzf(tmp_path / "sorted.bam") == raw
