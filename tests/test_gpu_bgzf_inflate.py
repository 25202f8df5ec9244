"""BGZF blocks inflated on the device: k_bgzf_inflate through Context.bgzf_inflate on every block of
tests/inflate_cases.py -- Python's zlib is the reference: zlib's bytes for every block it accepts, a non-zero status
for exactly the blocks it refuses -- and the BAM readers on it: one BAM written as 0xff00-byte blocks and as 997-byte
blocks of every encoding gives the same session, the same written file and the same region split."""
import gzip
import os
import re
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest
from umiclust import _lib

import bam_ref
import inflate_cases as ic
from test_gpu_bam_filter import check_columns

pytestmark = pytest.mark.gpu

EFORMAT = -74
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_decoder(tmp_path_factory):
    """tools/inflate_check_main.cpp built WITHOUT sanitizers (`make inflate_check INFLATE_SAN=`): the host restatement
    as a plain program.  Its run under ASan + UBSan belongs to the CPU suite (tests/test_bgzf_inflate_cpu.py, the same
    seeded blocks)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("inflate_check_plain")
    b = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ont-tcrconsensus_amd"), "inflate_check", "INFLATE_SAN=",
                        f"SAN_OUT={out}"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr

    def run(blocks, path):
        ic.write_case_file(path, blocks)
        r = subprocess.run([str(out / "inflate_check"), "cases", str(path)], capture_output=True, text=True, timeout=300)
        accepted = sum(b.expect is not None for b in blocks)
        assert r.returncode == 0 and re.search(
            rf"blocks={len(blocks)} accepted={accepted} rejected={len(blocks) - accepted} bad=0\n", r.stdout), r.stdout[-2000:]
    return run


def offsets(blocks):
    return np.concatenate([[0], np.cumsum([b.isize for b in blocks])])


def test_all_valid_blocks(gpu_ctx):
    blocks = ic.valid_blocks()
    data = ic.bgzf_file(blocks)
    want = b"".join(b.expect for b in blocks)
    L = _lib.lib()
    nblk = _lib.C.c_int64(0)
    src = np.frombuffer(data, np.uint8)
    assert L.umiclust_bgzf_inflate(gpu_ctx._h, src.ctypes.data, len(src), None, 0, None, _lib.C.byref(nblk), None) == len(want)
    assert nblk.value == len(blocks) + 1
    out, status, err = gpu_ctx.bgzf_inflate(data, want_status=True)
    assert err is None and status.tolist() == [0] * (len(blocks) + 1)
    got, off = out.tobytes(), offsets(blocks)
    for k, b in enumerate(blocks):  # name the first block that differs
        assert got[off[k]:off[k + 1]] == b.expect, b.name
    assert got == want
    assert gpu_ctx.bgzf_inflate(data).tobytes() == want
    assert gpu_ctx.bgzf_times["kernel_s"] > 0
    assert len(gpu_ctx.bgzf_inflate(ic.EOF_BLOCK)) == 0 and len(gpu_ctx.bgzf_inflate(b"")) == 0


def test_all_damaged_blocks(gpu_ctx, host_decoder, tmp_path):
    """Error handling in a decoder whose loops are bounded: one file, one call, one launch -- after the host
    restatement of the kernel has passed the same blocks (and, in the CPU suite, passed them under ASan + UBSan)."""
    blocks = list(ic.damaged())
    host_decoder(blocks, tmp_path / "cases.bin")
    data = ic.bgzf_file(blocks)
    out, status, err = gpu_ctx.bgzf_inflate(data, want_status=True)
    assert len(status) == len(blocks) + 1 and status[-1] == 0
    rejected = [k for k, b in enumerate(blocks) if b.expect is None]
    assert np.flatnonzero(status).tolist() == rejected
    assert isinstance(err, _lib.UmiclustError) and err.code == EFORMAT
    assert f"BGZF block {rejected[0]}:" in str(err) and f"(class {status[rejected[0]]})" in str(err)
    with pytest.raises(_lib.UmiclustError) as e:
        gpu_ctx.bgzf_inflate(data)
    assert e.value.code == EFORMAT and f"BGZF block {rejected[0]}:" in str(e.value)
    got, off = out.tobytes(), offsets(blocks)
    for k, b in enumerate(blocks):
        if b.expect is not None:
            assert got[off[k]:off[k + 1]] == b.expect, b.name
    with pytest.raises(_lib.UmiclustError) as e:  # framing: refused before any launch
        gpu_ctx.bgzf_inflate(data[:-1], want_status=True)
    assert e.value.code == EFORMAT and "framing" in str(e.value)


# ---------------------------------------------------------------- the BAM readers on it
def small_block_file(raw: bytes, size: int = 997) -> bytes:
    """raw as `size`-byte blocks cycling stored / fixed / dynamic, an ISIZE-0 block in the middle, the EOF block"""
    pieces = [raw[i:i + size] for i in range(0, len(raw), size)]
    out = []
    for k, p in enumerate(pieces):
        if k == len(pieces) // 2:
            out.append(ic.EOF_BLOCK)
        payload = (ic.deflate(p, 0), ic.deflate(p, 6, zlib.Z_FIXED), ic.deflate(p, 6))[k % 3]
        out.append(ic.frame(payload, len(p), zlib.crc32(p)))
    return b"".join(out) + ic.EOF_BLOCK


def session_records():
    refs = [["regA", 760], ["regB", 720], ["regC", 700], ["other", 690]]
    recs = []
    for i in range(320):
        ref = i % 4
        ln = refs[ref][1] - (i % 7) * (i % 3)
        recs.append({"name": "read%d_%d" % (i, 1 + i % 9), "flag": (0, 0, 16, 0, 4, 0x100, 0, 0x800)[i % 8], "ref": ref, "pos": i % 5,
                     "cigar": "%dS%dM%dI%dM" % (i % 4 + 1, ln // 2, i % 3 + 1, ln - ln // 2),
                     "tags": [["NM", "i", i % 11], ["cs", "Z", ":%d*ag:%d" % (10 + i % 13, 20 + i % 5)]]})
    return refs, recs


def session_bam():
    refs, recs = session_records()
    return refs, bam_ref.build_raw(refs, recs)


@pytest.fixture(scope="module")
def two_layouts(tmp_path_factory):
    d = tmp_path_factory.mktemp("layouts")
    refs, raw = session_bam()
    assert 100_000 < len(raw) < 400_000
    bam_ref.write_bgzf(d / "big.bam", raw, block=0xff00)
    (d / "small.bam").write_bytes(small_block_file(raw))
    assert gzip.decompress((d / "small.bam").read_bytes()) == raw  # gzip takes it, CRCs and all
    return d, refs, raw


def test_bam_session_on_both_layouts(gpu_ctx, two_layouts, tmp_path):
    d, refs, raw = two_layouts
    col = bam_ref.Columns(raw)
    keep = (np.arange(col.n) % 3 != 1).astype(np.uint8)
    for name in ("big.bam", "small.bam"):
        size = os.path.getsize(d / name)
        data = (d / name).read_bytes()
        nblocks, nonempty, o = 0, 0, 0
        while o < size:
            bs = struct.unpack_from("<H", data, o + 16)[0] + 1
            nblocks, nonempty, o = nblocks + 1, nonempty + (struct.unpack_from("<I", data, o + bs - 4)[0] > 0), o + bs
        with gpu_ctx.bam_open(d / name) as s:
            check_columns(s, col)
            assert s.inflate_info() == (nblocks, nonempty, size)
            assert s.times["inflate_s"] > 0 and s.times["h2d_s"] > 0
            assert s.write(keep, tmp_path / ("kept_" + name)) == int(keep.sum())
            assert bam_ref.check_bgzf(tmp_path / ("kept_" + name)) == col.expected_stream(keep)
    assert nblocks == -(-len(raw) // 997) + 2 and nonempty == nblocks - 2
    assert min(len(bam_ref.encode_record(r)) for r in session_records()[1]) > 997  # every record straddles a block boundary


def test_region_split_on_both_layouts(gpu_ctx, two_layouts, tmp_path):
    d, refs, raw = two_layouts
    names, lengths = [r[0] for r in refs[:3]] + ["absent"], [r[1] for r in refs[:3]] + [100]
    got = {}
    for name in ("big.bam", "small.bam"):
        out, cut = tmp_path / name, tmp_path / ("cut_" + name)
        out.mkdir(), cut.mkdir()
        with pytest.raises(KeyError) as e:  # a record of "other", which is no region, ends the loop
            gpu_ctx.region_split(str(d / name), names, lengths, [0, 2, 0, 1], 0.8, 10, 10, str(cut))
        counts, rpc, det = gpu_ctx.region_split(str(d / name), names + ["other"], lengths + [690], [0, 2, 0, 1, 2], 0.8,
                                                10, 10, str(out))
        got[name] = (str(e.value), counts.tolist(), rpc.tolist(), det.tolist(),
                     {(p is cut, fn): (p / fn).read_bytes() for p in (out, cut) for fn in sorted(os.listdir(p))})
    assert got["big.bam"] == got["small.bam"]
    key, counts, rpc, det, files = got["big.bam"]
    assert key == "'other'" and sum(rpc) > 100 and det[3] == 0 and sum(det) == 4 and all(files.values())
