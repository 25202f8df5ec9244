"""The DEFLATE decoder of the device inflate without a GPU: csrc/inflate.h is HIP-free, and
uc::inflate_block -- the serial decoder on the pieces k_bgzf_inflate runs -- goes through every block of
tests/inflate_cases.py under ASan + UBSan (tools/inflate_check_main.cpp, `make inflate_check`).  Python's zlib is the
reference: a block is accepted exactly when zlib accepts it under the host reader's rule, and gives zlib's bytes.  The
framing walk io::bgzf_blocks is checked on damaged framing.  A sanitizer report fails the test."""
import gzip
import os
import re
import shutil
import struct
import subprocess

import pytest

import inflate_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")


def test_the_case_set():
    """the conditions on the set, before anything else uses it"""
    v, d = ic.valid_blocks(), ic.damaged()
    assert len(v) == 48 and all(b.expect == ic.valid()[b.name][1] for b in v)
    for n in (1, 63, 64, 65, 257, 258, 259, 4096, 0xff00, 65536):
        assert len(ic.valid()[f"dyn_{n}"][1]) == len(ic.valid()[f"fixed_{n}"][1]) == n
    assert "stored_65536" not in ic.valid() and len(ic.valid()["stored_65280"][1]) == 0xff00
    # the encodings are what their names say: the first block's BTYPE
    btype = {k: (c[0] >> 1) & 3 for k, (c, _) in ic.valid().items()}
    assert all(btype[k] == 0 for k in btype if k.startswith("stored_") or k == "empty_stored")
    # (zlib stores the shortest payloads whatever it was asked for: their 36 random header bytes do not compress)
    assert all(btype[f"fixed_{n}"] == 1 for n in (257, 258, 259, 4096, 0xff00, 65536)) and btype["one_byte_fixed"] == 1
    assert all(btype[f"dyn_{n}"] == 2 for n in (4096, 0xff00, 65536)) and btype["level9"] == 2
    flips = [b for b in d if b.kind == "flip"]
    rejected = sum(b.expect is None for b in flips)
    assert rejected >= 300 and len(flips) - rejected >= 300, (rejected, len(flips))
    assert len(flips) == 24 * sum(len(c) >= 8 for c, _ in ic.valid().values())
    assert all(b.expect is None for b in d if b.kind in ("cut", "isize"))  # zlib refuses every one of them
    assert sum(b.expect is not None and b.expect != ic.valid()[b.name.split("/")[0]][1] for b in flips) >= 300
    assert ic.damaged() is d  # built once


@pytest.fixture(scope="module")
def inflate_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("inflate_check")
    b = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ont-tcrconsensus_amd"), "inflate_check", f"SAN_OUT={out}"],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    assert "warning" not in b.stderr, b.stderr

    def run(mode, path, rc=0):
        r = subprocess.run([str(out / "inflate_check"), mode, str(path)], capture_output=True, text=True, timeout=300,
                           env=SAN_ENV)
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
        assert r.returncode == rc, (r.stdout[-2000:], r.stderr[-2000:])
        return r.stdout
    return run


def test_inflate_h_is_hip_free():
    """the header compiles with a plain C++ compiler and defines its host/device macro only under hipcc"""
    src = open(os.path.join(ROOT, "ont-tcrconsensus_amd", "csrc", "inflate.h")).read()
    assert "#include <hip" not in src
    assert re.search(r"#if defined\(__HIPCC__\)\s*\n#define UC_HD __host__ __device__\s*\n#else\s*\n#define UC_HD\s*\n#endif", src)


def run_cases(inflate_check, tmp_path, blocks):
    ic.write_case_file(tmp_path / "cases.bin", blocks)
    out = inflate_check("cases", tmp_path / "cases.bin")
    accepted = sum(b.expect is not None for b in blocks)
    assert f"blocks={len(blocks)} accepted={accepted} rejected={len(blocks) - accepted} bad=0" in out, out[-2000:]
    return {int(k): int(n) for k, n in re.findall(r"class (\d+) (\d+)", out)}


def test_valid_blocks_on_the_host_decoder(inflate_check, tmp_path):
    cls = run_cases(inflate_check, tmp_path, ic.valid_blocks())
    assert cls[0] == 48 and sum(cls.values()) == 48


def test_damaged_blocks_on_the_host_decoder(inflate_check, tmp_path):
    """accepted exactly when zlib accepts, zlib's bytes where both do; the damage reaches most error classes"""
    cls = run_cases(inflate_check, tmp_path, list(ic.damaged()))
    assert sum(1 for k, n in cls.items() if k and n) >= 8, cls


def hand_made():
    """streams no compressor writes: each decision of inflate.h that the flips may miss, zlib's verdict beside it"""
    def bits(*fields):  # (value, nbits) lowest bit first
        v = n = 0
        for x, w in fields:
            v |= x << n
            n += w
        return v.to_bytes((n + 7) // 8, "little")
    out = [("btype3", bits((1, 1), (3, 2)), 0),
           ("stored_bad_nlen", bits((1, 1), (0, 2), (0, 5)) + struct.pack("<HH", 3, 3) + b"abc", 3),
           ("stored_short_input", bits((1, 1), (0, 2), (0, 5)) + struct.pack("<HH", 3, 0xfffc) + b"ab", 3),
           ("hlit_287", bits((1, 1), (2, 2), (30, 5), (0, 5), (0, 4)) + b"\0" * 8, 0),
           ("hdist_31", bits((1, 1), (2, 2), (0, 5), (30, 5), (0, 4)) + b"\0" * 8, 0),
           # fixed code: literal 'a' (0x30 + 97 = 0x91, 8 bits, sent highest bit first), then a match of length 3 at
           # distance 2 (one byte written: too far), and the same at distance 1 (accepted: "aaaa")
           ("fixed_dist_too_far", bits((1, 1), (1, 2), (0b10001001, 8), (0b1000000, 7), (0b10000, 5), (0, 7)), 4),
           ("fixed_dist_1", bits((1, 1), (1, 2), (0b10001001, 8), (0b1000000, 7), (0b00000, 5), (0, 7)), 4),
           # the fixed code's two unused distance symbols 30 and 31, and the unused literal/length symbols 286 and 287
           ("fixed_dist_30", bits((1, 1), (1, 2), (0b10001001, 8), (0b1000000, 7), (0b01111, 5), (0, 7)), 4),
           ("fixed_len_286", bits((1, 1), (1, 2), (0b10001001, 8), (0b01100011, 8), (0, 7)), 1),
           # two blocks, the first not final and empty: a final-block bit that is clear keeps the decoder going
           ("two_blocks", bits((0, 1), (1, 2), (0, 7), (1, 1), (1, 2), (0b10001001, 8), (0, 7)), 1),
           ("no_final_block", bits((0, 1), (1, 2), (0b10001001, 8), (0, 7)), 1)]
    return [ic.Block(k, "hand", p, n, ic.reference(p, n)) for k, p, n in out]


def test_hand_made_streams(inflate_check, tmp_path):
    blocks = hand_made()
    verdict = {b.name: b.expect for b in blocks}
    assert verdict["fixed_dist_1"] == b"aaaa" and verdict["two_blocks"] == b"a"
    assert all(v is None for k, v in verdict.items() if k not in ("fixed_dist_1", "two_blocks")), verdict
    cls = run_cases(inflate_check, tmp_path, blocks)
    assert cls[0] == 2 and cls[2] == 1 and cls[3] == 1 and cls[4] == 2 and cls[8] == 1, cls


def test_framing_walk(inflate_check, tmp_path):
    blocks = ic.valid_blocks()[:5]
    good = ic.bgzf_file(blocks)

    def frames(data):
        (tmp_path / "f.bgzf").write_bytes(data)
        return inflate_check("frames", tmp_path / "f.bgzf").strip()
    assert frames(good) == "frames ok 6 %d" % sum(b.isize for b in blocks)
    assert frames(b"") == "frames ok 0 0"
    assert frames(ic.EOF_BLOCK) == "frames ok 1 0"
    first = len(ic.frame(blocks[0].payload, blocks[0].isize))
    assert frames(b"\x1f\x8c" + good[2:]) == "frames bad"  # bad magic
    assert frames(good[:first] + b"\x1f\x8b\x09" + good[first + 3:]) == "frames bad"  # ... of a later block
    assert frames(gzip.compress(b"x" * 100)) == "frames bad"  # plain gzip: no extra field
    noBC = bytearray(good)
    noBC[12:14] = b"XY"
    assert frames(bytes(noBC)) == "frames bad"  # an extra field, but not BC
    big = bytearray(good)
    big[first + 16:first + 18] = struct.pack("<H", 0xffff)
    assert frames(bytes(big[:first + 3000])) == "frames bad"  # BSIZE past the end
    assert frames(good[:-1]) == "frames bad" and frames(good + good[:17]) == "frames bad"  # a trailing partial block
    assert frames(good + b"\0") == "frames bad"
    small = bytearray(ic.EOF_BLOCK)
    small[16:18] = struct.pack("<H", 18)  # BSIZE + 1 = 19: smaller than header + trailer
    assert frames(bytes(small[:19])) == "frames bad"
    xlen = bytearray(ic.EOF_BLOCK)
    xlen[10:12] = struct.pack("<H", 4000)  # XLEN past the end
    assert frames(bytes(xlen)) == "frames bad"
