"""The DEFLATE encoder of the device writer without a GPU: csrc/deflate.h is HIP-free, and
uc::deflate_block -- the serial restatement of k_bgzf_deflate, 64 lanes in a loop -- goes through every input of
tests/deflate_cases.py under ASan + UBSan (tools/deflate_check_main.cpp, `make deflate_check`).  The program inflates
every block with C zlib and with uc::inflate_block and checks the payload bound and the code sets; here Python's gzip
reads every member, which also checks CRC32 and ISIZE.  A sanitizer report fails the test."""
import collections
import gzip
import os
import re
import shutil
import subprocess

import pytest

import deflate_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
STORED, FIXED, DYNAMIC = 0, 1, 2
LIT_LIMITED, DIST_LIMITED, CLEN_LIMITED, DIST_NONE, DIST_ONE = 1, 2, 4, 8, 16


def test_the_case_set():
    """the conditions on the set, before anything else uses it"""
    c = dc.cases()
    assert dc.cases() is c  # built once
    for n in (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 257, 258, 259, 260, 0xfeff, 0xff00):
        assert len(c[f"len_{n}"]) == n
    assert c["zeros"] == b"\0" * 0xff00 and len(c["random"]) == 0xff00
    for p in (1, 2, 3, 7, 63, 64, 65, 257, 258, 259):
        d = c[f"period_{p}"]
        assert len(d) > 2 * p + 258 and all(d[i] == d[i - p] for i in range(p, len(d)))
    for name, dist in (("dist_32768", 32768), ("dist_32769", 32769)):
        d = c[name]
        assert d[:300] == d[dist:dist + 300] and len(d) == dist + 304 <= 0xff00
        keep = {dc.hash4(d[i:i + 4]) for i in range(297)}
        assert not any(dc.hash4(d[i:i + 4]) in keep for i in range(297, dist))  # the candidates survive the filler
    assert sorted(c["all_bytes"]) == list(range(256)) and len(set(c["one_value"])) == 1 and len(set(c["two_values"])) == 2
    fib = c["fibonacci"]
    assert len({fib[i:i + 4] for i in range(len(fib) - 3)}) == len(fib) - 3 <= 0xff00  # no match is possible
    counts = sorted(collections.Counter(fib).values())
    assert counts[:14] == [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610]
    assert dc.huffman_depth(counts + [1]) > 15  # + the end-of-block symbol
    cl = c["code_lengths"]
    assert len({cl[i:i + 4] for i in range(len(cl) - 3)}) == len(cl) - 3 == 4092
    per_count = collections.Counter(collections.Counter(cl).values())  # symbols per literal count 2^(12 - l)
    per_count[1] += 1  # the end-of-block symbol
    assert {12 - n.bit_length() + 1: k for n, k in per_count.items()} == dc.code_length_plan()
    # (these eleven counts alone give a 7-bit code-length code; the zero lengths' symbols make it longer)
    assert dc.huffman_depth(list(dc.code_length_plan().values())) == 7
    assert dc.n_blocks(c["bam"]) >= 4
    assert len(c["three_blocks_text"]) == len(c["three_blocks_random"]) == 3 * 0xff00 + 17
    assert c["everything"] == b"".join(v for k, v in c.items() if k != "everything")


@pytest.fixture(scope="module")
def deflate_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("deflate_check")
    b = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ont-tcrconsensus_amd"), "deflate_check", f"SAN_OUT={out}"],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    assert "warning" not in b.stderr, b.stderr

    def run(*args, rc=0):
        r = subprocess.run([str(out / "deflate_check"), *map(str, args)], capture_output=True, text=True, timeout=600,
                           env=SAN_ENV)
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
        assert r.returncode == rc, (r.stdout[-2000:], r.stderr[-2000:])
        return r.stdout
    return run


@pytest.fixture(scope="module")
def encoded(deflate_check, tmp_path_factory):
    """every case through the host restatement, once: name -> (its BGZF bytes, [(kind, payload, tokens, flags)])"""
    d = tmp_path_factory.mktemp("deflate_cases")
    c = dc.cases()
    dc.write_case_file(d / "cases.bin", list(c.values()))
    out = deflate_check("cases", d / "cases.bin", d / "out.bgzf")
    nblocks = sum(dc.n_blocks(v) for v in c.values())
    assert f"cases={len(c)} blocks={nblocks} bad=0" in out and "bad " not in out, out[-2000:]
    data, names, res = (d / "out.bgzf").read_bytes(), list(c), {}
    blocks = collections.defaultdict(list)
    for i, k, kind, nbytes, ntok, flags in re.findall(r"block (\d+) (\d+) kind=(\d) bytes=(\d+) tokens=(\d+) flags=(\d+)", out):
        assert int(k) == len(blocks[int(i)])
        blocks[int(i)].append((int(kind), int(nbytes), int(ntok), int(flags)))
    spans = re.findall(r"case (\d+) off=(\d+) size=(\d+)", out)
    assert len(spans) == len(c) and sum(int(s) for _, _, s in spans) == len(data)
    for i, off, size in spans:
        res[names[int(i)]] = (data[int(off):int(off) + int(size)], blocks[int(i)])
    return res


def test_deflate_h_is_hip_free():
    src = open(os.path.join(ROOT, "ont-tcrconsensus_amd", "csrc", "deflate.h")).read()
    assert "#include <hip" not in src and "__shfl" not in src and "atomic" not in src


def test_every_member_inflates_to_its_input(encoded):
    """Python's gzip on each member: the bytes, CRC32 and ISIZE; the payload bound n + 5; the EOF block last"""
    for name, data in dc.cases().items():
        bgzf, blocks = encoded[name]
        mem = dc.members(bgzf)
        assert mem[-1] == dc.EOF_BLOCK and len(mem) == dc.n_blocks(data) + 1 == len(blocks) + 1, name
        for k, m in enumerate(mem[:-1]):
            part = data[k * dc.BLOCK:(k + 1) * dc.BLOCK]
            assert gzip.decompress(m) == part, (name, k)
            assert len(m) - 26 == blocks[k][1] <= len(part) + 5, (name, k)
    assert encoded["len_0"][0] == dc.EOF_BLOCK


def test_every_branch_is_reached(encoded):
    kinds = {name: [b[0] for b in blocks] for name, (_, blocks) in encoded.items()}
    flags = {name: [b[3] for b in blocks] for name, (_, blocks) in encoded.items()}
    assert kinds["random"] == [STORED] and kinds["three_blocks_random"][:3] == [STORED] * 3
    assert kinds["dist_32769"] == [STORED] and flags["dist_32769"][0] & DIST_NONE  # 32769 back: no match
    assert flags["dist_32768"][0] & DIST_ONE and encoded["dist_32768"][1][0][2] < len(dc.cases()["dist_32768"]) - 290
    assert encoded["dist_32769"][1][0][2] == len(dc.cases()["dist_32769"])  # every token a literal
    assert kinds["len_1"] == [FIXED] and kinds["len_5"] == [FIXED]
    assert kinds["zeros"] == [DYNAMIC] and set(kinds["bam"]) == {DYNAMIC} and kinds["three_blocks_text"][:3] == [DYNAMIC] * 3
    assert flags["fibonacci"][0] & LIT_LIMITED and flags["fibonacci"][0] & DIST_NONE and kinds["fibonacci"] == [DYNAMIC]
    assert flags["code_lengths"][0] & CLEN_LIMITED and kinds["code_lengths"] == [DYNAMIC]
    every = [f for fl in flags.values() for f in fl]
    for bit in (LIT_LIMITED, CLEN_LIMITED, DIST_NONE, DIST_ONE):
        assert any(f & bit for f in every), bit
    assert {k for ks in kinds.values() for k in ks} == {STORED, FIXED, DYNAMIC}


def test_zeros_and_periods_compress(encoded):
    """0xff00 zeros: 64 literals in the first step, then 258-byte matches -- about 253 of them, every token under 13
    bits even in the fixed code -- so under 1 KiB; a periodic text is matches after its first steps"""
    bgzf, blocks = encoded["zeros"]
    assert len(bgzf) - 28 < 1024
    assert 64 + 253 <= blocks[0][2] <= 64 + 256
    for p in (1, 2, 3, 7, 63, 64, 65, 257, 258, 259):
        n = len(dc.cases()[f"period_{p}"])
        assert encoded[f"period_{p}"][1][0][2] <= max(64, p) + 64 + n // 258 + 2, p


def test_the_code_builder(deflate_check):
    out = deflate_check("builder")
    assert "builder bad=0" in out and "bad builder" not in out, out
    rows = {m[0]: tuple(int(x) for x in m[1:]) for m in re.findall(
        r"builder (\w+) used=(\d+) max=(\d+) limited=(\d) kraft=(\d+)/(\d+)", out)}
    assert rows["fibonacci"] == (286, 15, 1, 32768, 32768)  # the limiter ran and left a complete code
    assert rows["equal"] == (286, 9, 0, 32768, 32768)
    assert rows["one"] == (1, 1, 0, 16384, 32768) and rows["only256"] == (1, 1, 0, 16384, 32768)  # the single code
    assert rows["two"] == (2, 1, 0, 32768, 32768)
    assert rows["clen_fibonacci"] == (19, 7, 1, 128, 128)
    assert rows["clen_one"] == (1, 1, 0, 128, 128)  # a second code makes the code-length code complete
    assert rows["dist_none"] == (0, 0, 0, 0, 32768)
