"""The SAM rules of csrc/sam_text.h on the CPU (policy O9): the host restatement of the kernels,
sam::encode_host, runs over every text of tests/sam_cases.py in a stand-alone program built with ASan + UBSan
(tools/sam_check_main.cpp, `make sam_check`) and is compared with the plain Python reference tests/sam_ref.py, which was
written from the SAM specification alone; the reference's bytes are in turn read back with bam_ref.decode.  Nothing is
loaded into Python under a sanitizer."""
import os
import struct
import subprocess

import bam_ref
import pytest
import sam_cases
import sam_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sam_cases.cases()


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    """one run of the sanitized program over all cases: {name: its output line}"""
    out = tmp_path_factory.mktemp("sam_check")
    b = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ont-tcrconsensus_amd"), "sam_check", f"SAN_OUT={out}"],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    path = out / "cases.bin"
    with open(path, "wb") as fh:
        for _, text, _ in CASES:
            fh.write(struct.pack("<I", len(text)) + text)
    r = subprocess.run([str(out / "sam_check"), str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(CASES)
    return {name: ln for (name, _, _), ln in zip(CASES, lines)}


@pytest.mark.parametrize("name,text,refusal", CASES, ids=[c[0] for c in CASES])
def test_host_restatement_equals_the_reference(verdicts, name, text, refusal):
    got = verdicts[name]
    if refusal is None:
        raw, roff = sam_ref.encode(text)
        word, n, hexed, offs = got.split(" ")
        assert word == "ok" and int(n) == len(roff)
        assert ([int(x) for x in offs.split(",")] if offs != "-" else []) == roff
        assert bytes.fromhex(hexed) == raw
    else:
        code, lineno, field, holds = refusal
        with pytest.raises(sam_ref.Refused) as e:
            sam_ref.encode(text)
        assert (e.value.code, e.value.line, e.value.field) == (code, lineno, field)
        assert got.startswith("refused %s line %d: %s" % (code, lineno, field)), got
        if holds:
            assert holds in got


@pytest.mark.parametrize("name,text,refusal", [c for c in CASES if c[2] is None], ids=[c[0] for c in CASES if c[2] is None])
def test_reference_bytes_decode_as_bam(name, text, refusal):
    """the reference's own check: bam_ref.decode reads back what the text says, in coordinate order"""
    raw, roff = sam_ref.encode(text)
    refs, start, recs = bam_ref.decode(raw)
    head, lines = sam_ref.split(text)
    assert [r.off for r in recs] == roff and len(recs) == len(lines)
    assert [nm for nm, _ in refs] == [f.split(b"SN:")[1].split(b"\t")[0].decode() for f in head if f.startswith(b"@SQ")]
    by_name = {}
    for ln in lines:
        by_name.setdefault(ln.split(b"\t")[0].decode("latin-1"), []).append(ln.split(b"\t"))
    keys = []
    for r in recs:
        f = by_name[r.query_name].pop(0)  # equal names keep their input order only if the sort is stable
        assert r.flag == int(f[1]) and r.pos == int(f[3]) - 1
        assert (refs[r.ref][0].encode() if r.ref >= 0 else b"*") == f[2]
        assert r.l_seq == (0 if f[9] == b"*" else len(f[9]))
        if f[5] != b"*":
            assert "".join("%d%s" % (ln, bam_ref.CIGAR_OPS[op]) for op, ln in r.cigar).encode() == f[5]
        assert len(r.tags()) == len(f) - 11
        keys.append((r.ref if r.ref >= 0 else 2 ** 32, r.pos, r.flag & 16))
    assert keys == sorted(keys)
    text_len = struct.unpack_from("<i", raw, 4)[0]
    hd = raw[8:8 + text_len].split(b"\n")[0]
    assert hd.startswith(b"@HD\t") and b"SO:coordinate" in hd and b"GO:" not in hd and b"@PG\tID:samtools" not in raw


def test_stable_order_of_equal_keys():
    """same (tid, pos, strand) keeps input order; reverse after forward; tid -1 last in input order; flag 4 with an
    RNAME is placed by it; POS 0 is first on its reference"""
    text = dict((c[0], c[1]) for c in CASES)["order_ties_strands_and_unmapped"]
    raw, _ = sam_ref.encode(text)
    names = [r.query_name for r in bam_ref.decode(raw)[2]]
    assert names == ["pos0", "fwd", "rev", "placed", "t1", "t2", "t3", "other", "u1", "u2", "u3"]
    rec = {r.query_name: r for r in bam_ref.decode(raw)[2]}
    assert struct.unpack_from("<H", raw, rec["u1"].off + 14)[0] == 4680 and rec["pos0"].pos == -1
