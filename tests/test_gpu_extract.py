"""§8f row f1 on the GPU: the Myers kernel (umiclust_extract_umis) and the file-level drop-in
(umiclust.extract_umis) against the CPU restatement of edlib's HW/path semantics (oracle/extract.py) on
seeded reads.  Parity against edlib itself is unpinned (not installed; the reference has no fixture)."""
import os
import random

import extract as ox
import pytest
from umiclust import extract_umis as ge
from umiclust import synth

pytestmark = pytest.mark.gpu

FWD, REV = synth.UMI_FWD, synth.UMI_REV


def _mut(rng, s, n):
    s = list(s)
    for _ in range(n):
        x = rng.randrange(len(s))
        u = rng.random()
        if u < 0.4:
            s[x] = rng.choice("ACGT")
        elif u < 0.7:
            s.insert(x, rng.choice("ACGT"))
        elif len(s) > 1:
            del s[x]
    return "".join(s)


def _inst(rng, pat):
    return "".join(rng.choice("ACG") if c == "V" else rng.choice("CGT") if c == "B" else c for c in pat)


def _reads(seed, n):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        body = "".join(rng.choice("ACGT") for _ in range(rng.randint(150, 400)))
        kind = rng.random()
        u5 = _mut(rng, _inst(rng, FWD), rng.choice([0, 0, 1, 2, 3, 4]))
        u3 = _mut(rng, _inst(rng, REV), rng.choice([0, 0, 1, 2, 3, 5]))
        pre = "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 40)))
        suf = "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 30)))
        if kind < 0.1:
            seq = body  # no UMI
        elif kind < 0.15:
            seq = (pre + u5 + "TTTTT" + body + "AAAAA" + u3 + suf).lower()  # lowercase read
        elif kind < 0.2:
            seq = pre + u5[:20]  # short read: windows overlap / truncated
        else:
            seq = pre + u5 + body + u3 + suf
        if rng.random() < 0.05:
            x = rng.randrange(len(seq))
            seq = seq[:x] + "N" + seq[x + 1:]
        out.append((f"read{i};strand={'+' if rng.random() < 0.5 else '-'}", seq))
    return out


@pytest.mark.parametrize("seed,k", [(1, 3), (2, 0), (3, 6)])
def test_windows_vs_oracle(gpu_ctx, seed, k):
    recs = _reads(seed, 600)
    seqs = [s for _, s in recs]
    got = gpu_ctx.extract_umis(seqs, 73, 68, k, FWD, REV)
    for i, s in enumerate(seqs):
        for w, (pat, win) in enumerate(((FWD, s[:73]), (REV, s[-68:]))):
            want = ox.hw_locate(pat, win, k)
            g = tuple(int(x) for x in got[i, 3 * w:3 * w + 3])
            assert g == (want if want else (-1, -1, -1)), (i, w, win)


@pytest.mark.parametrize("a5,a3", [(73, 68), (81, 76), (0, 40), (250, 0), (400, 300), (5, 255)])
def test_window_sizes_vs_oracle(gpu_ctx, a5, a3):
    """Both device paths: host-gathered windows (short windows) and whole reads (a3 == 0: the whole read as
    Python's seq[-0:] gives; windows past the gather limit), against Python slicing semantics."""
    seqs = [s for _, s in _reads(8, 250)]
    got = gpu_ctx.extract_umis(seqs, a5, a3, 3, FWD, REV)
    for i, s in enumerate(seqs):
        for w, (pat, win) in enumerate(((FWD, s[:a5]), (REV, s[-a3:]))):
            want = ox.hw_locate(pat, win, 3)
            g = tuple(int(x) for x in got[i, 3 * w:3 * w + 3])
            assert g == (want if want else (-1, -1, -1)), (i, w, a5, a3)


def _check_every_window(ctx, seqs, a5, a3, k, fwd, rev, note=()):
    """Every window of every read against hw_locate, exactly (Python slicing: seq[:a5], seq[-a3:])."""
    got = ctx.extract_umis(seqs, a5, a3, k, fwd, rev)
    assert got.shape == (len(seqs), 6)
    for i, s in enumerate(seqs):
        for w, (pat, win) in enumerate(((fwd, s[:a5]), (rev, s[-a3:]))):
            want = ox.hw_locate(pat, win, k)
            g = tuple(int(x) for x in got[i, 3 * w:3 * w + 3])
            assert g == (want if want else (-1, -1, -1)), (note, i, w, a5, a3, k, pat, win)


IUPAC = {"M": "AC", "R": "AG", "W": "AT", "S": "CG", "Y": "CT", "K": "GT", "V": "ACG", "H": "ACT", "D": "AGT",
         "B": "CGT", "N": "ACGT"}


def _instance(rng, pat):
    return "".join(rng.choice(IUPAC.get(c, c)) for c in pat)


# both orders of each pair, so that a swap of the two pattern lengths (or of their match masks) shows; 64 fills the
# kernel's word (mask ~0, high bit 1 << 63), 1 leaves only the high bit, 31 / 32 / 33 lie around the half word
@pytest.mark.parametrize("path", ["staged", "whole_read"])
@pytest.mark.parametrize("m_fwd,m_rev", [(1, 64), (64, 1), (2, 63), (63, 2), (31, 33), (33, 32), (32, 31), (64, 63)])
def test_pattern_lengths_vs_oracle(gpu_ctx, m_fwd, m_rev, path):
    """Patterns over the 15 IUPAC letters; a read is an instance of each pattern with 0..6 edits between random flanks;
    k below, at and above the pattern lengths.  Once through the LDS-staged kernel (a5 = a3 = 100) and once through the
    whole-read kernel (a5 = 256, a3 = 0: the 3' window is the whole read)."""
    rng = random.Random(1000 * m_fwd + m_rev)
    fwd = "".join(rng.choice("ACGTMRWSYKVHDBN") for _ in range(m_fwd))
    rev = "".join(rng.choice("ACGTMRWSYKVHDBN") for _ in range(m_rev))
    a5, a3 = (100, 100) if path == "staged" else (256, 0)
    for k in sorted({0, 3, m_fwd, m_fwd + 3, m_rev, m_rev + 3}):
        seqs = []
        for _ in range(16 if m_fwd + m_rev > 100 else 24):
            flank = ["".join(rng.choice("ACGT") for _ in range(rng.randint(0, 15))) for _ in range(3)]
            u5 = _mut(rng, _instance(rng, fwd), rng.randint(0, 6))
            u3 = _mut(rng, _instance(rng, rev), rng.randint(0, 6))
            seqs.append(flank[0] + u5 + flank[1] + u3 + flank[2])
        _check_every_window(gpu_ctx, seqs, a5, a3, k, fwd, rev)


def test_pattern_lengths_outside_one_word_are_refused(gpu_ctx):
    from umiclust import _lib
    for fwd, rev in (("", "ACG"), ("ACG", ""), ("A" * 65, "ACG"), ("ACG", "A" * 65)):
        with pytest.raises(_lib.UmiclustError) as e:
            gpu_ctx.extract_umis(["ACGTACGT"], 73, 68, 3, fwd, rev)
        assert e.value.code == -22  # UMICLUST_EINVAL
    _check_every_window(gpu_ctx, ["ACGTACGT"], 73, 68, 3, "A" * 64, "C")  # and the context still works


# slot S = (a5 + a3 + 3) & ~3: every residue of (a5 + a3) mod 4, the largest slot (252) reached two ways, and one
# byte more (S = 256), which goes to the whole-read kernel
@pytest.mark.parametrize("a5,a3", [(0, 1), (1, 1), (1, 2), (73, 68), (126, 126), (251, 1), (127, 126)])
def test_staged_geometry_vs_oracle(gpu_ctx, a5, a3):
    """Read counts on both sides of the 128 reads a workgroup stages (1, 127, 128, 129, 257) and read lengths at every
    boundary of the window arithmetic: 0 (the reference accepts an empty sequence: no UMI), 1, below the pattern
    length, below a3, below a5, exactly a5, below and at a5 + a3 (overlapping windows), and longer."""
    fwd, rev = "ACVBT", "TNGA"
    rng = random.Random(100 * a5 + a3)
    edges = sorted({max(0, x) for x in (0, 1, len(rev) - 1, len(fwd) - 1, a3 - 1, a3, a5 - 1, a5, a5 + 1, a5 + a3 - 1,
                                       a5 + a3, a5 + a3 + 1, a5 + a3 + 40)})
    for n in (1, 127, 128, 129, 257):
        seqs = []
        for i in range(n):
            ln = edges[i % len(edges)] if rng.random() < 0.7 else rng.randint(0, a5 + a3 + 60)
            s = [rng.choice("ACGT") for _ in range(ln)]
            for pat in (fwd, rev):  # an instance somewhere, often against either end
                if ln >= len(pat) and rng.random() < 0.6:
                    at = rng.choice([0, ln - len(pat), rng.randint(0, ln - len(pat))])
                    s[at:at + len(pat)] = _instance(rng, pat)
            seqs.append("".join(s))
        if n == 1:
            _check_every_window(gpu_ctx, [""], a5, a3, 1, fwd, rev, note="one empty read")
        _check_every_window(gpu_ctx, seqs, a5, a3, 1, fwd, rev, note=n)
    _check_every_window(gpu_ctx, [""] * 130, a5, a3, 1, fwd, rev, note="all empty")


@pytest.mark.parametrize("a5,a3", [(40, 40), (256, 0)])
def test_ties_vs_oracle(gpu_ctx, a5, a3):
    """Windows full of equally good locations: locations[0] is the first end, and its start the leftmost one.
    Homopolymer and dinucleotide-repeat windows under repeat patterns, two exact copies of the instance, all-N windows
    (N equals A, C, G, T but no other code), lowercase reads under uppercase patterns (a equals A, but not V)."""
    rng = random.Random(a5)
    pats = ["A" * 8, "AC" * 6, "TTTVVVVTTT"]
    seqs = []
    for unit in ("A", "C", "T", "N", "AC", "CA", "TA", "TG", "AN", "a", "ac", "n", "Ac"):
        for ln in (1, 7, 8, 9, 13, 40, 41, 81):
            seqs.append((unit * ln)[:ln])
    for pat in pats:
        for _ in range(20):
            u = _instance(rng, pat)
            mid = "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 6)))
            pre = "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 5)))
            s = pre + u + mid + u + pre[::-1]  # two exact copies inside one window
            seqs.append(s.lower() if rng.random() < 0.3 else s)
    for fwd, rev in zip(pats, pats[1:] + pats[:1]):
        for k in (0, 2, 8):
            _check_every_window(gpu_ctx, seqs, a5, a3, k, fwd, rev)


def test_single_window_helper(gpu_ctx):
    for name, s in _reads(4, 50):
        assert ge.extract_umi(s[:73], FWD, 3) == ox.extract_umi(s[:73], FWD, 3)


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_file_dropin_vs_oracle(tmp_path, fmt):
    recs = _reads(5, 3000)
    src = tmp_path / f"region_cluster12.{fmt}"
    with open(src, "w") as fh:
        for name, s in recs:
            if fmt == "fasta":
                fh.write(f">{name} extra comment\n{s[:70]}\n{s[70:]}\n" if len(s) > 70 else f">{name}\n{s}\n")
            else:
                fh.write(f"@{name}\n{s}\n+\n{'I' * len(s)}\n")
    out = ge.extract_umis.remote(str(src), str(tmp_path), True, 73, 68, 3, FWD, REV)
    want, n = ox.extract_records(recs, 73, 68, 3, FWD, REV)
    assert out == os.path.join(str(tmp_path), "region_cluster12_detected_umis.fasta")
    assert open(out).read() == want and n > 0


def test_missing_strand_writes_earlier_records_then_raises(tmp_path):
    from umiclust import _lib
    recs = _reads(6, 20)
    recs[12] = ("read12", recs[12][1])
    src = tmp_path / "r.fasta"
    src.write_text("".join(f">{n}\n{s}\n" for n, s in recs))
    with pytest.raises(_lib.UmiclustError):
        ge.extract_umis(str(src), str(tmp_path), False)
    want, _ = ox.extract_records(recs[:12], 73, 68, 3, ge.UMI_FWD_DEFAULT, ge.UMI_REV_DEFAULT)
    assert open(tmp_path / "_detected_umis.fasta").read() == want


def test_no_umi_returns_none(tmp_path):
    src = tmp_path / "r.fasta"
    src.write_text(">a;strand=+\n" + "ACGT" * 50 + "\n")
    assert ge.extract_umis(str(src), str(tmp_path), True) is None
    assert (tmp_path / "r_detected_umis.fasta").read_text() == ""


# ---- pinned by the reference itself: tests/golden/extract (make_golden_extract.py ran extract_umis.py here) ----
import glob as _glob
import json as _json

_EXTRACT_FIX = sorted(_glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "extract",
                                              "*.json")))


@pytest.mark.parametrize("path", _EXTRACT_FIX, ids=[os.path.basename(p)[:-5] for p in _EXTRACT_FIX])
def test_extract_umis_vs_reference_fixtures(tmp_path, path):
    """umiclust.extract_umis byte for byte against the reference's extract_umis outputs: FASTA and multi-line
    FASTQ input, write_region True/False (the output-path rule), a zero 3' window (`seq[-0:]` = the whole read),
    a zero 5' window, the run_config.json patterns at k = 0 and 3, extra `;` fields after strand=, lowercase
    reads, `N`s, no read with both UMIs (returns None, empty file), and a record without `strand=` (the records
    before it written, then the exception)."""
    case = _json.load(open(path))
    src = tmp_path / case["file_name"]
    src.write_text(case["input"])
    out = tmp_path / "out"
    out.mkdir()
    if case["error"]:
        with pytest.raises(Exception):
            ge.extract_umis(str(src), str(out), **case["args"])
    else:
        ret = ge.extract_umis(str(src), str(out), **case["args"])
        assert (None if ret is None else os.path.relpath(ret, out)) == case["returned"]
    assert {f: open(os.path.join(out, f)).read() for f in sorted(os.listdir(out))} == case["files"]
