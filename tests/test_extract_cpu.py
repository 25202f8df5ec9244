"""Oracle for SURVEY.md §8f row f1 (extract_umis, /root/reference/ont_tcr_consensus/extract_umis.py:19-267).

The edlib HW/path semantics restated in oracle/extract.py are checked on hand-derived cases.  Parity against
edlib itself is unpinned: python-edlib (pyproject.toml:34) is not installed and the reference has no fixture.
"""
import extract as ox
import pytest

FWD = "TTTVVTTVVVVTTVVVVTTVVVVTTVVVVTTT"  # run_config.json:11


def test_exact_match_span():
    u = "TTTACTTGACGTTCAGCTTGGAATTACGCTTT"  # FWD instantiated
    w = "GGCCGGCC" + u + "GGCCGG"
    assert ox.extract_umi(w, FWD, 3) == (0, u)


def test_iupac_equalities():
    assert ox.eq("V", "A") and ox.eq("A", "V") and ox.eq("v", "a") and ox.eq("a", "A")
    assert not ox.eq("V", "T") and not ox.eq("V", "a") and not ox.eq("N", "n")
    # a T where the pattern has V is a substitution
    u = "TTTATTTGACGTTCAGCTTGGAATTACGCTTT"
    assert ox.extract_umi("GGGGCCCC" + u + "CCCC", FWD, 3)[0] == 1


def test_insertion_and_deletion():
    u = "TTTACTTGACGTTCAGCTTGGAATTACGCTTT"
    ins = u[:10] + "A" + u[10:]
    d, got = ox.extract_umi("GGCCGGCC" + ins + "GGCC", FWD, 3)
    assert d == 1 and got == ins
    dele = u[:12] + u[13:]
    d, got = ox.extract_umi("GGCCGGCC" + dele + "GGCC", FWD, 3)
    assert d == 1 and got == dele


def test_beyond_k_is_none():
    assert ox.extract_umi("ACGT" * 20, FWD, 3) == (None, None)


def test_first_end_and_leftmost_start():
    # pattern "AAC", target "AACAAC": two exact ends (2 and 5); locations[0] is the first
    assert ox.hw_locate("AAC", "AACAAC", 0) == (0, 0, 2)
    # pattern "TA", target "TTA": end 2 (0 edits); the start of the optimal alignment is 1
    assert ox.hw_locate("TA", "TTA", 1) == (0, 1, 2)
    # one edit: pattern "ACG" vs "AG": end 1, SHW picks the last reversed column -> the leftmost start 0
    assert ox.hw_locate("ACG", "AG", 1) == (1, 0, 1)


def test_hw_locate_vs_brute_force_definition():
    """hw_locate (the GPU kernels' checker) against tests/extract_ref.py, which takes the minimum over every substring
    with a plain Levenshtein distance and shares no code with it: 1,500 seeded cases, patterns of 1..8 symbols over
    ACGTVBN, windows of 0..14 over alphabets of 1, 2, 4 and 5 letters, k in {0, 1, 2, m, m + 1}."""
    import random

    import extract_ref
    rng = random.Random(20261020)
    found = 0
    for case in range(1500):
        m = rng.randint(1, 8)
        pat = "".join(rng.choice("ACGTVBN") for _ in range(m))
        alpha = rng.choice(["A", "AC", "ACGT", "ACGTN"])
        w = "".join(rng.choice(alpha) for _ in range(rng.randint(0, 14)))
        k = rng.choice([0, 1, 2, m, m + 1])
        want = extract_ref.locate(pat, w, k)
        assert ox.hw_locate(pat, w, k) == want, (case, pat, w, k)
        found += want is not None
    assert 300 < found < 1400  # both outcomes are well covered
    for a in "ACGTMRWSYKVHDBNacgtmrwsykvhdbn=X":
        for b in "ACGTMRWSYKVHDBNacgtmrwsykvhdbn=X":
            assert ox.eq(a, b) == extract_ref.eq(a, b), (a, b)


def test_pattern_of_64_symbols():
    """m = 64 fills the kernel's word: hand-derived answers, the last pattern symbol (the word's high bit) decisive."""
    a64 = "A" * 64
    assert ox.hw_locate(a64, a64, 0) == (0, 0, 63)
    assert ox.hw_locate(a64, "C" + a64 + "C", 0) == (0, 1, 64)
    assert ox.hw_locate(a64, "A" * 63, 0) is None
    assert ox.hw_locate(a64, "A" * 63, 1) == (1, 0, 62)  # one deletion, and only the whole window reaches it
    # exactly 63 A and the closing C: the end is the C, the start 63 before it
    assert ox.hw_locate("A" * 63 + "C", "A" * 70 + "C", 0) == (0, 7, 70)
    assert ox.hw_locate("C" + "A" * 63, "C" + "A" * 70, 0) == (0, 0, 63)  # the first end with the distance
    assert ox.hw_locate("A" * 63 + "C", "A" * 70 + "G", 0) is None
    assert ox.hw_locate("A" * 63 + "C", "A" * 70 + "G", 1) == (1, 0, 62)  # 63 A, the C deleted: first end 62
    assert ox.hw_locate("A" * 63 + "V", "T" + "A" * 63 + "G", 0) == (0, 1, 64)  # V = G in the high bit


def test_k_at_least_the_pattern_length():
    """With k >= m every non-empty window has a location: the empty alignment costs m.  Hand-derived."""
    assert ox.hw_locate("ACG", "TTTT", 2) is None
    assert ox.hw_locate("ACG", "TTTT", 3) == (3, 0, 0)  # nothing matches: distance m at the first column
    assert ox.hw_locate("ACG", "TTTT", 6) == (3, 0, 0)
    assert ox.hw_locate("A", "C", 1) == (1, 0, 0) and ox.hw_locate("A", "C", 5) == (1, 0, 0)
    assert ox.hw_locate("A", "", 5) is None  # an empty window has no location at any k
    # AC in GA: "A" alone costs 1 (end 1), "GA" costs 2, so the start is 1
    assert ox.hw_locate("AC", "GA", 2) == (1, 1, 1)
    assert ox.hw_locate("AC", "GA", 1) == (1, 1, 1) and ox.hw_locate("AC", "GA", 0) is None
    import extract_ref
    for pat, w, k in [("ACG", "TTTT", 3), ("A", "C", 5), ("AC", "GA", 2), ("A", "", 5)]:
        assert extract_ref.locate(pat, w, k) == ox.hw_locate(pat, w, k)


def test_records_and_strand():
    u5 = "TTTACTTGACGTTCAGCTTGGAATTACGCTTT"
    u3 = "AAACGTCAACTGCAATGTCAAGGCTAACTAAA"
    rev = "AAABBBBAABBBBAABBBBAABBBBAABBAAA"
    seq = "GG" + u5 + "C" * 60 + u3 + "G"
    txt, n = ox.extract_records([("r1;strand=-", seq)], 73, 68, 3, FWD, rev)
    assert n == 1
    assert txt.startswith(f">r1;strand=-;umi_fwd_dist=0;umi_rev_dist=0;umi_fwd_seq={u5};umi_rev_seq={u3};seq={seq}\n")
    assert txt.endswith(ox.reverse_complement(u3) + ox.reverse_complement(u5) + "\n")
    with pytest.raises(Exception):
        ox.extract_records([("r1", seq)], 73, 68, 3, FWD, rev)


# ---- pinned by the reference itself: tests/golden/extract (make_golden_extract.py ran extract_umis.py here) ----
import glob as _glob
import json as _json
import os as _os

EXTRACT_FIX = sorted(_glob.glob(_os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "golden", "extract",
                                              "*.json")))


def _records(text):
    """pysam.FastxFile's view of a FASTA/FASTQ text: (name up to whitespace, joined sequence)."""
    lines = [x.rstrip("\r") for x in text.split("\n")]
    fastq = any(x for x in lines) and next(x for x in lines if x).startswith("@")
    recs, i = [], 0
    while i < len(lines):
        if not lines[i]:
            i += 1
            continue
        name = lines[i][1:].split()[0]
        i += 1
        seq = []
        while i < len(lines) and not lines[i].startswith(">") and not (fastq and lines[i].startswith("+")):
            seq.append(lines[i].strip())
            i += 1
        s = "".join(seq)
        if fastq:
            i += 1
            q = 0
            while i < len(lines) and q < len(s):
                q += len(lines[i])
                i += 1
        recs.append((name, s))
    return recs


@pytest.mark.parametrize("path", EXTRACT_FIX, ids=[_os.path.basename(p)[:-5] for p in EXTRACT_FIX])
def test_oracle_glue_matches_reference_fixtures(path):
    """The oracle's restated glue (oracle/extract.extract_records: strand split, read name, windows, skips,
    header and combined-UMI format) reproduces the reference's output records."""
    case = _json.load(open(path))
    a = dict(case["args"])
    a.pop("write_region")
    recs = _records(case["input"])
    want = list(case["files"].values())[0]
    if case["error"]:
        bad = next(i for i, (n, _s) in enumerate(recs) if "strand=" not in n)
        got, _n = ox.extract_records(recs[:bad], **a)
        with pytest.raises(Exception, match="Read strand not annotated!"):
            ox.extract_records(recs, **a)
    else:
        got, _n = ox.extract_records(recs, **a)
    assert got == want
