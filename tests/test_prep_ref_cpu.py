"""The load kernel's reference and case list (tests/prep_ref.py, tests/prep_cases.py), checked without a GPU.

 * on every case prep_ref equals the C oracle (orc.dust, orc.unique_kmers) and oracle/pyref.py (dust, kmers), with and
   without qmask_dust;
 * every case has the property its name promises (a best score of exactly 20 or 21, the kind of tie, the crossing
   interval, ...), asserted from wo()'s scores, not from a recorded answer;
 * every rule of the operation decides at least one case: prep_ref has one switch per rule, and a flipped switch changes
   the reference's output on a case.  A kernel with exactly that mistake therefore fails tests/test_gpu_prep.py.  Two
   switches cannot be seen by any input; that is shown instead (test_unreachable_rules).
"""
import numpy as np
import orc
import prep_cases as C
import prep_ref as R
import pyref
import pytest

IDS = [c.name for c in C.CASES]
_REF = {}


def ref(case, dust=1, rules=()):
    """the reference of one case, computed once and shared (never modified)"""
    k = (case.name, dust, tuple(rules))
    if k not in _REF:
        _REF[k] = R.prep(case.records, dust, rules)
    return _REF[k]


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_reference_equals_oracle(case):
    for dust in (1, 0):
        r = ref(case, dust)
        for i, s in enumerate(case.records):
            m = r["masked"][i]
            assert m == (orc.dust(s) if dust else s), (s, m)
            assert not dust or m == pyref.dust(s)
            for st, strand in enumerate((m, pyref.revcomp(m))):
                want = sorted(orc.unique_kmers(strand, 8, bool(dust)))
                assert r["kmers"][i][st] == want == sorted(pyref.kmers(strand, 8, bool(dust))), (s, st)
                assert r["nk"][i][st] == len(want) <= R.MAX_LEN - 7
                # the code words: one nibble per residue of the strand as vsearch's 4-bit map reads it, 0 beyond
                nib = [(int(r["codes"][i, st, p // 8]) >> (4 * (p % 8))) & 15 for p in range(R.MAX_LEN)]
                assert nib == [pyref.c4(ch) for ch in strand] + [0] * (R.MAX_LEN - len(s))
            assert r["lens"][i] == len(s)
            assert r["changed"][i] == (m != s)
        assert r["n_changed"] == sum(m != s for m, s in zip(r["masked"], case.records))
        assert r["ambig"] == any(ch.upper() not in "ACGTU" for s in case.records for ch in s)


# ------------------------------------------------------------------ the property of every case, by name
def _w0(name):
    return R.windows(C.BY_NAME[name].records[0])[0]


def _p_len(name):
    c = C.BY_NAME[name]
    assert tuple(len(s) for s in c.records) == C.LENGTHS
    for lo, hi in ((0, 17), (31, 34), (39, 41), (63, 66), (71, 73), (95, 98), (103, 105), (110, 112)):
        assert set(range(lo, hi + 1)) <= set(C.LENGTHS)
    r = ref(c)
    if name == "len_random":
        assert all(set(s) <= set("ACGT") for s in c.records)
        assert all(r["nk"][i][0] == 0 for i, s in enumerate(c.records) if len(s) < 8)
    else:
        # masked end to end from the smallest region (8) on, untouched below it
        k = 1 if name == "len_homopolymer" else 2
        assert all(len(set(s[:len(s) // k * k])) <= k for s in c.records)
        for s, m in zip(c.records, r["masked"]):
            if name == "len_homopolymer":
                assert m == (s.lower() if len(s) >= 8 else s)
            else:  # a two-letter repeat scores 20 at 13 residues and 21 at 14
                assert sum(ch.islower() for ch in m) >= len(s) - 1 if len(s) >= 14 else m == s
        # a last window of 1..8 residues at every window start
        for i0 in (32, 64, 96):
            assert {len(s) - i0 for s in c.records} >= set(range(1, 9))


def _p_empty(name):
    r = ref(C.BY_NAME[name])
    assert not r["codes"].any() and not r["nk"].any() and not r["lens"].any() and r["n_changed"] == 0 == r["ambig"]


def _p_score20(name):
    w = _w0(name)
    assert w["bestv"] == 20 and ref(C.BY_NAME[name])["n_changed"] == 0


def _p_score21(name):
    w = _w0(name)
    assert w["bestv"] == 21 and len(w["ties"]) == 1 and ref(C.BY_NAME[name])["n_changed"] == 1


def _p_tie_starts(name):
    w = _w0(name)
    starts = [i for i, _ in w["ties"]]
    assert w["bestv"] == 21 and len(starts) >= 2 and len(set(starts)) == len(starts)
    assert (w["besti"], w["bestj"]) == w["ties"][0] and w["besti"] == min(starts)


def _p_tie_within(name):
    w = _w0(name)
    assert w["bestv"] == 21 and len(w["ties"]) >= 2 and {i for i, _ in w["ties"]} == {w["besti"]}
    assert w["bestj"] == min(j for _, j in w["ties"])


def _p_cross(name):
    s = C.BY_NAME[name].records[0]
    assert [j for j, b in enumerate(R.mask_bits(s)) if b] == list(range(60, 71))


def _p_half(name):
    """the run's bounds, and the k-mers next to it: the last window before the run and the first after it are kept,
    every window that holds one of its positions is dropped"""
    c = C.BY_NAME[name]
    s = c.records[0]
    lo, hi = (64, 74) if name == "dust_from_64" else (53, 63)
    assert [j for j, b in enumerate(R.mask_bits(s)) if b] == list(range(lo, hi + 1))
    kept = {R.kmer_code(s[x:x + 8]) for x in range(len(s) - 7) if x + 7 < lo or x > hi}
    assert ref(c)["kmers"][0][0] == sorted(kept)
    assert R.kmer_code(s[lo - 8:lo]) in kept and R.kmer_code(s[hi + 1:hi + 9]) in kept
    dropped = {R.kmer_code(s[x:x + 8]) for x in range(lo - 7, hi + 1)}
    assert not dropped & kept


def _p_merge(name):
    s = C.BY_NAME[name].records[0]
    iv = R.intervals(s)
    assert C._overlapping(iv)
    m = R.mask_bits(s)
    lo, hi = min(a for a, _ in iv), max(b for _, b in iv)
    assert all(m[lo:hi + 1]) and hi - lo + 1 > 64  # one run, longer than any one window


def _p_only96(name):
    s = C.BY_NAME[name].records[0]
    assert C._only_96(s)
    by = {w["i0"]: w for w in R.windows(s)}
    assert by[96]["bestv"] > 20 and 96 + by[96]["besti"] >= 96
    # without the window at 96 its run stays unmasked: step 33 ends the windows at 99
    assert R.dust(s)[100:] == s[100:].lower() and R.dust(s[:96]) + s[96:] != R.dust(s)


def _p_window_starts(name):
    """each record's short run is the choice of the window at 32 alone: its other windows choose a stronger run, or
    hold fewer than 8 of its residues"""
    for s, (lo, hi) in zip(C.BY_NAME[name].records, ((32, 39), (88, 95))):
        assert len(set(s[lo:hi + 1])) == 1 and all(R.mask_bits(s)[lo:hi + 1])
        covering = [w["i0"] for w in R.windows(s) if w["bestv"] > 20 and
                    w["i0"] + w["besti"] <= hi and lo <= w["i0"] + w["besti"] + w["bestj"]]
        assert covering == [32]
    a, b = C.BY_NAME[name].records
    assert not any(R.mask_bits(a, ("step33",))[32:40]) and not any(R.mask_bits(b, ("step31",))[88:96])


def _p_all112(name):
    c = C.BY_NAME[name]
    r = ref(c)
    assert all(len(s) == 112 and m == s.lower() for s, m in zip(c.records, r["masked"])) and not r["nk"].any()


def _p_ends(name):
    c = C.BY_NAME[name]
    s = c.records[0]
    r = ref(c)
    assert r["masked"][0] == s[:8] + s[8:-8].lower() + s[-8:]
    assert r["kmers"][0][0] == sorted({R.kmer_code(s[:8]), R.kmer_code(s[-8:])}) and r["nk"][0][1] == 2


def _p_distinct(name):
    r = ref(C.BY_NAME[name])
    assert tuple(r["nk"][0]) == (105, 105) and r["n_changed"] == 0


def _p_repeated(name):
    c = C.BY_NAME[name]
    r = ref(c, 0)
    assert [list(k) for k in r["kmers"][0]] == [[0], [0xffff]] and [list(k) for k in r["kmers"][1]] == [[0xffff], [0]]
    assert r["kmers"][3] == [[0xffff], [0]] and (r["nk"] == 1).all()
    assert not ref(c, 1)["nk"].any()


def _p_straddle(name):
    s = C.BY_NAME[name].records[0]
    assert s[:56] == s[56:] and C._straddle(s)
    assert ref(C.BY_NAME[name])["nk"][0][0] == 56  # 49 twice, 7 across the joint once


def _p_ffff(name):
    c = C.BY_NAME[name]
    assert all(0xffff in ref(c, 0)["kmers"][i][0] for i in range(2))
    assert all(0xffff not in ref(c, 1)["kmers"][i][0] and "tttttttt" in ref(c, 1)["masked"][i] for i in range(2))


def _p_palindrome(name):
    c = C.BY_NAME[name]
    s = c.records[0]
    r = ref(c)
    assert pyref.revcomp(s) == s and r["kmers"][0][0] == r["kmers"][0][1] and r["nk"][0][0] > 90
    assert (r["codes"][0, 0] == r["codes"][0, 1]).all()


def _p_lower(name):
    c = C.BY_NAME[name]
    r = ref(c)
    assert all(s == s.lower() for s in c.records) and r["changed"].all() and r["ambig"] == 0
    assert r["masked"][0] == c.records[0].upper() and any(ch.islower() for ch in r["masked"][-1])
    assert ref(c, 0)["n_changed"] == 0


def _p_mixed(name):
    c = C.BY_NAME[name]
    s = c.records[0]
    assert s != s.lower() and s != s.upper() and list(ref(c)["changed"]) == [1, 0, 1]


def _p_u(name):
    c = C.BY_NAME[name]
    r = ref(c)
    assert all("U" in s.upper() and "T" not in s.upper() for s in c.records) and r["ambig"] == 0
    t = ref(C.Case("t", tuple(s.replace("U", "T").replace("u", "t") for s in c.records), ""))
    assert (r["codes"] == t["codes"]).all() and r["kmers"] == t["kmers"] and "uuuu" in r["masked"][2]


def _p_last_ambig(name):
    c = C.BY_NAME[name]
    (s,) = c.records
    assert len(s) == 65 and set(s[:64]) <= set("ACGT") and s[64] == "N" and ref(c)["ambig"] == 1
    assert ref(C.Case("t", (s[:64],), ""))["ambig"] == 0


def _p_first_ambig(name):
    c = C.BY_NAME[name]
    (s,) = c.records
    assert s[0] == "N" and set(s[1:]) <= set("ACGT") and ref(c)["ambig"] == 1


def _p_none_ambig(name):
    c = C.BY_NAME[name]
    assert ref(c)["ambig"] == 0 == ref(c, 0)["ambig"] and len(c.records) > 1


def _p_iupac(name):
    c = C.BY_NAME[name]
    for ch in C.IUPAC:
        assert any(ch in s for s in c.records) and any(ch.lower() in s for s in c.records)
    assert ref(c)["ambig"] == 1


def _p_outside(name):
    c = C.BY_NAME[name]
    r = ref(c)
    for ch in C.OUTSIDE:
        inside = [i for i, s in enumerate(c.records) if ("AAAAAA" + ch + "AAAAAA") in s]
        assert inside and all(("aaaaaa" + ch + "aaaaaa") in r["masked"][i] for i in inside)  # masked around, kept
        alone = c.records.index(ch * 20)
        assert r["masked"][alone] == ch * 20 and not r["changed"][alone] and r["kmers"][alone] == [[0], [0]]
    assert r["ambig"] == 1


PROPERTY = {"len_random": _p_len, "len_homopolymer": _p_len, "len_two_letter": _p_len, "len_empty_batch": _p_empty,
            "dust_score20": _p_score20, "dust_score21": _p_score21, "dust_tie_starts": _p_tie_starts,
            "dust_tie_within": _p_tie_within, "dust_cross_63_64": _p_cross, "dust_merge": _p_merge,
            "dust_from_64": _p_half, "dust_to_63": _p_half, "dust_only_window_96": _p_only96,
            "dust_window_starts": _p_window_starts, "dust_all_112": _p_all112, "dust_ends_unmasked": _p_ends,
            "kmers_105_distinct": _p_distinct, "kmers_one_repeated": _p_repeated, "kmers_straddle_halves": _p_straddle,
            "kmers_ffff_unmasked": _p_ffff, "kmers_palindrome": _p_palindrome, "alpha_lower": _p_lower,
            "alpha_mixed": _p_mixed, "alpha_u": _p_u, "alpha_last_ambig_65": _p_last_ambig,
            "alpha_first_ambig": _p_first_ambig, "alpha_none_ambig": _p_none_ambig, "alpha_iupac": _p_iupac,
            "alpha_outside": _p_outside}


def test_every_case_has_a_property():
    assert set(PROPERTY) == set(C.BY_NAME)


@pytest.mark.parametrize("name", IDS)
def test_case_property(name):
    PROPERTY[name](name)


def test_perm_of_is_a_nontrivial_permutation():
    for c in C.CASES:
        p = C.perm_of(c)
        n = len(c.records)
        assert p.dtype == np.int32 and sorted(p) == list(range(n))
        assert n < 2 or list(p) != list(range(n))


# ------------------------------------------------------------------ one switch per rule
UNREACHABLE = ("l1_plus", "ambig_from_input")
REACHABLE = [r for r in R.RULES if r not in UNREACHABLE]
FIELDS = ("masked", "codes", "lens", "kmers", "nk", "changed", "n_changed", "ambig")


def _differs(a, b):
    return [f for f in FIELDS if not np.array_equal(np.asarray(a[f], object) if f in ("masked", "kmers") else a[f],
                                                    np.asarray(b[f], object) if f in ("masked", "kmers") else b[f])]


def witnesses(rule):
    """the cases (and fields) on which the flipped rule changes the reference under qmask_dust"""
    return {c.name: d for c in C.CASES for d in [_differs(ref(c), ref(c, 1, (rule,)))] if d}


# the case built for each rule: flipping the rule has to change that case, whatever else it changes
AIMED = {"best_ge": ("dust_tie_starts", "dust_tie_within"), "level_ge": ("dust_score20",),
         "l1_minus": ("len_homopolymer",), "step31": ("dust_window_starts",), "step33": ("dust_window_starts",),
         "end_exclusive": ("dust_score21", "dust_cross_63_64"), "kwin7": ("dust_ends_unmasked", "dust_cross_63_64"),
         "kwin9": ("dust_ends_unmasked", "dust_cross_63_64"), "minus_unmirrored": ("dust_cross_63_64",),
         "u_not_t": ("alpha_u",), "no_upper_unmasked": ("alpha_lower", "alpha_mixed")}


@pytest.mark.parametrize("rule", REACHABLE)
def test_every_rule_decides_a_case(rule):
    w = witnesses(rule)
    assert w, f"no case notices the rule {rule} flipped"
    for name in AIMED[rule]:
        assert name in w, (rule, name, sorted(w))


def test_rule_witnesses_by_field():
    """what each flip shows in: the mask rules in the masked bytes and the k-mers, the k-mer window rules in the k-mers
    alone, U in the codes and the ambiguity bit, the case rule in the masked bytes and the changed flags"""
    assert "masked" in witnesses("best_ge")["dust_tie_within"]
    assert "kmers" in witnesses("end_exclusive")["dust_cross_63_64"]
    for rule in ("kwin7", "kwin9", "minus_unmirrored"):
        assert set(f for d in witnesses(rule).values() for f in d) <= {"kmers", "nk"}
    assert {"codes", "ambig", "kmers"} <= set(witnesses("u_not_t")["alpha_u"])
    assert {"masked", "changed", "n_changed"} <= set(witnesses("no_upper_unmasked")["alpha_mixed"])
    assert set(witnesses("no_upper_unmasked")["alpha_lower"]) >= {"masked", "n_changed"}


def test_unreachable_rules():
    """Two switches change no output for any input, so no case can see them; each gets its reason instead of a witness.

    l1_plus (one more start, with 7 residues to the window's end): a start with n residues left scores at most
    10 * C(j - 1, 2) // j at its end j <= n - 1 (every triplet word equal), 16 for n = 7.  That is below the level, so
    the extra start masks nothing, and a smaller best score that it replaces masked nothing either.

    ambig_from_input: the output bytes differ from the input bytes in letter case only, and the 4-bit map reads both
    cases of a letter alike, so the bit is the same from either."""
    assert max(10 * ((j - 1) * (j - 2) // 2) // j for j in range(2, 7)) == 16 < 20
    assert R.windows("A" * 7, ("l1_plus",))[0]["bestv"] == 16
    for b in range(128):
        assert pyref.c4(chr(b)) == pyref.c4(chr(b).upper()) == pyref.c4(chr(b).lower())
    for rule in UNREACHABLE:
        for dust in (1, 0):
            assert not any(_differs(ref(c, dust), ref(c, dust, (rule,))) for c in C.CASES), rule
