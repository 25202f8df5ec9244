"""The smallest inputs at which the load kernel (K1, k_prep_wave) can go wrong (test infrastructure, no GPU).

Each case is one batch of a few records with the property it pins; tests/test_prep_ref_cpu.py asserts every property
by the case's name against tests/prep_ref.py, tests/test_gpu_prep.py runs every batch through the kernel with
qmask_dust 1 and 0 and once under perm_of().  The flag words are per batch, so a case about them is a batch of its
own.  The DUST shapes (a best score of exactly 20 or 21, tied bests) and the k-mer layouts that depend on a sort order
are found by a seeded random search when this module is imported (a few hundredths of a second): nothing here is a
recorded answer.

Where the kernel takes another path, and the case that stands there:
  len < 7 (wo()'s `l1 < 0` cut-off), 7 (no start), 8 (one start, the first k-mer), a last window of 1..8 residues at
  i0 = 32, 64, 96, positions 63 / 64 (the two halves m0 / m1, in0 / in1, the win8 shifts at p = 0, 57..63 and 64),
  code word boundaries (multiples of 8), 105 k-mers (both sort halves full), len = 112 (every lane holds two residues).
"""
from __future__ import annotations

import random
from dataclasses import dataclass

import numpy as np
import prep_ref as R
from pyref import revcomp

# 0..17, and around every window start (a last window of 1..9 residues at i0 = 32, 64, 96) up to the longest record
LENGTHS = tuple(range(0, 18)) + tuple(range(31, 42)) + tuple(range(63, 74)) + tuple(range(95, 106)) + (110, 111, 112)
IUPAC = "ACGTURYSWKMBDHVN"
OUTSIDE = "-.059@[_"  # bytes that are no letters: 0x40 and 0x5B..0x5F sit between the two cases of the ASCII letters


@dataclass(frozen=True)
class Case:
    name: str
    records: tuple
    pins: str


def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _plain(s):
    """no window of s reaches DUST's level: nothing is masked, also not with the level one lower"""
    return all(w["bestv"] < 20 for w in R.windows(s))


def _rand_plain(rng, n):
    for _ in range(10000):
        s = _rand(rng, n)
        if _plain(s):
            return s
    raise AssertionError("no unmasked random sequence found")


def _search(seed, make, want, tries=200000):
    rng = random.Random(seed)
    for _ in range(tries):
        s = make(rng)
        if want(s):
            return s
    raise AssertionError("search exhausted")


def _two_letter(rng):
    a, b = rng.sample("ACGT", 2)
    pa = rng.choice((0.5, 0.6, 0.7))
    return "".join(a if rng.random() < pa else b for _ in range(40))


def _shape(s):
    """(best score, starts that reach it, (start, end) pairs that reach it) of the first window of a 40-mer whose short
    second window (8 residues at i0 = 32) masks nothing"""
    w = R.windows(s)
    if len(w) != 2 or w[1]["bestv"] >= 20:
        return None
    t = w[0]["ties"]
    return w[0]["bestv"], len({i for i, _ in t}), len(t)


def _dust_shapes():
    return [
        Case("dust_score20", (_search(1, _two_letter, lambda s: (_shape(s) or (0,))[0] == 20),),
             "a window whose best score is exactly 20: not masked"),
        Case("dust_score21", (_search(2, _two_letter, lambda s: _shape(s) == (21, 1, 1)),),
             "a window whose best score is exactly 21, reached once: masked"),
        Case("dust_tie_starts", (_search(3, _two_letter, lambda s: (_shape(s) or (0, 0, 0))[0] == 21 and
                                         _shape(s)[1] >= 2 and _shape(s)[1] == _shape(s)[2]),),
             "the best score 21 reached from several starts, once each: the first start wins"),
        Case("dust_tie_within", (_search(4, _two_letter, lambda s: (_shape(s) or (0, 0, 0))[0] == 21 and
                                         _shape(s)[1] == 1 and _shape(s)[2] >= 2),),
             "the best score 21 reached at several ends of one start: the first end wins"),
    ]


def _dust_layouts():
    out = []
    # positions 60..70 masked, nothing else: lane 60..63's m0 and lanes 0..6's m1, the win8 shifts around p = 57..64
    out.append(Case("dust_cross_63_64", (_search(12, lambda r: _rand_plain(r, 60) + "A" * 11 + _rand_plain(r, 29),
                                                 lambda s: R.mask_bits(s) == [60 <= j <= 70 for j in range(100)]),),
                    "one masked run at exactly 60..70, across the two lane halves"))
    # a run that starts at position 64, and one that ends at 63: a k-mer window at p = 57..63 is dropped for mask bits
    # of the second half alone, a window at p = 64 reads none of the first half's
    out.append(Case("dust_from_64", (_search(18, lambda r: _rand_plain(r, 64) + "G" * 11 + _rand_plain(r, 25),
                                             lambda s: R.mask_bits(s) == [64 <= j <= 74 for j in range(100)]),),
                    "one masked run at exactly 64..74: the first half's lanes hold no mask bit"))
    out.append(Case("dust_to_63", (_search(19, lambda r: _rand_plain(r, 53) + "C" * 11 + _rand_plain(r, 36),
                                           lambda s: R.mask_bits(s) == [53 <= j <= 63 for j in range(100)]),),
                    "one masked run at exactly 53..63: the second half's lanes hold no mask bit"))
    # a long two-letter repeat: the windows at 0, 32 and 64 mask overlapping intervals, neither inside the other
    out.append(Case("dust_merge", (_search(13, lambda r: _rand_plain(r, 10) + "AC" * 40 + _rand_plain(r, 10),
                                           lambda s: _overlapping(R.intervals(s))),),
                    "the masks of two overlapping windows merge into one run"))
    # a strong run that the windows at 32 and 64 choose, and a weaker one at 100..111 that only the window at 96 chooses
    out.append(Case("dust_only_window_96", (_search(14, lambda r: _rand_plain(r, 66) + "A" * 20 + _rand_plain(r, 14) +
                                                    "C" * 12, _only_96),),
                    "a low-complexity run that only the window at i0 = 96 masks"))
    # a window masks its one best interval.  Record 0: a strong run at 0..19 and 8 x C at 32..39, which the window at 0
    # passes over and the window at 32 masks (a window at 33 holds 7 of it: score 16).  Record 1: 8 x G at 88..95, the
    # last residues of the window at 32, and a strong run at 96..111 that every later window prefers (a window at 31
    # ends at 94)
    out.append(Case("dust_window_starts",
                    (_search(16, lambda r: "A" * 20 + _rand_plain(r, 12) + "C" * 8 + _rand_plain(r, 30),
                             lambda s: all(R.mask_bits(s)[32:40]) and not any(R.mask_bits(s, ("step33",))[32:40])),
                     _search(17, lambda r: _rand_plain(r, 88) + "G" * 8 + "T" * 16,
                             lambda s: all(R.mask_bits(s)[88:96]) and not any(R.mask_bits(s, ("step31",))[88:96]))),
                    "runs that one window alone masks, at its first and at its last 8 residues: the windows start "
                    "every 32 residues"))
    out.append(Case("dust_all_112", ("A" * 112, "GT" * 56), "a fully masked 112-mer: no k-mer on either strand"))
    out.append(Case("dust_ends_unmasked", (_search(15, lambda r: _rand_plain(r, 8) + "CT" * 20 + _rand_plain(r, 8),
                                                   lambda s: R.mask_bits(s) == [8 <= j < 48 for j in range(56)]),),
                    "everything masked but the first and the last 8 residues: one k-mer window at each end"))
    return out


def _overlapping(iv):
    return any(a[0] < b[0] <= a[1] < b[1] for a in iv for b in iv)


def _only_96(s):
    by = {w["i0"]: w for w in R.windows(s)}
    if len(s) != 112 or by[96]["bestv"] <= 20:
        return False
    lo = 96 + by[96]["besti"]
    mine = set(range(lo, lo + by[96]["bestj"] + 1))
    others = set()
    for i0 in (0, 32, 64):
        if by[i0]["bestv"] > 20:
            others |= set(range(i0 + by[i0]["besti"], i0 + by[i0]["besti"] + by[i0]["bestj"] + 1))
    return bool(mine) and not (mine & others) and bool(others)


def _distinct105(s):
    r = R.prep([s])
    return r["n_changed"] == 0 and tuple(r["nk"][0]) == (105, 105)


def _straddle(s):
    """no masking, and the sorted k-mer keys of the plus strand hold a duplicate pair at sorted elements 63 and 64, the
    last of the first lane half and the first of the second"""
    if not _plain(s):
        return False
    keys = sorted(R.kmer_code(s[x:x + 8]) for x in range(len(s) - 7))
    return len(keys) == 105 and keys[63] == keys[64]


def _kmer_cases():
    x = _search(23, lambda r: _rand(r, 56), lambda h: _plain(h + revcomp(h)))
    return [
        Case("kmers_105_distinct", (_search(21, lambda r: _rand(r, 112), _distinct105),),
             "105 distinct unmasked 8-mers on both strands: every key of the sort is a k-mer"),
        Case("kmers_one_repeated", ("A" * 112, "T" * 112, "C" * 8, "T" * 8, "A" * 8),
             "without masking one 8-mer 105 times (and once); T x 8 = 0xffff, the largest code, next to the sentinels"),
        Case("kmers_straddle_halves", (_search(22, lambda r: (lambda h: h + h)(_rand(r, 56)), _straddle),),
             "a record repeated within itself: a duplicate pair at sorted elements 63 / 64, across the lane halves"),
        Case("kmers_ffff_unmasked", (_search(24, lambda r: _rand_plain(r, 30) + "TTTTTTTT" + _rand_plain(r, 30),
                                             lambda s: True), "TTTTTTTT" + _rand_plain(random.Random(25), 50)),
             "TTTTTTTT inside a record: masked under qmask_dust, the largest code without it"),
        Case("kmers_palindrome", (x + revcomp(x),), "a record equal to its reverse complement: both lists are equal"),
    ]


def _alphabet_cases():
    rng = random.Random(31)
    base = [_rand_plain(rng, n) for n in (64, 65, 70, 58)]
    mixed = "".join(ch.lower() if rng.random() < 0.5 else ch for ch in base[2])
    low = "ACACACACACACACACACACACACAC"
    out = [
        Case("alpha_lower", tuple(s.lower() for s in base) + ((base[0][:20] + low + base[0][20:40]).lower(),),
             "all-lower-case input, unmasked and masked: every record changes, no symbol is ambiguous"),
        Case("alpha_mixed", (mixed, base[1], base[3].lower()), "mixed-case input beside untouched upper case"),
        Case("alpha_u", (base[0].replace("T", "U"), base[1].replace("T", "u"), "U" * 20, "ACGU" * 10 + "uuuuuuuuuuuu"),
             "U and u read as T: no ambiguity, T's codes, k-mers and DUST words"),
        Case("alpha_last_ambig_65", (base[0] + "N",),
             "the only ambiguous symbol is residue 64 of a 65-mer: only the second lane half sees it"),
        Case("alpha_none_ambig", (base[0], base[2], base[1].lower(), "ACGU" * 12),
             "no ambiguous symbol in the batch: the ambiguity bit stays 0"),
        Case("alpha_first_ambig", ("N" + base[0][1:],), "the only ambiguous symbol is residue 0"),
    ]
    recs = []
    for k, ch in enumerate(IUPAC):
        b = _rand_plain(rng, 40)
        recs += [b[:k + 3] + ch + b[k + 3:], (b[:20] + ch.lower() + b[20:]).lower()]
    recs += [IUPAC + IUPAC.lower() + IUPAC[::-1], "N" * 30, "n" * 30, "RY" * 20]
    out.append(Case("alpha_iupac", tuple(recs), "each IUPAC letter in both cases: its code, its complement, k-mer "
                    "code 0 for ambiguous letters"))
    b = _rand_plain(rng, 60)
    recs = []
    for k, ch in enumerate(OUTSIDE):
        recs += [b[:10 + k] + ch + b[10 + k:],                       # outside a masked run
                 b[:12] + "AAAAAA" + ch + "AAAAAA" + b[12:30],       # inside one
                 ch * 20]                                             # a run of nothing else
    recs.append(b[:8] + OUTSIDE + OUTSIDE + "acacacacacacacacac" + OUTSIDE)
    out.append(Case("alpha_outside", tuple(recs),
                    "bytes that are no letters, inside and outside a masked run: code 0, ambiguous, never re-cased"))
    return out


def _length_cases():
    rng = random.Random(41)
    return [
        Case("len_random", tuple(_rand(rng, n) for n in LENGTHS),
             "every length at which the kernel takes another path, random ACGT"),
        Case("len_homopolymer", tuple("ACGT"[k % 4] * n for k, n in enumerate(LENGTHS)),
             "the same lengths as homopolymers: masked end to end from 8 residues on"),
        Case("len_two_letter",
             tuple(("CA", "GT", "AG")[k % 3] * (n // 2) + "C" * (n % 2) for k, n in enumerate(LENGTHS)),
             "the same lengths as two-letter repeats: long masked runs with a last window of 1..8 residues"),
        Case("len_empty_batch", ("", "", ""), "records of length 0 only: no byte is read, every output is 0"),
    ]


CASES = _length_cases() + _dust_shapes() + _dust_layouts() + _kmer_cases() + _alphabet_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def perm_of(case) -> np.ndarray:
    """a permutation of the case's records that is not the identity (where there are two or more)"""
    n = len(case.records)
    p = list(range(n))
    random.Random(case.name).shuffle(p)
    if p == list(range(n)):
        p.reverse()
    return np.array(p, np.int32)
