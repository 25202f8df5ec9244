"""Scoring sets and pair families for the alignment kernels' pair-by-pair tests (test infrastructure, no GPU).

tests/test_gpu_align_kernels.py runs these through Context.align_pairs on each of the four alignment kernels
(k_align_pk, k_align_band, k_align<QL, true>, k_trace_wave) and compares with the C oracle;
tests/test_align_ref_cpu.py checks the oracle against oracle/pyref.py (nw + trim_id) on them and shows that every
rule of the operation decides at least one case.

Scoring sets: the presets and the corners of load.cpp validate()'s domain (DESIGN.md section 6, K3P range argument),
each at both boundary policies, plus the sets validate() has to refuse.
Families: inputs that make the rules fire which separate a right kernel from a nearly right one -- ties (strict
priorities), overhangs (terminal penalties, trailing-run counters), all-gap paths, short targets and targets on the
8-base code-word boundaries, identical pairs (largest summaries) and ordinary random pairs.
"""
from __future__ import annotations

import random
import re
from dataclasses import dataclass

MIN_QL, MAX_LEN = 32, 112
QLENS = tuple(range(MIN_QL, MAX_LEN + 1))
W = 66  # validate(): 2 * MAX_LEN * max(|match| + |mismatch|, go[k] + ge[k]) <= 15000
# gap penalties are indexed QL, TL, QI, TI, QR, TR (query / target; left end, interior, right end)


@dataclass(frozen=True)
class Scoring:
    name: str
    match: int
    mismatch: int
    go: tuple
    ge: tuple
    bopen: int
    refused: str | None = None  # validate() refuses the set with a message naming this field

    def lib_params(self):
        from umiclust import _lib
        p = _lib.params(1, 0.93, MIN_QL, MAX_LEN)
        return self._fill(p, p.gap_open, p.gap_ext)

    def orc_params(self):
        import orc
        p = orc.params(1, 0.93, MIN_QL, MAX_LEN)
        return self._fill(p, p.gap_open, p.gap_ext)

    def _fill(self, p, go, ge):
        p.match, p.mismatch, p.policy_boundary_open = self.match, self.mismatch, self.bopen
        for k in range(6):
            go[k], ge[k] = self.go[k], self.ge[k]
        return p

    def py_params(self):
        import pyref
        p = pyref.P(1, 0.93, MIN_QL, MAX_LEN)
        p.match, p.mismatch, p.go, p.ge, p.boundary_open = self.match, self.mismatch, list(self.go), list(self.ge), \
            bool(self.bopen)
        return p


def _scorings():
    out = []
    presets = {"preset1": (10, -40, (0, 0, 40, 40, 0, 0), (1, 1, 2, 2, 1, 1)),
               "preset2": (2, -4, (2, 2, 20, 20, 2, 2), (1, 1, 2, 2, 1, 1))}
    # the corners of validate()'s domain: |match| + |mismatch| = W in its three splits and DELTA = match - mismatch = 0
    subs = {"m33x33": (33, -33), "m0x66": (0, -66), "m66x0": (66, 0), "m5x5": (5, 5)}
    gaps = {"ext66": ((0,) * 6, (W,) * 6),                               # every gap column costs W, no opening
            "open66": ((W,) * 6, (0,) * 6),                              # every run costs W, extensions free
            "interior": ((0, 0, 40, 40, 0, 0), (0, 0, 26, 26, 0, 0))}    # interior penalties only, free ends
    for bo in (1, 0):
        for n, (ma, mi, go, ge) in presets.items():
            out.append(Scoring(f"{n}_bo{bo}", ma, mi, go, ge, bo))
        for sn, (ma, mi) in subs.items():
            for gn, (go, ge) in gaps.items():
                out.append(Scoring(f"{sn}_{gn}_bo{bo}", ma, mi, go, ge, bo))
    # A positive mismatch score with large extensions: the packed kernels' row potential (mismatch + ge[QI]) per row
    # puts the closed boundary state kNegInf above real cells of column 0, so validate() refuses the closed policy
    # where go[TL] + 111 (ge[TL] + mismatch + ge[QI]) + max(0, mismatch - match) + max(go[QI], go[QR]) > 16000
    # (DESIGN.md section 6); the open policy has no kNegInf state and is accepted.  At ext66, mismatch 12 is the
    # last accepted (111 * 144 = 15984) and 13 the first refused (111 * 145 + 13 = 16108).
    out.append(Scoring("m0x+66_ext66_bo1", 0, 66, (0,) * 6, (W,) * 6, 1))
    out.append(Scoring("m12x+12_ext66_bo0", 12, 12, (0,) * 6, (W,) * 6, 0))
    out.append(Scoring("m0x+66_ext66_bo0", 0, 66, (0,) * 6, (W,) * 6, 0, refused="policy_boundary_open"))
    out.append(Scoring("m0x+13_ext66_bo0", 0, 13, (0,) * 6, (W,) * 6, 0, refused="policy_boundary_open"))
    # A match that is not the best move (mismatch > match above, match < 0 here with free ends): the identical pair's
    # optimum is not the all-M path, which k_trace_wave writes without a DP only where a match is the best move.
    out.append(Scoring("m-5x-40_interior_bo1", -5, -40, (0, 0, 40, 40, 0, 0), (0, 0, 26, 26, 0, 0), 1))
    out.append(Scoring("m-5x-40_interior_bo0", -5, -40, (0, 0, 40, 40, 0, 0), (0, 0, 26, 26, 0, 0), 0))
    # outside the domain
    out.append(Scoring("mx67", 34, -33, (0,) * 6, (1,) * 6, 1, refused="16-bit"))
    out.append(Scoring("ext67", 10, -40, (0,) * 6, (1, 1, 67, 1, 1, 1), 1, refused="16-bit"))
    # negative gap components: the sums pass the bound from above, the components do not fit the 16-bit cells
    out.append(Scoring("go-20000", 10, -40, (-20000,) * 6, (20010,) * 6, 1, refused="gap_open"))
    out.append(Scoring("go-1_QI", 10, -40, (0, 0, -1, 40, 0, 0), (1, 1, 2, 2, 1, 1), 1, refused="gap_open"))
    out.append(Scoring("ge-1_TR", 10, -40, (0, 0, 40, 40, 0, 0), (1, 1, 2, 2, 1, -1), 1, refused="gap_ext"))
    out.append(Scoring("ge-20000", 2, -4, (20010,) * 6, (-20000,) * 6, 0, refused="gap_ext"))
    return out


SCORINGS = _scorings()
ACCEPTED = [s for s in SCORINGS if s.refused is None]
REFUSED = [s for s in SCORINGS if s.refused is not None]
BY_NAME = {s.name: s for s in SCORINGS}


# ------------------------------------------------------------------ pair families
def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _repeat(unit, n):
    return (unit * (n // len(unit) + 1))[:n]


_UNITS = ("A", "AC", "ACG")
_DROPS = (0, 1, 5)
TARGET_LENS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 111, 112)


def ties(ql):
    """Repeats of period 1, 2, 3 against the same repeat two and one shorter, one longer and with one unit replaced:
    the gap (or the mismatches) can sit anywhere and the strict priorities place it."""
    out = []
    for u in _UNITS:
        q = _repeat(u, ql)
        for tl in (ql - 2, ql - 1, ql + 1):
            if tl <= MAX_LEN:
                out.append(("ties", q, _repeat(u, tl)))
        x = (ql // 2 // len(u)) * len(u)
        out.append(("ties", q, q[:x] + "T" * len(u) + q[x + len(u):]))
    return out


def ends_targets(rng, ql):
    """(q, t) with t an infix of q and q an infix of t, 0 / 1 / 5 bases dropped from (added to) each side: leading and
    trailing D and I runs under the terminal penalties, a D run in the last column against an I run in the last row."""
    q = _rand(rng, ql)
    out = []
    for a in _DROPS:
        for b in _DROPS:
            if a or b:
                out.append((q, q[a:ql - b]))
            if ql + a + b <= MAX_LEN and (a or b):
                out.append((q, _rand(rng, a) + q + _rand(rng, b)))
    # the query's ends against a target one base short inside as well: a trailing run next to an interior gap
    out.append((q, q[1:ql // 2] + q[ql // 2 + 1:ql - 1]))
    return out


def ends(rng, ql):
    return [("ends", q, t) for q, t in ends_targets(rng, ql)]


def no_diagonal(ql):
    """A^ql against C^tl: no cell matches; under preset 1 the path is all gaps (internal length 0), under the
    mismatch-only sets it is the lowest reachable score."""
    return [("no_diagonal", "A" * ql, "C" * tl) for tl in sorted({1, 2, ql - 1, ql, MAX_LEN})]


def target_lengths(rng, ql):
    """Targets of 1, 2, 3 bases (the degenerate forms of the packed kernel's two last steps), on both sides of the 8-base
    code words, and of the largest lengths; random, homopolymer and identical-prefix queries.  Short and long targets
    alternate, so neighbours in a DPP row finish at different steps."""
    out = []
    rq = _rand(rng, ql)
    order = [TARGET_LENS[(k // 2) if k % 2 == 0 else len(TARGET_LENS) - 1 - k // 2] for k in range(len(TARGET_LENS))]
    for tl in order:
        out.append(("target_lengths", rq, _rand(rng, tl)))
        out.append(("target_lengths", "G" * ql, _repeat("G", tl) if tl % 2 else _rand(rng, tl, "GT")))
        pre = _rand(rng, MAX_LEN)
        out.append(("target_lengths", pre[:ql], pre[:tl]))
    return out


def identical(rng, ql):
    q = _rand(rng, ql)
    return [("identical", q, q)]


def _mutate(rng, a, nedits, alphabet="ACGT"):
    b = list(a)
    for _ in range(nedits):
        x = rng.randrange(len(b))
        u = rng.random()
        if u < 0.4:
            b[x] = rng.choice(alphabet)
        elif u < 0.7:
            b.insert(x, rng.choice(alphabet))
        elif len(b) > 1:
            del b[x]
    return "".join(b)


def random_pairs(seed, n, tl_lo=1):
    """tests/test_gpu_parity.py's _pairs (mutated copies, random targets, suffixes), non-ambiguous."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        ql = rng.choice(QLENS)
        q = _rand(rng, ql)
        kind = rng.random()
        if kind < 0.6:
            t = _mutate(rng, q, rng.randint(0, 10))
        elif kind < 0.8:
            t = _rand(rng, rng.randint(tl_lo, MAX_LEN))
        else:
            t = q[rng.randint(0, 6):] + _rand(rng, rng.randint(0, 6))
        out.append(("random", q, t[:MAX_LEN] if t else "A"))
    return out


def iupac():
    """Ambiguous symbols in query and target at rows 0 and QL-1 and at columns 0 and tl-1 (they score 0 and match by
    code intersection), N against N, targets from one base."""
    rng = random.Random(77)
    out = []
    for ql in (32, 33, 57, 64, 65, 112):
        q = _rand(rng, ql)
        for tl in (1, 2, 9, ql - 1, ql, min(MAX_LEN, ql + 3)):
            t = (q + _rand(rng, 3))[:tl] if tl > 3 else _rand(rng, tl)
            for sym in "NRK":
                qa = sym + q[1:-1] + sym
                ta = sym + t[1:-1] + sym if tl > 1 else sym
                out += [("iupac", qa, t), ("iupac", q, ta), ("iupac", qa, ta)]
            out.append(("iupac", "N" * ql, "N" * tl))
            out.append(("iupac", q[:ql // 2] + "N" + q[ql // 2 + 1:], t[:tl // 2] + "Y" + t[tl // 2 + 1:]))
    return out


_CACHE = {}


def base_cases():
    """[(family, query, target)] for every query length 32..112, in launch order within a length."""
    if "base" not in _CACHE:
        rng = random.Random(20261)
        out = []
        for ql in QLENS:
            out += ties(ql) + ends(rng, ql) + no_diagonal(ql) + target_lengths(rng, ql) + identical(rng, ql)
        out += random_pairs(515, 300)
        _CACHE["base"] = out
    return _CACHE["base"]


def kernel_cases(kernel):
    """The pairs of one align_pairs call per kernel: pk and band the base cases, amb and trace the base cases and the
    IUPAC family (one ambiguous symbol in a call sends the whole call to k_align<QL, true>)."""
    assert kernel in KERNELS
    if kernel in ("pk", "band"):
        return base_cases()
    if "amb" not in _CACHE:
        _CACHE["amb"] = base_cases() + iupac()
    return _CACHE["amb"]


KERNELS = ("pk", "band", "amb", "trace")
BAND_ENV = {"pk": "0", "band": str(1 << 30)}  # UMICLUST_BAND, read when the context is created

SHAPE_QLENS = (32, 56, 57, 64, 65, 105, 112)  # G = 4 / 8 lanes per pair, virtual rows P in {0, 7}


def band_lanes(ql):
    return 8 if ql >= 57 else 4


def launch_shapes():
    """[(name, [(q, t)])]: each item is one align_pairs call of one query length, so its pair count is the launch size.
    Partial and full waves and lane groups, short targets beside long ones in one DPP row, one target shared by all."""
    if "shapes" in _CACHE:
        return _CACHE["shapes"]
    rng = random.Random(99)
    out = []
    for ql in SHAPE_QLENS:
        g = band_lanes(ql)
        pool = []
        while len(pool) < 65:
            pool += ends_targets(rng, ql)
        for n in sorted({1, 64 // g - 1, 64 // g, 64 // g + 1, 63, 64, 65}):
            out.append((f"ql{ql}_n{n}", pool[:n]))
        q = _rand(rng, ql)
        alt = [(q, q[k % 4] if k % 2 == 0 else (q[k % 5:] + _rand(rng, MAX_LEN))[:MAX_LEN])
               for k in range(2 * (64 // g) + 1)]
        out.append((f"ql{ql}_alt_1_112", alt))
        out.append((f"ql{ql}_alt_112_1", alt[1:]))
        t = q[2:ql - 3]
        out.append((f"ql{ql}_shared", [(_mutate(rng, q, k % 4)[:ql].ljust(ql, "A"), t) for k in range(64 // g + 3)]))
    _CACHE["shapes"] = out
    return out


# ------------------------------------------------------------------ references
def expand(cigar):
    return "".join(o * (int(n) if n else 1) for n, o in re.findall(r"(\d*)([MDI])", cigar))


def orc_ref(s: Scoring, q, t):
    """(score, matches, internal_len, ops) by the C oracle"""
    import orc
    o = orc.align(_orc_params(s), q, t)
    return o["score"], o["matches"], o["internal_len"], expand(o["cigar"])


_ORC_P = {}


def _orc_params(s):
    if s.name not in _ORC_P:
        _ORC_P[s.name] = s.orc_params()
    return _ORC_P[s.name]


def py_ref(s: Scoring, q, t, rules=()):
    """(score, matches, internal_len, ops) by oracle/pyref.py: nw + trim_id, with `rules` switched"""
    import pyref
    score, cigar, m = pyref.nw(s.py_params(), q, t, rules)
    _, internal = pyref.trim_id(cigar, m, rules)
    return score, m, internal, expand(cigar)


_EXPECT = {}


def expected(s: Scoring, key, pairs):
    """The oracle's results for a list of (q, t), computed once per (scoring set, key) and shared by the kernels."""
    k = (s.name, key)
    if k not in _EXPECT:
        _EXPECT[k] = [orc_ref(s, q, t) for q, t in pairs]
    return _EXPECT[k]
