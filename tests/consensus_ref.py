"""Plain reference of the consensus kernel (k_consensus) and the input families of tests/test_gpu_consensus.py, which
also checks the member tracebacks (k_trace_wave) as the pipeline launches them.  Pure Python on top of the oracle's
pairwise aligner; no GPU.

The rule (oracle/umiclust_oracle.c msa_consensus, vsearch msa.cc), for one cluster of m sequences, centroid first.
A member's ops are in alignment order: M = a member residue against a centroid residue, D = a member residue against
a gap in the centroid (an insertion), I = a centroid residue against a gap in the member.
  slot p    = the insertions before centroid position p (p = clen: after the last); maxi[p] columns wide
  columns   = slot 0, centroid residue 0, slot 1, ..., centroid residue clen - 1, slot clen: clen + sum(maxi)
  a column  = one symbol per sequence: a residue or a gap, so gaps = m - residues
  output    = for every column outside slot 0 and slot clen: the best of A, C, G, T, if its count >= gaps
msa_ref states it with one switch per rule; every switch at its default is pyref.msa (asserted on every case by
tests/test_consensus_ref_cpu.py), and flipping one switch gives what a kernel with exactly that mistake would emit:
  (a) tie_first        a tie among A, C, G, T takes the first in that order             | the last
  (b) emit_on_equal    a column is emitted iff best count >= gap count                  | best > gaps
  (c) censor_left      the maxi[0] columns of slot 0 are never emitted                  | they are voted on
  (d) censor_right     the maxi[clen] columns of slot clen are never emitted            | they are voted on
  (e) n_last           N wins only when no A/C/G/T was seen in the column               | N wins when it outnumbers them
  (f) iupac_as_n       any other IUPAC letter counts as N (U is T)                      | as the first base it stands for
  (g) left_justify     an insertion run starts at its slot's first column               | ends at its last
  (h) minus_revcomp    a minus-strand member is read as its reverse complement          | as it is
  (i) maxi_is_max      maxi[p] is the longest run any member has in slot p              | the shortest; longer runs are cut
  (j) tail_slot_clen   a run after the last centroid residue belongs to slot clen       | to slot clen - 1
(For (j), a kernel that merely forgot the trailing run would emit the same bytes: slot clen is censored either way.
The flip that shows is the run booked one slot early.)
"""
from __future__ import annotations

import functools
import random
import re

import orc
import pyref
from pyref import revcomp

MAX_LEN = 112            # kMaxLen
OPS_STRIDE = 2 * MAX_LEN  # kOpsStride
MSA_COLS = 2048          # kMsaCols
CONS_CAP = 2 * MAX_LEN    # kConsCap
TW_SPLIT = 64            # plan.h kTwSplit: queries up to this length go to the first traceback launch
RULES = ("tie_first", "emit_on_equal", "censor_left", "censor_right", "n_last", "iupac_as_n", "left_justify",
         "minus_revcomp", "maxi_is_max", "tail_slot_clen")
_FIRST_BASE = dict(zip("RYSWKMBDHV", "ACCAGAACAA"))  # the first of A, C, G, T an ambiguity code stands for


def expand(cigar: str) -> str:
    """'3MD2I' or 'MMMDII' -> 'MMMDII'"""
    return "".join(o * (int(n) if n else 1) for n, o in re.findall(r"(\d*)([MDI])", cigar))


def compress(ops: str) -> str:
    """'MMMDII' -> '3MD2I', the form orc.align and pyref use"""
    return "".join((str(len(g.group(0))) if len(g.group(0)) > 1 else "") + g.group(0)[0]
                   for g in re.finditer(r"M+|D+|I+", ops))


def _runs(ops: str, clen: int, tail_slot_clen: bool):
    """[(slot, first member residue, length)] of the D runs, and per centroid position the member residue or -1"""
    runs, at, pos, t, x = [], [-1] * clen, 0, 0, 0
    while x < len(ops):
        if ops[x] == "D":
            y = x
            while y < len(ops) and ops[y] == "D":
                y += 1
            slot = pos if (pos < clen or tail_slot_clen) else clen - 1
            runs.append((slot, t, y - x))
            t += y - x
            x = y
            continue
        if ops[x] == "M":
            at[pos] = t
            t += 1
        pos += 1
        x += 1
    return runs, at


def msa_ref(db, mem, strand, cig, *, tie_first=True, emit_on_equal=True, censor_left=True, censor_right=True,
            n_last=True, iupac_as_n=True, left_justify=True, minus_revcomp=True, maxi_is_max=True,
            tail_slot_clen=True) -> str:
    """The consensus of the cluster mem (indices into db, centroid first); strand[s] and cig[s] (either CIGAR form) for
    the members s = mem[1:]."""
    cen = db[mem[0]]
    clen = len(cen)
    walked = {s: _runs(expand(cig[s]), clen, tail_slot_clen) for s in mem[1:]}
    maxi = [0] * (clen + 1)
    for runs, _ in walked.values():
        for slot, _t, n in runs:
            maxi[slot] = max(maxi[slot], n) if (maxi_is_max or maxi[slot] == 0) else min(maxi[slot], n)
    first = [0] * (clen + 1)  # first column of slot p; centroid residue p sits at first[p] + maxi[p]
    for p in range(clen):
        first[p + 1] = first[p] + maxi[p] + 1
    ncols = clen + sum(maxi)
    prof = [dict.fromkeys("ACGTN", 0) for _ in range(ncols)]

    def count(col, ch):
        ch = ch.upper()
        if ch == "U":
            ch = "T"
        if ch not in "ACGTN":
            ch = "N" if iupac_as_n else _FIRST_BASE.get(ch, "N")
        prof[col][ch] += 1

    for p in range(clen):
        count(first[p] + maxi[p], cen[p])
    for s in mem[1:]:
        seq = revcomp(db[s]) if (strand[s] and minus_revcomp) else db[s]
        runs, at = walked[s]
        for p in range(clen):
            if at[p] >= 0:
                count(first[p] + maxi[p], seq[at[p]])
        for slot, t, n in runs:
            n = min(n, maxi[slot])  # only ever shorter when maxi is not the maximum
            c0 = first[slot] + (0 if left_justify else maxi[slot] - n)
            for x in range(n):
                count(c0 + x, seq[t + x])
    lo = maxi[0] if censor_left else 0
    hi = ncols - (maxi[clen] if censor_right else 0)
    out = []
    for col in range(lo, hi):
        pr = prof[col]
        best, bc = "A", 0
        for b in "ACGT":
            if pr[b] > bc or (not tie_first and pr[b] == bc and bc > 0):
                best, bc = b, pr[b]
        if pr["N"] > 0 and (bc == 0 if n_last else pr["N"] > bc):
            best, bc = "N", pr["N"]
        gaps = len(mem) - sum(pr.values())
        if bc >= gaps if emit_on_equal else bc > gaps:
            out.append(best)
    return "".join(out)


def msa_width(db, mem, cig) -> int:
    """columns of the cluster's alignment: clen + sum(maxi), what k_consensus holds against kMsaCols"""
    clen = len(db[mem[0]])
    maxi = [0] * (clen + 1)
    for s in mem[1:]:
        for slot, _t, n in _runs(expand(cig[s]), clen, True)[0]:
            maxi[slot] = max(maxi[slot], n)
    return clen + sum(maxi)


def ops_valid(ops: str, clen: int, mlen: int) -> bool:
    """what umiclust_consensus demands of a member's given ops before it launches anything"""
    return (set(ops) <= set("MDI") and len(ops) <= OPS_STRIDE and ops.count("M") + ops.count("I") == clen
            and ops.count("M") + ops.count("D") == mlen)


# ---------------------------------------------------------------- cases
# A case is (seqs, clusters, strands, cigars): clusters = lists of indices into seqs (centroid first), strands and
# cigars in the same shape (the centroid's entries 0 and ""); cigars is None for a traced case, whose ops are the
# aligner's.
class _Build:
    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.seqs, self.clusters, self.strands, self.cigars = [], [], [], []

    def rand(self, n, alphabet="ACGT"):
        return "".join(self.rng.choice(alphabet) for _ in range(n))

    def cluster(self, cen, members, strands=None, cigars=None):
        """members: sequences as the records hold them (a minus-strand member already reverse-complemented)"""
        i0 = len(self.seqs)
        self.seqs += [cen] + list(members)
        self.clusters.append(list(range(i0, i0 + 1 + len(members))))
        self.strands.append([0] + list(strands or [0] * len(members)))
        self.cigars.append([""] + list(cigars or [""] * len(members)))

    def loose(self, seq):
        """a record in no cluster"""
        self.seqs.append(seq)

    def done(self, given=False):
        return self.seqs, self.clusters, self.strands, (self.cigars if given else None)

    def member(self, cen, length=None, subs=1, minus=False, ends=False):
        """cen with `subs` substitutions, then single-base indels (near the ends if `ends`) until it is `length` long
        (default: one insertion and one deletion, the length kept)"""
        rng = self.rng
        b = list(cen)
        for _ in range(subs):
            b[rng.randrange(len(b))] = rng.choice("ACGT")

        def where(n):
            if ends and n > 8:
                return rng.choice([rng.randrange(0, 4), rng.randrange(n - 4, n)])
            return rng.randrange(n)
        if length is None:
            b.insert(where(len(b) + 1), rng.choice("ACGT"))
            del b[where(len(b))]
        else:
            while len(b) < length:
                b.insert(where(len(b) + 1), rng.choice("ACGT"))
            while len(b) > length:
                del b[where(len(b))]
        s = "".join(b)
        return revcomp(s) if minus else s


def _traced_maxl(L):
    """a call whose longest record is exactly L: lengths on both sides of the launch split wherever L allows, the
    centroid not always the longest of its cluster"""
    def build():
        b = _Build(1000 + L)
        lens = sorted({x for x in (L, L - 1, L - 7, L // 2, TW_SPLIT - 1, TW_SPLIT, TW_SPLIT + 1, 33, 40) if 1 <= x <= L})
        for cl in lens:
            cen = b.rand(cl)
            mem, st = [], []
            for ml in lens:
                if abs(ml - cl) > 40:
                    continue
                for minus in (False, True):
                    mem.append(b.member(cen, ml, subs=2, minus=minus))
                    st.append(int(minus))
            b.cluster(cen, mem, st)
        assert max(map(len, b.seqs)) == L
        return b.done()
    return build


def _traced_long_only():
    """every member longer than 64: the first launch is empty (one centroid is short)"""
    b = _Build(2001)
    for cl in (60, 66, 90, 112):
        cen = b.rand(cl)
        lens = [65, 66, 80, 100, 111, 112]
        b.cluster(cen, [b.member(cen, ml, minus=ml % 2 == 0) for ml in lens], [int(ml % 2 == 0) for ml in lens])
    return b.done()


def _traced_short_vs_long():
    """members of at most 64 nt against centroids of 65 .. 112: the one-stripe launch with targets longer than a
    stripe; the second launch is empty"""
    b = _Build(2002)
    for cl in (65, 72, 100, 112):
        cen = b.rand(cl)
        mem, st = [], []
        for ml in (20, 40, 63, 64):
            for minus in (False, True):
                a = b.rng.randrange(0, cl - ml + 1)
                mem.append(b.member(cen[a:a + ml], ml, subs=1, minus=minus))
                st.append(int(minus))
        b.cluster(cen, mem, st)
    return b.done()


def _traced_edges():
    """lengths 63, 64, 65, 111, 112 against each other; members equal to the centroid (the all-M shortcut), equal but
    for one N or R on either side (the shortcut must not fire), of equal length with one other base; lengths 1 and 2"""
    b = _Build(2003)
    for cl in (63, 64, 65, 111, 112):
        cen = b.rand(cl)
        x = cl // 2
        other = "ACGT"["ACGT".index(cen[x]) - 1]
        mem = [cen, revcomp(cen), cen[:x] + "N" + cen[x + 1:], cen[:x] + "R" + cen[x + 1:],
               revcomp(cen[:-1] + "N"), cen[:x] + other + cen[x + 1:], other + cen[1:], cen[:-1] + other,
               cen.lower(), cen.replace("T", "U")]
        st = [0, 1, 0, 0, 1, 0, 0, 0, 0, 0]
        for ml in (63, 64, 65, 111, 112):
            if abs(ml - cl) <= 2:
                mem += [b.member(cen, ml, minus=False), b.member(cen, ml, minus=True)]
                st += [0, 1]
        b.cluster(cen, mem, st)
        # an ambiguous centroid and members equal to it: code-for-code identical, yet not one-hot
        amb = cen[:x] + "N" + cen[x + 1:]
        b.cluster(amb, [amb, cen, revcomp(amb)], [0, 0, 1])
    for cen in ("A", "AC", "ACGTACGTAC", b.rand(40)):
        mem = ["A", "C", "AC", "CA", "GT", "N", "G" + cen, cen + "T", cen]
        b.cluster(cen, mem, [0, 0, 0, 0, 1, 0, 0, 0, 0])
    return b.done()


def _traced_minus_indels():
    """minus-strand members with indels near both ends"""
    b = _Build(2004)
    for cl in (34, 60, 64, 68, 100):
        cen = b.rand(cl)
        mem, st = [], []
        for d in (-3, -1, 0, 1, 3):
            for minus in (True, True, False):
                mem.append(b.member(cen, max(1, min(MAX_LEN, cl + d)) if d else None, subs=1, minus=minus, ends=True))
                st.append(int(minus))
        b.cluster(cen, mem, st)
    return b.done()


def _traced_sizes():
    """cluster sizes around k_consensus's 256-thread stride, the members past a stride carrying the majority"""
    b = _Build(2005)
    for size in (1, 2, 3, 255, 256, 257, 513):
        cen = b.rand(b.rng.choice((36, 44, 66)))
        var = b.member(cen, len(cen) + 1, subs=1)  # what most of the members past the first few look like
        mem = [b.member(cen, subs=1, minus=i % 3 == 0) if i < size // 2 - 1 else
               (revcomp(var) if i % 3 == 0 else var) for i in range(size - 1)]
        b.cluster(cen, mem, [int(i % 3 == 0) for i in range(size - 1)])
    return b.done()


def _traced_many():
    """several hundred small clusters (one workgroup each), records in no cluster between them, the members not
    stored next to their centroid"""
    b = _Build(2006)
    for k in range(400):
        cl = b.rng.choice((33, 58, 63, 64, 65, 68, 72))
        cen = b.rand(cl)
        nm = b.rng.randrange(0, 6)
        st = [b.rng.randrange(2) for _ in range(nm)]
        b.cluster(cen, [b.member(cen, cl + b.rng.randrange(-2, 3), minus=bool(s)) for s in st], st)
        if k % 7 == 0:
            b.loose(b.rand(50))
    seqs, clusters, strands, _ = b.done()
    perm = list(range(len(seqs)))
    b.rng.shuffle(perm)  # record i moves to perm[i]
    moved = [None] * len(seqs)
    for i, s in enumerate(seqs):
        moved[perm[i]] = s
    return moved, [[perm[i] for i in m] for m in clusters], strands, None


TRACED = {**{f"maxl{L}": _traced_maxl(L) for L in (33, 64, 65, 72, 112)},
          "long_only": _traced_long_only, "short_vs_long": _traced_short_vs_long, "edges": _traced_edges,
          "minus_indels": _traced_minus_indels, "sizes": _traced_sizes, "many": _traced_many}
SCORINGS = [(1, 1), (2, 1), (1, 0), (2, 0)]  # (preset, policy_boundary_open)


def _given_disagree():
    """two-sequence clusters that disagree in every column: every vote is a tie"""
    b = _Build(3001)
    for rot in (1, 2, 3):
        cen = b.rand(40)
        b.cluster(cen, ["".join("ACGT"[("ACGT".index(c) + rot) % 4] for c in cen)], cigars=["M" * 40])
    cen = b.rand(33)
    mem = "".join("ACGT"[("ACGT".index(c) + 2) % 4] for c in cen)
    b.cluster(cen, [revcomp(mem)], [1], ["M" * 33])
    return b.done(True)


def _given_best_vs_gaps():
    """columns whose best count equals the gap count (emitted) or is one short of it (not), among centroid columns
    and among inserted ones"""
    b = _Build(3002)
    cen = b.rand(36)
    other = lambda c: "ACGT"[("ACGT".index(c) + 1) % 4]  # noqa: E731
    # 4 sequences; at 10 and 20 two members have a gap: best 2 == gaps 2 at 10, best 1 == gaps - 1 at 20 (the third
    # member disagrees with the centroid there)
    gap = lambda s, ps: "".join(c for i, c in enumerate(s) if i not in ps)  # noqa: E731
    ops = lambda ps: "".join("I" if i in ps else "M" for i in range(36))  # noqa: E731
    m3 = cen[:20] + other(cen[20]) + cen[21:]
    b.cluster(cen, [gap(cen, {10, 20}), gap(cen, {10, 20}), m3], cigars=[ops({10, 20}), ops({10, 20}), "M" * 36])
    ins = lambda at, ch: cen[:at] + ch + cen[at:]  # noqa: E731
    iops = lambda at: "M" * at + "D" + "M" * (36 - at)  # noqa: E731
    # 6 sequences; slot 12: three members insert the same base (best 3 == gaps 3: emitted); slot 24: two do (2 < 4)
    b.cluster(cen, [ins(12, "G")] * 3 + [ins(24, "T")] * 2, cigars=[iops(12)] * 3 + [iops(24)] * 2)
    # 6 sequences; slot 24: two members insert T and one C (best 2 == gaps 3 - 1: not emitted)
    b.cluster(cen, [ins(24, "T")] * 2 + [ins(24, "C"), cen, cen], cigars=[iops(24)] * 3 + ["M" * 36] * 2)
    # 5 sequences; the same slot: best 2 == gaps 2 though 3 residues stand in the column (emitted)
    b.cluster(cen, [ins(24, "T")] * 2 + [ins(24, "C"), cen], cigars=[iops(24)] * 3 + ["M" * 36])
    return b.done(True)


def _given_insertions():
    """insertion runs in slot 0, in slot clen, in both, and in an interior slot by several members with runs of
    different lengths -- each carried by a majority, so censoring and justification decide the bytes"""
    b = _Build(3003)
    cen = b.rand(35)
    L = len(cen)
    b.cluster(cen, ["GT" + cen] * 3 + [cen], cigars=["DD" + "M" * L] * 3 + ["M" * L])                    # slot 0
    b.cluster(cen, [cen + "CA"] * 3 + [cen], cigars=["M" * L + "DD"] * 3 + ["M" * L])                    # slot clen
    b.cluster(cen, ["G" + cen + "CA", "GT" + cen + "C", "G" + cen], cigars=["D" + "M" * L + "DD", "DD" + "M" * L + "D",
                                                                            "D" + "M" * L])               # both
    at = 17
    two = cen[:at] + "AC" + cen[at:]
    one = cen[:at] + "C" + cen[at:]
    ops2, ops1 = "M" * at + "DD" + "M" * (L - at), "M" * at + "D" + "M" * (L - at)
    b.cluster(cen, [two, two, one, one], cigars=[ops2, ops2, ops1, ops1])  # left-justified: A / C tie, then C loses
    b.cluster(cen, [two, two, two, cen[:at] + "A" + cen[at:]], cigars=[ops2, ops2, ops2, ops1])  # runs 2, 2, 2, 1
    three = cen[:at] + "TTG" + cen[at:]
    b.cluster(cen, [three, two, one, three, revcomp(three)], [0, 0, 0, 0, 1],
              cigars=["M" * at + "DDD" + "M" * (L - at), ops2, ops1, "M" * at + "DDD" + "M" * (L - at),
                      "M" * at + "DDD" + "M" * (L - at)])
    # an insertion just before the last centroid residue beside one after it
    b.cluster(cen, [cen[:-1] + "GG" + cen[-1], cen + "GG", cen + "GG"],
              cigars=["M" * (L - 1) + "DD" + "M", "M" * L + "DD", "M" * L + "DD"])
    return b.done(True)


def _given_iupac():
    """N, R, Y, U and lower-case residues in members and centroids"""
    b = _Build(3004)
    cen = b.rand(34, "ACG")  # no T: R and Y stand for A|G and C|T, so 'first base' differs from the centroid's often
    L = len(cen)
    sub = lambda s, x, ch: s[:x] + ch + s[x + 1:]  # noqa: E731
    b.cluster(cen, [sub(cen, 5, "N")] * 3, cigars=["M" * L] * 3)                          # N 3, one base 1: the base
    b.cluster(sub(cen, 5, "N"), [sub(cen, 5, "N")] * 2, cigars=["M" * L] * 2)             # only N: N
    b.cluster(sub(sub(cen, 7, "C"), 9, "G"), [sub(sub(cen, 7, "R"), 9, "Y")] * 2, cigars=["M" * L] * 2)
    b.cluster(cen.lower(), [sub(cen, 3, "u"), sub(cen, 3, "U"), sub(cen.lower(), 3, "t")], cigars=["M" * L] * 3)
    b.cluster(sub(cen, 11, "R"), [revcomp(sub(cen, 11, "Y")), revcomp(sub(cen, 11, "k"))], [1, 1], ["M" * L] * 2)
    b.cluster(cen, ["NR" + cen, "ny" + cen, "NN" + cen[:20] + "RYU" + cen[20:]],
              cigars=["DD" + "M" * L, "DD" + "M" * L, "DD" + "M" * 20 + "DDD" + "M" * (L - 20)])
    return b.done(True)


def _given_all_d_all_i():
    """members sharing no column with their centroid: all D then all I, and all I then all D"""
    b = _Build(3005)
    cen = b.rand(40)
    mem = b.rand(37)
    b.cluster(cen, [mem], cigars=["D" * 37 + "I" * 40])
    b.cluster(cen, [mem], cigars=["I" * 40 + "D" * 37])
    b.cluster(cen, [mem, revcomp(mem), cen], [0, 1, 0], ["D" * 37 + "I" * 40, "I" * 40 + "D" * 37, "M" * 40])
    b.cluster("G", ["A"], cigars=["DI"])
    b.cluster("G", ["A", "A"], cigars=["ID", "DI"])
    return b.done(True)


def _given_stride():
    """257 and 513 sequences with hand-built ops: the members past k_consensus's first 256-thread stride carry the
    majority, a substitution and an insertion the earlier members do not have"""
    b = _Build(3006)
    for size in (255, 256, 257, 513):
        cen = b.rand(33)
        x = 9
        var = cen[:x] + "ACGT"[("ACGT".index(cen[x]) + 1) % 4] + cen[x + 1:20] + "GA" + cen[20:]
        vops = "M" * 20 + "DD" + "M" * 13
        nvar = size // 2 + 1
        mem = [cen] * (size - 1 - nvar) + [var] * nvar
        b.cluster(cen, mem, cigars=["M" * 33] * (size - 1 - nvar) + [vops] * nvar)
    return b.done(True)


def _given_cons224():
    """the longest consensus there can be: two sequences of 112 sharing no column, none of it in an end slot"""
    b = _Build(3007)
    b.cluster(b.rand(112), [b.rand(112)], cigars=["I" + "D" * 112 + "I" * 111])
    return b.done(True)


def _wide(nd):
    """a 112-nt centroid; 17 members each inserting all their 112 residues in a slot of their own (slots 1 .. 17), one
    member inserting nd residues in slot 18, and 20 copies of the centroid: 112 + 17 * 112 + nd columns"""
    b = _Build(3008)
    cen = b.rand(112)
    mem = [b.rand(112) for _ in range(17)]
    ops = ["I" * (k + 1) + "D" * 112 + "I" * (111 - k) for k in range(17)]
    mem.append(b.rand(nd))
    ops.append("I" * 18 + "D" * nd + "I" * 94)
    b.cluster(cen, mem + [cen] * 20, cigars=ops + ["M" * 112] * 20)
    b.cluster(cen[:50], [cen[1:50]], cigars=["I" + "M" * 49])  # a plain cluster beside it
    return b.done(True)


GIVEN = {"disagree": _given_disagree, "best_vs_gaps": _given_best_vs_gaps, "insertions": _given_insertions,
         "iupac": _given_iupac, "all_d_all_i": _given_all_d_all_i, "stride": _given_stride,
         "cons224": _given_cons224, "msa2048": lambda: _wide(32), "msa2049": lambda: _wide(33)}


@functools.lru_cache(maxsize=None)
def case(name: str):
    return (TRACED.get(name) or GIVEN[name])()


def oriented(seqs, clusters, strands):
    """per cluster and member entry, the member as the aligner reads it ('' for the centroid's entry)"""
    return [[""] + [revcomp(seqs[r]) if st else seqs[r] for r, st in zip(m[1:], sts[1:])]
            for m, sts in zip(clusters, strands)]


@functools.lru_cache(maxsize=None)
def oracle_alignments(name: str, preset: int, boundary_open: int):
    """per cluster and member entry of the traced case, orc.align(oriented member, centroid) under the preset's scoring
    (None for the centroid's entry)"""
    seqs, clusters, strands, _ = case(name)
    p = orc.params(preset, 0.93, 1, MAX_LEN)
    p.policy_boundary_open = boundary_open
    return [[None] + [orc.align(p, q, seqs[m[0]]) for q in qs[1:]]
            for m, qs in zip(clusters, oriented(seqs, clusters, strands))]


def reference(seqs, clusters, strands, cigars, msa=msa_ref, **rules) -> list:
    """every cluster's consensus by msa (msa_ref with **rules, or pyref.msa)"""
    out = []
    for m, sts, cg in zip(clusters, strands, cigars):
        st = {r: s for r, s in zip(m, sts)}
        cig = {r: compress(expand(c)) for r, c in zip(m[1:], cg[1:])}
        out.append(msa(seqs, m, st, cig, **rules))
    return out


@functools.lru_cache(maxsize=None)
def expected(name: str, preset: int = 1, boundary_open: int = 1):
    """(cigars, consensus per cluster) of a case: its own ops, or the oracle aligner's under that scoring"""
    seqs, clusters, strands, cigars = case(name)
    if cigars is None:
        cigars = [[""] + [expand(a["cigar"]) for a in al[1:]] for al in oracle_alignments(name, preset, boundary_open)]
    return cigars, reference(seqs, clusters, strands, cigars)


def pyref_consensus(seqs, clusters, strands, cigars) -> list:
    return reference(seqs, clusters, strands, cigars, msa=pyref.msa)


def clusters_of(out: dict):
    """(clusters, strands) from what orc.cluster or Context.fetch returns per input record (cluster number, -1 for a
    filtered record; strand; centroid flag): the centroid first, the members in input order"""
    K = int(out["n_clusters"])
    clusters, strands = [[] for _ in range(K)], [[] for _ in range(K)]
    for i, (k, st, ce) in enumerate(zip(out["cluster"], out["strand"], out["centroid"])):
        if k < 0:
            continue
        if ce:
            clusters[k].insert(0, i)
            strands[k].insert(0, 0)
        else:
            clusters[k].append(i)
            strands[k].append(int(st))
    return clusters, strands
