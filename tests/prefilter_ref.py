"""Plain reference of the k-mer prefilter (k_pf_count / k_pf_full / k_pf_merge) and the input families of
tests/test_gpu_prefilter.py.  Pure Python / numpy on top of the oracle's DUST and 8-mer extraction; no GPU and
nothing of umiclust_prep's output.

The rule (oracle/umiclust_oracle.c search_strand, vsearch searchcore.cc):
  K(s)      = set(orc.unique_kmers(orc.dust(s), 8, True)); the minus strand of a query is pyref.revcomp of the
              masked sequence
  thr       = min(minwordmatches, |K(q, strand)|)
  top list  = the centroids c with |K(q, strand) & K+(c)| >= thr (all of them when thr == 0), ordered by count
              descending, length ascending, seqno ascending; the first 41
  peers     = the window seqnos x in [w0, q) with |K(q, strand) & K+(x)| >= thr; more than 128: overflow (255);
              listed grouped by part ((x - first seqno of x's block) % 8, the blocks being the window's nq-query
              blocks from w0), the parts in order, within a part by count descending, length ascending, window id
              (x - w0) ascending -- the order stated above k_pf_merge.
Sequences are given in vsearch's order (length non-increasing), so seqno = index.
"""
from __future__ import annotations

import functools

import numpy as np
import orc
from pyref import revcomp

TOP = 41        # kTopHits
PEER_CAP = 128  # kPeerCap
PARTS = 8       # kParts
PART_CAND = 64  # kPartCand: more candidates in one part hand the unit to k_pf_full
RANK_SEL = 512  # kRankSel: k_pf_full selects by rank up to this many candidates of a part, by bitonic sort above
PF_CAND = 1024  # kPfCand: more candidates in a part switch k_pf_full to its chunked scan
PAD = 65536     # k-mer matrix padding (8-mer codes are < 65536)


def kmer_set(seq: str, minus: bool = False) -> list[int]:
    m = orc.dust(seq)
    return sorted(set(orc.unique_kmers(revcomp(m) if minus else m, 8, True)))


class Pool:
    """Sequences in vsearch's order with their plus-strand k-mer sets as a padded matrix."""

    def __init__(self, seqs: list[str]):
        lens = [len(s) for s in seqs]
        assert all(a >= b for a, b in zip(lens, lens[1:])), "sequences must be sorted by length, longest first"
        self.seqs = seqs
        self.lens = np.array(lens, np.int32)
        sets = [kmer_set(s) for s in seqs]
        w = max([len(k) for k in sets] + [1])
        self.kp = np.full((len(seqs), w), PAD, np.int32)
        for i, k in enumerate(sets):
            self.kp[i, :len(k)] = k
        self.nk = np.array([len(k) for k in sets], np.int32)

    def __len__(self):
        return len(self.seqs)

    def query_kmers(self, q: int, strand: int) -> np.ndarray:
        if strand == 0:
            return self.kp[q, :self.nk[q]]
        return np.array(kmer_set(self.seqs[q], True), np.int32)

    def counts(self, qk: np.ndarray, rows: np.ndarray) -> np.ndarray:
        """|qk & K+(x)| for every x of rows"""
        mark = np.zeros(PAD + 1, np.int32)
        mark[qk] = 1
        return mark[self.kp[rows]].sum(axis=1)


def prefilter_ref(pool: Pool, cent, q0: int, nq: int, nprev: int = 0, both: int = 2, minwordmatches: int = 12) -> dict:
    """What umiclust_prefilter returns for the block [q0, q0 + nq) against the centroids `cent` (increasing seqnos)
    and the peer window [q0 - nprev * nq, q0 + nq), per query-strand qs = (q - q0) * both + strand:
      ntop[qs], top_seqno[qs, :ntop], top_count[qs, :ntop]; npeer[qs] (255 = overflow), peers[qs] = (ids, counts)
      in the expected order (None on overflow);
    and what the path assertions need: nk[qs], thr[qs], ncand[qs] (candidates before the cut at 41),
    part_max[qs] (most candidates in one part, part = centroid ordinal % 8), npeer_all[qs] (before the cap),
    units[qs] (the parts k_pf_count hands to k_pf_full: those with more than 64 candidates, all 8 when thr == 0)."""
    cent = np.asarray(cent, np.int64)
    w0 = q0 - nprev * nq
    assert nprev in (0, 1, 2) and w0 >= 0 and q0 + nq <= len(pool)
    assert len(cent) == 0 or (np.all(np.diff(cent) > 0) and cent[-1] < w0 and cent[0] >= 0)
    nqs = nq * both
    out = dict(ntop=np.zeros(nqs, np.int32), top_seqno=np.zeros((nqs, TOP), np.int64),
               top_count=np.zeros((nqs, TOP), np.int32), npeer=np.zeros(nqs, np.int32), peers=[None] * nqs,
               nk=np.zeros(nqs, np.int32), thr=np.zeros(nqs, np.int32), ncand=np.zeros(nqs, np.int32),
               part_max=np.zeros(nqs, np.int32), npeer_all=np.zeros(nqs, np.int32), units=np.zeros(nqs, np.int32))
    clen = pool.lens[cent]
    for qi in range(nq):
        q = q0 + qi
        win = np.arange(w0, q, dtype=np.int64)
        part = ((win - w0) % nq) % PARTS
        for strand in range(both):
            qs = qi * both + strand
            qk = pool.query_kmers(q, strand)
            thr = min(minwordmatches, len(qk))
            out["nk"][qs], out["thr"][qs] = len(qk), thr
            cnt = pool.counts(qk, cent) if len(cent) else np.zeros(0, np.int32)
            ok = np.nonzero(cnt >= thr)[0]
            out["ncand"][qs] = len(ok)
            per_part = np.bincount(ok % PARTS, minlength=PARTS)
            out["part_max"][qs] = per_part.max()
            out["units"][qs] = PARTS if thr == 0 else int((per_part > PART_CAND).sum())
            order = ok[np.lexsort((cent[ok], clen[ok], -cnt[ok]))][:TOP]
            out["ntop"][qs] = len(order)
            out["top_seqno"][qs, :len(order)] = cent[order]
            out["top_count"][qs, :len(order)] = cnt[order]
            pc = pool.counts(qk, win) if len(win) else np.zeros(0, np.int32)
            pk = np.nonzero(pc >= thr)[0]
            out["npeer_all"][qs] = len(pk)
            if len(pk) > PEER_CAP:
                out["npeer"][qs] = 255
            else:
                po = pk[np.lexsort((pk, pool.lens[win[pk]], -pc[pk], part[pk]))]
                out["npeer"][qs] = len(po)
                out["peers"][qs] = (po.astype(np.int64), pc[po].astype(np.int32))
    return out


def prefilter_brute(seqs: list[str], cent, q0: int, nq: int, nprev: int = 0, both: int = 2,
                    minwordmatches: int = 12) -> dict:
    """The same lists by plain set intersections (the vectorised reference's own check; small inputs only)."""
    kp = [set(kmer_set(s)) for s in seqs]
    w0 = q0 - nprev * nq
    ntop, tops, npeer, peers = [], [], [], []
    for q in range(q0, q0 + nq):
        for strand in range(both):
            kq = kp[q] if strand == 0 else set(kmer_set(seqs[q], True))
            thr = min(minwordmatches, len(kq))
            cand = [(-len(kq & kp[c]), len(seqs[c]), c) for c in cent if len(kq & kp[c]) >= thr]
            cand.sort()
            cand = cand[:TOP]
            ntop.append(len(cand))
            tops.append([(c, -n) for n, _, c in cand])
            pe = [(((x - w0) % nq) % PARTS, -len(kq & kp[x]), len(seqs[x]), x - w0) for x in range(w0, q)
                  if len(kq & kp[x]) >= thr]
            pe.sort()
            npeer.append(255 if len(pe) > PEER_CAP else len(pe))
            peers.append(None if len(pe) > PEER_CAP else [(i, -n) for _, n, _, i in pe])
    return dict(ntop=ntop, tops=tops, npeer=npeer, peers=peers)


# ---------------------------------------------------------------------------------------------- input families

_ACGT = np.frombuffer(b"ACGT", np.uint8)


def _by_length(seqs: list[str]) -> list[str]:
    return sorted(seqs, key=lambda s: -len(s))  # stable: vsearch's order for equal lengths is input order


def master48() -> str:
    return "".join("ACGT"[i] for i in np.random.default_rng(20240607).integers(0, 4, 48))


def shared_core(n: int, seed: int, min_core: int = 15, short_zones=()) -> list[str]:
    """n sequences of length 58..68, longest first; sequence i holds master48()[:c_i] at a random offset between
    random flanks, c_i uniform in min_core..40.  Two of them share about min(c) - 7 8-mers, so cores under 19 nt fall
    just below the threshold of 12 and everything else is a mutual candidate with heavily tied counts.  Positions
    inside one of short_zones ([lo, hi) pairs of sorted positions) draw c from 15..40 whatever min_core is: the
    query blocks of a pool whose centroids all hit each other."""
    rng = np.random.default_rng(seed)
    m = np.frombuffer(master48().encode(), np.uint8)
    lens = np.sort(rng.integers(58, 69, n))[::-1]
    core = rng.integers(min_core, 41, n)
    wide = rng.integers(15, 41, n)
    for lo, hi in short_zones:
        core[lo:hi] = wide[lo:hi]
    offs = (rng.random(n) * (lens - core + 1)).astype(np.int64)
    body = _ACGT[rng.integers(0, 4, (n, 68))]
    cols = np.arange(68)[None, :]
    inside = (cols >= offs[:, None]) & (cols < (offs + core)[:, None])
    body = np.where(inside, m[np.clip(cols - offs[:, None], 0, 47)], body)
    return [body[i, :lens[i]].tobytes().decode() for i in range(n)]


LOW_SPECIALS = ["AC" * 32, "A" * 60, "ACG" * 21, "ACGTTGCA" * 8, "N" * 60, "A" * 64, "N" * 64, "ACG" * 21, "AC" * 32]


def low_complexity(seed: int, n: int = 140, ntails: int = 5) -> list[str]:
    """"AC" * r (r in 20..26) + a random tail to length 64 (DUST leaves 1..17 unmasked 8-mers: thr = nk < 12 and
    thr = 12 both occur), the tails shared within a group so that its members hit each other, then LOW_SPECIALS
    (no unmasked 8-mer at all: thr = 0)."""
    rng = np.random.default_rng(seed)
    tails = ["".join("ACGT"[i] for i in rng.integers(0, 4, 24)) for _ in range(ntails)]
    out = []
    for i in range(n):
        r = int(rng.integers(20, 27))
        out.append("AC" * r + tails[i % ntails][:64 - 2 * r])
    return out + LOW_SPECIALS


def low_mix(seed: int = 7) -> list[str]:
    """700 shared-core sequences and the low-complexity set, shuffled and put in vsearch's order; the specials of
    length 63 come first among their length and the others last among theirs (low_case cuts its query block there)."""
    rng = np.random.default_rng(seed)
    a = shared_core(700, seed + 1) + low_complexity(seed + 2)[:-len(LOW_SPECIALS)]
    a = [a[i] for i in rng.permutation(len(a))]
    first = [s for s in LOW_SPECIALS if len(s) == 63]
    return _by_length(first + a + [s for s in LOW_SPECIALS if len(s) != 63])


def max_counts(seed: int = 11) -> list[str]:
    """Identical random 112-mers, their reverse complements and 1-substitution copies (count 105 = every 8-mer of a
    112-mer, the top of the u8 / 127 - count key range, and minus-strand hits): 110 of length 112, then 50 truncated
    copies of lengths 111..84 (a greedy block spans at most 32 lengths, so not down to 80)."""
    rng = np.random.default_rng(seed)
    base = "".join("ACGT"[i] for i in rng.integers(0, 4, 112))

    def variant(s):
        v = int(rng.integers(0, 4))
        if v >= 2:  # one substitution
            p = int(rng.integers(0, len(s)))
            s = s[:p] + "ACGT"[("ACGT".index(s[p]) + 1 + int(rng.integers(0, 3))) % 4] + s[p + 1:]
        return revcomp(s) if v % 2 else s
    out = [variant(base) for _ in range(110)]
    for i in range(50):
        L = 111 - (i * 28) // 50
        o = int(rng.integers(0, 112 - L + 1))
        out.append(variant(base[o:o + L]))
    return _by_length(out)


def control() -> list[str]:
    from umiclust import synth
    return _by_length([s for s in synth.make_umis(200, seed=31).as_list() if 58 <= len(s) <= 68])


BIG_N = 66064       # 66,000 centroids + the 64 queries at the tail
MID_Q0 = 36163      # the other cases' query block: 32 queries of length 63, then 32 of length 62


def spread(ncent: int, below: int) -> np.ndarray:
    """ncent increasing seqnos spread evenly over [0, below)"""
    assert ncent <= below
    return (np.arange(ncent, dtype=np.int64) * below) // max(ncent, 1)


@functools.lru_cache(maxsize=None)
def pool(name: str) -> Pool:
    """The pools the cases share (built once per process)."""
    if name == "core":      # every core >= 19 (all mutual candidates) but the query zones' (15..40)
        return Pool(shared_core(BIG_N, 101, 19, ((MID_Q0, MID_Q0 + 64), (BIG_N - 64, BIG_N))))
    if name == "peers":     # 50 centroids + 200 window queries, every core >= 19
        return Pool(shared_core(250, 103, 19))
    if name == "low":
        return Pool(low_mix())
    if name == "max":
        return Pool(max_counts())
    if name == "control":
        return Pool(control())
    raise KeyError(name)


def low_case(p: Pool) -> tuple[np.ndarray, int]:
    """(300 centroids: 200 shared-core + 100 low-complexity, q0) of the low-complexity case: the 64 queries are the
    last 56 of length 64 (the specials among them) and the first 8 of length 63 (the "ACG" repeats among them)."""
    q0 = int(np.nonzero(p.lens >= 64)[0][-1]) + 1 - 56
    low = np.array([s.startswith("ACACACAC") for s in p.seqs[:q0]])
    a, b = np.nonzero(~low)[0], np.nonzero(low)[0]
    assert len(a) >= 200 and len(b) >= 100
    return np.sort(np.concatenate([a[spread(200, len(a))], b[spread(100, len(b))]])), q0


# ---------------------------------------------------------------------------------------------- the cases
ALL = 1 << 30  # append_step: every centroid in one append

# name -> (pool, centroids, q0, nq, nprev, append_step); centroids: a count (spread evenly below the window) or a
# callable of the pool
CASES = {
    "tiny0": ("core", 0, MID_Q0, 64, 0, ALL),
    "tiny1": ("core", 1, MID_Q0, 64, 0, ALL),
    "tiny7": ("core", 7, MID_Q0, 64, 0, ALL),
    "tiny8": ("core", 8, MID_Q0, 64, 0, ALL),
    "tiny9": ("core", 9, MID_Q0, 64, 0, ALL),
    "cap512": ("core", 512, MID_Q0, 64, 0, ALL),
    "cap516": ("core", 516, MID_Q0, 64, 0, ALL),  # parts 0..3 hold 65 centroids, parts 4..7 hold 64
    "cap520": ("core", 520, MID_Q0, 64, 0, ALL),
    "rank4096": ("core", 4096, MID_Q0, 64, 0, ALL),
    "bitonic4200": ("core", 4200, MID_Q0, 64, 0, ALL),
    "scan9000": ("core", 9000, MID_Q0, 64, 0, ALL),
    "lsm20000_step3000": ("core", 20000, MID_Q0, 64, 0, 3000),
    "lsm20000": ("core", 20000, MID_Q0, 64, 0, ALL),
    "sealed66000": ("core", 66000, BIG_N - 64, 64, 0, ALL),
    "low": ("low", None, None, 64, 0, 100),
    "max": ("max", 64, 96, 64, 0, ALL),
    "control": ("control", 1000, 1000, 64, 0, 256),
    "peers60x2": ("peers", 50, 170, 60, 2, ALL),
    "peers90x1": ("peers", 50, 140, 90, 1, ALL),
    "peers200": ("peers", 50, 50, 200, 0, ALL),
}


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """A case's inputs and its reference lists (computed once per process, shared by the tests; read-only)."""
    pname, ncent, q0, nq, nprev, step = CASES[name]
    p = pool(pname)
    if pname == "low":
        cent, q0 = low_case(p)
    else:
        cent = spread(ncent, q0 - nprev * nq)
    return dict(pool=p, cent=cent, q0=q0, nq=nq, nprev=nprev, step=step, ref=prefilter_ref(p, cent, q0, nq, nprev))
