"""Plain reference of one device pass after the prefilter -- the batch-of-8 walk (k_walk), the relevant and the
speculatively aligned in-window peers (k_peer_rel, k_peer_pairs) and what k_pack hands the host (HostQs, the
records, the pass counters) -- and the input families of tests/test_gpu_pass.py.  Pure Python / numpy: the lists come
from prefilter_ref.prefilter_ref, every alignment from the oracle (orc.align); no GPU.

The rules (vsearch searchcore.cc search_onequery / align_delayed as oracle/umiclust_oracle.c search_strand restates
them, and the pass description of DESIGN.md):
  result word  matches | internal_len << 8 | (score & 0xffff) << 16 of orc.align(query, target); strand 1 aligns
               pyref.revcomp of the query
  accept       100.0 * m / L >= 100.0 * id in IEEE double, with L > 0 and m <= L
  rank         dense rank of 100.0 * m / L over the whole table L in 0..224, m in 0..112 (id = 0 for L = 0)
  walk         candidates best first in batches of 8, stopping after the batch that holds an accept, after 32
               candidates or at the end of the list; best hit = highest rank, then smallest seqno; w = candidates
               walked; cells = sum of ql * len(t) over them
  e            results exist for candidates [0, e): the first launch emits min(nt, 32) if the top candidate's count
               is below 30, else min(nt, 8); after the first evaluation every walk still open emits up to min(nt, 32).
               S0 = the walk state after that first evaluation
  relevant     (final state) the walk's last batch is open -- w % 8 != 0, or w == 0, or no accept and w < 32 -- or the
               peer's key (count descending, length ascending, seqno ascending) sorts before the last walked
               candidate's
  aligned      (S0) relevant under S0, not expected to be a member (no strand of the peer has an accept in the peer's
               own S0 for an in-block peer, in its final state for a peer of the previous block when that block's
               pass was run first), peers not lazy, npeer neither 0 nor 255
  record       iff a finally-relevant peer: nt | np << 8, seqno[nt], res[nt] (0 from e on), counts packed 4 per
               word, peer[np] = id | count << 16 | rel << 24 | aligned << 25, peer_res[np] (0 if not aligned); nt is
               capped at 32
  counters     [8] aligned peers; [12..13] / [14..15] sums of ql * tl over the emitted walk pairs / the peer pairs
Sequences are given in vsearch's order (length non-increasing), so seqno = index.
"""
from __future__ import annotations

import functools

import numpy as np
import orc
import prefilter_ref as PR
from pyref import revcomp

TOP, PEER_CAP, BATCH, WALK, INLINE_REL, SPEC_THR = 41, 128, 8, 32, 6, 30
MAXL = 112
NONE = 0xffffffff


# ------------------------------------------------------------------------------------------ acceptance and rank
@functools.lru_cache(maxsize=None)
def tables(identity: float):
    """(accept[L, m], rank[L, m]) over L in 0..2 * 112, m in 0..112"""
    L = np.arange(2 * MAXL + 1, dtype=np.float64)[:, None]
    m = np.arange(MAXL + 1, dtype=np.float64)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        idv = np.where(L > 0, 100.0 * m / L, 0.0)
    acc = (L > 0) & (m <= L) & (idv >= 100.0 * identity)
    vals = np.unique(idv)  # sorted distinct values: the dense rank is the index
    rank = np.searchsorted(vals, idv)
    return acc, rank.astype(np.int64)


class Aligner:
    """The oracle's result words of a pool, cached by (query, strand, target)."""

    def __init__(self, pool: PR.Pool, preset: int = 1, identity: float = 0.93):
        self.pool, self.identity = pool, identity
        self.p = orc.params(preset, identity, int(pool.lens.min()), int(pool.lens.max()))
        self.cache: dict = {}
        self.masked = [orc.dust(s) for s in pool.seqs]  # the oracle aligns the masked sequences (case is ignored)
        self.acc, self.rank = tables(identity)

    def word(self, q: int, strand: int, t: int) -> int:
        k = (q, strand, t)
        w = self.cache.get(k)
        if w is None:
            qs = revcomp(self.masked[q]) if strand else self.masked[q]
            a = orc.align(self.p, qs, self.masked[t])
            w = a["matches"] | a["internal_len"] << 8 | (a["score"] & 0xffff) << 16
            self.cache[k] = w
        return w

    def judge(self, w: int) -> tuple[bool, int]:
        m, L = w & 0xff, (w >> 8) & 0xff
        return bool(self.acc[L, m]), int(self.rank[L, m])


# ------------------------------------------------------------------------------------------ the walk
def key(count: int, length: int, seqno: int) -> tuple:
    return (-int(count), int(length), int(seqno))


def pack_key(count: int, length: int, seqno: int) -> int:
    """WalkState.lastkey: the key as one integer (umiclust_pass_walk)"""
    return (127 - int(count)) << 56 | int(length) << 48 | int(seqno)


def walk_upto(accs, ranks, seqnos, nt: int, limit: int) -> dict:
    """The walk over a list of nt candidates batch by batch, as far as results exist: candidates [0, limit) (limit =
    min(nt, 32): the whole walk; limit = 8: the first evaluation of a list whose first launch emitted one batch)."""
    st = dict(w=0, acc=0, best_rank=0, best_t=NONE, done=1 if nt == 0 else 0)
    while not st["done"] and st["w"] < limit:
        b0, b1 = st["w"], min(nt, st["w"] + BATCH)
        for x in range(b0, b1):
            if accs[x]:
                if not st["acc"] or (ranks[x], -seqnos[x]) > (st["best_rank"], -st["best_t"]):
                    st["best_rank"], st["best_t"] = int(ranks[x]), int(seqnos[x])
                st["acc"] = 1
        st["w"] = b1
        if st["acc"] or b1 >= nt or b1 >= WALK:
            st["done"] = 1
    return st


def walk_brute(accs, seqnos_ranks) -> tuple:
    """(accept, best seqno, walked) without batches, as search_onequery counts: candidates are popped while fewer than
    32 are finalized or delayed and nothing is accepted, 8 at a time; every popped candidate is aligned."""
    nt = len(accs)
    finalized = accepts = rejects = pos = 0
    while True:
        delayed = 0
        while finalized + delayed < WALK and rejects < 32 and accepts < 1 and pos < nt and delayed < BATCH:
            pos += 1
            delayed += 1
        if delayed == 0:
            break
        for x in range(finalized, finalized + delayed):
            if accs[x]:
                accepts += 1
            else:
                rejects += 1
        finalized += delayed
    hits = [(-r, s) for a, (s, r) in zip(accs[:finalized], seqnos_ranks[:finalized]) if a]
    return (1, min(hits)[1], finalized) if hits else (0, NONE, finalized)


def is_open(st: dict) -> bool:
    return st["w"] % BATCH != 0 or st["w"] == 0 or (not st["acc"] and st["w"] < WALK)


def relevant(st: dict, last: tuple | None, peer_key: tuple) -> bool:
    return is_open(st) or peer_key < last


def block_walks(pool: PR.Pool, al: Aligner, lists: dict, q0: int, nq: int, both: int = 2) -> list[dict]:
    """Per query-strand: the final walk state (w, acc, best_rank, best_t, done, e, cells, last, lastkey), S0 under
    "s0" with its own "last", and the oracle's words of the candidates [0, e) under "res"."""
    out = []
    for qs in range(nq * both):
        q, strand = q0 + qs // both, qs % both
        nt = int(lists["ntop"][qs])
        seq = [int(x) for x in lists["top_seqno"][qs, :nt]]
        cnt = [int(x) for x in lists["top_count"][qs, :nt]]
        ntw = min(nt, WALK)
        spec = nt > 0 and cnt[0] < SPEC_THR
        e0 = min(nt, WALK if spec else BATCH)
        words = {x: al.word(q, strand, seq[x]) for x in range(e0)}
        j = [al.judge(words[x]) for x in range(e0)]
        s0 = walk_upto([a for a, _ in j], [r for _, r in j], seq[:e0], nt, e0)
        e = e0 if s0["done"] else ntw
        for x in range(e0, e):
            words[x] = al.word(q, strand, seq[x])
        j = [al.judge(words[x]) for x in range(e)]
        fin = walk_upto([a for a, _ in j], [r for _, r in j], seq[:e], nt, e)
        assert fin["done"] == 1
        ql = int(pool.lens[q])
        for st in (s0, fin):
            w = st["w"]
            st["last"] = key(cnt[w - 1], pool.lens[seq[w - 1]], seq[w - 1]) if w else None
            st["lastkey"] = pack_key(cnt[w - 1], pool.lens[seq[w - 1]], seq[w - 1]) if w else 0
            st["cells"] = sum(ql * int(pool.lens[t]) for t in seq[:w]) & 0xffffffff
        fin.update(e=e, s0=s0, res=[words[x] for x in range(e)], nt=nt, seq=seq, cnt=cnt,
                   emitted_cells=sum(ql * int(pool.lens[t]) for t in seq[:e]))
        out.append(fin)
    return out


# ------------------------------------------------------------------------------------------ the pass
def pass_ref(pool: PR.Pool, cent, q0: int, nq: int, nprev: int = 0, lazy: bool = False, prev: bool = False,
             identity: float = 0.93, al: Aligner | None = None, lists: dict | None = None) -> dict:
    """What umiclust_pass returns for the block [q0, q0 + nq): lists (prefilter_ref), per query-strand walks[qs]
    (block_walks), rel[qs] / aligned[qs] (bool per peer, list order), peer_res[qs] (words, 0 if not aligned),
    hostqs[qs] (dict of the HostQs fields but rec; has_rec), records[qs] (the record's words or None), masks[qs]
    (two 64-bit words) and counters {8, 12, 14}."""
    both = 2
    al = al or Aligner(pool, 1, identity)
    lists = lists or PR.prefilter_ref(pool, cent, q0, nq, nprev)
    w0 = q0 - nprev * nq
    walks = block_walks(pool, al, lists, q0, nq)
    acc_prev = None
    if prev:
        assert nprev >= 1
        pl = PR.prefilter_ref(pool, cent, q0 - nq, nq, nprev - 1)
        pw = block_walks(pool, al, pl, q0 - nq, nq)
        acc_prev = [any(pw[i * both + s]["acc"] for s in range(both)) for i in range(nq)]
    acc_s0 = [any(walks[i * both + s]["s0"]["acc"] for s in range(both)) for i in range(nq)]

    def expected(ps: int) -> bool:
        if q0 <= ps < q0 + nq:
            return acc_s0[ps - q0]
        if acc_prev is not None and q0 - nq <= ps < q0:
            return acc_prev[ps - (q0 - nq)]
        return False

    nqs = nq * both
    out = dict(lists=lists, walks=walks, rel=[], rel0=[], aligned=[], peer_res=[], hostqs=[], records=[], masks=[])
    n_al = cells_p = 0
    for qs in range(nqs):
        q, strand = q0 + qs // both, qs % both
        st = walks[qs]
        np_ = int(lists["npeer"][qs])
        ql = int(pool.lens[q])
        rel, rel0, alg, pres = [], [], [], []
        if np_ != 255:
            ids, cnts = lists["peers"][qs]
            for i, c in zip(ids.tolist(), cnts.tolist()):
                ps = w0 + i
                k = key(c, pool.lens[ps], ps)
                r = relevant(st, st["last"], k)
                r0 = relevant(st["s0"], st["s0"]["last"], k)
                a = r0 and not expected(ps) and not lazy and np_ != 0
                rel.append(r)
                rel0.append(r0)
                alg.append(a)
                pres.append(al.word(q, strand, ps) if a else 0)
                if a:
                    n_al += 1
                    cells_p += ql * int(pool.lens[ps])
        nrel = sum(rel)
        relids = [int(i) for i, r in zip(lists["peers"][qs][0], rel) if r][:INLINE_REL] if np_ != 255 else []
        hq = dict(best_t=st["best_t"], cells=st["cells"], best_rank=st["best_rank"], w=st["w"],
                  flags=(1 if st["acc"] else 0) | (2 if np_ == 255 else 0), nrel=nrel, e=st["e"], npeer=np_,
                  rel=relids + [0] * (INLINE_REL - len(relids)), has_rec=nrel > 0)
        rec = None
        if nrel > 0:
            nt = min(st["nt"], WALK)
            ids, cnts = lists["peers"][qs]
            rec = [nt | np_ << 8] + st["seq"][:nt] + [st["res"][x] if x < st["e"] else 0 for x in range(nt)]
            cw = [0] * ((nt + 3) // 4)
            for x in range(nt):
                cw[x // 4] |= st["cnt"][x] << (8 * (x % 4))
            rec += cw
            rec += [int(i) | int(c) << 16 | (1 << 24 if r else 0) | (1 << 25 if a else 0)
                    for i, c, r, a in zip(ids, cnts, rel, alg)]
            rec += pres
        mask = [0, 0]
        for y, a in enumerate(alg):
            if a:
                mask[y // 64] |= 1 << (y % 64)
        out["rel"].append(rel)
        out["rel0"].append(rel0)
        out["aligned"].append(alg)
        out["peer_res"].append(pres)
        out["hostqs"].append(hq)
        out["records"].append(rec)
        out["masks"].append(mask)
    out["counters"] = {8: n_al, 12: sum(w["emitted_cells"] for w in walks), 14: cells_p}
    out["total"] = sum(len(r) for r in out["records"] if r is not None)
    return out


def single_peer_failures(pool: PR.Pool, al: Aligner, ref: dict, q0: int, nq: int, nprev: int) -> list[str]:
    """The independent check of the relevance rule: for every query-strand and every single peer, the peer is
    inserted into the candidate order as if it were a centroid, with the oracle's alignment of the pair, and the list
    re-walked (walk_brute).  A peer whose insertion changes the outcome (accept, best hit, number walked) must be in
    the reference's relevant set.  Returns the violations."""
    both, w0, bad = 2, q0 - nprev * nq, []
    lists = ref["lists"]
    for qs in range(nq * both):
        if int(lists["npeer"][qs]) in (0, 255):
            continue
        q, strand = q0 + qs // both, qs % both
        nt = int(lists["ntop"][qs])
        cand = [(key(lists["top_count"][qs, x], pool.lens[lists["top_seqno"][qs, x]], lists["top_seqno"][qs, x]),
                 int(lists["top_seqno"][qs, x])) for x in range(nt)]
        judged: dict = {}

        def outcome(cs):
            cs = cs[:TOP]
            accs, sr = [], []
            for x, (_, t) in enumerate(cs):
                if x >= WALK:
                    break
                if t not in judged:
                    judged[t] = al.judge(al.word(q, strand, t))
                accs.append(judged[t][0])
                sr.append((t, judged[t][1]))
            return walk_brute(accs, sr)
        base = outcome(cand)
        ids, cnts = lists["peers"][qs]
        for y, (i, c) in enumerate(zip(ids.tolist(), cnts.tolist())):
            ps = w0 + i
            k = key(c, pool.lens[ps], ps)
            if outcome(sorted(cand + [(k, ps)])) != base and not ref["rel"][qs][y]:
                bad.append(f"query-strand {qs}: peer {ps} (count {c}) changes the walk but is not relevant")
    return bad


# ---------------------------------------------------------------------------------------------- input families
_P1 = None


def _params():
    global _P1
    if _P1 is None:
        _P1 = orc.params(1, 0.93, 32, 112)
    return _P1


def rand_seq(rng, n: int) -> str:
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def subst(rng, s: str, positions) -> str:
    b = list(s)
    for p in positions:
        b[p] = "ACGT"[("ACGT".index(b[p]) + 1 + int(rng.integers(0, 3))) % 4]
    return "".join(b)


def pad(rng, s: str, length: int) -> str:
    return s + rand_seq(rng, length - len(s))


def accepts(q: str, t: str, identity: float = 0.93) -> bool:
    a = orc.align(_params(), q, t)
    return a["internal_len"] > 0 and 100.0 * a["matches"] / a["internal_len"] >= 100.0 * identity


def count(q: str, t: str) -> int:
    return len(set(PR.kmer_set(q)) & set(PR.kmer_set(t)))


def decoy(rng, base: str, lo: int = 40, hi: int = 57, blocks: int = 1) -> str:
    """5..6 adjacent substitutions (per block), padded to 64..68 (or left at the base's length when longer); kept only
    if the oracle rejects it against the base and its k-mer count is in lo..hi"""
    for _ in range(400):
        s = base
        for b in range(blocks):
            k = int(rng.integers(5, 7))
            seg = len(base) // blocks
            p = b * seg + int(rng.integers(8, seg - 8 - k))
            s = subst(rng, s, range(p, p + k))
        s = pad(rng, s, max(len(base), int(rng.integers(64, 69))))
        if not accepts(base, s) and lo <= count(base, s) <= hi:
            return s
    raise RuntimeError("no decoy")


def hit(rng, base: str, nsub: int, length: int, lo: int = 12, hi: int = 38) -> str:
    """nsub substitutions 16 nt apart, padded to `length`; kept only if the oracle accepts it and its count is in
    lo..hi"""
    for _ in range(400):
        p0 = int(rng.integers(4, 12))
        s = pad(rng, subst(rng, base, [p0 + 16 * i for i in range(nsub)]), max(length, len(base)))
        if accepts(base, s) and lo <= count(base, s) <= hi:
            return s
    raise RuntimeError("no hit")


def weak(rng, base: str, lo: int, hi: int, nsub: int = 5) -> str:
    """nsub substitutions at random places, accepted or not; kept if its count is in lo..hi"""
    for _ in range(2000):
        pos = sorted(rng.choice(len(base), nsub, replace=False).tolist())
        s = pad(rng, subst(rng, base, pos), max(len(base), int(rng.integers(64, 69))))
        if lo <= count(base, s) <= hi:
            return s
    raise RuntimeError("no weak candidate")


def variant(rng, base: str, nsub: int, minus: bool = False) -> str:
    """a query of the base's family: nsub substitutions at random places"""
    s = subst(rng, base, sorted(rng.choice(len(base), nsub, replace=False).tolist())) if nsub else base
    return revcomp(s) if minus else s


class Family:
    """One base UMI: its centroids (decoys first in every list of the base, then hits, then weak candidates) and the
    base itself, the pivot query the D of the family holds for exactly."""

    def __init__(self, rng, D: int = 0, hits=(), nweak: int = 0, weak_range=(12, 24), length: int = 64,
                 decoy_blocks: int = 1, hit_range=(25, 38), decoy_lo: int | None = None):
        self.rng = rng
        self.base = rand_seq(rng, length)
        lo = hit_range[1] + 2 if decoy_lo is None else decoy_lo
        self.cents = [decoy(rng, self.base, lo=lo, hi=length - 7, blocks=decoy_blocks) for _ in range(D)]
        self.cents += [hit(rng, self.base, ns, ln, *hit_range) for ns, ln in hits]
        self.cents += [weak(rng, self.base, *weak_range) for _ in range(nweak)]

    def q(self, nsub: int = 0, minus: bool = False) -> str:
        return variant(self.rng, self.base, nsub, minus)


def assemble(cents: list[str], window: list[str]) -> tuple[PR.Pool, np.ndarray]:
    """centroids (sorted longest first, stably) in front of the window's queries (given in order, lengths
    non-increasing and none longer than the shortest centroid)"""
    cents = sorted(cents, key=lambda s: -len(s))
    assert not cents or not window or len(cents[-1]) >= len(window[0])
    return PR.Pool(cents + window), np.arange(len(cents), dtype=np.int64)


def fill(rng, slots: list, length: int = 64) -> list[str]:
    """unrelated random queries in the free slots: no candidate, no peer"""
    return [s if s is not None else rand_seq(rng, length) for s in slots]


def _walk_case(seed: int = 501):
    """nq = 129, no earlier block.  One family per D (0, 7, 8, 15, 16, 31, 32 with 41 candidates), per list length
    (1, 7, 8, 9, 32; the unrelated fillers have none) and per top count (29, 30), each with its pivot, light and
    heavy variants of it (peers with high and low counts) and a reverse-complemented pivot in the block."""
    rng = np.random.default_rng(seed)
    fams = {f"D{d}": Family(rng, d, [(3, 64), (3, 66)] if d % 2 else [(3, 65), (4, 64)]) for d in (0, 7, 8, 15, 16, 31)}
    fams["D32"] = Family(rng, 32, [(3, 64)] * 9)
    fams["n1"] = Family(rng, 0, [(3, 66)])
    fams["n7"] = Family(rng, 5, [(3, 64), (4, 66)])
    fams["n8"] = Family(rng, 6, [(3, 64), (3, 64)])
    fams["n9"] = Family(rng, 7, [(4, 64), (3, 65)])
    fams["n32"] = Family(rng, 30, [(3, 64), (3, 67)])
    fams["top29"] = Family(rng, 0, [], nweak=12, weak_range=(14, 28))
    fams["top29"].cents[0] = weak(rng, fams["top29"].base, 29, 29, 4)
    fams["top30"] = Family(rng, 0, [], nweak=12, weak_range=(14, 28))
    fams["top30"].cents[0] = weak(rng, fams["top30"].base, 30, 30, 4)
    window = []
    names = list(fams)
    for f in fams.values():  # 8 queries per family: heavy and light variants first, the pivots last
        window += [f.q(4), f.q(1), f.q(3), f.q(2), f.q(0), f.q(5), f.q(0, True), f.q(0)]
    window = window[:129] + [None] * max(0, 129 - len(window))
    window = fill(rng, window)
    pool, cent = assemble([c for f in fams.values() for c in f.cents], window)
    pivots = {n: len(cent) + 8 * i + 7 for i, n in enumerate(names) if 8 * i + 7 < 129}
    return dict(pool=pool, cent=cent, q0=len(cent), nq=129, nprev=0, pivots=pivots)


def _crowd_case(seed: int = 502):
    """nq = 129 with one earlier block.  `late`: a closed walk (7 decoys, then the hit) whose pivot sits last in the
    block behind 70 heavy variants (counts below the hit's) in parts 0..6 and 3 light ones (counts above it) in part
    7: its only relevant peers have list positions >= 64.  `big`: 150 queries of one family with an open walk (5
    candidates): peer lists of 65..128 entries, overflows past that, every peer relevant.  `mid`: a family accepting
    at the end of its second batch (a closed walk that was open after the first evaluation), spread over both blocks."""
    rng = np.random.default_rng(seed)
    nq = 129
    late = Family(rng, 7, [(3, 64)], hit_range=(30, 36))
    big = Family(rng, 3, [(3, 64), (4, 66)])
    mid = Family(rng, 15, [(3, 64), (3, 66)])
    slots: list = [None] * (2 * nq)
    hc = count(late.base, late.cents[-1])
    lows, highs = [], []
    while len(lows) < 70:
        v = late.q(4)
        if 12 <= count(late.base, v) < hc - 1:
            lows.append(v)
    while len(highs) < 3:
        v = late.q(1)
        if count(late.base, v) > hc + 1:
            highs.append(v)
    # parts are ((x - w0) % nq) % 8: the block's positions nq + 0 .. nq + 127
    lowpos = [nq + i for i in range(128) if i % 8 < 7][:70]
    highpos = [nq + i for i in range(128) if i % 8 == 7][:3]
    for p, s in zip(lowpos + highpos, lows + highs):
        slots[p] = s
    slots[2 * nq - 1] = late.base
    free = [i for i in range(2 * nq) if slots[i] is None]
    for n, i in enumerate(free[:150]):
        slots[i] = big.q(int(rng.integers(0, 4)), minus=(n % 11 == 5))
    for n, i in enumerate(free[150:170]):
        slots[i] = mid.q(0 if n % 3 == 0 else int(rng.integers(1, 5)))
    pool, cent = assemble(late.cents + big.cents + mid.cents, fill(rng, slots))
    return dict(pool=pool, cent=cent, q0=len(cent) + nq, nq=nq, nprev=1, pivots=dict(late=len(cent) + 2 * nq - 1))


def _small_case(seed: int, nq: int, lens3: bool):
    """Two earlier blocks and the block under test, nq queries each, of three families (accept in the first batch,
    accept in the second, no accept) present in every block: peers of the block itself, of the previous block and of
    two blocks back.  lens3: the last block holds three query lengths (64, 63, 62)."""
    rng = np.random.default_rng(seed)
    fams = [Family(rng, 2, [(3, 64), (4, 65)]), Family(rng, 9, [(3, 64)]), Family(rng, 11, [])]
    window = []
    for b in range(3):
        for i in range(nq):
            f = fams[(i + b) % 3] if nq > 1 else fams[0]
            s = f.q(int(rng.integers(0, 3)) if i % 4 else 0)
            if lens3 and b == 2:
                s = s[:64 - (3 * i) // nq]
            window.append(s)
    pool, cent = assemble([c for f in fams for c in f.cents], window)
    return dict(pool=pool, cent=cent, q0=len(cent) + 2 * nq, nq=nq, nprev=2, pivots={})


def _len32_case(seed: int = 505):
    """One block of 32 queries of 32 distinct lengths, 112 down to 81 (kSegLens): every pair segment meets in one
    wave of k_walk.  Three families of 112-mers (centroids of length 112), the queries truncated copies."""
    rng = np.random.default_rng(seed)
    kw = dict(length=112, decoy_blocks=2, hit_range=(60, 90), decoy_lo=60)
    fams = [Family(rng, 3, [(3, 112), (4, 112)], **kw), Family(rng, 9, [(4, 112)], **kw), Family(rng, 2, [], **kw)]
    window = [fams[i % 3].q(int(rng.integers(0, 3)), minus=(i % 7 == 3))[:112 - i] for i in range(32)]
    pool, cent = assemble([c for f in fams for c in f.cents], window)
    return dict(pool=pool, cent=cent, q0=len(cent), nq=32, nprev=0, pivots={})


def _ambig_case(seed: int = 506):
    """The small three-block layout with an N in a third of the sequences: the pass runs the ambiguity aligner."""
    c = _small_case(seed, 9, False)
    rng = np.random.default_rng(seed + 1)
    seqs = list(c["pool"].seqs)
    for i in range(0, len(seqs), 3):
        p = int(rng.integers(0, len(seqs[i])))
        seqs[i] = seqs[i][:p] + "N" + seqs[i][p + 1:]
    c["pool"] = PR.Pool(seqs)
    return c


# name -> (builder, lazy, prev): the pass flags of the case
CASES = {
    "walk129": (_walk_case, False, False),
    "crowd129": (_crowd_case, False, True),
    "crowd129_noprev": (_crowd_case, False, False),
    "crowd129_lazy": (_crowd_case, True, True),
    "tri9x2": (lambda: _small_case(503, 9, True), False, True),
    "one1x2": (lambda: _small_case(504, 1, False), False, True),
    "len32": (_len32_case, False, False),
    "ambig9x2": (_ambig_case, False, True),
}


@functools.lru_cache(maxsize=None)
def _built(builder):
    c = builder()
    c["al"] = Aligner(c["pool"])
    c["lists"] = PR.prefilter_ref(c["pool"], c["cent"], c["q0"], c["nq"], c["nprev"])
    return c


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """A case's inputs and its reference (computed once per process, shared by the tests; read-only).  Cases built by
    the same builder share the pool, the lists and the alignment cache."""
    builder, lazy, prev = CASES[name]
    b = _built(builder)
    ref = pass_ref(b["pool"], b["cent"], b["q0"], b["nq"], b["nprev"], lazy, prev, al=b["al"], lists=b["lists"])
    return dict(b, lazy=lazy, prev=prev, ref=ref)
