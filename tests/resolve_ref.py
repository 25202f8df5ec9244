"""Plain reference of the host's resolve step (csrc/resolve.cpp resolve_block, csrc/pass.cpp resolve_pass / round_b)
and the input worlds of tests/test_resolve_cpu.py and tests/test_gpu_resolve.py.  Pure Python; no GPU.

greedy_block restates what the resolve step has to compute, from the rule alone: it reads no HostQs and no record.
For every query of the block in sorted order and every strand

  candidates  every member of `cent`, plus every window entry before the query whose state is centroid, with
              count >= thr; ordered by (count descending, length ascending, seqno ascending), cut at 41
  walk        batches of 8; stops after the batch that holds an accept, after 32 candidates or at the list's end
  best hit    highest rank, then smallest seqno; the plus strand wins a tie between the strands

which is pyref.cluster's inner loop over a given centroid set.  With o4_T > 0 it restates cluster_core_parallel as
oracle/umiclust_oracle.c does: rounds of o4_T queries counted from the first sorted seqno of the query's own bin;
the search sees the centroids that existed before the round; the round's new centroids with count >= thr are then
inserted into the whole hit list by key (unaligned), the list is walked again from the top one hit at a time -- a
hit without a result is aligned -- until maxaccepts accepts, maxrejects rejects or its end, and the best hit is the
best accepted one among all aligned hits.

Two kinds of world feed it.  The real one: the pools of pass_ref.CASES with the oracle Aligner.  The abstract one
(World): lengths, per-(query, strand, target) counts, thresholds and result words come from a seeded hash or are
scripted entry by entry; World.lists() builds the prefilter's lists under the device's ordering and
pass_ref.pass_ref turns them, with World.aligner(), into HostQs and records under the device's contract.  No
sequence exists and no alignment is computed, so thousands of blocks cost seconds.
"""
from __future__ import annotations

import types

import numpy as np
import pass_ref as R

UNDET, CENT, MEMBER = 0, 1, 2
TOP, BATCH, WALK, PEER_CAP, PARTS = 41, 8, 32, 128, 8
K_INLINE_REL, K_DEPS, K_PAR_INORDER_MIN = 6, 8, 4096   # umiclust_consts.h, resolve.cpp, resolve.h
OK, OVERFLOW, STUCK, BAD_PEER = 0, 1, 2, 3             # resolve.h kResolve*
NONE = 0xffffffff


def _bin_first(bin_start, q: int) -> int:
    if bin_start is None:
        return 0
    if isinstance(bin_start, (int, np.integer)):
        return int(bin_start)
    return int(bin_start[q])


def greedy_block(lens, count, thr, word, accept_rank, cent, state_in, q0, nq, w0, both=2, o4_T=0, bin_start=None,
                 maxaccepts=1, maxrejects=32) -> dict:
    """lens[seqno]; count(q, strand, t), thr(q, strand), word(q, strand, t) -> int; accept_rank(word) -> (accept,
    rank); cent: the centroids before the window; state_in: the states of [w0, q0).  bin_start: None (the bin starts
    at seqno 0), an integer, or an array seqno -> first sorted seqno of its bin.
    Returns state / target / strand per query of the block (target -1 and strand 0 for a centroid), new_cents,
    n_alignments, cells, final (seqno -> state over the window and the block), rechecks (strands whose O4 re-check
    inserted a hit) and recheck_stops (re-checks ended by maxrejects)."""
    assert len(state_in) == q0 - w0 and all(s in (CENT, MEMBER) for s in state_in)
    state = {w0 + i: int(s) for i, s in enumerate(state_in)}
    cent = [int(c) for c in cent]
    out = dict(state=[], target=[], strand=[], new_cents=[], n_alignments=0, cells=0, rechecks=0, recheck_stops=0)
    for q in range(q0, q0 + nq):
        b0 = _bin_first(bin_start, q)
        rs = b0 + (q - b0) // o4_T * o4_T if o4_T else q   # the first query of q's round
        assert not o4_T or rs >= w0 or all(c < rs for c in cent), "the window must hold the whole round"
        ql = int(lens[q])
        best = None   # (rank, -t, -strand)
        for s in range(both):
            t_ = thr(q, s)
            known = cent + [x for x in range(w0, min(q, rs)) if state[x] == CENT]
            hits = sorted((R.key(count(q, s, c), lens[c], c), c) for c in known if count(q, s, c) >= t_)[:TOP]
            hits = [dict(key=k, t=c, res=None) for k, c in hits]

            def align(h):
                h["res"] = accept_rank(word(q, s, h["t"]))
                out["n_alignments"] += 1
                out["cells"] += ql * int(lens[h["t"]])
            w, acc = 0, False
            while w < len(hits) and w < WALK and not acc:
                b1 = min(len(hits), w + BATCH, WALK)
                for h in hits[w:b1]:
                    align(h)
                    acc |= h["res"][0]
                w = b1
            if o4_T:
                extra = [x for x in range(max(rs, w0), q) if state[x] == CENT and count(q, s, x) >= t_]
                if extra:
                    out["rechecks"] += 1
                    hits = sorted(hits + [dict(key=R.key(count(q, s, x), lens[x], x), t=x, res=None) for x in extra],
                                  key=lambda h: h["key"])
                    na = nr = 0
                    for h in hits:
                        if na >= maxaccepts or nr >= maxrejects:
                            break
                        if h["res"] is None:
                            align(h)
                        na, nr = na + bool(h["res"][0]), nr + (not h["res"][0])
                    out["recheck_stops"] += nr >= maxrejects
            for h in hits:
                if h["res"] is not None and h["res"][0]:
                    c = (h["res"][1], -h["t"], -s)
                    if best is None or c > best:
                        best = c
        if best is None:
            state[q] = CENT
            out["new_cents"].append(q)
            out["state"].append(CENT), out["target"].append(-1), out["strand"].append(0)
        else:
            state[q] = MEMBER
            out["state"].append(MEMBER), out["target"].append(-best[1]), out["strand"].append(-best[2])
    out["final"] = state
    return out


def greedy_pool(al: R.Aligner, cent, state_in, q0, nq, w0, **kw) -> dict:
    """greedy_block over real sequences: counts and thresholds from the pool's k-mer sets, words from the oracle"""
    pool = al.pool
    cache: dict = {}

    def cnt(q, s, t):
        k = (q, s)
        if k not in cache:
            cache[k] = pool.counts(pool.query_kmers(q, s), np.arange(len(pool)))
        return int(cache[k][t])

    def thr(q, s):
        return min(12, len(pool.query_kmers(q, s)))
    return greedy_block(pool.lens, cnt, thr, al.word, al.judge, cent, state_in, q0, nq, w0, **kw)


# ------------------------------------------------------------------------------------------------ abstract world
_M = (1 << 64) - 1


def mix(*a: int) -> int:
    h = 0x9E3779B97F4A7C15
    for v in a:
        h = ((h ^ (v & _M)) * 0xBF58476D1CE4E5B9) & _M
        h ^= h >> 29
    h = (h * 0x94D049BB133111EB) & _M
    return h ^ (h >> 32)


def word_of(m: int, L: int = 64) -> int:
    return m | L << 8


ACC, REJ = word_of(62), word_of(55)      # 62 / 64 is accepted at identity 0.93, 55 / 64 is not
ACC_HI, ACC_LO = word_of(64), word_of(60)  # the highest and the lowest accepted rank of L = 64


class _Words(R.Aligner):
    def __init__(self, world):
        self.world, self.identity = world, 0.93
        self.acc, self.rank = R.tables(0.93)

    def word(self, q, strand, t):
        return self.world.word(q, strand, t)


class World:
    """Lengths, counts, thresholds and result words without sequences.  Scripted entries (set) win
    over the hash; with seed None everything not scripted has count 0 and rejects."""

    def __init__(self, lens, cent, seed=None, nfam=4, p_share=60, p_minus=20, p_acc=35, both=2):
        self.lens = np.asarray(lens, np.int32)
        assert np.all(self.lens >= 32) and np.all(self.lens <= 112)
        self.cent = [int(c) for c in cent]
        self.seed, self.nfam, self.p_share, self.p_minus, self.p_acc, self.both = seed, nfam, p_share, p_minus, p_acc, both
        self.cnt_ov, self.word_ov, self.thr_ov = {}, {}, {}
        self._bucket, self._ov_t = None, {}
        self.bin_of = None   # seqno -> load bin (a pack: nothing is shared across bins)
        self._fam = [mix(seed, 1, x) % nfam for x in range(len(self.lens))] if seed is not None else None

    def count(self, q, s, t):
        c = self.cnt_ov.get((q, s, t))
        if c is not None:
            return c
        if self.seed is None or self._fam[q] != self._fam[t] or (s == 1 and self.both == 1):
            return 0
        if self.bin_of is not None and self.bin_of[q] != self.bin_of[t]:
            return 0
        h = mix(self.seed, 2, q, s, t)
        c = 0 if h % 100 >= (self.p_minus if s else self.p_share) else 12 + (h >> 8) % 40   # 12..51: either side
        self.cnt_ov[(q, s, t)] = c                                                         # of the spec threshold 30
        return c

    def thr(self, q, s):
        return self.thr_ov.get((q, s), 12)

    def _maybe(self, q, lo, hi, cent=False):
        """the seqnos of [lo, hi) (or of cent) that can share anything with q: its family, or a scripted entry"""
        if self._bucket is None:
            fam = {}
            for x in range(len(self.lens)):
                fam.setdefault(self._fam[x] if self._fam else 0, []).append(x)
            self._bucket = fam
        pool = self._bucket[self._fam[q] if self._fam else 0]
        if self._fam:
            pool = sorted(set(pool) | self._ov_t.get(q, set()))
        if cent:
            cs = self._cset = getattr(self, "_cset", None) or set(self.cent)
            return [x for x in pool if x in cs]
        return [x for x in pool if lo <= x < hi]

    def word(self, q, s, t):
        w = self.word_ov.get((q, s, t))
        if w is not None:
            return w
        if self.seed is None:
            return REJ
        h = mix(self.seed, 3, q, s, t)
        return word_of(60 + (h >> 8) % 5) if h % 100 < self.p_acc else word_of(48 + (h >> 8) % 11)

    def set(self, q, s, t, count, word=REJ):
        self.cnt_ov[(q, s, t)] = count
        self.word_ov[(q, s, t)] = word
        self._ov_t.setdefault(q, set()).add(t)

    def aligner(self):
        return _Words(self)

    def lists(self, q0, nq, nprev):
        """the prefilter's output (prefilter_ref's ntop / top_seqno / top_count / npeer / peers) of this world"""
        both, w0 = 2, q0 - nprev * nq
        nqs = nq * both
        out = dict(ntop=np.zeros(nqs, np.int32), top_seqno=np.zeros((nqs, TOP), np.int64),
                   top_count=np.zeros((nqs, TOP), np.int32), npeer=np.zeros(nqs, np.int32), peers=[None] * nqs)
        for qs in range(nqs):
            q, s = q0 + qs // both, qs % both
            t_ = self.thr(q, s)
            top = sorted((R.key(self.count(q, s, c), self.lens[c], c), c) for c in self._maybe(q, 0, 0, True)
                         if self.count(q, s, c) >= t_)[:TOP]
            out["ntop"][qs] = len(top)
            for x, (k, c) in enumerate(top):
                out["top_seqno"][qs, x], out["top_count"][qs, x] = c, -k[0]
            pk = [(((x - w0) % nq) % PARTS, *R.key(self.count(q, s, x), self.lens[x], x), x)
                  for x in self._maybe(q, w0, q) if self.count(q, s, x) >= t_]
            if len(pk) > PEER_CAP:
                out["npeer"][qs] = 255
            else:
                pk.sort()
                out["npeer"][qs] = len(pk)
                out["peers"][qs] = (np.array([p[-1] - w0 for p in pk], np.int64),
                                    np.array([-p[1] for p in pk], np.int32))
        return out

    def greedy(self, state_in, q0, nq, w0, both=2, **kw):
        return greedy_block(self.lens, self.count, self.thr, self.word, self.aligner().judge, self.cent, state_in,
                            q0, nq, w0, both=both, **kw)

    def device(self, q0, nq, nprev, lazy=False):
        """pass_ref of the block: what the device hands resolve_block"""
        pool = types.SimpleNamespace(lens=self.lens)
        return R.pass_ref(pool, self.cent, q0, nq, nprev, lazy, False, al=self.aligner(),
                          lists=self.lists(q0, nq, nprev))


# --------------------------------------------------------------------------------------- the harness's input text
def tables_text(identity: float = 0.93) -> str:
    acc, rank = R.tables(identity)
    return " ".join(map(str, acc.astype(np.int64).ravel().tolist() + rank.ravel().tolist()))


# every configuration of the matrix: (pre_resolve, pre_spec, par_inorder, par_min, threads)
MATRIX = [(pr, ps, pi, pm, t) for pr in (1, 0) for ps in (1, 0) for pi in (1, 0) for pm in (1, K_PAR_INORDER_MIN)
          for t in (1, 3, 8)]


def hostqs_and_records(ref: dict, both: int = 2):
    """pass_ref's hostqs / records -> (rows of 15 integers per query-strand, the record words); both = 1 keeps the
    plus strands only (the world's minus strands must be empty)"""
    rows, recs = [], []
    for qs, (h, rec) in enumerate(zip(ref["hostqs"], ref["records"])):
        if both == 1 and qs % 2:
            assert h["nrel"] == 0 and h["w"] == 0
            continue
        off = NONE
        if rec is not None:
            off = len(recs)
            recs += [int(x) for x in rec]
        rows.append([h["best_t"], h["cells"], off, h["best_rank"], h["w"], h["flags"], h["nrel"], h["e"], h["npeer"],
                     *h["rel"]])
    return rows, recs


def case_text(lens, state_in, rows, recs, answers, q0, nq, w0, s0=0, both=2, o4_T=0, maxaccepts=1, maxrejects=32,
              bin_s=None, configs=MATRIX) -> str:
    """one case of tools/resolve_check_main.cpp.  answers: {(query << 1 | strand, target): word}; bin_s: the load
    bins' first seqnos (a pack) or None"""
    n = q0 + nq
    v = [q0, nq, w0, s0, both, o4_T, maxaccepts, maxrejects]
    if bin_s is None:
        v.append(0)
    else:
        bin_s = [int(b) for b in bin_s]
        hqbin = [max(i for i, b in enumerate(bin_s) if b <= x) for x in range(n)]
        v += [len(bin_s), *bin_s, *hqbin]
    v += [int(x) for x in lens[:n]]
    v += [int(x) for x in state_in]
    assert len(rows) == nq * both
    for r in rows:
        v += [int(x) for x in r]
    v += [len(recs), *recs]
    v.append(len(answers))
    for (pq, pt), w in answers.items():
        v += [pq, pt, w]
    v.append(len(configs))
    for c in configs:
        v += list(c)
    return " ".join(map(str, v))


def all_answers(world: World, q0, nq, w0, both=2) -> dict:
    """every pair round B may ask for: (query-strand of the block, any earlier seqno it shares enough k-mers with)"""
    out = {}
    for q in range(q0, q0 + nq):
        for s in range(both):
            t_ = world.thr(q, s)
            for t in world._maybe(q, 0, 0, True) + world._maybe(q, w0, q):
                if world.count(q, s, t) >= t_:
                    out[(q << 1 | s, t)] = world.word(q, s, t)
    return out


def norm(line: str) -> str:
    return " ".join(line.split())


def parse_result(lines: list[str]) -> list[dict]:
    """the harness's output of one case: per configuration `R rc | states | targets | strands | cents | aln cells` and
    `S deferred pairs merged trips largest-trip | kinds[6] | pq:pt ...`, `K kind per query-strand` (+ `E ...` lines for round-B pairs missing from the table)"""
    out = []
    for ln in lines:
        if ln.startswith("R "):
            out.append(dict(R=norm(ln), S=None, E=[]))
        elif ln.startswith("S "):
            out[-1]["S"] = ln
        elif ln.startswith("K"):
            out[-1]["K"] = ln[2:].strip()
        elif ln.startswith("E "):
            out[-1]["E"].append(ln)
    return out


def expected_line(rc: int, g: dict | None, nq: int) -> str:
    """the R line of a configuration whose block resolves to g (None: nothing written)"""
    if g is None:
        st, tg, sd, nc, aln, cells = [UNDET] * nq, [-1] * nq, [0] * nq, [], 0, 0
    else:
        st, tg, sd, nc, aln, cells = g["state"], g["target"], g["strand"], g["new_cents"], g["n_alignments"], g["cells"]
    j = lambda v: " ".join(map(str, v))
    return norm(f"R {rc} | {j(st)} | {j(tg)} | {j(sd)} | {j(nc)} | {aln} {cells}")


def parse_stats(line: str) -> dict:
    a, b, c = line[2:].split("|")
    d, p, m, t, big = map(int, a.split())
    pairs = [tuple(map(int, x.split(":"))) for x in c.split()]
    return dict(n_deferred=d, pairs_round_b=p, n_merged_walks=m, trips=t, largest_trip=big, kinds=list(map(int, b.split())), pairs=pairs)


def round_b_violations(ref: dict, g: dict, pairs, q0: int, w0: int, both: int = 2) -> list[str]:
    """Round-B requests judged from the references alone: each is a T_old entry at or past e, or a peer without the
    aligned bit whose final state (greedy_block) is not member; none is a pair the record already carried; none is
    asked twice."""
    bad, seen = [], set()
    for pq, pt in pairs:
        q, s = pq >> 1, pq & 1
        qs = (q - q0) * 2 + s if both == 2 else (q - q0) * 2
        w = ref["walks"][qs]
        if (pq, pt) in seen:
            bad.append(f"({pq}, {pt}) asked twice")
        seen.add((pq, pt))
        if ref["records"][qs] is None:
            bad.append(f"({pq}, {pt}): the query-strand has no record")
            continue
        nt = min(w["nt"], WALK)
        if pt in w["seq"][:nt]:
            if w["seq"].index(pt) < w["e"]:
                bad.append(f"({pq}, {pt}): T_old entry {w['seq'].index(pt)} < e = {w['e']} is in the record")
            continue
        ids = [int(i) + w0 for i in ref["lists"]["peers"][qs][0]]
        if pt not in ids:
            bad.append(f"({pq}, {pt}): neither a T_old entry nor a peer")
        elif ref["aligned"][qs][ids.index(pt)]:
            bad.append(f"({pq}, {pt}): the peer was aligned by the pass")
        elif g["final"][pt] == MEMBER:
            bad.append(f"({pq}, {pt}): the peer ends up a member")
    return bad


# ------------------------------------------------------------------------------------------------------ the fuzz
def fuzz_case(seed: int) -> dict:
    """One block of a hash world: block size, window depth (0..2 blocks), centroid rate, family count, sharing and
    accept rates, lazy peers and O4 (a third of the cases; the window then starts at a round's first query) all
    drawn from the seed."""
    r = lambda i, n: mix(seed, 77, i) % n
    nq = (1, 2, 3, 5, 8, 9, 13, 17, 24, 33, 40, 64)[r(0, 12)]
    nprev = r(1, 3)
    o4_T = (0, 0, 0, 0, 1, 2, 7, 25)[r(2, 8)]
    pre = 20 + r(3, 60)
    if o4_T:
        pre = (pre + o4_T - 1) // o4_T * o4_T
    w0, q0 = pre, pre + nprev * nq
    n = q0 + nq
    lens = np.sort(60 + np.array([mix(seed, 78, i) % 9 for i in range(n)]))[::-1]
    cent_rate = (15, 30, 60)[r(4, 3)]
    cent = [x for x in range(pre) if mix(seed, 79, x) % 100 < (40, 70, 90)[r(9, 3)]]
    state_in = [CENT if mix(seed, 80, x) % 100 < cent_rate else MEMBER for x in range(w0, q0)]
    world = World(lens, cent, seed=seed, nfam=(1, 2, 3, 6)[r(5, 4)], p_share=(25, 50, 80)[r(6, 3)],
                  p_minus=(0, 10, 30)[r(7, 3)], p_acc=(3, 10, 25, 50)[r(8, 4)])
    return dict(world=world, q0=q0, nq=nq, w0=w0, nprev=nprev, o4_T=o4_T, lazy=bool(r(10, 3) == 0),
                state_in=state_in, maxrejects=(32, 32, 4)[r(11, 3)] if o4_T else 32)


# ------------------------------------------------------------------------------------------ real sequences
def _staged(ndec: int, nvar: int, seed: int):
    """Three families whose window is 3 * ndec mutually rejecting, k-mer-sharing centroids (pass_ref.decoy: every one
    shares the base's k-mers, none is within the identity of another) and whose block holds nvar variants of each base:
    with lazy peers every variant needs all of its family's window centroids from round B."""
    rng = np.random.default_rng(seed)
    assert ndec % 2 == 0
    fams = [R.Family(rng, ndec, []) for _ in range(3)]
    window = sorted([s for f in fams for s in f.cents], key=lambda s: -len(s))
    nq = 3 * ndec // 2
    block = [fams[i % 3].q(1 + i % 3) for i in range(3 * nvar)]
    block = R.fill(rng, block + [None] * (nq - 3 * nvar))
    pool = R.PR.Pool(window + block)
    return dict(pool=pool, cent=np.zeros(0, np.int64), q0=3 * ndec, nq=nq, nprev=2, pivots={})


def _overflow0(seed: int = 611):
    """130 window queries and a block of 65 of one family: the block's query 0 has 130 peers, past the cap of 128"""
    rng = np.random.default_rng(seed)
    f = R.Family(rng, 0, [(3, 64)])
    pool, cent = R.assemble(f.cents, [f.q(int(rng.integers(0, 3))) for _ in range(195)])
    return dict(pool=pool, cent=cent, q0=len(cent) + 130, nq=65, nprev=2, pivots={})


# name -> (builder, lazy, prev): the cases of tests/test_gpu_resolve.py beyond pass_ref.CASES
REAL_CASES = {
    "staged_big": (lambda: _staged(84, 40, 601), True, False),
    "staged_small": (lambda: _staged(30, 10, 602), True, False),
    "tri9x2_lazy": (lambda: R._small_case(503, 9, True), True, False),
    "ambig9x2_lazy": (R._ambig_case, True, True),
    "overflow0": (_overflow0, False, False),
}
_real: dict = {}


def real_case(name: str) -> dict:
    """A case of pass_ref.CASES or REAL_CASES with what the resolve tests add: state_in (the greedy states of the
    window, clustered from `cent` as one block), k (the first query with an overflowing peer list, nq without one),
    g (greedy_block of the block's first k queries).  Computed once per process; read-only."""
    if name in _real:
        return _real[name]
    if name in R.CASES:
        c = dict(R.case(name))
    else:
        builder, lazy, prev = REAL_CASES[name]
        b = R._built(builder)
        ref = R.pass_ref(b["pool"], b["cent"], b["q0"], b["nq"], b["nprev"], lazy, prev, al=b["al"], lists=b["lists"])
        c = dict(b, lazy=lazy, prev=prev, ref=ref)
    w0 = c["q0"] - c["nprev"] * c["nq"]
    win = greedy_pool(c["al"], c["cent"], [], w0, c["q0"] - w0, w0)
    over = [qs // 2 for qs, h in enumerate(c["ref"]["hostqs"]) if h["flags"] & 2]
    c.update(w0=w0, state_in=win["state"], k=min(over) if over else c["nq"])
    c["g"] = greedy_pool(c["al"], c["cent"], c["state_in"], c["q0"], c["k"], w0)
    _real[name] = c
    return c


def real_answers(c: dict) -> dict:
    """every pair round B may ask for in a real case: the listed candidates and peers of every query-strand"""
    out, lists = {}, c["lists"]
    for qs in range(2 * c["k"]):
        q, s = c["q0"] + qs // 2, qs % 2
        ts = [int(t) for t in lists["top_seqno"][qs, :int(lists["ntop"][qs])]]
        if lists["peers"][qs] is not None:
            ts += [c["w0"] + int(i) for i in lists["peers"][qs][0]]
        for t in ts:
            out[(q << 1 | s, t)] = c["al"].word(q, s, t)
    return out


def needed_pairs(c: dict) -> set:
    """the alignments the greedy walk of the block's first k queries uses and the pass does not hand over: a lower
    bound of round B's pairs.  (greedy_block is re-run with a recording word function.)"""
    used = set()
    al = c["al"]

    class Rec:
        pool, judge = al.pool, al.judge

        @staticmethod
        def word(q, s, t):
            used.add((q << 1 | s, t))
            return al.word(q, s, t)
    greedy_pool(Rec, c["cent"], c["state_in"], c["q0"], c["k"], c["w0"])
    have = set()
    for qs in range(2 * c["k"]):
        q, s = c["q0"] + qs // 2, qs % 2
        w = c["ref"]["walks"][qs]
        have |= {(q << 1 | s, t) for t in w["seq"][:w["e"]]}
        if c["lists"]["peers"][qs] is not None:
            have |= {(q << 1 | s, c["w0"] + int(i)) for i, a in zip(c["lists"]["peers"][qs][0], c["ref"]["aligned"][qs])
                     if a}
    return used - have


def most_pairs(c: dict) -> int:
    """an upper bound of round B's pairs: every T_old entry from e on and every peer the pass did not align, of every
    query-strand of the first k queries that has a record"""
    n = 0
    for qs in range(2 * c["k"]):
        if c["ref"]["records"][qs] is not None:
            w = c["ref"]["walks"][qs]
            n += min(w["nt"], WALK) - w["e"] + sum(not a for a in c["ref"]["aligned"][qs])
    return n
