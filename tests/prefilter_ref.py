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

The modes production runs are restated on the same rule: prefilter_split_ref (a split pass: the counting half's
flagged hits, kept by the merge if they became centroids), prefilter_pack_ref (a pack of a multi-bin load: a query
sees its own bin only; every bin in vsearch's order on its own) and the two-segment case (segment_case: more than
7 x 65,536 centroids).  bin_mask restates the per-bin k-mer scrambling of load.cpp, for pack_would_be_hits only.
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
    """Sequences in vsearch's order with their plus-strand k-mer sets as a padded matrix.  bin_start (record
    boundaries of a multi-bin load, first 0 and last len(seqs)): every bin is in vsearch's order on its own, as
    umiclust_load_bins lays the bins out one after another; bin_s and qbin (seqno -> bin) name them."""

    def __init__(self, seqs: list[str], bin_start=None, sets=None):
        """sets: the sequences' k-mer sets where the caller has them already (kmer_set of each otherwise)"""
        lens = [len(s) for s in seqs]
        self.bin_s = np.array([0, len(seqs)] if bin_start is None else bin_start, np.int64)
        assert self.bin_s[0] == 0 and self.bin_s[-1] == len(seqs) and np.all(np.diff(self.bin_s) > 0)
        for lo, hi in zip(self.bin_s[:-1], self.bin_s[1:]):
            assert all(a >= b for a, b in zip(lens[lo:hi], lens[lo + 1:hi])), \
                "sequences must be sorted by length, longest first"
        self.qbin = np.repeat(np.arange(len(self.bin_s) - 1), np.diff(self.bin_s))
        self.seqs = seqs
        self.lens = np.array(lens, np.int32)
        if isinstance(sets, np.ndarray):  # the padded matrix itself (rows ascending, PAD behind the k-mers)
            self.kp = sets
            self.nk = (sets != PAD).sum(axis=1).astype(np.int32)
            return
        sets = [kmer_set(s) for s in seqs] if sets is None else sets
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


def prefilter_ref(pool: Pool, cent, q0: int, nq: int, nprev: int = 0, both: int = 2, minwordmatches: int = 12,
                  pack: bool = False) -> dict:
    """What umiclust_prefilter returns for the block [q0, q0 + nq) against the centroids `cent` (increasing seqnos)
    and the peer window [q0 - nprev * nq, q0 + nq), per query-strand qs = (q - q0) * both + strand:
      ntop[qs], top_seqno[qs, :ntop], top_count[qs, :ntop]; npeer[qs] (255 = overflow), peers[qs] = (ids, counts)
      in the expected order (None on overflow);
    and what the path assertions need: nk[qs], thr[qs], ncand[qs] (candidates before the cut at 41),
    part_max[qs] (most candidates in one part, part = centroid ordinal % 8), npeer_all[qs] (before the cap),
    units[qs] (the parts k_pf_count hands to k_pf_full: those with more than 64 candidates, all 8 when thr == 0).
    pack (prefilter_pack_ref): a query sees its own bin only."""
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
        lo = int(pool.bin_s[pool.qbin[q]]) if pack else 0  # packs: the query's bin starts here
        win = np.arange(max(w0, lo), q, dtype=np.int64)
        part = ((win - w0) % nq) % PARTS
        for strand in range(both):
            qs = qi * both + strand
            qk = pool.query_kmers(q, strand)
            thr = min(minwordmatches, len(qk))
            out["nk"][qs], out["thr"][qs] = len(qk), thr
            cnt = pool.counts(qk, cent) if len(cent) else np.zeros(0, np.int32)
            ok = np.nonzero((cnt >= thr) & (cent >= lo))[0]
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
                out["peers"][qs] = ((win[po] - w0).astype(np.int64), pc[po].astype(np.int32))
    return out


def prefilter_split_ref(pool: Pool, cent, newcent, w0: int, nq: int, both: int = 2, minwordmatches: int = 12) -> dict:
    """What umiclust_prefilter_split returns: block j = [w0 + 2 nq, w0 + 3 nq) as a split pass, block j-2 =
    [w0, w0 + nq) flagged in the counting half and `newcent` (increasing seqnos of block j-2) appended before the
    second half.  The invariant: the lists equal prefilter_ref(pool, sorted(cent + newcent), w0 + 2 nq, nq, nprev=1)
    -- a flagged hit is kept exactly if it became a centroid, and peer ids are relative to w0 + nq.  The units differ
    (they are the counting half's) and are computed here from the flagged hits: a (query-strand, part) unit
    overflows when thr == 0 or when the centroid candidates of `cent` with ordinal % 8 == part plus the entries x of
    block j-2 with count >= thr and (x - w0) % 8 == part, in newcent or not, exceed 64.  Added per query-strand:
    part_sum (the largest such sum), cent_part_max (the same without the flagged hits), flag_kept / flag_dropped
    (flagged hits over the threshold inside / outside newcent), tied_kept (the top list holds a kept flagged hit and an
    indexed centroid of `cent` with equal counts)."""
    cent, newcent = np.asarray(cent, np.int64), np.asarray(newcent, np.int64)
    assert len(newcent) == 0 or (np.all(np.diff(newcent) > 0) and newcent[0] >= w0 and newcent[-1] < w0 + nq)
    q0 = w0 + 2 * nq
    out = prefilter_ref(pool, np.concatenate([cent, newcent]), q0, nq, 1, both, minwordmatches)
    nqs = nq * both
    flagged = np.arange(w0, w0 + nq, dtype=np.int64)
    isnew = np.isin(flagged, newcent)
    for k in ("part_sum", "cent_part_max", "flag_kept", "flag_dropped", "tied_kept"):
        out[k] = np.zeros(nqs, np.int32)
    for qs in range(nqs):
        qk = pool.query_kmers(q0 + qs // both, qs % both)
        thr = int(out["thr"][qs])
        cc = np.bincount(np.nonzero(pool.counts(qk, cent) >= thr)[0] % PARTS, minlength=PARTS) if len(cent) \
            else np.zeros(PARTS, np.int64)
        hit = pool.counts(qk, flagged) >= thr
        fc = np.bincount(np.nonzero(hit)[0] % PARTS, minlength=PARTS)
        out["part_sum"][qs], out["cent_part_max"][qs] = (cc + fc).max(), cc.max()
        out["units"][qs] = PARTS if thr == 0 else int((cc + fc > PART_CAND).sum())
        out["flag_kept"][qs], out["flag_dropped"][qs] = (hit & isnew).sum(), (hit & ~isnew).sum()
        n = int(out["ntop"][qs])
        ts, tc = out["top_seqno"][qs, :n], out["top_count"][qs, :n]
        out["tied_kept"][qs] = len(np.intersect1d(tc[ts >= w0], tc[ts < w0])) > 0
    return out


def prefilter_pack_ref(pool: Pool, cent, q0: int, nq: int, nprev: int = 0, both: int = 2,
                       minwordmatches: int = 12) -> dict:
    """What umiclust_prefilter_pack returns on the pack `pool` (a Pool with bin_start): a query of bin b takes only
    the centroids with seqno >= bin_s[b] and only the peers x >= bin_s[b] of the window, with counts on the
    unscrambled k-mers; a centroid's part is its ordinal in the whole pack % 8."""
    return prefilter_ref(pool, cent, q0, nq, nprev, both, minwordmatches, pack=True)


def bin_mask(b: int) -> int:
    """The 16-bit XOR mask of load bin b's k-mers (load.cpp prepare_impl: the murmur3 finaliser of the bin index)."""
    h = (b * 0x9E3779B1 + 0x7F4A7C15) & 0xffffffff
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xffffffff
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xffffffff
    h ^= h >> 16
    return (h ^ (h >> 16)) & 0xffff


def pack_would_be_hits(pool: Pool, cent, q0: int, nq: int, nprev: int = 0, both: int = 2,
                       minwordmatches: int = 12) -> dict:
    """What a prefilter without the per-bin cuts would have listed, per query-strand, counting on the scrambled
    k-mers (code ^ bin_mask(bin)) as the device's counters do: cross_cent / cross_peer (hits >= thr among the earlier
    bins' centroids / window entries; every one of them when thr == 0) and own_cent / own_peer (the query's own bin).
    Only for the case conditions: the expected lists never come from here."""
    cent = np.asarray(cent, np.int64)
    w0 = q0 - nprev * nq
    xm = np.array([bin_mask(b) for b in range(len(pool.bin_s) - 1)], np.int32)
    skp = np.where(pool.kp == PAD, PAD, pool.kp ^ xm[pool.qbin][:, None])
    out = {k: np.zeros(nq * both, np.int32) for k in ("cross_cent", "cross_peer", "own_cent", "own_peer")}
    for qs in range(nq * both):
        q = q0 + qs // both
        lo = int(pool.bin_s[pool.qbin[q]])
        qk = pool.query_kmers(q, qs % both)
        thr = min(minwordmatches, len(qk))
        mark = np.zeros(PAD + 1, np.int32)
        mark[qk ^ xm[pool.qbin[q]]] = 1
        win = np.arange(w0, q, dtype=np.int64)
        for rows, name in ((cent, "cent"), (win, "peer")):
            hit = mark[skp[rows]].sum(axis=1) >= thr
            out["cross_" + name][qs], out["own_" + name][qs] = (hit & (rows < lo)).sum(), (hit & (rows >= lo)).sum()
    return out


def monotone_lengths(pool: Pool, cent) -> np.ndarray:
    """The length a cnt_ge lookup would give each centroid ordinal (the largest L with more than `ordinal` centroids
    of length >= L): right only while lengths do not rise with the ordinal, which a pack's do at every bin."""
    clen = pool.lens[np.asarray(cent, np.int64)]
    ge = np.array([(clen >= L).sum() for L in range(int(clen.max()) + 2)])
    return np.array([np.nonzero(ge > o)[0].max() for o in range(len(clen))], np.int32)


def prefilter_brute(seqs: list[str], cent, q0: int, nq: int, nprev: int = 0, both: int = 2,
                    minwordmatches: int = 12, bin_start=None, newcent=None) -> dict:
    """The same lists by plain set intersections (the vectorised reference's own check; small inputs only).
    bin_start: the pack mode (a query's candidates and peers are its own bin's).  newcent: the split mode -- q0, nq,
    nprev = 2 name the three-block window as the counting half sees it; the lists are those of cent + newcent with
    the window cut to its two newer blocks, and `units` counts per query-strand the parts whose candidates among
    `cent` plus flagged hits (every hit of the oldest block) exceed 64 (all 8 when thr == 0)."""
    kp = [set(kmer_set(s)) for s in seqs]
    w0 = q0 - nprev * nq
    ntop, tops, npeer, peers, units = [], [], [], [], []
    flagged = []
    if newcent is not None:
        assert nprev == 2
        flagged, w0 = list(range(w0, w0 + nq)), w0 + nq
    old, cent = list(cent), list(cent) + list(newcent if newcent is not None else [])
    for q in range(q0, q0 + nq):
        lo = 0 if bin_start is None else max(b for b in bin_start if b <= q)
        for strand in range(both):
            kq = kp[q] if strand == 0 else set(kmer_set(seqs[q], True))
            thr = min(minwordmatches, len(kq))
            cand = [(-len(kq & kp[c]), len(seqs[c]), c) for c in cent if len(kq & kp[c]) >= thr and c >= lo]
            per = [0] * PARTS
            for o, c in enumerate(old):
                per[o % PARTS] += len(kq & kp[c]) >= thr and c >= lo
            for x in flagged:
                per[(x - flagged[0]) % PARTS] += len(kq & kp[x]) >= thr
            units.append(PARTS if thr == 0 else sum(n > PART_CAND for n in per))
            cand.sort()
            cand = cand[:TOP]
            ntop.append(len(cand))
            tops.append([(c, -n) for n, _, c in cand])
            pe = [(((x - w0) % nq) % PARTS, -len(kq & kp[x]), len(seqs[x]), x - w0) for x in range(max(w0, lo), q)
                  if len(kq & kp[x]) >= thr]
            pe.sort()
            npeer.append(255 if len(pe) > PEER_CAP else len(pe))
            peers.append(None if len(pe) > PEER_CAP else [(i, -n) for _, n, _, i in pe])
    return dict(ntop=ntop, tops=tops, npeer=npeer, peers=peers, units=units)


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


def kmer_text(code: int) -> str:
    """the 8-mer of a code (2 bits per base, A C G T = 0..3, first base in the top bits)"""
    return "".join("ACGT"[(code >> (14 - 2 * i)) & 3] for i in range(8))


NOISE_TAIL = "GTATCGGCTACCGCAAAAATAGTA"


def noise_queries() -> list[str]:
    """The low_complexity construction at its sparse end: an "AC" repeat and 8..10 nt of NOISE_TAIL, length 64.  DUST
    leaves 1, 2 or 3 unmasked 8-mers on either strand (thr = nk; tests/test_prefilter_ref_cpu.py asserts it), all
    inside NOISE_TAIL[:10]."""
    return ["AC" * 28 + NOISE_TAIL[:8], "C" + "AC" * 27 + NOISE_TAIL[:9], "AC" * 27 + NOISE_TAIL[:10]]


def colliders(n: int, from_bin: int, in_bin: int, seed: int) -> list[str]:
    """n sequences of length 60..68, longest first, for load bin in_bin: each carries, between random flanks, the
    8-mers whose codes are v ^ bin_mask(from_bin) ^ bin_mask(in_bin) for the three plus-strand 8-mers v of
    noise_queries()[2] -- after the per-bin scrambling they land on the lists a noise query of bin from_bin reads, so
    every one of them would be a hit of such a query if the prefilter did not cut earlier bins out.  A draw in
    which DUST masks one of the built 8-mers is thrown away and drawn again with other flanks."""
    rng = np.random.default_rng(seed)
    codes = [v ^ bin_mask(from_bin) ^ bin_mask(in_bin) for v in kmer_set(noise_queries()[2])]
    assert len(codes) == 3
    lens = np.sort(rng.integers(60, 69, n))[::-1]
    out = []
    for L in lens:
        while True:
            rnd = "".join("ACGT"[i] for i in rng.integers(0, 4, int(L)))
            cut = np.sort(rng.integers(0, int(L) - 24 + 1, 3))  # where the three 8-mers go (gaps of random text)
            t, at = "", 0
            for c, k in zip(cut, codes):
                t += rnd[at:c] + kmer_text(k)
                at = c
            t += rnd[at:int(L) - 24]
            assert len(t) == L
            if set(codes) <= set(kmer_set(t)):
                out.append(t)
                break
    return out


SEG_CENT = 7 * 65536            # kSegCentroids: centroids per counter segment
SEG_N = SEG_CENT + 2000         # the two-segment pool: its last 8 sequences are the queries
SEG_FAMILY = 40                 # shared-core sequences in each segment


def plain_kmer_matrix(base: np.ndarray) -> np.ndarray:
    """The unique 8-mers of every row of an (n, L) matrix of A C G T bytes, as Pool's padded matrix, with no DUST:
    right for the rows DUST leaves alone (segment_pool checks each row and sends the others through the oracle)."""
    code = (np.searchsorted(_ACGT, base)).astype(np.int32)
    n, L = code.shape
    km = np.zeros((n, L - 7), np.int32)
    for j in range(8):
        km |= code[:, j:L - 7 + j] << (14 - 2 * j)
    km.sort(axis=1)
    km[:, 1:][km[:, 1:] == km[:, :-1]] = PAD
    km.sort(axis=1)
    return km


def segment_pool(n: int = SEG_N, seed: int = 401) -> tuple[list[str], np.ndarray]:
    """n sequences of length 64 past one counter segment when all but the last 8 are centroids (umiclust.synth's
    segment_stress is the model): random filler, SEG_FAMILY shared-core sequences (master48()[:c], c in 19..40, at a
    random offset) spread over each counter segment's ordinals, and 8 queries at the end -- 7 shared-core ones and
    "A" * 64 (thr = 0).  Returns the sequences and their k-mer matrix: the filler's 8-mers are computed in numpy for
    the rows DUST leaves unchanged (orc.dust is still run on every row), the oracle's extraction does the rest."""
    rng = np.random.default_rng(seed)
    base = _ACGT[rng.integers(0, 4, (n, 64))]
    m = np.frombuffer(master48().encode(), np.uint8)
    fam = np.concatenate([np.sort(rng.choice(SEG_CENT, SEG_FAMILY, replace=False)),
                          np.sort(rng.choice(np.arange(SEG_CENT, n - 8), SEG_FAMILY, replace=False)),
                          np.arange(n - 8, n - 1)])
    for i in fam:
        c = int(rng.integers(19, 41))
        o = int(rng.integers(0, 64 - c + 1))
        base[i, o:o + c] = m[:c]
    base[n - 1] = ord("A")
    flat = base.tobytes()
    seqs = [flat[i:i + 64].decode() for i in range(0, n * 64, 64)]
    kp = plain_kmer_matrix(base)
    masked = [i for i, s in enumerate(seqs) if orc.dust(s) != s]
    for i in masked:
        k = kmer_set(seqs[i])
        kp[i] = PAD
        kp[i, :len(k)] = k
    return seqs, kp


PACK_BINS = (1, 2)    # the packs are load bins 1 and 2; bin 0 is a bin of its own in front (absolute seqnos)
PACK_N1 = 140         # pack: colliders in bin 1
PACK_CENT2, PACK_NQ = 24, 32  # pack: bin 2's centroids, then the blocks j-1 and j of 32 queries each


def _front_bin() -> list[str]:
    return control()[:20]


def pack_noise_pool() -> tuple[list[str], list[int]]:
    """Three load bins: 20 plain UMIs; 140 colliders(from bin 2); bin 2, every sequence 64 long -- 24 noise queries
    (its centroids), then two blocks of 32: noise queries with the four 64-long LOW_SPECIALS (thr = 0) spread among
    them, two in block j-1 and all four in block j."""
    a, b = _front_bin(), colliders(PACK_N1, 2, 1, 211)
    nz = noise_queries()
    sp = [x for i, x in enumerate(LOW_SPECIALS) if len(x) == 64 and x not in LOW_SPECIALS[:i]]
    assert len(sp) == 4
    c = [nz[i % 3] for i in range(PACK_CENT2 + 2 * PACK_NQ)]
    for at, x in ((30, sp[0]), (45, sp[2]), (58, sp[0]), (63, sp[1]), (70, sp[2]), (85, sp[3])):
        c[at] = x
    return a + b + c, [0, len(a), len(a) + len(b), len(a) + len(b) + len(c)]


PACKLEN_N1, PACKLEN_LONG, PACKLEN_64 = 400, 300, 436  # pack_lengths: bin-1 centroids; bin 2's of 65..68 and of 64


def fixed_core(lens, flank: str, seed: int) -> list[str]:
    """One sequence per length: master48()[:30] at a random offset between random flanks, the base on each side of the
    core set to `flank`.  Two of them with different flank bases share exactly the core's 23 8-mers (but for chance
    hits among the random flanks), and the 8-mers across the core's ends never extend the match."""
    rng = np.random.default_rng(seed)
    m = master48()[:30]
    out = []
    for L in lens:
        L = int(L)
        o = int(rng.integers(1, L - 30))
        f = "".join("ACGT"[i] for i in rng.integers(0, 4, L))
        out.append(f[:o - 1] + flank + m + flank + f[o + 31:])
        assert len(out[-1]) == L
    return out


def pack_length_pool() -> tuple[list[str], list[int]]:
    """Three load bins: 20 plain UMIs; 400 fixed-core sequences of length 58..60; in bin 2, 300 of length 65..68,
    436 of length 64 and the 64 queries (length 64, the other flank base) -- a pack whose lengths rise with the
    ordinal at the bin boundary, every bin-2 centroid a candidate of every query at one count, 23.  So a part's
    92 candidates are tied, its best 41 are decided by length alone, and the 400 ordinals in front of bin 2 shift a
    length looked up from the ordinal by 50 entries a part: more than the 41 a part keeps."""
    rng = np.random.default_rng(313)
    a = _front_bin()
    b = fixed_core(np.sort(rng.integers(58, 61, PACKLEN_N1))[::-1], "C", 315)
    c = fixed_core(np.sort(rng.integers(65, 69, PACKLEN_LONG))[::-1], "C", 317) + \
        fixed_core([64] * PACKLEN_64, "C", 319) + fixed_core([64] * 64, "A", 321)
    return a + b + c, [0, len(a), len(a) + len(b), len(a) + len(b) + len(c)]


def two_step_tops(pool: Pool, cent, q0: int, nq: int, ref: dict, clen: np.ndarray) -> list[np.ndarray]:
    """A model of how the kernels reach a plus- or minus-strand top list in a pack, with `clen` as the centroid
    lengths the full kernel uses: a part of more than 64 candidates keeps its best 41 by (count, clen, ordinal); the
    merge orders what the parts kept by (count, true length, seqno).  With the true lengths this is the reference's
    list; with monotone_lengths it is what a cnt_ge lookup in k_pf_full would list.  Per query-strand, seqnos."""
    cent = np.asarray(cent, np.int64)
    out = []
    for qs in range(len(ref["ntop"])):
        q = q0 + qs // 2
        cnt = pool.counts(pool.query_kmers(q, qs % 2), cent)
        ok = np.nonzero((cnt >= ref["thr"][qs]) & (cent >= pool.bin_s[pool.qbin[q]]))[0]
        keep = []
        for part in range(PARTS):
            o = ok[ok % PARTS == part]
            if len(o) > PART_CAND or ref["thr"][qs] == 0:
                o = o[np.lexsort((o, clen[o], -cnt[o]))][:TOP]
            keep.append(o)
        o = np.concatenate(keep)
        out.append(cent[o[np.lexsort((cent[o], pool.lens[cent[o]], -cnt[o]))][:TOP]])
    return out


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
    if name == "pack":
        return Pool(*pack_noise_pool())
    if name == "packlen":
        return Pool(*pack_length_pool())
    if name == "segments":
        seqs, kp = segment_pool()
        return Pool(seqs, sets=kp)
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


# ---- split passes: name -> (pool, centroids before w0 (a count, spread evenly), w0, nq, newcent, append_step);
# newcent: a callable of the block j-2's seqnos.  Block j is [w0 + 2 nq, w0 + 3 nq).
def _third(b):
    return b[::3]


SPLIT_CASES = {
    "split_some": ("peers", 40, 50, 60, _third, ALL),
    "split_none": ("peers", 40, 50, 60, lambda b: b[:0], ALL),
    "split_all": ("peers", 40, 50, 60, lambda b: b, ALL),
    # every core >= 19 in this zone, so every centroid and every flagged entry is a hit of every plus strand: 448
    # centroids (56 a part) and 64 flagged hits (8 a part) fill every part to exactly 64; with 452 the parts 0..3 hold
    # 57 + 8 = 65 beside parts 4..7 at 64
    "split_cap64": ("core", 448, 1000, 64, _third, ALL),
    "split_cap65": ("core", 452, 1000, 64, _third, ALL),
    # 8,100 + 104 > 8,192: the append between the halves folds the delta tile into the base tile (104 queries a
    # block: the fold needs 100 new centroids out of one block)
    "split_fold": ("core", 8100, 20000, 104, lambda b: b, ALL),
    "split_low": ("low", None, None, 64, _third, 100),
    # 70 queries a block: the 128 / 129 boundary needs a two-block window of at least 130 entries
    "split_peers": ("peers", 40, 40, 70, _third, ALL),
}


@functools.lru_cache(maxsize=None)
def split_case(name: str) -> dict:
    pname, ncent, w0, nq, pick, step = SPLIT_CASES[name]
    p = pool(pname)
    if pname == "low":  # block j: low_case's queries; its centroids before the window
        cent, q0 = low_case(p)
        w0 = q0 - 2 * nq
        cent = cent[cent < w0]
    else:
        cent = spread(ncent, w0)
    newcent = np.asarray(pick(np.arange(w0, w0 + nq, dtype=np.int64)), np.int64)
    return dict(pool=p, cent=cent, newcent=newcent, w0=w0, nq=nq, step=step,
                ref=prefilter_split_ref(p, cent, newcent, w0, nq))


# ---- packs (load bins PACK_BINS of a three-bin load): name -> (pool, bin-1 centroids, bin-2 centroids, q0 relative
# to bin 2's start, nq, nprev).  The centroids are the first ones of each bin (a bin's first sequence is a centroid).
# bin 2's first centroid ordinal: the residue classes of pack_cmin (72: the third word of a uint4, which the others miss)
PACK_ORD0 = (1, 7, 8, 9, 33, 72, 127, 128, 129, 136)
PACK_CASES = {f"pack_ord{k}": ("pack", k, PACK_CENT2, PACK_CENT2 + PACK_NQ, PACK_NQ, 1) for k in PACK_ORD0}
# bin 2 starts d entries into the window: d = 1..32 inside block j-1 (every (part, byte) of pack_pmin), d = 33..63
# inside block j itself (the block crosses the bin boundary)
PACK_CASES.update({f"pack_win{d}": ("pack", 70, 0, 2 * PACK_NQ - PACK_NQ - d, PACK_NQ, 1) for d in range(1, 64)})
PACK_CASES["pack_lengths"] = ("packlen", PACKLEN_N1, PACKLEN_LONG + PACKLEN_64, PACKLEN_LONG + PACKLEN_64, 64, 0)


@functools.lru_cache(maxsize=None)
def pack_case(name: str) -> dict:
    pname, n1, n2, rel, nq, nprev = PACK_CASES[name]
    p = pool(pname)
    s1, s2 = int(p.bin_s[1]), int(p.bin_s[2])
    cent = np.concatenate([np.arange(s1, s1 + n1), np.arange(s2, s2 + n2)]).astype(np.int64)
    q0 = s2 + rel
    return dict(pool=p, cent=cent, q0=q0, nq=nq, nprev=nprev, step=ALL, first=PACK_BINS[0], nbins=len(PACK_BINS),
                ref=prefilter_pack_ref(p, cent, q0, nq, nprev), would=pack_would_be_hits(p, cent, q0, nq, nprev))


@functools.lru_cache(maxsize=None)
def segment_case() -> dict:
    """Two counter segments: every sequence before the 8 queries is a centroid (SEG_CENT + 1,992 of them)."""
    p = pool("segments")
    q0 = len(p) - 8
    cent = np.arange(q0, dtype=np.int64)
    return dict(pool=p, cent=cent, q0=q0, nq=8, nprev=0, step=ALL, ref=prefilter_ref(p, cent, q0, 8, 0))
