"""The HIP-free planning core (ont-tcrconsensus_amd/csrc/plan.cpp) under ASan + UBSan, without a GPU:
tools/plan_check_main.cpp drives the block planner (how a bin's sorted queries are cut into greedy blocks, re-cut after
a peer overflow and regrown after clean blocks), the cluster numbering and the plan of the member tracebacks (which
member goes to which launch and slot).  Expected plans of the smallest shapes that
can go wrong are written out by hand; seeded random inputs check the invariants every plan must keep; the numbering
is compared with a numpy restatement and, for one case, with the CPU oracle.  A sanitizer report fails the test."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
K_SEG_LENS = 32     # umiclust_consts.h kSegLens
K_PEER_CAP = 128    # umiclust_consts.h kPeerCap
BIG_HINT = 1 << 30  # a context's first bin: no block size carried over


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("plan_check")
    b = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ont-tcrconsensus_amd"), "plan_check", f"SAN_OUT={out}"],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    assert "warning" not in b.stderr, b.stderr
    count = [0]

    def run(mode, cases):
        """cases: lists of integers, one per case -> the checker's output lines, split per case"""
        count[0] += 1
        path = out / f"in{count[0]}.txt"
        path.write_text("\n".join(" ".join(map(str, c)) for c in cases) + "\n")
        r = subprocess.run([str(out / "plan_check"), mode, str(path)], capture_output=True, text=True, timeout=300,
                           env=SAN_ENV)
        assert r.returncode == 0, r.stderr[-4000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
        got = [chunk.strip().split("\n") for chunk in r.stdout.split("case\n")[1:]]
        assert len(got) == len(cases)
        return got
    return run


# ---- mode 1: blocks ----
OVERFLOW, RESOLVED, HALVE = 0, 1, 2


def blocks_case(hlen, B, mix=0, o4_T=0, regrow=0, b_hint=BIG_HINT, bin_s=None, pack=0, bin0=0, ops=()):
    """hlen: lengths from seqno 0 on; bin_s: bin boundaries (default: one bin over all of hlen)"""
    bin_s = list(bin_s) if bin_s is not None else [0, len(hlen)]
    assert bin_s[-1] == len(hlen)
    flat = [x for op in ops for x in op]
    return [B, mix, o4_T, regrow, b_hint, pack, bin0, len(bin_s) - 1, *bin_s, *hlen, len(ops), *flat]


def parse_plan(line):
    head, _, tail = line.partition(":")
    ret, b_eff, clean = map(int, head.split())
    return ret, b_eff, clean, [tuple(map(int, b.split(","))) for b in tail.split()]


def plans(plan_check, case):
    return [parse_plan(line) for line in plan_check("blocks", [case])[0]]


def test_blocks_one_length_per_block(plan_check):
    hlen = [68] * 5 + [67] * 3 + [66]
    assert plans(plan_check, blocks_case(hlen, B=4))[0][3] == [(0, 4), (4, 1), (5, 3), (8, 1)]


def test_blocks_mixed_lengths_cut_at_span(plan_check):
    # 100 .. 69 is a span of 31: the first 68 would make it kSegLens, so the block ends before it (7 queries, below the
    # cap of 8); the next run (68 .. 60, span 8) is cut by the cap
    hlen = [100] * 3 + [80] * 2 + [69] * 2 + [68] * 3 + [60] * 7
    assert plans(plan_check, blocks_case(hlen, B=8, mix=1))[0][3] == [(0, 7), (7, 8), (15, 2)]


def test_blocks_pack_halving_is_per_bin(plan_check):
    def lens(n):
        return [int(x) for x in np.linspace(70, 60, n).round()]
    hlen = lens(2500) + lens(2500) + lens(300)  # lengths restart at each bin boundary
    got = plans(plan_check, blocks_case(hlen, B=1024, mix=1, bin_s=[0, 2500, 5000, 5300], pack=1,
                                        ops=[(OVERFLOW, 0), (OVERFLOW, 4)]))
    assert got[0][1:] == (1024, 0, [(0, 1024), (1024, 1024), (2048, 1024), (3072, 1024), (4096, 1024), (5120, 180)])
    # block 0 (bin 0) overflowed: 512 until the end of bin 0 -- the block that starts in bin 0 may end in bin 1 --, B
    # again from the first block that starts in bin 1
    assert got[1][1:] == (512, 0, [(0, 1024), (1024, 512), (1536, 512), (2048, 512), (2560, 1024), (3584, 1024),
                                   (4608, 692)])
    # block 4 (bin 1) overflowed: halved from B (512, not 256: bin 0's size does not carry over), until the end of bin 1
    assert got[2][1:] == (512, 0, [(0, 1024), (1024, 512), (1536, 512), (2048, 512), (2560, 1024), (3584, 512),
                                   (4096, 512), (4608, 512), (5120, 180)])


def test_blocks_o4_trim_to_round_start(plan_check):
    # rounds of 3 from seqno 0: each cap-cut block of 4 is trimmed to the round start, which keeps 3 > 4 / 2
    assert plans(plan_check, blocks_case([70] * 11, B=4, o4_T=3))[0][3] == [(0, 3), (3, 3), (6, 3), (9, 2)]
    # block (1, 4) ends at 5, the round start before it is 3: trimming would keep 2, not more than half, so it stays;
    # block (5, 4) ends at a round start (9) as it is
    assert plans(plan_check, blocks_case([70] + [69] * 9, B=4, o4_T=3))[0][3] == [(0, 1), (1, 4), (5, 4), (9, 1)]
    # a pack counts the rounds from the bin's first seqno: bin 1 starts at 1, so 4 is a round start (counted from 0
    # the first block would be trimmed to 3), then 7 and 10
    got = plans(plan_check, blocks_case([70] * 12, B=4, o4_T=3, bin_s=[0, 1, 12], pack=1))
    assert got[0][3] == [(0, 4), (4, 3), (7, 3), (10, 2)]


def test_blocks_halving_floor(plan_check):
    got = plans(plan_check, blocks_case([70] * 10, B=2048, ops=[(HALVE, 0)] * 4))
    assert [(g[0], g[1]) for g in got] == [(0, 2048), (1, 1024), (1, 512), (1, 256), (0, 256)]


def test_blocks_start_from_hint(plan_check):
    got = plans(plan_check, blocks_case([70] * 1200, B=2048, b_hint=256))
    assert got[0][1:] == (512, 0, [(0, 512), (512, 512), (1024, 176)])
    # a pack ignores the hint
    got = plans(plan_check, blocks_case([70] * 1200, B=2048, b_hint=256, bin_s=[0, 600, 1200], pack=1))
    assert got[0][1:] == (2048, 0, [(0, 1200)])


def test_blocks_regrowth(plan_check):
    hlen = [70] * 2048
    eight = [(256 * i, 256) for i in range(8)]
    # two clean blocks double the size; passes 1 and 2 (D = 2) are queued, so the re-cut starts at block k + D = 3
    got = plans(plan_check, blocks_case(hlen, B=2048, regrow=2, b_hint=128,
                                        ops=[(RESOLVED, 0, 2, 0), (RESOLVED, 1, 2, K_PEER_CAP // 4 - 1)]))
    assert got[0][1:] == (256, 0, eight)
    assert got[1] == (0, 256, 1, eight)
    assert got[2] == (1, 512, 0, eight[:3] + [(768, 512), (1280, 512), (1792, 256)])
    # a block whose deepest peer list reaches kPeerCap / 4 resets the count: no two clean blocks in a row, no regrowth
    ops = [(RESOLVED, k, 2, 0 if k % 2 == 0 else K_PEER_CAP // 4) for k in range(6)]
    got = plans(plan_check, blocks_case(hlen, B=2048, regrow=2, b_hint=128, ops=ops))
    assert [g[:3] for g in got[1:]] == [(0, 256, 1), (0, 256, 0)] * 3
    assert all(g[3] == eight for g in got)
    # at the full block size, or with regrowth off, nothing happens (and nothing is counted)
    three = [(RESOLVED, k, 2, 0) for k in range(3)]
    got = plans(plan_check, blocks_case(hlen, B=256, regrow=2, ops=three))
    assert all(g == (0, 256, 0, eight) for g in got)
    got = plans(plan_check, blocks_case(hlen, B=2048, regrow=0, b_hint=128, ops=three))
    assert all(g == (0, 256, 0, eight) for g in got)
    # the last D blocks are all queued: nothing left to re-cut
    got = plans(plan_check, blocks_case(hlen, B=2048, regrow=2, b_hint=128,
                                        ops=[(RESOLVED, 5, 2, 0), (RESOLVED, 6, 2, 0)]))
    assert got[2] == (0, 256, 2, eight)


def _check_plan(blocks, hlen, s0, s1, cap, mix):
    pos = s0
    for first, n in blocks:
        assert first == pos and 1 <= n <= cap
        span = hlen[first:first + n]
        if mix:
            assert max(span) - min(span) < K_SEG_LENS
        else:
            assert max(span) == min(span)
        pos += n
    assert pos == s1


def test_blocks_random_plans_keep_the_invariants(plan_check):
    rng = np.random.default_rng(20240611)
    cases, meta = [], []
    for i in range(300):
        nbins = int(rng.choice([1, 1, 2, 3, 5]))
        pack = int(nbins > 1)
        sizes = rng.integers(1, max(2, 2000 // nbins), nbins)
        s0 = int(rng.integers(0, 50))  # the bins need not start at seqno 0
        bin_s = np.concatenate([[s0], s0 + np.cumsum(sizes)])
        hlen = list(rng.integers(32, 113, s0))
        for n in sizes:  # non-increasing per bin, over a narrow or a wide range of lengths
            lo = int(rng.integers(32, 113))
            hlen += sorted(rng.integers(lo, int(rng.integers(lo, 113)) + 1, n).tolist(), reverse=True)
        B = int(rng.choice([3, 64, 300, 512, 1024, 2048, 8192]))
        mix = int(rng.integers(0, 2))
        ops = []
        # block k overflows or resolves, k = 0, 1, ... as in the pipeline; a k past the last block re-cuts nothing
        # (overflowed and resolved touch only blocks that exist)
        for k in range(120):
            if rng.random() < 0.2:
                ops.append((OVERFLOW, k))
            else:
                ops.append((RESOLVED, k, 2, int(rng.choice([0, 10, 31, 32, 128]))))
        cases.append(blocks_case(hlen, B, mix=mix, o4_T=int(rng.choice([0, 0, 3, 25])), regrow=int(rng.integers(0, 4)),
                                 b_hint=int(rng.choice([BIG_HINT, 256, 700])), bin_s=bin_s.tolist(), pack=pack,
                                 bin0=int(rng.integers(0, 4)), ops=ops))
        meta.append((hlen, s0, int(bin_s[-1]), B, mix))
    for lines, (hlen, s0, s1, B, mix) in zip(plan_check("blocks", cases), meta):
        assert len(lines) == 121
        prev = None
        for k, line in enumerate(lines):
            ret, b_eff, clean, blocks = parse_plan(line)
            assert 1 <= b_eff <= B and clean >= 0
            _check_plan(blocks, hlen, s0, s1, B, mix)
            if prev is not None:  # op k - 1 re-cut only blocks after block k - 1
                assert blocks[:k] == prev[:k]
            prev = blocks


# ---- mode 2: number ----
def number_case(bin_s, cent, target, sort, pack, bin0=0):
    return [int(sort), int(pack), bin0, len(bin_s) - 1, *bin_s, len(cent), *cent, *target]


def parse_numbers(lines):
    out = {}
    for line in lines:
        name, *vals = line.split()
        out[name] = np.array(vals, dtype=np.int64)
    return out


def random_clustering(rng, bin_s, p_new):
    """cent (creation = seqno order) and target over [bin_s[0], bin_s[-1]): a bin's first read is a centroid, every
    later read a new centroid or a member of an earlier centroid of its bin"""
    cent, target = [], []
    for b in range(len(bin_s) - 1):
        mine = []
        for s in range(bin_s[b], bin_s[b + 1]):
            if not mine or rng.random() < p_new:
                mine.append(s)
                target.append(-1)
            else:
                target.append(mine[int(rng.integers(0, len(mine)) ** 2 // max(1, len(mine)))])  # early ones grow larger
        cent += mine
    return cent, target


def numpy_numbers(bin_s, cent, target, sort, pack, bin0):
    """the numbering restated: sizes by bincount, a stable argsort on (bin, -size), members in seqno order"""
    s0, s1 = bin_s[0], bin_s[-1]
    n, K = s1 - s0, len(cent)
    cent, target = np.array(cent, dtype=np.int64), np.array(target, dtype=np.int64)
    seq = np.arange(s0, s1)
    own = np.where(target < 0, seq, target)
    cno = np.searchsorted(cent, own)
    size = np.bincount(cno, minlength=K)
    sbin = np.searchsorted(np.array(bin_s[1:]), seq, side="right") if pack else np.zeros(n, dtype=np.int64)
    cbin = sbin[cent - s0] if K else np.zeros(0, dtype=np.int64)
    order = np.argsort(cbin * (n + 1) + (n - size), kind="stable") if sort else np.arange(K)
    rank_of = np.empty(K, dtype=np.int64)
    rank_of[order] = np.arange(K)
    ocl = rank_of[cno]
    ostart = np.concatenate([[0], np.cumsum(np.bincount(ocl, minlength=K))])
    omemb = seq[np.argsort(ocl, kind="stable")]
    nbins = len(bin_s) - 1
    bin_k = np.concatenate([[0], np.cumsum(np.bincount(cbin, minlength=nbins))]) if pack else np.array([0, K])
    if pack:
        ocl = ocl - bin_k[sbin]
    if K:
        assert (omemb[ostart[:-1]] == cent[order]).all()  # centroid first
    return dict(cno=cno, rank_of=rank_of, ocl=ocl, ostart=ostart, omemb=omemb, bin_k=bin_k)


def test_number_vs_numpy(plan_check):
    rng = np.random.default_rng(77)
    shapes = [([0, 400], 0), ([37, 437], 0), ([5, 5], 0), ([9, 10], 0),            # one bin; an empty range; n = 1
              ([0, 150, 151, 420], 1), ([11, 12, 300, 301], 1), ([3, 200, 390], 1)]  # packs, with one-read bins
    cases, want = [], []
    for bin_s, pack in shapes:
        for sort in (0, 1):
            for p_new in (0.05, 0.5):
                bin0 = int(rng.integers(0, 5))
                cent, target = random_clustering(rng, bin_s, p_new)
                cases.append(number_case(bin_s, cent, target, sort, pack, bin0))
                want.append(numpy_numbers(bin_s, cent, target, sort, pack, bin0))
    for lines, w in zip(plan_check("number", cases), want):
        got = parse_numbers(lines)
        for name in ("cno", "rank_of", "ocl", "ostart", "omemb", "bin_k"):
            assert np.array_equal(got[name], w[name]), name


def test_number_vs_oracle(plan_check):
    import orc
    from umiclust import synth
    seqs = synth.make_umis(40, seed=99, max_reads=300, orient_mix=0.2).as_list()
    p = orc.params(1, 0.93, 58, 68)
    assert p.clusterout_sort
    o = orc.cluster(p, seqs)
    srt = o["sorted"]  # sorted seqno -> input index
    n = len(srt)
    assert n > 200 and 1 < o["n_clusters"] < n
    cl, is_cent = o["cluster"][srt], o["centroid"][srt].astype(bool)
    cent = np.flatnonzero(is_cent)  # creation order = sorted seqno order
    cent_of = np.empty(o["n_clusters"], dtype=np.int64)
    cent_of[cl[cent]] = cent
    target = np.where(is_cent, -1, cent_of[cl])
    got = parse_numbers(plan_check("number", [number_case([0, n], cent.tolist(), target.tolist(), 1, 0)])[0])
    assert np.array_equal(got["ocl"], cl)
    assert np.array_equal(got["omemb"][got["ostart"][:-1]], cent[np.argsort(got["rank_of"])])


# ---- mode 3: trace ----
def trace_case(hlen, target, strand=None, lo=0, hi=None, x0=0):
    n = len(hlen)
    return [lo, n if hi is None else hi, x0, n, *hlen, *target, *(strand or [0] * n)]


def parse_trace(lines):
    out = {}
    for line in lines:
        name, *vals = line.split()
        out[name] = [int(v) for v in vals]
    out["maxl"] = out["maxl"][0]
    return out


def trace(plan_check, **kw):
    return parse_trace(plan_check("trace", [trace_case(**kw)])[0])


def test_trace_split_at_64(plan_check):
    # seqno 0 is the centroid; 64 is the last length of the first launch, 65 the first of the second; within a launch
    # the members keep their seqno order, and the first launch's slots come first
    got = trace(plan_check, hlen=[70, 65, 64, 112, 63, 1], target=[-1, 0, 0, 0, 0, 0], strand=[0, 1, 0, 0, 1, 1])
    assert got["tp"] == [0, 3, 2, 64, 112]
    assert got["slot"] == [-1, 3, 0, 4, 1, 2]
    assert got["pq"] == [2 << 1, (4 << 1) | 1, (5 << 1) | 1, (1 << 1) | 1, 3 << 1]
    assert got["pt"] == [0] * 5
    assert got["maxl"] == 112


def test_trace_empty_launches(plan_check):
    # every member short: the second launch is empty and its maxq stays 0 (launch_traceback sends nothing); maxl is
    # the centroid's length, longer than every query
    got = trace(plan_check, hlen=[100, 40, 33], target=[-1, 0, 0])
    assert (got["tp"], got["slot"], got["maxl"]) == ([0, 2, 0, 40, 0], [-1, 0, 1], 100)
    # every member long: the first launch is empty
    got = trace(plan_check, hlen=[66, 65, 65], target=[-1, 0, 0])
    assert (got["tp"], got["slot"], got["maxl"]) == ([0, 0, 2, 0, 65], [-1, 0, 1], 66)
    # centroids only, and no sequence at all (an empty range sizes the LDS for kMaxLen)
    got = trace(plan_check, hlen=[66, 65], target=[-1, -1])
    assert (got["tp"], got["slot"], got["pq"], got["maxl"]) == ([0, 0, 0, 0, 0], [-1, -1], [], 66)
    got = trace(plan_check, hlen=[], target=[])
    assert (got["tp"], got["slot"], got["maxl"]) == ([0, 0, 0, 0, 0], [], 112)


def test_trace_range_and_slot_offset(plan_check):
    # only the seqnos [lo, hi) are planned, slots count from x0, targets may lie outside the range, and maxl looks at
    # the range alone
    got = trace(plan_check, hlen=[112, 80, 70, 64, 30, 90], target=[-1, 0, -1, 2, 0, 0], strand=[0, 0, 0, 1, 0, 0],
                lo=1, hi=5, x0=7)
    assert got["tp"] == [7, 2, 1, 64, 80]
    assert got["slot"] == [9, -1, 7, 8]
    assert got["pq"] == [(3 << 1) | 1, 4 << 1, 1 << 1] and got["pt"] == [2, 0, 0]
    assert got["maxl"] == 80


def test_trace_random_plans_keep_the_invariants(plan_check):
    rng = np.random.default_rng(4242)
    cases, meta = [], []
    for _ in range(200):
        n = int(rng.integers(0, 60))
        hlen = rng.integers(1, 113, n).tolist()
        if n and rng.random() < 0.5:  # lengths at the split
            hlen = [int(rng.choice([63, 64, 65, 112, 1])) for _ in range(n)]
        target = [int(rng.integers(0, n)) if rng.random() < 0.7 else -1 for _ in range(n)]
        strand = rng.integers(0, 2, n).tolist()
        lo = int(rng.integers(0, n + 1))
        hi = int(rng.integers(lo, n + 1))
        x0 = int(rng.integers(0, 5))
        cases.append(trace_case(hlen, target, strand, lo, hi, x0))
        meta.append((hlen, target, strand, lo, hi, x0))
    for lines, (hlen, target, strand, lo, hi, x0) in zip(plan_check("trace", cases), meta):
        got = parse_trace(lines)
        mem = [s for s in range(lo, hi) if target[s] >= 0]
        short = [s for s in mem if hlen[s] <= 64]
        long_ = [s for s in mem if hlen[s] > 64]
        assert got["tp"] == [x0, len(short), len(long_), max([hlen[s] for s in short] + [0]),
                             max([hlen[s] for s in long_] + [0])]
        order = short + long_  # slot order
        assert got["slot"] == [x0 + order.index(s) if s in order else -1 for s in range(lo, hi)]
        assert got["pq"] == [(s << 1) | strand[s] for s in order] and got["pt"] == [target[s] for s in order]
        assert got["maxl"] == (max(hlen[lo:hi]) if hi > lo else 112)
