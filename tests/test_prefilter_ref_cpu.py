"""The prefilter reference checks itself (tests/prefilter_ref.py): the vectorised lists equal plain set
intersections, and the generated input families have the properties tests/test_gpu_prefilter.py relies on to reach
every selection path of k_pf_count / k_pf_full / k_pf_merge.  No GPU."""
import numpy as np
import prefilter_ref as R
import pytest


@pytest.mark.parametrize("name", ["peers60x2", "peers90x1", "low", "max", "tiny9"])
def test_vectorised_equals_brute_force(name):
    c = R.case(name)
    p, r = c["pool"], c["ref"]
    if name == "tiny9":  # a few hundred sequences of the big pool: the 9 centroids and the window
        cent, q0 = np.arange(9), 9
        seqs = [p.seqs[i] for i in c["cent"]] + p.seqs[c["q0"]:c["q0"] + c["nq"]]
        back = np.concatenate([c["cent"], np.arange(c["q0"], c["q0"] + c["nq"])])
    else:
        cent, q0, seqs, back = c["cent"], c["q0"], p.seqs, np.arange(len(p))
    b = R.prefilter_brute(seqs, list(cent), q0, c["nq"], c["nprev"])
    assert list(r["ntop"]) == b["ntop"] and list(r["npeer"]) == b["npeer"]
    for qs in range(len(b["ntop"])):
        n = b["ntop"][qs]
        assert [(int(back[s]), k) for s, k in b["tops"][qs]] == list(zip(r["top_seqno"][qs, :n], r["top_count"][qs, :n])), qs
        if b["peers"][qs] is None:
            assert r["peers"][qs] is None
        else:
            assert b["peers"][qs] == list(zip(*r["peers"][qs])), qs


def test_pools_are_in_vsearch_order_and_blocks_fit():
    for name in R.CASES:
        c = R.case(name)
        p = c["pool"]
        assert np.all(np.diff(p.lens) <= 0)
        blk = p.lens[c["q0"]:c["q0"] + c["nq"]]
        assert blk.max() - blk.min() + 1 <= 32  # kSegLens: the lengths one greedy block may span
        assert p.lens.min() >= 32 and p.lens.max() <= 112


def test_tiny_cases_cover_every_part_boundary():
    for n in (0, 1, 7, 8, 9):
        r = R.case(f"tiny{n}")["ref"]
        assert r["ntop"].max() <= n and r["units"].sum() == 0
    assert R.case("tiny9")["ref"]["ntop"].max() == 9 and R.case("tiny9")["ref"]["part_max"].max() == 2
    assert R.case("tiny8")["ref"]["ntop"].max() == 8 and R.case("tiny8")["ref"]["part_max"].max() == 1


def test_part_cap_pair_sits_on_the_threshold():
    a, b = R.case("cap512")["ref"], R.case("cap520")["ref"]
    assert a["part_max"].max() == R.PART_CAND and a["units"].sum() == 0
    assert b["part_max"].max() == R.PART_CAND + 1 and b["units"].sum() > 0
    m = R.case("cap516")["ref"]  # overflowing parts beside exactly full ones
    assert m["part_max"].max() == R.PART_CAND + 1 and (m["units"] == 4).sum() >= 32 and m["units"].max() == 4


def test_rank_bitonic_scan_cases_cross_their_thresholds():
    r = R.case("rank4096")["ref"]
    assert r["part_max"].max() == R.RANK_SEL and r["units"].sum() > 0  # rank selection at its largest size
    for name, thr in (("bitonic4200", R.RANK_SEL), ("scan9000", R.PF_CAND), ("lsm20000", R.PF_CAND),
                      ("sealed66000", R.PF_CAND)):
        r = R.case(name)["ref"]
        plus = r["part_max"][0::2]  # one per query
        assert (plus > thr).sum() * 2 >= len(plus), name
    assert R.case("bitonic4200")["ref"]["part_max"].max() <= R.PF_CAND  # bitonic, not yet the chunked scan


def test_shared_core_lists_are_tied_and_have_near_misses():
    for name in ("cap520", "scan9000", "sealed66000"):
        r = R.case(name)["ref"]
        full = r["top_count"][r["ntop"] == R.TOP]
        assert len(full) >= 32
        # the cut at 41 falls inside a run of equal counts for most lists: the tie-break decides who is kept
        assert (r["ncand"][r["ntop"] == R.TOP] > 2 * R.TOP).all()
        assert (full[:, 0] > full[:, -1]).any() and (full[:, 1:] == full[:, :-1]).sum() > full.shape[0] * 10
    # short cores: short lists beside full ones (a core under 19 nt reaches 12 shared 8-mers only through its flanks)
    r = R.case("cap520")["ref"]
    assert ((r["ntop"][0::2] > 0) & (r["ntop"][0::2] < R.TOP)).sum() >= 1


def test_low_complexity_case_has_every_threshold_kind():
    r = R.case("low")["ref"]
    assert (r["nk"] == 0).sum() >= 5 and ((r["nk"] > 0) & (r["nk"] < 12)).sum() >= 5 and (r["nk"] >= 12).sum() >= 5
    assert np.array_equal(r["thr"], np.minimum(r["nk"], 12))
    zero = r["nk"] == 0
    assert (r["ntop"][zero] == R.TOP).all() and (r["top_count"][zero] == 0).all()  # every centroid is a candidate
    assert r["units"].sum() >= 8 * zero.sum()
    some = (r["nk"] > 0) & (r["nk"] < 12)
    assert (r["ntop"][some] > 0).sum() >= 5  # thr = nk candidates exist


def test_max_count_case_reaches_105_on_both_strands():
    r = R.case("max")["ref"]
    assert r["top_count"].max() == 105
    assert (r["top_count"][0::2, 0] == 105).any() and (r["top_count"][1::2, 0] == 105).any()


def test_peer_cases_straddle_the_cap():
    for name in ("peers60x2", "peers90x1", "peers200"):
        r = R.case(name)["ref"]
        assert (r["npeer"] == 255).sum() >= 5 and ((r["npeer"] > 64) & (r["npeer"] <= R.PEER_CAP)).sum() >= 5, name
        assert (r["npeer_all"] == R.PEER_CAP).any() and (r["npeer_all"] == R.PEER_CAP + 1).any(), name


def test_control_never_overflows():
    r = R.case("control")["ref"]
    assert r["units"].sum() == 0 and (r["npeer"] != 255).all() and (r["ntop"] > 0).any()


# ---------------------------------------------------------------- split passes
def _same_lists(r, b, qs_n):
    assert list(r["ntop"]) == b["ntop"] and list(r["npeer"]) == b["npeer"]
    for qs in range(qs_n):
        n = b["ntop"][qs]
        assert b["tops"][qs] == list(zip(r["top_seqno"][qs, :n], r["top_count"][qs, :n])), qs
        assert (b["peers"][qs] is None and r["peers"][qs] is None) or b["peers"][qs] == list(zip(*r["peers"][qs])), qs


@pytest.mark.parametrize("name", ["split_some", "split_none", "split_all", "split_low", "split_peers"])
def test_split_reference_equals_brute_force_and_whole_pass(name):
    """prefilter_split_ref against plain set intersections, units included, and the invariant: its lists are those of
    a whole pass over cent and newcent together with the two newer blocks as the window."""
    c = R.split_case(name)
    p, r, nq = c["pool"], c["ref"], c["nq"]
    b = R.prefilter_brute(p.seqs, list(c["cent"]), c["w0"] + 2 * nq, nq, 2, newcent=list(c["newcent"]))
    _same_lists(r, b, 2 * nq)
    assert list(r["units"]) == b["units"]
    w = R.prefilter_ref(p, sorted(set(c["cent"]) | set(c["newcent"])), c["w0"] + 2 * nq, nq, nprev=1)
    for k in ("ntop", "top_seqno", "top_count", "npeer"):
        assert np.array_equal(r[k], w[k]), k
    for a, bb in zip(r["peers"], w["peers"]):
        assert (a is None and bb is None) or (np.array_equal(a[0], bb[0]) and np.array_equal(a[1], bb[1]))


def test_split_cases_reach_their_paths():
    some, none, all_ = (R.split_case(n)["ref"] for n in ("split_some", "split_none", "split_all"))
    # a kept flagged hit tied with an indexed centroid inside a top list; a flagged hit over the threshold dropped
    assert some["tied_kept"].sum() >= 10 and some["flag_dropped"].sum() > 0 and some["flag_kept"].sum() > 0
    assert none["flag_kept"].sum() == 0 and none["flag_dropped"].sum() > 0
    assert all_["flag_dropped"].sum() == 0 and all_["flag_kept"].sum() > 0
    for r in (some, none, all_):
        assert r["units"].sum() == 0
    c64, c65 = R.split_case("split_cap64")["ref"], R.split_case("split_cap65")["ref"]
    assert c64["part_sum"].max() == R.PART_CAND and c64["units"].sum() == 0
    assert c65["part_sum"].max() == R.PART_CAND + 1 and c65["cent_part_max"].max() <= R.PART_CAND
    assert (c65["units"] == 4).sum() >= 32 and c65["units"].max() == 4  # parts at 65 beside parts at exactly 64
    f = R.split_case("split_fold")
    assert len(f["cent"]) == 8100 and len(f["newcent"]) >= 100 and len(f["cent"]) <= 8192 < len(f["cent"]) + len(f["newcent"])
    low = R.split_case("split_low")
    r = low["ref"]
    assert (r["thr"] == 0).sum() >= 5 and ((r["thr"] > 0) & (r["thr"] < 12)).sum() >= 5
    zero = r["thr"] == 0
    assert (r["flag_kept"][zero] + r["flag_dropped"][zero] == low["nq"]).all() and (r["units"][zero] == 8).all()
    pe = R.split_case("split_peers")["ref"]
    assert (pe["npeer"] == R.PEER_CAP).any() and (pe["npeer"] == 255).any()
    assert (pe["npeer_all"] == R.PEER_CAP).any() and (pe["npeer_all"] == R.PEER_CAP + 1).any()
    for name in R.SPLIT_CASES:
        c = R.split_case(name)
        blk = c["pool"].lens[c["w0"] + 2 * c["nq"]:c["w0"] + 3 * c["nq"]]
        assert blk.max() - blk.min() + 1 <= 32 and (len(c["cent"]) == 0 or c["cent"][-1] < c["w0"])


# ---------------------------------------------------------------- packs
def test_bin_mask_and_noise_construction():
    assert [len(R.kmer_set(s)) for s in R.noise_queries()] == [1, 2, 3]
    assert [len(R.kmer_set(s, True)) for s in R.noise_queries()] == [1, 2, 3]
    assert len({R.bin_mask(b) for b in range(64)}) == 64 and all(0 <= R.bin_mask(b) < 65536 for b in range(64))
    assert R.kmer_text(R.kmer_set("ACGTTGCA")[0]) == "ACGTTGCA"
    p = R.pool("pack")
    s1, s2 = int(p.bin_s[1]), int(p.bin_s[2])
    want = {v ^ R.bin_mask(2) ^ R.bin_mask(1) for v in R.kmer_set(R.noise_queries()[2])}
    for x in range(s1, s2):  # every collider carries all three built 8-mers, unmasked
        assert want <= set(p.kp[x, :p.nk[x]].tolist()), x


@pytest.mark.parametrize("name", ["pack_ord9", "pack_ord136", "pack_win5", "pack_win40"])
def test_pack_reference_equals_brute_force(name):
    c = R.pack_case(name)
    p, r = c["pool"], c["ref"]
    b = R.prefilter_brute(p.seqs, list(c["cent"]), c["q0"], c["nq"], c["nprev"], bin_start=[int(x) for x in p.bin_s])
    _same_lists(r, b, 2 * c["nq"])
    assert list(r["units"]) == b["units"]


def test_pack_cases_reach_their_paths():
    p = R.pool("pack")
    s2 = int(p.bin_s[2])
    for k in R.PACK_ORD0:  # pack_boundaries: the second bin's first centroid ordinal
        c = R.pack_case(f"pack_ord{k}")
        assert int(np.searchsorted(c["cent"], s2)) == k and c["cent"][k] == s2
    # pack_cmin of a part: the first counter of the later bin, ceil((ord0 - part) / 8) -- every byte of a counter
    # word, every word of a uint4 (the third one through ordinal 72), and the sweep starting in a later uint4
    cmin = {max(0, -(-(k - part) // 8)) for k in R.PACK_ORD0 for part in range(8)}
    assert {k % 8 for k in R.PACK_ORD0} >= {0, 1, 7} and {m % 4 for m in cmin} == {0, 1, 2, 3}
    assert {(m // 4) % 4 for m in cmin} == {0, 1, 2, 3} and {m // 16 for m in cmin} == {0, 1}
    ds = [s2 - (R.pack_case(f"pack_win{d}")["q0"] - R.PACK_NQ) for d in range(1, 64)]
    assert ds == list(range(1, 64)) and {d % 32 for d in ds if d <= 32} == set(range(32))
    assert {d % 32 for d in ds if d > 32} >= set(range(1, 32))
    assert any(R.pack_case(f"pack_win{d}")["q0"] < s2 for d in ds)  # a block across the bin boundary
    # pack_thr0: more cross-bin than own-bin would-be candidates for the thr = 0 queries
    c = R.pack_case("pack_ord136")
    r, w = c["ref"], c["would"]
    zero = r["thr"] == 0
    assert zero.sum() >= 4 and (w["cross_cent"][zero] > w["own_cent"][zero]).all()
    assert (r["ntop"][zero] == R.PACK_CENT2).all() and (r["top_seqno"][zero, :R.PACK_CENT2] >= s2).all()
    # pack_noise: thr = nk = 1..3 queries whose scrambled 8-mers the earlier bin carries
    some = (r["thr"] > 0) & (r["thr"] <= 3)
    assert set(r["thr"][some]) == {1, 2, 3}
    assert w["cross_cent"][some].sum() >= 20 and (r["ncand"][some] == w["own_cent"][some]).all()
    c5 = R.pack_case("pack_win5")
    some5 = (c5["ref"]["thr"] > 0) & (c5["ref"]["thr"] <= 3)
    assert c5["would"]["cross_peer"][some5].sum() >= 5
    for cc in (c, c5):
        n = cc["ref"]["ntop"]
        assert (cc["ref"]["top_seqno"][np.arange(41)[None, :] < n[:, None]] >= s2).all()
        for qs, pr in enumerate(cc["ref"]["peers"]):
            assert pr is None or (pr[0] + (cc["q0"] - cc["nq"]) >= s2).all(), qs
        assert (cc["ref"]["npeer_all"] == cc["would"]["own_peer"]).all()


def test_pack_lengths_case_orders_by_true_length():
    c = R.pack_case("pack_lengths")
    p, r, cent = c["pool"], c["ref"], c["cent"]
    s1, s2 = int(p.bin_s[1]), int(p.bin_s[2])
    assert p.lens[s1:s2].max() <= 60 and p.lens[s2:].min() >= 64  # lengths rise with the ordinal
    assert int(np.searchsorted(cent, s2)) >= 8 * R.TOP          # the lookup is off by more than a part keeps
    plus = np.arange(0, 2 * c["nq"], 2)
    assert (r["units"][plus] == 8).all() and r["part_max"].max() > R.PART_CAND
    # the best counts are tied deeper than a part's 41 in every part: length alone decides who is kept
    for qs in plus:
        cnt = p.counts(p.query_kmers(c["q0"] + qs // 2, 0), cent)
        top = np.nonzero((cnt == r["top_count"][qs, R.TOP - 1]) & (cent >= s2))[0]
        assert np.bincount(top % 8, minlength=8).min() > R.TOP, qs
    # the two steps the kernels take (a part's best 41 by the full kernel's length, the merge by the true length):
    # with the true lengths they give the expected lists, with lengths looked up from the ordinal every plus-strand
    # list differs
    want = [r["top_seqno"][qs, :r["ntop"][qs]] for qs in range(2 * c["nq"])]
    true = R.two_step_tops(p, cent, c["q0"], c["nq"], r, p.lens[cent])
    mono = R.two_step_tops(p, cent, c["q0"], c["nq"], r, R.monotone_lengths(p, cent))
    assert all(np.array_equal(a, b) for a, b in zip(true, want))
    assert all(not np.array_equal(mono[qs], want[qs]) for qs in plus)


# ---------------------------------------------------------------- two counter segments
def test_segment_case_ties_across_the_segments():
    c = R.segment_case()
    p, r = c["pool"], c["ref"]
    assert len(c["cent"]) > R.SEG_CENT and len(c["cent"]) <= 2 * R.SEG_CENT and c["nq"] == 8
    assert np.all(p.lens == 64) and p.seqs[-1] in R.LOW_SPECIALS and (r["thr"][-2:] == 0).all()
    good = 0
    for qs in range(16):
        n = r["ntop"][qs]
        ts, tc = r["top_seqno"][qs, :n], r["top_count"][qs, :n]
        lo, hi = ts < R.SEG_CENT, ts >= R.SEG_CENT
        good += r["ncand"][qs] > R.TOP and lo.sum() >= 10 and hi.sum() >= 10 and len(np.intersect1d(tc[lo], tc[hi])) > 0
    assert good >= 3
    # the numpy k-mers of the filler against the oracle's DUST and extraction
    for i in np.random.default_rng(3).integers(0, len(p), 1000):
        k = R.kmer_set(p.seqs[i])
        assert p.nk[i] == len(k) and p.kp[i, :len(k)].tolist() == k, i
