"""The pass reference checks itself (tests/pass_ref.py): its batched walk equals a batch-free restatement, the
restated relevance rule is not too narrow (every single peer that changes a walk when inserted as a centroid is in
the relevant set), and the generated cases have the properties tests/test_gpu_pass.py relies on to reach every path
of k_walk / k_peer_rel / k_peer_pairs / k_pack.  No GPU."""
import numpy as np
import pass_ref as R
import prefilter_ref as PR
import pytest


def _judged(c, qs):
    """(accept, rank, seqno) of the walked candidates of query-strand qs"""
    w = c["ref"]["walks"][qs]
    return [(*c["al"].judge(w["res"][x]), w["seq"][x]) for x in range(w["w"])]


def _first_accept(c, qs):
    j = [a for a, _, _ in _judged(c, qs)]
    return j.index(True) if True in j else None


def _all_qs(*names):
    for n in names:
        c = R.case(n)
        for qs in range(2 * c["nq"]):
            yield c, qs


@pytest.mark.parametrize("name", ["walk129", "tri9x2", "len32", "ambig9x2"])
def test_batched_walk_equals_batch_free_restatement(name):
    c = R.case(name)
    for qs, w in enumerate(c["ref"]["walks"]):
        q, strand = c["q0"] + qs // 2, qs % 2
        j = [c["al"].judge(c["al"].word(q, strand, t)) for t in w["seq"][:R.WALK]]
        got = R.walk_brute([a for a, _ in j], [(t, r) for t, (_, r) in zip(w["seq"], j)])
        assert got == (w["acc"], w["best_t"], w["w"]), qs
        assert w["e"] >= w["w"] and w["done"] == 1


@pytest.mark.parametrize("name", ["walk129", "crowd129", "tri9x2", "one1x2", "len32", "ambig9x2"])
def test_single_peer_insertions_stay_inside_the_relevant_set(name):
    c = R.case(name)
    bad = R.single_peer_failures(c["pool"], c["al"], c["ref"], c["q0"], c["nq"], c["nprev"])
    assert not bad, bad[:5]


def test_rank_table_is_dense_and_orders_identities():
    acc, rank = R.tables(0.93)
    assert rank[0, 0] == 0 and rank[64, 64] == rank[112, 112] > rank[112, 111] > rank[64, 63]
    assert rank[1, 112] == rank.max()  # the table ranks m > L too (never accepted)
    assert rank[64, 60] == rank[32, 30] and rank[64, 61] > rank[64, 60] > rank[66, 61]
    assert acc[64, 60] and not acc[66, 61] and not acc[0, 0] and not acc[10, 11]
    assert len(np.unique(rank)) == rank.max() + 1


def test_pools_are_in_vsearch_order_and_small():
    for name in R.CASES:
        c = R.case(name)
        assert np.all(np.diff(c["pool"].lens) <= 0) and len(c["pool"]) < 1500 and c["nq"] <= 130
        assert len(c["cent"]) == 0 or c["cent"][-1] < c["q0"] - c["nprev"] * c["nq"]
        assert c["q0"] + c["nq"] == len(c["pool"])


def test_walk_case_realises_every_hit_position():
    """the first accept at list index 0, 7, 8, 15, 16 and 31; 32 decoys in a list of 41: w = 32 and no accept"""
    c = R.case("walk129")
    firsts = {_first_accept(c, qs) for qs in range(2 * c["nq"])}
    assert {0, 7, 8, 15, 16, 31} <= firsts
    W = c["ref"]["walks"]
    assert any(w["nt"] == 41 and w["w"] == 32 and not w["acc"] and w["best_t"] == R.NONE for w in W)
    for n, d in (("D0", 0), ("D7", 7), ("D8", 8), ("D15", 15), ("D16", 16), ("D31", 31)):
        qs = 2 * (c["pivots"][n] - c["q0"])
        assert _first_accept(c, qs) == d and W[qs]["w"] == min(W[qs]["nt"], 8 * (d // 8 + 1)), n
    assert {w["w"] for w in W} >= {0, 1, 7, 8, 16, 32}


def test_walk_case_realises_every_list_length():
    c = R.case("walk129")
    assert {0, 1, 7, 8, 9, 32, 41} <= {int(x) for x in c["lists"]["ntop"]}


def test_top_count_threshold_sits_between_29_and_30():
    """a top count of 29 emits the whole list at once, one of 30 only the first batch"""
    W = R.case("walk129")["ref"]["walks"]
    a = [w for w in W if w["nt"] > 8 and w["cnt"][0] == 29]
    b = [w for w in W if w["nt"] > 8 and w["cnt"][0] == 30]
    assert a and b
    assert all(w["e"] == min(w["nt"], 32) for w in a)
    assert any(w["e"] == 8 and w["s0"]["done"] for w in b)  # accepted in the first batch: the rest never emitted
    assert all(w["s0"]["w"] == 8 for w in b)


def test_best_hit_selection_cases():
    two_ranks = tie_bites = tie_first = minus = False
    for c, qs in _all_qs("walk129", "crowd129", "len32"):
        w = c["ref"]["walks"][qs]
        j = _judged(c, qs)
        hits = [(r, t) for a, r, t in j if a]
        if len(hits) >= 2:
            two_ranks |= len({r for r, _ in hits}) >= 2 and hits[0][0] != max(r for r, _ in hits)
            best = [t for r, t in hits if r == w["best_rank"]]
            tie_bites |= len(best) >= 2 and best[0] != min(best)  # the first listed is not the smallest seqno
            tie_first |= len(best) >= 2 and best[-1] != min(best)  # nor is the last listed
            assert w["best_rank"] == max(r for r, _ in hits) and w["best_t"] == min(best)
        minus |= qs % 2 == 1 and bool(w["acc"])
    assert two_ranks and tie_bites and tie_first and minus


def test_peer_counts_cover_every_range():
    np_ = np.concatenate([R.case(n)["lists"]["npeer"] for n in ("walk129", "crowd129")])
    assert (np_ == 0).any() and ((np_ >= 1) & (np_ <= 64)).sum() >= 5 and ((np_ >= 65) & (np_ <= 128)).sum() >= 5
    assert (np_ == 128).any() and (np_ == 255).sum() >= 3
    nrel = [h["nrel"] for n in ("walk129", "crowd129") for h in R.case(n)["ref"]["hostqs"]]
    assert sum(0 < x <= 6 for x in nrel) >= 5 and sum(x > 6 for x in nrel) >= 5 and max(nrel) > 64
    assert any(h["npeer"] == 255 and h["nrel"] == 0 and h["flags"] & 2 for h in R.case("crowd129")["ref"]["hostqs"])


def test_closed_walks_have_relevant_and_irrelevant_peers_and_both_ties():
    mixed = shorter = same = 0
    for c, qs in _all_qs("walk129", "crowd129"):
        r, w = c["ref"], c["ref"]["walks"][qs]
        if R.is_open(w) or not r["rel"][qs]:
            continue
        mixed += any(r["rel"][qs]) and not all(r["rel"][qs])
        ids, cnts = c["lists"]["peers"][qs]
        w0 = c["q0"] - c["nprev"] * c["nq"]
        lc, ll = -w["last"][0], w["last"][1]
        for i, k, rel in zip(ids, cnts, r["rel"][qs]):
            if k == lc and c["pool"].lens[w0 + i] < ll:
                assert rel
                shorter += 1
            if k == lc and c["pool"].lens[w0 + i] == ll:
                assert not rel  # a peer's seqno is past every centroid's
                same += 1
    assert mixed >= 5 and shorter >= 1 and same >= 1


def test_late_family_has_its_relevant_peers_past_position_64():
    c = R.case("crowd129")
    qs = 2 * (c["pivots"]["late"] - c["q0"])
    rel = c["ref"]["rel"][qs]
    assert len(rel) > 64 and 0 < sum(rel) <= 6 and not any(rel[:64])
    assert not R.is_open(c["ref"]["walks"][qs])


def test_member_expectation_cases():
    first = later = prevexp = widened = 0
    for c, qs in _all_qs("walk129", "crowd129"):
        r, q0, nq, w0 = c["ref"], c["q0"], c["nq"], c["q0"] - c["nprev"] * c["nq"]
        W = r["walks"]
        if int(c["lists"]["npeer"][qs]) in (0, 255):
            continue
        for i, rel0, al, rel in zip(c["lists"]["peers"][qs][0], r["rel0"][qs], r["aligned"][qs], r["rel"][qs]):
            ps = w0 + int(i)
            if ps >= q0:
                s0 = any(W[2 * (ps - q0) + s]["s0"]["acc"] for s in range(2))
                fin = any(W[2 * (ps - q0) + s]["acc"] for s in range(2))
                first += rel0 and s0 and not al       # accepted in its first batch: not aligned
                later += rel0 and fin and not s0 and al  # accepted only later: aligned
            else:
                prevexp += rel0 and not al            # a previous-block peer whose final walk accepted
            widened += al and not rel                 # relevant under S0 only
            assert rel0 or not al                     # aligned implies relevant under S0
            assert rel0 or not rel                    # the final relevant set is inside S0's
    assert first >= 5 and later >= 5 and prevexp >= 5 and widened >= 5
    r = R.case("crowd129")["ref"]
    # without the previous block's pass those peers are aligned
    n = R.case("crowd129_noprev")["ref"]
    assert n["counters"][8] > r["counters"][8] and n["total"] == r["total"]
    assert [h for h in n["hostqs"]] == [h for h in r["hostqs"]]


@pytest.mark.parametrize("name", ["tri9x2", "one1x2"])
def test_a_peer_two_blocks_back_is_never_expected(name):
    c = R.case(name)
    r, q0, nq = c["ref"], c["q0"], c["nq"]
    w0 = q0 - 2 * nq
    far = R.block_walks(c["pool"], c["al"], PR.prefilter_ref(c["pool"], c["cent"], w0, nq, 0), w0, nq)
    hit = 0
    for qs in range(2 * nq):
        if int(c["lists"]["npeer"][qs]) in (0, 255):
            continue
        for i, al in zip(c["lists"]["peers"][qs][0], r["aligned"][qs]):
            if int(i) < nq and any(far[2 * int(i) + s]["acc"] for s in range(2)):
                assert al  # every walk of these cases is open: all peers are relevant
                hit += 1
    assert hit >= 1
    assert any(not al for qs in range(2 * nq) for al in r["aligned"][qs])  # previous block / in-block: expected


def test_lazy_peers_align_nothing_and_keep_the_records():
    a, b = R.case("crowd129")["ref"], R.case("crowd129_lazy")["ref"]
    assert b["counters"][8] == 0 and b["counters"][14] == 0 and all(m == [0, 0] for m in b["masks"])
    assert b["total"] == a["total"] > 0 and b["counters"][12] == a["counters"][12]
    assert [x is None for x in a["records"]] == [x is None for x in b["records"]]


def test_shapes():
    assert {R.case(n)["nq"] for n in R.CASES} >= {1, 9, 32, 129}
    c = R.case("len32")
    assert list(c["pool"].lens[c["q0"]:]) == list(range(112, 80, -1))
    assert sum(w["nt"] > 0 for w in c["ref"]["walks"]) >= 16 and c["ref"]["counters"][8] > 0
    c = R.case("tri9x2")
    assert sorted(set(c["pool"].lens[c["q0"]:])) == [62, 63, 64]
    c = R.case("ambig9x2")
    assert sum("N" in s for s in c["pool"].seqs) >= 10 and c["ref"]["counters"][8] > 0


def test_records_are_sized_as_their_layout_says():
    for name in R.CASES:
        r = R.case(name)["ref"]
        for h, rec in zip(r["hostqs"], r["records"]):
            assert (rec is not None) == h["has_rec"] == (h["nrel"] > 0)
            if rec is not None:
                nt, np_ = rec[0] & 0xff, rec[0] >> 8
                assert len(rec) == 1 + 2 * nt + (nt + 3) // 4 + 2 * np_ and np_ == h["npeer"] and nt <= 32
