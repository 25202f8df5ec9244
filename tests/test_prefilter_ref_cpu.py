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
