"""The pipeline's resolve step on the device side (pass.cpp resolve_pass: resolve_block on a real pass's outcomes and
records, round B on the copy stream) against the plain greedy reference of tests/resolve_ref.py: umiclust_resolve
queues the pass of a chosen block as umiclust_pass does and resolves it with the window's states as given.
Membership, target, strand, new centroids, alignments and cells are compared exactly, no query left out.  The same
cases run through resolve_block on the CPU in tests/test_resolve_cpu.py, where every round-B pair is visible; here
round B's pairs are counted on the device side and held between what the reference's walk needs and what the records
leave open, its trips between one and one more than the block's new centroids."""
import numpy as np
import orc
import pass_ref as R
import pytest
import resolve_ref as RR
from umiclust import _lib, synth

pytestmark = pytest.mark.gpu

K_RB_DIRECT = 4096  # cluster_ctx.h kRbDirect: more pairs go through device buffers


def _loaded(ctx, pool):
    ctx.load(_lib.params(1, 0.93, int(pool.lens.min()), int(pool.lens.max())), pool.seqs)
    return ctx


def _run(ctx, name, partial=True):
    c = RR.real_case(name)
    g = _loaded(ctx, c["pool"]).run_resolve(c["cent"], c["q0"], c["nq"], c["nprev"], c["state_in"], lazy=c["lazy"],
                                            prev=c["prev"], partial=partial)
    return c, g


def _differences(c, g) -> list[str]:
    """the block's first k queries against the reference; nothing written past them"""
    r, k, bad = c["g"], c["k"], []
    if g["resolved"] != k or g["all"] != (k == c["nq"]):
        bad.append(f"resolved {g['resolved']} (all: {g['all']}), expected {k} of {c['nq']}")
    for i in range(k):
        got = (int(g["state"][i]), int(g["target"][i]), int(g["strand"][i]) if g["state"][i] == RR.MEMBER else 0)
        if got != (r["state"][i], r["target"][i], r["strand"][i]):
            bad.append(f"query {c['q0'] + i}: state, target, strand {got} vs "
                       f"{(r['state'][i], r['target'][i], r['strand'][i])}")
    for i in range(k, c["nq"]):
        if g["state"][i] != RR.UNDET or g["target"][i] != -1:
            bad.append(f"query {c['q0'] + i} past the resolved prefix: state {g['state'][i]}, target {g['target'][i]}")
    if g["new_cents"].tolist() != r["new_cents"]:
        bad.append(f"new centroids {g['new_cents'].tolist()} vs {r['new_cents']}")
    if (g["n_alignments"], g["cells"]) != (r["n_alignments"], r["cells"]):
        bad.append(f"alignments, cells {(g['n_alignments'], g['cells'])} vs {(r['n_alignments'], r['cells'])}")
    return bad


def _round_b_bad(c, g) -> list[str]:
    need, most, bad = len(RR.needed_pairs(c)), RR.most_pairs(c), []
    if g["rb_pairs"] != g["pairs_round_b"]:
        bad.append(f"round B aligned {g['rb_pairs']} pairs, the resolve step asked for {g['pairs_round_b']}")
    if not need <= g["rb_pairs"] <= most:
        bad.append(f"round B aligned {g['rb_pairs']} pairs; the reference's walk needs {need}, the records leave {most}")
    # a trip past the first waits for a deferred query that turned out a centroid
    if not (1 if g["rb_pairs"] else 0) <= g["rb_trips"] <= (1 + len(c["g"]["new_cents"]) if g["rb_pairs"] else 0):
        bad.append(f"{g['rb_trips']} round-B trips for {g['rb_pairs']} pairs, {len(c['g']['new_cents'])} new centroids")
    return bad


@pytest.mark.parametrize("name", list(R.CASES) + ["ambig9x2_lazy"])
def test_resolve_equals_reference(name, gpu_ctx):
    """every case of the pass test (the blocks with an overflowing peer list up to their first such query), and the
    ambiguity case with lazy peers: round B on the general aligner"""
    c, g = _run(gpu_ctx, name)
    assert g["both"] == 2
    bad = _differences(c, g) + _round_b_bad(c, g)
    assert not bad, f"{len(bad)} differences:\n" + "\n".join(bad[:12])
    if c["lazy"]:
        assert g["rb_pairs"] > 0 and g["n_deferred"] > 0


@pytest.mark.parametrize("name,staged", [("staged_big", True), ("staged_small", False)])
def test_round_b_direct_and_staged(name, staged, gpu_ctx):
    """one block with a round-B trip of more than kRbDirect pairs (device buffers and copies) and its twin, whose
    trips all stay below (pinned memory)"""
    c, g = _run(gpu_ctx, name)
    bad = _differences(c, g) + _round_b_bad(c, g)
    assert not bad, f"{len(bad)} differences:\n" + "\n".join(bad[:12])
    assert (g["rb_staged"] >= 1) == staged and (g["rb_pairs"] > K_RB_DIRECT) == staged


def test_round_b_launches_once_per_query_length(gpu_ctx):
    c, g = _run(gpu_ctx, "tri9x2_lazy")
    assert sorted(set(c["pool"].lens[c["q0"]:])) == [62, 63, 64]
    bad = _differences(c, g) + _round_b_bad(c, g)
    assert not bad, bad[:12]
    assert g["rb_launches"] >= 3 and g["rb_trips"] == 1


def test_banded_and_packed_round_b_agree(monkeypatch):
    """UMICLUST_BAND is read by umiclust_create: one context per value"""
    c = RR.real_case("crowd129_lazy")
    out = {}
    for band in ("0", None):
        if band is None:
            monkeypatch.delenv("UMICLUST_BAND", raising=False)
        else:
            monkeypatch.setenv("UMICLUST_BAND", band)
        with _lib.Context(0) as ctx:
            _, g = _run(ctx, "crowd129_lazy")
        bad = _differences(c, g) + _round_b_bad(c, g)
        assert not bad, (band, bad[:12])
        out[band] = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in g.items()}
    assert out["0"] == out[None]


def test_partial_resolution(gpu_ctx):
    c, g = _run(gpu_ctx, "crowd129")
    assert 0 < c["k"] < c["nq"] and g["resolved"] == c["k"] and not g["all"]
    assert not _differences(c, g)
    _, g = _run(gpu_ctx, "crowd129", partial=False)  # without the flag nothing is written
    assert g["resolved"] == 0 and not g["all"] and not g["state"].any() and (g["target"] == -1).all()
    assert len(g["new_cents"]) == 0
    for partial in (True, False):  # query 0 overflows: nothing resolves, no state changes
        c, g = _run(gpu_ctx, "overflow0", partial=partial)
        assert c["k"] == 0 and c["ref"]["hostqs"][0]["npeer"] == 255
        assert g["resolved"] == 0 and not g["all"] and not g["state"].any() and (g["target"] == -1).all()


def test_context_state(gpu_ctx):
    """A, B, A on one context give equal results; the context stays loaded and not clustered"""
    key = lambda g: {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in g.items()}  # noqa: E731
    _, a1 = _run(gpu_ctx, "crowd129_lazy")
    _, b = _run(gpu_ctx, "walk129")
    _, a2 = _run(gpu_ctx, "crowd129_lazy")
    assert key(a1) == key(a2) and key(b) != key(a1)
    seqs = synth.make_umis(60, seed=1, max_reads=800).as_list()
    gpu_ctx.load(_lib.params(1, 0.93, 58, 68), seqs)
    gpu_ctx.cluster()
    g = gpu_ctx.run_resolve(np.arange(100), 164, 64, 1, [RR.MEMBER] * 64, append_step=30, prev=True)
    assert g["resolved"] == 64 and g["all"] and (g["state"] > 0).all()
    with pytest.raises(_lib.UmiclustError) as e:
        gpu_ctx.fetch()
    assert e.value.code == -77
    st = gpu_ctx.cluster()
    o = orc.cluster(orc.params(1, 0.93, 58, 68), seqs)
    f = gpu_ctx.fetch()
    assert f["n_clusters"] == o["n_clusters"] and f["consensus"] == o["consensus"]
    for k in ("cluster", "strand", "centroid"):
        assert np.array_equal(f[k], o[k]), k
    assert st["n_alignments"] == o["stats"]["alignments"] and st["cells"] == o["stats"]["cells"]


def test_resolve_refuses_what_it_does_not_cover():
    c = R.case("tri9x2")
    seqs = c["pool"].seqs
    with _lib.Context(0) as ctx:
        with pytest.raises(_lib.UmiclustError) as e:
            ctx.run_resolve([0], 10, 4)
        assert e.value.code == -77  # no load
        ctx.load(_lib.params(1, 0.93, 58, 68), seqs)
        M = RR.MEMBER
        for args in (([0, 12], 20, 4, 2, [M] * 8), ([3, 3], 20, 4, 0), ([0], 20, 8193, 0), ([0], 50, 20, 0),
                     ([0], 4, 4, 2, [M] * 8), ([0], 20, 4, 0, [], 0), ([0], 20, 4, 1, [M, 0, M, M]),
                     ([0], 20, 4, 1, [M, 3, M, M]), (np.arange(7 * 65536 + 1), 20, 4, 0)):  # (the last: two segments)
            with pytest.raises(_lib.UmiclustError) as e:
                ctx.run_resolve(*args)
            assert e.value.code == -22, args
        with pytest.raises(_lib.UmiclustError) as e:
            ctx.run_resolve([0], 20, 4, 0, prev=True)  # the previous block's pass without a previous block
        assert e.value.code == -22
        with pytest.raises(_lib.UmiclustError) as e:
            ctx.run_resolve([0], 20, 4, 3, [M] * 12)  # a window of three earlier blocks
        assert e.value.code == -22
        g = ctx.run_resolve([0], 20, 4, 1, [M, RR.CENT, M, M])
        assert g["resolved"] == 4 and g["all"]
        ctx.load(_lib.params(1, 0.93, 58, 68, threads=25), seqs)  # batched rounds (policy O4)
        with pytest.raises(_lib.UmiclustError) as e:
            ctx.run_resolve([0], 20, 4)
        assert e.value.code == -22
        buf, off = _lib._pack(seqs)
        ctx.load_bins(_lib.params(1, 0.93, 58, 68), buf, off, [0, 30, len(seqs)])  # several bins
        with pytest.raises(_lib.UmiclustError) as e:
            ctx.run_resolve([0], 20, 4)
        assert e.value.code == -22
