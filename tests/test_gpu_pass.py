"""One whole device pass (k_walk, the per-length alignment rounds, k_peer_rel / k_peer_pairs, k_pack) against the
plain reference of tests/pass_ref.py: umiclust_pass runs enqueue_pass on a chosen index and peer window and returns
what the host's resolve step reads of it.  Integers throughout: no tolerance, no query-strand left out.  What the
cases reach is asserted from the reference alone in tests/test_pass_ref_cpu.py."""
import numpy as np
import orc
import pass_ref as R
import pytest
from umiclust import _lib, synth

pytestmark = pytest.mark.gpu


def _loaded(ctx, pool):
    ctx.load(_lib.params(1, 0.93, int(pool.lens.min()), int(pool.lens.max())), pool.seqs)
    return ctx


def _run(ctx, name):
    c = R.case(name)
    g = _loaded(ctx, c["pool"]).run_pass(c["cent"], c["q0"], c["nq"], c["nprev"], lazy=c["lazy"], prev=c["prev"])
    return c, g


def _records(g):
    """per query-strand the record's words (None without one), and what is wrong with their placement"""
    recs, bad, spans = [], [], []
    total = g["rec_total"]
    for qs, h in enumerate(g["hostqs"]):
        off = int(h["rec"])
        if off == R.NONE:
            recs.append(None)
            continue
        if off >= total:
            bad.append(f"record of query-strand {qs} starts at {off}, past the total {total}")
            recs.append(None)
            continue
        nt, np_ = int(g["rec"][off]) & 0xff, int(g["rec"][off]) >> 8
        n = 1 + 2 * nt + (nt + 3) // 4 + 2 * np_
        if off + n > total:
            bad.append(f"record of query-strand {qs} [{off}, {off + n}) ends past the total {total}")
            recs.append(None)
            continue
        recs.append([int(x) for x in g["rec"][off:off + n]])
        spans.append((off, off + n, qs))
    spans.sort()
    for (a0, a1, qa), (b0, b1, qb) in zip(spans, spans[1:]):
        if b0 < a1:
            bad.append(f"records of query-strands {qa} [{a0}, {a1}) and {qb} [{b0}, {b1}) overlap")
    if sum(b - a for a, b, _ in spans) != total:
        bad.append(f"record total {total}, the records' sizes add up to {sum(b - a for a, b, _ in spans)}")
    return recs, bad


def _lists_bad(r, g):
    bad = []
    for qs in range(len(r["ntop"])):
        n, m = int(r["ntop"][qs]), int(r["npeer"][qs])
        if int(g["ntop"][qs]) != n or not np.array_equal(g["top_seqno"][qs, :n], r["top_seqno"][qs, :n]) or \
                not np.array_equal(g["top_count"][qs, :n], r["top_count"][qs, :n]):
            bad.append(f"top list of query-strand {qs}")
        if int(g["npeer"][qs]) != m:
            bad.append(f"npeer of query-strand {qs}: {g['npeer'][qs]} vs {m}")
        elif m != 255:
            ids, cnts = r["peers"][qs]
            if g["peer_id"][qs, :m].tolist() != ids.tolist() or g["peer_count"][qs, :m].tolist() != cnts.tolist():
                bad.append(f"peer list of query-strand {qs}")
    return bad


def _mismatches(c, g) -> list[str]:
    r = c["ref"]
    bad = _lists_bad(c["lists"], g)
    recs, rbad = _records(g)
    bad += rbad
    for qs, (h, w) in enumerate(zip(r["hostqs"], r["walks"])):
        gh, gw = g["hostqs"][qs], g["walk"][qs]
        for f in ("best_t", "cells", "best_rank", "w", "flags", "nrel", "e", "npeer"):
            if int(gh[f]) != h[f]:
                bad.append(f"HostQs.{f} of query-strand {qs}: {int(gh[f])} vs {h[f]}")
        if gh["rel"].tolist() != h["rel"]:
            bad.append(f"HostQs.rel of query-strand {qs}: {gh['rel'].tolist()} vs {h['rel']} (nrel {h['nrel']})")
        if (int(gh["rec"]) != R.NONE) != h["has_rec"]:
            bad.append(f"HostQs.rec of query-strand {qs}: {int(gh['rec']):#x}, record expected: {h['has_rec']}")
        for f in ("w", "e", "done", "acc", "best_rank", "best_t", "cells", "lastkey"):
            if int(gw[f]) != w[f]:
                bad.append(f"WalkState.{f} of query-strand {qs}: {int(gw[f])} vs {w[f]}")
        if g["res"][qs, :w["e"]].tolist() != w["res"]:
            bad.append(f"walk results of query-strand {qs}: {g['res'][qs, :w['e']].tolist()} vs {w['res']}")
        if [int(x) for x in g["aligned"][qs]] != r["masks"][qs]:
            bad.append(f"aligned masks of query-strand {qs}: {[hex(int(x)) for x in g['aligned'][qs]]} vs "
                       f"{[hex(x) for x in r['masks'][qs]]}")
        for y, a in enumerate(r["aligned"][qs]):
            if a and int(g["peer_res"][qs, y]) != r["peer_res"][qs][y]:
                bad.append(f"peer result {y} of query-strand {qs}: {int(g['peer_res'][qs, y]):#x} vs "
                           f"{r['peer_res'][qs][y]:#x}")
        if h["has_rec"] and recs[qs] is not None and recs[qs] != r["records"][qs]:
            d = [i for i, (a, b) in enumerate(zip(recs[qs], r["records"][qs])) if a != b]
            bad.append(f"record of query-strand {qs}: {len(recs[qs])} words vs {len(r['records'][qs])}, first "
                       f"differing words {d[:6]}")
    if g["rec_total"] != r["total"]:
        bad.append(f"record total {g['rec_total']} vs {r['total']}")
    ctr = g["counters"]
    got = {8: int(ctr[8]), 12: int(ctr[12]) | int(ctr[13]) << 32, 14: int(ctr[14]) | int(ctr[15]) << 32}
    if got != r["counters"]:
        bad.append(f"counters (peer pairs, walk cells, peer cells) {got} vs {r['counters']}")
    return bad


def _canonical(g):
    """a pass's outputs without the addresses the records happen to get"""
    hq = g["hostqs"].copy()
    hq["rec"] = np.where(hq["rec"] == R.NONE, R.NONE, 0)
    recs, bad = _records(g)
    assert not bad, bad[:4]
    e = g["walk"]["e"]
    res = np.where(np.arange(32)[None, :] < e[:, None], g["res"], 0)
    al = (g["aligned"][:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)
    pres = np.where(al.reshape(len(e), 128) == 1, g["peer_res"], 0)
    return dict(hq=hq.tobytes(), recs=recs, total=g["rec_total"], res=res.tobytes(), pres=pres.tobytes(),
                aligned=g["aligned"].tobytes(), walk=g["walk"].tobytes(),
                counters=g["counters"][[8, 12, 13, 14, 15]].tolist(), ntop=g["ntop"].tobytes(),
                npeer=g["npeer"].tobytes())


@pytest.mark.parametrize("name", list(R.CASES))
def test_pass_equals_reference(name, gpu_ctx):
    c, g = _run(gpu_ctx, name)
    assert g["both"] == 2 and len(g["hostqs"]) == 2 * c["nq"]
    bad = _mismatches(c, g)
    assert not bad, f"{len(bad)} differences:\n" + "\n".join(bad[:12])


def test_buffer_sets_are_left_clean_for_the_next_pass(gpu_ctx):
    """A, B, A on one context: k_pack leaves the record counter, its workgroup tickets and the pass counters zero for
    the next pass on the buffer set, so A's second run equals its first."""
    _, a1 = _run(gpu_ctx, "crowd129")
    _, b = _run(gpu_ctx, "crowd129_lazy")
    _, a2 = _run(gpu_ctx, "crowd129")
    x, y = _canonical(a1), _canonical(a2)
    for k in x:
        assert x[k] == y[k], k
    assert _canonical(b)["total"] == x["total"] and b["counters"][8] == 0


def test_cluster_after_pass_equals_oracle(gpu_ctx):
    """umiclust_pass leaves the context loaded and not clustered, and the passes it left on the buffer sets do not
    disturb the clustering that follows: it equals the oracle's, and a fetch in between is refused."""
    seqs = synth.make_umis(60, seed=1, max_reads=800).as_list()
    gpu_ctx.load(_lib.params(1, 0.93, 58, 68), seqs)
    gpu_ctx.cluster()
    g = gpu_ctx.run_pass(np.arange(100), 164, 64, 1, 30, prev=True)
    assert (g["ntop"] > 0).any() and (g["hostqs"]["w"] > 0).any()
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


def test_pass_refuses_what_it_does_not_cover():
    c = R.case("tri9x2")
    seqs = c["pool"].seqs
    with _lib.Context(0) as ctx:
        with pytest.raises(_lib.UmiclustError) as e:
            ctx.run_pass([0], 10, 4)
        assert e.value.code == -77  # no load
        ctx.load(_lib.params(1, 0.93, 58, 68), seqs)
        for args in (([0, 12], 20, 4, 2), ([3, 3], 20, 4, 0), ([0], 20, 8193, 0), ([0], 50, 20, 0), ([0], 20, 4, 3),
                     ([0], 4, 4, 2), ([0], 20, 4, 0, 0)):
            with pytest.raises(_lib.UmiclustError) as e:
                ctx.run_pass(*args)
            assert e.value.code == -22, args
        with pytest.raises(_lib.UmiclustError) as e:
            ctx.run_pass([0], 20, 4, 0, prev=True)  # the previous block's pass without a previous block
        assert e.value.code == -22
        with pytest.raises(_lib.UmiclustError) as e:
            ctx.run_pass(c["cent"], c["q0"], c["nq"], c["nprev"], prev=True, rec_cap=c["ref"]["total"] - 1)
        assert e.value.code == -34  # more record words than the caller has room for
        g = ctx.run_pass(c["cent"], c["q0"], c["nq"], c["nprev"], prev=True, rec_cap=c["ref"]["total"])
        assert g["rec_total"] == c["ref"]["total"]
        ctx.load(_lib.params(1, 0.93, 58, 68, threads=25), seqs)  # batched rounds (policy O4)
        with pytest.raises(_lib.UmiclustError) as e:
            ctx.run_pass([0], 20, 4)
        assert e.value.code == -22
        buf, off = _lib._pack(seqs)
        ctx.load_bins(_lib.params(1, 0.93, 58, 68), buf, off, [0, 30, len(seqs)])  # several bins
        with pytest.raises(_lib.UmiclustError) as e:
            ctx.run_pass([0], 20, 4)
        assert e.value.code == -22
