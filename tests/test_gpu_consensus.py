"""The member tracebacks (k_trace_wave) and the consensus kernel (k_consensus) through umiclust_consensus, against
the plain reference of tests/consensus_ref.py: traced mode runs the tracebacks exactly as a clustering call launches
them (two launches split at 64 nt, LDS sized by the call's longest record, members renumbered into slots) and checks
every member's ops against the oracle's aligner; given mode feeds k_consensus CIGARs no optimal alignment yields.
Every comparison is exact; every member and every cluster is compared."""
import consensus_ref as R
import pytest
from umiclust import _lib, synth

pytestmark = pytest.mark.gpu
EINVAL, ERANGE = -22, -34


def _params(preset=1, boundary_open=1):
    p = _lib.params(preset, 0.93, 1, _lib.MAX_LEN)
    p.policy_boundary_open = boundary_open
    return p


def _check_consensus(name, got, want, seqs, clusters):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, k, len(clusters[k]), seqs[clusters[k][0]], g, w)


@pytest.mark.parametrize("preset,boundary_open", R.SCORINGS)
@pytest.mark.parametrize("name", list(R.TRACED))
def test_traced_vs_oracle(gpu_ctx, name, preset, boundary_open):
    seqs, clusters, strands, _ = R.case(name)
    al = R.oracle_alignments(name, preset, boundary_open)
    cigars, want = R.expected(name, preset, boundary_open)
    got = gpu_ctx.consensus(_params(preset, boundary_open), seqs, clusters, strands)
    ori = R.oriented(seqs, clusters, strands)
    for k, m in enumerate(clusters):
        assert got["ops"][k][0] == ""
        for x in range(1, len(m)):
            where = (name, k, x, "member", ori[k][x], "centroid", seqs[m[0]], "got", got["ops"][k][x], "want",
                     cigars[k][x])
            assert got["ops"][k][x] == cigars[k][x], where
            o = al[k][x]
            assert (int(got["score"][k][x]), int(got["matches"][k][x]), int(got["internal_len"][k][x])) == \
                (o["score"], o["matches"], o["internal_len"]), where
    _check_consensus(name, got["consensus"], want, seqs, clusters)


@pytest.mark.parametrize("name", [n for n in R.GIVEN if n != "msa2049"])
def test_given_ops_vs_reference(gpu_ctx, name):
    seqs, clusters, strands, cigars = R.case(name)
    got = gpu_ctx.consensus(_params(), seqs, clusters, strands, ops=cigars)
    assert got["ops"] == cigars  # what k_consensus read from the slots is what was given, member for member
    _check_consensus(name, got["consensus"], R.expected(name)[1], seqs, clusters)


def test_msa_column_limit(gpu_ctx):
    """2048 columns fit, 2049 are UMICLUST_ERANGE with the pipeline's message; the context works on"""
    seqs, clusters, strands, cigars = R.case("msa2048")
    got = gpu_ctx.consensus(_params(), seqs, clusters, strands, ops=cigars)
    assert got["consensus"] == R.expected("msa2048")[1] and got["consensus"][0] == seqs[clusters[0][0]]
    s9, c9, st9, cg9 = R.case("msa2049")
    with pytest.raises(_lib.UmiclustError) as e:
        gpu_ctx.consensus(_params(), s9, c9, st9, ops=cg9)
    assert e.value.code == ERANGE and "1 clusters exceed the MSA column budget" in str(e.value)
    got = gpu_ctx.consensus(_params(), seqs, clusters, strands, ops=cigars)
    assert got["consensus"] == R.expected("msa2048")[1]
    seqs, clusters, strands, cigars = R.case("cons224")
    got = gpu_ctx.consensus(_params(), seqs, clusters, strands, ops=cigars)
    assert [len(c) for c in got["consensus"]] == [R.CONS_CAP] and got["consensus"] == R.expected("cons224")[1]


def _edit(cigars, k, x, ops):
    out = [list(c) for c in cigars]
    out[k][x] = ops
    return out


def test_invalid_arguments_are_rejected_on_the_host(gpu_ctx):
    """one edit to a valid case each; nothing invalid is launched, and a valid call afterwards answers right"""
    seqs, clusters, strands, cigars = R.case("insertions")
    want = R.expected("insertions")[1]
    p = _params()
    ops = cigars[0][1]
    assert ops.startswith("DD")
    bad_ops = {
        "D turned into M": "M" + ops[1:],
        "an op dropped": ops[:-1],
        "a D dropped": ops[1:],
        "a byte X": ops[:5] + "X" + ops[6:],
        "a lower-case op": ops[:5] + "m" + ops[6:],
        "an I added": ops + "I",
        "no ops": "",
        "more than 224 ops": ops + "ID" * 120,
    }
    for what, o in bad_ops.items():
        assert not R.ops_valid(o, len(seqs[clusters[0][0]]), len(seqs[clusters[0][1]])), what
        with pytest.raises(_lib.UmiclustError) as e:
            gpu_ctx.consensus(p, seqs, clusters, strands, ops=_edit(cigars, 0, 1, o))
        assert e.value.code == EINVAL, what
    # the last member of the last cluster too: every member is checked, not the first
    with pytest.raises(_lib.UmiclustError) as e:
        gpu_ctx.consensus(p, seqs, clusters, strands, ops=_edit(cigars, -1, -1, cigars[-1][-1][1:]))
    assert e.value.code == EINVAL
    twice = [list(m) for m in clusters]
    twice[2].append(clusters[1][1])  # a record listed in two clusters
    bad_clusters = {
        "a member listed twice": (twice, [st + [0] * (len(m) - len(st)) for m, st in zip(twice, strands)]),
        "a centroid listed twice": ([clusters[0], [clusters[0][0]] + clusters[1][1:]], strands[:2]),
        "an empty cluster": (clusters[:1] + [[]] + clusters[1:], strands[:1] + [[]] + strands[1:]),
        "a record index past the end": ([clusters[0][:-1] + [len(seqs)]], strands[:1]),
        "a negative record index": ([clusters[0][:-1] + [-1]], strands[:1]),
    }
    for what, (cl, st) in bad_clusters.items():
        for mode_ops in (None, [cigars[0]] * len(cl)):  # traced and given
            if mode_ops is not None and [len(m) for m in cl] != [len(clusters[0])] * len(cl):
                continue
            with pytest.raises(_lib.UmiclustError) as e:
                gpu_ctx.consensus(p, seqs, cl, st, ops=mode_ops)
            assert e.value.code == EINVAL, what
    for bad in ("", "A" * (_lib.MAX_LEN + 1)):  # a record length outside 1 .. 112
        with pytest.raises(_lib.UmiclustError) as e:
            gpu_ctx.consensus(p, seqs + [bad], clusters, strands)
        assert e.value.code == ERANGE
    got = gpu_ctx.consensus(p, seqs, clusters, strands, ops=cigars)
    assert got["ops"] == cigars and got["consensus"] == want


def test_short_ops_stride_is_rejected(gpu_ctx):
    import ctypes as C

    import numpy as np
    buf, off = _lib._pack(["ACGTACGT", "ACGTACGT"])
    cstart, member = np.array([0, 2], np.int32), np.array([0, 1], np.int32)
    mstr, olen = np.zeros(2, np.uint8), np.zeros(2, np.int32)
    ops = np.zeros(2 * 2 * _lib.MAX_LEN, np.uint8)
    P = C.POINTER
    i32 = lambda a: a.ctypes.data_as(P(C.c_int32))  # noqa: E731
    p = _params()
    for stride, want in ((2 * _lib.MAX_LEN - 1, EINVAL), (2 * _lib.MAX_LEN, 0)):
        rc = _lib.lib().umiclust_consensus(gpu_ctx._h, C.byref(p), buf.ctypes.data, _lib._i64(off), 2, i32(cstart), 1,
                                           i32(member), mstr.ctypes.data_as(P(C.c_uint8)), None, None, stride,
                                           ops.ctypes.data, i32(olen), None, None, None, None, 0, None)
        assert rc == want
    assert ops[2 * _lib.MAX_LEN:2 * _lib.MAX_LEN + 8].tobytes() == b"M" * 8 and list(olen) == [0, 8]


def test_entry_point_runs_what_the_pipeline_runs(gpu_ctx):
    """the clusters, strands and centroids a clustering call fetched, traced again through the entry point, give the
    call's own consensus cluster for cluster -- before and after, the context's results stay fetchable"""
    seqs = synth.make_umis(60, seed=71, max_reads=1200, orient_mix=0.3, error_rate=0.03).as_list()
    seqs[5] = seqs[5][:40]  # one record the length filter drops: it is in no cluster
    p = _lib.params(1, 0.93, 58, 68)
    gpu_ctx.load(p, seqs)
    gpu_ctx.cluster()
    f = gpu_ctx.fetch()
    clusters, strands = R.clusters_of(f)
    assert f["cluster"][5] == -1 and max(map(len, clusters)) > 10 and any(any(st) for st in strands)
    got = gpu_ctx.consensus(p, seqs, clusters, strands)
    _check_consensus("pipeline", got["consensus"], f["consensus"], seqs, clusters)
    again = gpu_ctx.fetch()
    assert again["consensus"] == f["consensus"] and list(again["cluster"]) == list(f["cluster"])
    gpu_ctx.load(p, seqs)
    gpu_ctx.cluster()
    assert gpu_ctx.fetch()["consensus"] == f["consensus"]
