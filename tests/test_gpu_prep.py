"""The load kernel (K1, k_prep_wave) against tests/prep_ref.py on every case of tests/prep_cases.py, output by output,
and the code its outputs steer: the cluster-file writer's three branches, and the pipeline on lower- and mixed-case
input.

Everything compared here is integer data: equal or wrong.  The k-mer lists are compared as the device holds them
(strictly ascending, element by element), not after a sort.  tests/test_prep_ref_cpu.py shows that the reference equals
the C oracle on these cases and that each rule of the operation decides one of them.
"""
import os
import re

import numpy as np
import orc
import prep_cases as C
import prep_ref as R
import pytest
from umiclust import _lib, synth

pytestmark = pytest.mark.gpu

_REF = {}


def _ref(records, dust):
    """the reference per record, computed once per (record, qmask_dust) and shared"""
    rows = []
    for s in records:
        if (s, dust) not in _REF:
            _REF[(s, dust)] = R.prep([s], dust)
        rows.append(_REF[(s, dust)])
    return rows


def _check(got, records, dust):
    """every output of one launch over `records` (in row order) against the reference"""
    rows = _ref(records, dust)
    n = len(records)
    assert len(got["masked"]) == n
    for s, (rec, r) in enumerate(zip(records, rows)):
        where = (s, rec, dust)
        assert got["lens"][s] == len(rec), where
        assert got["masked"][s] == r["masked"][0], where
        assert np.array_equal(got["codes"][s], r["codes"][0]), where
        assert got["changed"][s] == r["changed"][0], where
        for st in range(2):
            k = got["kmers"][s][st]
            assert got["nk"][s][st] == len(k) == r["nk"][0][st], where + (st,)
            assert all(a < b for a, b in zip(k, k[1:])), where + (st, "not strictly ascending")
            assert k == r["kmers"][0][st], where + (st,)
    assert got["ambig"] == int(any(r["ambig"] for r in rows))
    assert got["n_changed"] == sum(r["n_changed"] for r in rows)


@pytest.mark.parametrize("case", C.CASES, ids=[c.name for c in C.CASES])
def test_prep_outputs_vs_reference(gpu_ctx, case):
    """qmask_dust 1 and 0, and once under a permutation (row s is record perm[s], as the length sort launches it)"""
    p = _lib.params(1, 0.93, 1, _lib.MAX_LEN)
    for dust, perm in ((1, None), (0, None), (1, C.perm_of(case))):
        p.qmask_dust = dust
        got = gpu_ctx.prep_outputs(p, case.records, perm)
        order = range(len(case.records)) if perm is None else perm
        _check(got, [case.records[i] for i in order], dust)


def test_prep_outputs_all_cases_one_launch(gpu_ctx):
    """a few hundred records of every kind in one launch, shuffled: neighbours in the grid share nothing, the flag
    words are sums over the whole batch"""
    records = [s for c in C.CASES for s in c.records]
    perm = np.random.default_rng(5).permutation(len(records)).astype(np.int32)
    p = _lib.params(1, 0.93, 1, _lib.MAX_LEN)
    for dust in (1, 0):
        p.qmask_dust = dust
        _check(gpu_ctx.prep_outputs(p, records, perm), [records[i] for i in perm], dust)
    # no ambiguous symbol in a batch of many rows: the bit stays 0 whatever ran before on the context
    clean = [s for c in C.CASES for s in c.records if not R.prep([s])["ambig"]]
    assert len(clean) > 100 and gpu_ctx.prep_outputs(p, clean)["ambig"] == 0


def test_prep_outputs_refusals(gpu_ctx):
    p = _lib.params(1, 0.93, 1, _lib.MAX_LEN)
    recs = ["ACGTACGTAC", "TTGACCA", "GGGCATCAGT"]
    for bad in ([0, 1, 1], [0, 1, 3], [-1, 0, 1]):
        with pytest.raises(_lib.UmiclustError) as e:
            gpu_ctx.prep_outputs(p, recs, bad)
        assert e.value.code == -22
    with pytest.raises(_lib.UmiclustError) as e:
        gpu_ctx.prep_outputs(p, recs + ["A" * (_lib.MAX_LEN + 1)])
    assert e.value.code == -34
    assert gpu_ctx.prep_outputs(p, [])["masked"] == []
    assert gpu_ctx.prep_outputs(p, recs, [2, 0, 1])["lens"].tolist() == [10, 10, 7]


def test_prep_agrees_with_prep_outputs(gpu_ctx):
    """umiclust_prep, the older entry, returns the same masked bytes and lists"""
    c = C.BY_NAME["alpha_outside"]
    p = _lib.params(1, 0.93, 1, _lib.MAX_LEN)
    a, b = gpu_ctx.prep(p, c.records), gpu_ctx.prep_outputs(p, c.records)
    assert a["masked"] == b["masked"] and [[list(map(int, k)) for k in r] for r in a["kmers"]] == b["kmers"]


# ------------------------------------------------------------------ the writer's branches and the pipeline
N_UMI = 400


def _base_umis():
    """400 upper-case UMIs of 58..68 nt that DUST leaves alone, in a UmiSet"""
    u = synth.make_umis(40, seed=611, max_reads=700, orient_mix=0.25, error_rate=0.015)
    seqs = u.as_list()
    keep = [i for i, s in enumerate(seqs) if 58 <= len(s) <= 68 and orc.dust(s) == s][:N_UMI]
    assert len(keep) == N_UMI
    return u, keep


def _umiset(u, keep, seqs):
    off = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    k = np.asarray(keep)
    return synth.UmiSet(seq=np.frombuffer("".join(seqs).encode(), np.uint8), off=off, molecule=u.molecule[k],
                        strand=u.strand[k], fwd_dist=u.fwd_dist[k], rev_dist=u.rev_dist[k])


def _low(s, k):
    """s with a two-letter repeat of 30 residues in it: DUST masks it"""
    rep = ("AC", "GT", "AG", "CT")[k % 4] * 15
    at = 5 + k % 20
    out = s[:at] + rep + s[at + 30:]
    assert len(out) == len(s) and orc.dust(out) != out
    return out


_STATE = {}


def _writer_input():
    """the base records and the roles variant (b) needs, from one oracle clustering (shared, never modified)"""
    if not _STATE:
        u, keep = _base_umis()
        seqs = [u.get(i) for i in keep]
        o = orc.cluster(orc.params(1, 0.93, 58, 68), seqs)
        lens = [len(s) for s in seqs]
        size = np.bincount(o["cluster"], minlength=o["n_clusters"])
        roles = dict(
            longest=lens.index(max(lens)),                                   # sorted seqno 0
            shortest=len(lens) - 1 - lens[::-1].index(min(lens)),            # the last sorted seqno
            centroid=next(i for i in range(N_UMI) if o["centroid"][i] and size[o["cluster"][i]] > 2),
            minus_member=next(i for i in range(N_UMI) if o["strand"][i] and not o["centroid"][i]))
        assert int(o["sorted"][0]) == roles["longest"] and int(o["sorted"][-1]) == roles["shortest"]
        _STATE.update(u=u, keep=keep, seqs=seqs, roles=roles)
    return _STATE


def _variant(name):
    """(records, changed rows expected, masked rows the writer has to download)"""
    st = _writer_input()
    seqs = list(st["seqs"])
    pick = [int(i) for i in np.random.default_rng(77).permutation(N_UMI)]
    if name == "untouched":
        return seqs, 0, 0
    if name.startswith("one_lower_"):
        i = st["roles"][name[len("one_lower_"):]]
        seqs[i] = seqs[i].lower()
        return seqs, 1, 1
    if name == "one_masked":
        seqs[pick[0]] = _low(seqs[pick[0]], 0)
        return seqs, 1, 1
    if name in ("sparse_24", "dense_25"):
        k = 24 if name == "sparse_24" else 25  # 24 * 16 < 400 <= 25 * 16
        for x, i in enumerate(pick[:k]):
            seqs[i] = seqs[i].lower() if x % 2 else _low(seqs[i], x)
        return seqs, k, k if name == "sparse_24" else N_UMI
    assert name == "all_lower"
    return [s.lower() for s in seqs], N_UMI, N_UMI


VARIANTS = ["untouched", "one_lower_longest", "one_lower_shortest", "one_lower_centroid", "one_lower_minus_member",
            "one_masked", "sparse_24", "dense_25", "all_lower"]


@pytest.fixture(scope="module")
def debug_ctx():
    """a context that prints the file path's debug line (the switches are read when a context is created)"""
    old = os.environ.get("UMICLUST_DEBUG")
    os.environ["UMICLUST_DEBUG"] = "1"
    try:
        ctx = _lib.Context(0)
    finally:
        if old is None:
            del os.environ["UMICLUST_DEBUG"]
        else:
            os.environ["UMICLUST_DEBUG"] = old
    yield ctx
    ctx.close()


def _read_dir(d):
    return {fn: open(os.path.join(d, fn), "rb").read() for fn in sorted(os.listdir(d))}


@pytest.mark.parametrize("name", VARIANTS)
def test_writer_branches_vs_oracle(debug_ctx, tmp_path, capfd, name):
    """The cluster files and the consout byte for byte against the oracle where no record changed (the input bytes are
    written), where a few did (their rows alone are fetched through the changed flags), and from 1 in 16 on (the whole
    masked buffer); the branch is read from the debug line's counts, not assumed."""
    st = _writer_input()
    seqs, n_changed, n_rows = _variant(name)
    assert sum(orc.dust(s) != s for s in seqs) == n_changed
    fa = tmp_path / "in.fasta"
    synth.write_umi_fasta(str(fa), _umiset(st["u"], st["keep"], seqs))
    for width in (0, 60):
        out, ref = tmp_path / f"gpu{width}", tmp_path / f"orc{width}"
        out.mkdir()
        ref.mkdir()
        op = orc.params(1, 0.93, 58, 68)
        op.fasta_width = width
        orc.run_fasta(op, str(fa), str(ref) + "/cluster", str(ref / "consensus.fasta"))
        p = _lib.params(_lib.PRESET_ROUND1, 0.93, 58, 68)
        p.fasta_width = width
        capfd.readouterr()
        stats = debug_ctx.run_fasta(p, str(fa), str(out) + "/cluster", str(out / "consensus.fasta"), None)
        debug_ctx.wait_host()
        err = capfd.readouterr().err
        m = re.search(r"\((\d+) changed, (\d+) of (\d+) rows\)", err)
        assert m, err[-2000:]
        assert tuple(map(int, m.groups())) == (n_changed, n_rows, N_UMI)
        assert stats["n_kept"] == N_UMI
        got, want = _read_dir(out), _read_dir(ref)
        assert sorted(got) == sorted(want)
        for fn in want:
            assert got[fn] == want[fn], (name, width, fn)


def _cmp_cluster(gpu, ora):
    assert gpu["n_clusters"] == ora["n_clusters"]
    assert np.array_equal(gpu["cluster"], ora["cluster"])
    assert np.array_equal(gpu["strand"], ora["strand"])
    assert np.array_equal(gpu["centroid"], ora["centroid"])
    assert gpu["consensus"] == ora["consensus"]


@pytest.mark.parametrize("ambiguous", [False, True], ids=["acgt", "one_n"])
@pytest.mark.parametrize("casing", ["lower", "mixed"])
def test_pipeline_on_recased_input(gpu_ctx, casing, ambiguous):
    """load + cluster + fetch on lower- and mixed-case copies of one input, without an ambiguous symbol (the one-hot
    aligners) and with a single N (the IUPAC ones): the oracle's clustering, and the upper-case input's."""
    seqs = list(_writer_input()["seqs"])
    if ambiguous:
        seqs[123] = seqs[123][:40] + "N" + seqs[123][41:]
    rng = np.random.default_rng(9)
    if casing == "lower":
        re_cased = [s.lower() for s in seqs]
    else:
        re_cased = ["".join(ch.lower() if f else ch for ch, f in zip(s, rng.random(len(s)) < 0.5)) for s in seqs]
    assert any("n" in s or "N" in s for s in re_cased) == ambiguous
    gpu_ctx.load(_lib.params(1, 0.93, 58, 68), re_cased)
    st = gpu_ctx.cluster()
    g = gpu_ctx.fetch()
    o = orc.cluster(orc.params(1, 0.93, 58, 68), re_cased)
    _cmp_cluster(g, o)
    _cmp_cluster(g, orc.cluster(orc.params(1, 0.93, 58, 68), seqs))
    assert st["n_alignments"] == o["stats"]["alignments"] and st["cells"] == o["stats"]["cells"]
