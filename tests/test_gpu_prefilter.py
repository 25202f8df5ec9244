"""The k-mer prefilter (k_pf_count, k_pf_full, k_pf_merge) against the plain reference of tests/prefilter_ref.py,
list by list: umiclust_prefilter runs one whole pass of the pipeline on a chosen index and peer window and returns
every query-strand's top-41 and peer list.  Integers throughout: no tolerance, no query-strand left out.  Each case
runs under both workgroup layouts of k_pf_count (UMICLUST_PF1) and asserts from info[] the path it is named after."""
import numpy as np
import orc
import prefilter_ref as R
import pytest
from umiclust import _lib, synth

pytestmark = pytest.mark.gpu

PF1 = ["0", str(1 << 30)]
K_TILE, K_DELTA = 65536, 8192  # sealed tile size, delta tile fold threshold (cluster_ctx.h)


@pytest.fixture(scope="module")
def contexts():
    """One context per UMICLUST_PF1 value (the switch is read by umiclust_create), kept for the module."""
    made = {}

    def get(pf1: str, monkeypatch):
        if pf1 not in made:
            monkeypatch.setenv("UMICLUST_PF1", pf1)
            made[pf1] = dict(ctx=_lib.Context(0), pool=None)
        return made[pf1]
    yield get
    for m in made.values():
        m["ctx"].close()


def _loaded(slot, p: R.Pool):
    if slot["pool"] is not p:
        slot["ctx"].load(_lib.params(1, 0.93, int(p.lens.min()), int(p.lens.max())), p.seqs)
        slot["pool"] = p
    return slot["ctx"]


def _tiles(ncent: int, step: int) -> int:
    """non-empty index tiles after appending ncent centroids `step` at a time (append_centroids' LSM policy)"""
    sealed = base_end = end = 0
    while end < ncent:
        end = min(ncent, end + step)
        while end - sealed >= K_TILE:
            sealed += K_TILE
            base_end = max(base_end, sealed)
        if end - base_end > K_DELTA:
            base_end = end
    return sealed // K_TILE + (base_end > sealed) + (end > base_end)


def _mismatches(r: dict, g: dict) -> list[str]:
    bad = []
    for qs in range(len(r["ntop"])):
        n = int(r["ntop"][qs])
        gn = int(g["ntop"][qs])
        if gn != n or not np.array_equal(g["top_seqno"][qs, :n], r["top_seqno"][qs, :n]) or \
                not np.array_equal(g["top_count"][qs, :n], r["top_count"][qs, :n]):
            bad.append(f"top list of query-strand {qs} (nk {r['nk'][qs]}, thr {r['thr'][qs]}, {r['ncand'][qs]} candidates): "
                       f"ntop {gn} vs {n}; got {list(zip(g['top_seqno'][qs, :gn].tolist(), g['top_count'][qs, :gn].tolist()))[:12]} "
                       f"want {list(zip(r['top_seqno'][qs, :n].tolist(), r['top_count'][qs, :n].tolist()))[:12]}")
        m = int(r["npeer"][qs])
        gm = int(g["npeer"][qs])
        if gm != m:
            bad.append(f"npeer of query-strand {qs}: {gm} vs {m} ({r['npeer_all'][qs]} before the cap)")
        elif m != 255:
            ids, cnts = r["peers"][qs]
            got = list(zip(g["peer_id"][qs, :m].tolist(), g["peer_count"][qs, :m].tolist()))
            want = list(zip(ids.tolist(), cnts.tolist()))
            if sorted(got) != sorted(want):
                bad.append(f"peer set of query-strand {qs}: got {sorted(got)[:12]} want {sorted(want)[:12]}")
            elif got != want:
                bad.append(f"peer order of query-strand {qs}: got {got[:16]} want {want[:16]}")
    return bad


def _run(name, pf1, contexts, monkeypatch):
    c = R.case(name)
    ctx = _loaded(contexts(pf1, monkeypatch), c["pool"])
    g = ctx.prefilter(c["cent"], c["q0"], c["nq"], c["nprev"], c["step"])
    r = c["ref"]
    assert g["both"] == 2 and len(g["ntop"]) == len(r["ntop"])
    bad = _mismatches(r, g)
    assert not bad, f"{len(bad)} lists differ:\n" + "\n".join(bad[:8])
    info = g["info"]
    ncent = len(c["cent"])
    assert info[0] == r["units"].sum()             # units the lean kernel handed to the full kernel
    assert info[1] == _tiles(ncent, c["step"])     # centroid tiles read
    assert info[2] == (1 if ncent else 0)          # counter segments
    assert info[3] == (1 if pf1 != "0" else 0)     # the one-wave layout of k_pf_count
    return c, g


@pytest.mark.parametrize("pf1", PF1)
@pytest.mark.parametrize("ncent", [0, 1, 7, 8, 9])
def test_tiny_index(ncent, pf1, contexts, monkeypatch):
    """0..9 centroids: ntop 0..9 and every part boundary (part = ordinal % 8)."""
    c, g = _run(f"tiny{ncent}", pf1, contexts, monkeypatch)
    assert g["ntop"].max() == min(ncent, c["ref"]["ntop"].max()) and g["info"][0] == 0


@pytest.mark.parametrize("pf1", PF1)
@pytest.mark.parametrize("ncent", [512, 516, 520])
def test_part_cap(ncent, pf1, contexts, monkeypatch):
    """Exactly 64 candidates in a part stay in the lean kernel, 65 go to the full kernel as a unit; with 516
    centroids a part that overflows sits next to one that is exactly full (a 65th entry written one slot too far
    would land in the neighbour's list)."""
    c, g = _run(f"cap{ncent}", pf1, contexts, monkeypatch)
    assert (g["info"][0] == 0) == (ncent == 512)


@pytest.mark.parametrize("pf1", PF1)
@pytest.mark.parametrize("name", ["rank4096", "bitonic4200", "scan9000"])
def test_full_kernel_selection_paths(name, pf1, contexts, monkeypatch):
    """k_pf_full's three selections: by rank (a part's candidates <= 512), the bitonic sort above that, the chunked
    scan with its running top-41 merge past 1,024 (tests/test_prefilter_ref_cpu.py asserts the sizes)."""
    c, g = _run(name, pf1, contexts, monkeypatch)
    pm = c["ref"]["part_max"].max()
    assert g["info"][0] > 0
    assert {"rank4096": pm == 512, "bitonic4200": 512 < pm <= 1024, "scan9000": pm > 1024}[name]


@pytest.mark.parametrize("pf1", PF1)
@pytest.mark.parametrize("name", ["lsm20000_step3000", "lsm20000", "sealed66000"])
def test_index_tile_states(name, pf1, contexts, monkeypatch):
    """The LSM states the kernels read: base + delta after folds, one arranged base tile (>= 16,384 centroids:
    k_list_arrange's posting order), a sealed tile beside the open ones."""
    c, g = _run(name, pf1, contexts, monkeypatch)
    assert g["info"][1] == {"lsm20000_step3000": 2, "lsm20000": 1, "sealed66000": 2}[name]
    assert g["info"][0] > 0


@pytest.mark.parametrize("pf1", PF1)
def test_low_complexity_thresholds(pf1, contexts, monkeypatch):
    """thr = 0 (no unmasked 8-mer: every centroid and every earlier window query is a hit, the units go to the full
    kernel's scan mode) and thr = nk < 12."""
    c, g = _run("low", pf1, contexts, monkeypatch)
    zero = c["ref"]["nk"] == 0
    assert zero.sum() >= 5 and g["info"][0] >= 8 * zero.sum()
    assert (g["ntop"][zero] == 41).all()


@pytest.mark.parametrize("pf1", PF1)
def test_max_counts(pf1, contexts, monkeypatch):
    """Count 105 (all 8-mers of a 112-mer) on both strands: the top of the u8 / 127 - count key range."""
    c, g = _run("max", pf1, contexts, monkeypatch)
    assert g["top_count"][0::2, 0].max() == 105 and g["top_count"][1::2, 0].max() == 105


@pytest.mark.parametrize("pf1", PF1)
def test_control_synthetic_umis(pf1, contexts, monkeypatch):
    """Plain synthetic UMIs: nothing overflows, the lean kernel finishes every unit."""
    c, g = _run("control", pf1, contexts, monkeypatch)
    assert g["info"][0] == 0


@pytest.mark.parametrize("pf1", PF1)
@pytest.mark.parametrize("name", ["peers60x2", "peers90x1", "peers200"])
def test_peer_lists(name, pf1, contexts, monkeypatch):
    """The peer window of 0, 1 and 2 earlier blocks with the 128 / 129 boundary inside the block: lists up to 128
    entries and overflows (255) both occur."""
    c, g = _run(name, pf1, contexts, monkeypatch)
    assert (g["npeer"] == 255).any() and (g["npeer"] == 128).any()


def test_cluster_after_prefilter_equals_oracle(gpu_ctx):
    """umiclust_prefilter leaves the context loaded and not clustered: a clustering of the same load still equals the
    oracle's, and a fetch in between is refused."""
    seqs = synth.make_umis(60, seed=1, max_reads=800).as_list()
    gpu_ctx.load(_lib.params(1, 0.93, 58, 68), seqs)
    gpu_ctx.cluster()
    g = gpu_ctx.prefilter(np.arange(100), 100, 64, 0, 30)
    assert (g["ntop"] > 0).any()
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


def test_prefilter_refuses_what_it_does_not_cover():
    seqs = R.pool("peers").seqs
    with _lib.Context(0) as ctx:
        with pytest.raises(_lib.UmiclustError) as e:
            ctx.prefilter([0], 10, 4)
        assert e.value.code == -77  # no load
        ctx.load(_lib.params(1, 0.93, 58, 68), seqs)
        for args in (([0, 12], 20, 4, 2), ([3, 3], 20, 4, 0), ([0], 20, 8193, 0), ([0], 240, 20, 0), ([0], 20, 4, 3),
                     ([0], 4, 4, 2), ([0], 20, 4, 0, 0)):
            with pytest.raises(_lib.UmiclustError) as e:
                ctx.prefilter(*args)
            assert e.value.code == -22, args
        ctx.load(_lib.params(1, 0.93, 58, 68, threads=25), seqs)  # batched rounds (policy O4)
        with pytest.raises(_lib.UmiclustError) as e:
            ctx.prefilter([0], 20, 4)
        assert e.value.code == -22
        buf, off = _lib._pack(seqs)
        ctx.load_bins(_lib.params(1, 0.93, 58, 68), buf, off, [0, 100, len(seqs)])  # several bins
        with pytest.raises(_lib.UmiclustError) as e:
            ctx.prefilter([0], 20, 4)
        assert e.value.code == -22
