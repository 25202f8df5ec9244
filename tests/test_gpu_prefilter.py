"""The k-mer prefilter (k_pf_count, k_pf_full, k_pf_merge) against the plain reference of tests/prefilter_ref.py,
list by list: umiclust_prefilter runs one whole pass of the pipeline on a chosen index and peer window and returns
every query-strand's top-41 and peer list.  Integers throughout: no tolerance, no query-strand left out.  Each case
runs under both workgroup layouts of k_pf_count (UMICLUST_PF1) and asserts from info[] the path it is named after.
The single-bin pipeline's split passes (umiclust_prefilter_split) and the multi-bin loads' packs
(umiclust_prefilter_pack) are compared the same way."""
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
        prm = _lib.params(1, 0.93, int(p.lens.min()), int(p.lens.max()))
        if len(p.bin_s) > 2:  # a multi-bin load: every bin is in vsearch's order already, so seqno = index
            slot["ctx"].load_bins(prm, *_lib._pack(p.seqs), p.bin_s)
        else:
            slot["ctx"].load(prm, p.seqs)
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


def _tiles_after(appends) -> tuple[int, int]:
    """(non-empty index tiles, centroids in the sealed and base tiles) after appends of these sizes"""
    sealed = base_end = end = 0
    for n in appends:
        if n == 0:
            continue
        end += n
        while end - sealed >= K_TILE:
            sealed += K_TILE
            base_end = max(base_end, sealed)
        if end - base_end > K_DELTA:
            base_end = end
    return sealed // K_TILE + (base_end > sealed) + (end > base_end), base_end


def _steps(ncent: int, step: int) -> list[int]:
    return [min(step, ncent - i) for i in range(0, ncent, step)]


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


def _run_split(name, pf1, contexts, monkeypatch):
    c = R.split_case(name)
    ctx = _loaded(contexts(pf1, monkeypatch), c["pool"])
    g = ctx.prefilter_split(c["cent"], c["newcent"], c["w0"], c["nq"], c["step"])
    r = c["ref"]
    assert g["both"] == 2 and len(g["ntop"]) == len(r["ntop"])
    bad = _mismatches(r, g)
    assert not bad, f"{len(bad)} lists differ:\n" + "\n".join(bad[:8])
    info = g["info"]
    before = _steps(len(c["cent"]), c["step"])
    assert info[0] == r["units"].sum()                              # units of the counting half, flagged hits included
    assert info[5] == _tiles_after(before)[0]                       # tiles the counting half read
    assert (info[1], info[6]) == _tiles_after(before + [len(c["newcent"])])  # tiles of the second half; folded?
    assert info[2] == 1 and info[3] == (1 if pf1 != "0" else 0)
    return c, g


@pytest.mark.parametrize("pf1", PF1)
@pytest.mark.parametrize("name", ["split_some", "split_none", "split_all"])
def test_split_flagged_hits(name, pf1, contexts, monkeypatch):
    """A split pass: the counting half flags every hit of block j-2, the merge keeps those that became centroids --
    a third of them, none, all -- and orders them among the indexed centroids of equal count by length and seqno."""
    c, g = _run_split(name, pf1, contexts, monkeypatch)
    r = c["ref"]
    assert g["info"][0] == 0  # every unit stays in the lean kernel: the merge alone decides about the flagged hits
    new = np.isin(g["top_seqno"], c["newcent"]) & (np.arange(41)[None, :] < g["ntop"][:, None])
    assert new.any() == (name != "split_none")
    assert (r["flag_dropped"].sum() > 0) == (name != "split_all")


@pytest.mark.parametrize("pf1", PF1)
@pytest.mark.parametrize("name", ["split_cap64", "split_cap65"])
def test_split_part_cap(name, pf1, contexts, monkeypatch):
    """Centroid candidates and flagged hits share a part's 64 slots: exactly 64 stay lean, 65 become a unit of the
    second half's full kernel (which counts again, against the index with the new centroids)."""
    c, g = _run_split(name, pf1, contexts, monkeypatch)
    assert (g["info"][0] == 0) == (name == "split_cap64")
    assert c["ref"]["part_sum"].max() == (64 if name == "split_cap64" else 65) and c["ref"]["cent_part_max"].max() <= 64


@pytest.mark.parametrize("pf1", PF1)
def test_split_fold_between_the_halves(pf1, contexts, monkeypatch):
    """The append between the halves folds the delta tile into the base tile, rebuilt in place on the side stream while
    the counting half that reads both is queued: the fold's wait for that half and the second half's wait for the fold
    are the pipeline's own events."""
    c, g = _run_split("split_fold", pf1, contexts, monkeypatch)
    n = len(c["cent"]) + len(c["newcent"])
    assert len(c["cent"]) <= K_DELTA < n and (g["info"][1], g["info"][5], g["info"][6]) == (1, 1, n)
    assert g["info"][0] > 0


@pytest.mark.parametrize("pf1", PF1)
def test_split_low_complexity(pf1, contexts, monkeypatch):
    """thr = 0 and thr = nk < 12 queries as block j: with thr = 0 every entry of block j-2 is a flagged hit and every
    part a unit."""
    c, g = _run_split("split_low", pf1, contexts, monkeypatch)
    zero = c["ref"]["thr"] == 0
    assert zero.sum() >= 5 and g["info"][0] >= 8 * zero.sum()
    assert (g["ntop"][zero] == 41).all()


@pytest.mark.parametrize("pf1", PF1)
def test_split_peer_ids(pf1, contexts, monkeypatch):
    """The peers of the two-block window out of the counting half's three-block one (ids moved by one block), with the
    128 / 129 boundary inside block j."""
    c, g = _run_split("split_peers", pf1, contexts, monkeypatch)
    assert (g["npeer"] == 255).any() and (g["npeer"] == 128).any()


def _run_pack(name, pf1, contexts, monkeypatch):
    c = R.pack_case(name)
    ctx = _loaded(contexts(pf1, monkeypatch), c["pool"])
    g = ctx.prefilter_pack(c["first"], c["nbins"], c["cent"], c["q0"], c["nq"], c["nprev"], c["step"])
    r = c["ref"]
    assert g["both"] == 2 and len(g["ntop"]) == len(r["ntop"])
    bad = _mismatches(r, g)
    assert not bad, f"{len(bad)} lists differ:\n" + "\n".join(bad[:8])
    info = g["info"]
    ncent = len(c["cent"])
    assert info[0] == r["units"].sum() and info[1] == _tiles(ncent, c["step"]) and info[2] == (1 if ncent else 0)
    assert info[3] == (1 if pf1 != "0" else 0)
    return c, g


@pytest.mark.parametrize("pf1", PF1)
@pytest.mark.parametrize("ord0", R.PACK_ORD0)
def test_pack_centroid_cut(ord0, pf1, contexts, monkeypatch):
    """The later bin's first centroid ordinal at every residue of pack_cmin (% 8, the byte of a counter word, the word
    of a uint4): the earlier bin's centroids all carry the queries' scrambled 8-mers (thr = nk = 1..3: the lean
    kernel's sweep) or are hits anyway (thr = 0: the full kernel's scan), and none may be listed."""
    c, g = _run_pack(f"pack_ord{ord0}", pf1, contexts, monkeypatch)
    lo = int(c["pool"].bin_s[2])
    listed = g["top_seqno"][np.arange(41)[None, :] < g["ntop"][:, None]]
    assert len(listed) > 0 and (listed >= lo).all()
    zero = c["ref"]["thr"] == 0
    assert zero.sum() >= 4 and g["info"][0] == 8 * zero.sum()
    assert (g["ntop"][zero] == min(41, R.PACK_CENT2)).all()


@pytest.mark.parametrize("pf1", PF1)
@pytest.mark.parametrize("d", range(1, 64))
def test_pack_peer_cut(d, pf1, contexts, monkeypatch):
    """The later bin starting d entries into the window, at every (part, byte) residue of pack_pmin: inside the
    earlier block's tile (d <= 32) and inside the block itself, which then crosses the bin boundary.  The earlier
    bin's window entries carry the queries' scrambled 8-mers and none may be a peer."""
    c, g = _run_pack(f"pack_win{d}", pf1, contexts, monkeypatch)
    s2 = int(c["pool"].bin_s[2])
    w0 = c["q0"] - c["nq"]
    assert w0 + d == s2 and (c["q0"] < s2) == (d > c["nq"])
    for qs in range(len(g["npeer"])):
        if c["q0"] + qs // 2 >= s2:
            assert (g["peer_id"][qs, :g["npeer"][qs]] >= d).all(), qs


@pytest.mark.parametrize("pf1", PF1)
def test_pack_lengths_rise_with_the_ordinal(pf1, contexts, monkeypatch):
    """A short bin in front of a long one, every candidate of a part tied at one count: which 41 of its 92 the full
    kernel keeps is decided by the centroid length table alone.  A length looked up from the ordinal is off by the 400
    ordinals of the short bin, 50 entries a part, and keeps none of the right ones (tests/test_prefilter_ref_cpu.py
    models both)."""
    c, g = _run_pack("pack_lengths", pf1, contexts, monkeypatch)
    assert g["info"][0] > 0 and c["ref"]["part_max"].max() > 64


def test_two_counter_segments(contexts, monkeypatch):
    """More than 458,752 centroids: k_pf_full counts every unit segment by segment and merges the running top-41 by
    binary search; lists with tied counts from both segments, and a thr = 0 query (every centroid a candidate, the
    chunked scan in both segments).  The lean kernel does not run: no units handed over, no one-wave layout."""
    c = R.segment_case()
    ctx = _loaded(contexts("0", monkeypatch), c["pool"])
    g = ctx.prefilter(c["cent"], c["q0"], c["nq"], c["nprev"], c["step"])
    bad = _mismatches(c["ref"], g)
    assert not bad, f"{len(bad)} lists differ:\n" + "\n".join(bad[:8])
    assert list(g["info"]) == [0, _tiles(len(c["cent"]), c["step"]), 2, 0] and g["info"][1] == 8
    both = (g["top_seqno"] >= R.SEG_CENT) & (np.arange(41)[None, :] < g["ntop"][:, None])
    assert (both.sum(axis=1) >= 10).any()
    # what stays refused past one segment: a split pass (the pipeline does not split there) and umiclust_pass
    for call in (lambda: ctx.prefilter_split(c["cent"][:R.SEG_CENT], [R.SEG_CENT], R.SEG_CENT, 8),
                 lambda: ctx.run_pass(c["cent"], c["q0"], c["nq"])):
        with pytest.raises(_lib.UmiclustError) as e:
            call()
        assert e.value.code == -22


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


def test_cluster_after_split_prefilter_equals_oracle(gpu_ctx):
    """umiclust_prefilter_split leaves the context loaded and not clustered, the appends back on the main stream: a
    clustering of the same load (split passes) still equals the oracle's, and a fetch in between is refused."""
    seqs = synth.make_umis(60, seed=1, max_reads=800).as_list()
    gpu_ctx.load(_lib.params(1, 0.93, 58, 68), seqs)
    gpu_ctx.cluster()
    g = gpu_ctx.prefilter_split(np.arange(100), np.arange(100, 164, 2), 100, 64, 30)
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


def test_cluster_pack_after_pack_prefilter_equals_oracle(gpu_ctx):
    """umiclust_prefilter_pack leaves the load as it was and no bin clustered: a clustering of the same pack still
    equals the oracle's bin by bin, and a fetch in between is refused."""
    bins, seqs = [0], []
    for b in range(3):
        seqs += synth.make_umis(20 + 10 * b, seed=40 + b, max_reads=300).as_list()
        bins.append(len(seqs))
    gpu_ctx.load_bins(_lib.params(1, 0.93, 58, 68), *_lib._pack(seqs), bins)
    gpu_ctx.cluster_pack(1, 2)
    prm = orc.params(1, 0.93, 58, 68)
    lens = [sorted((len(s) for s in seqs[bins[b]:bins[b + 1]] if 58 <= len(s) <= 68), reverse=True) for b in range(3)]
    s1 = len(lens[0])
    s2 = s1 + len(lens[1])
    g = gpu_ctx.prefilter_pack(1, 2, list(range(s1, s1 + 30)) + list(range(s2, s2 + 10)), s2 + 20, 10, 1, 16)
    assert (g["ntop"] > 0).any()
    with pytest.raises(_lib.UmiclustError) as e:
        gpu_ctx.fetch_bin(1)
    assert e.value.code == -77
    st = gpu_ctx.cluster_pack(1, 2)
    want = 0
    for b in (1, 2):
        o = orc.cluster(prm, seqs[bins[b]:bins[b + 1]])
        f = gpu_ctx.fetch_bin(b)
        assert f["n_clusters"] == o["n_clusters"] and f["consensus"] == o["consensus"]
        for k in ("cluster", "strand", "centroid"):
            assert np.array_equal(f[k], o[k]), (b, k)
        want += o["stats"]["alignments"]
    assert st["n_alignments"] == want


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
        with pytest.raises(_lib.UmiclustError) as e:
            ctx.prefilter_split([0], [10], 10, 4)
        assert e.value.code == -22
        ctx.load(_lib.params(1, 0.93, 58, 68), seqs)
        # split passes: new centroids outside block j-2, not increasing, a centroid in the window, a block past the load
        for args in (([0], [14], 10, 4), ([0], [9], 10, 4), ([0], [11, 11], 10, 4), ([0, 10], [11], 10, 4),
                     ([0], [10], 240, 4), ([0], [10], 10, 4, 0)):
            with pytest.raises(_lib.UmiclustError) as e:
                ctx.prefilter_split(*args)
            assert e.value.code == -22, args
        with pytest.raises(_lib.UmiclustError) as e:
            ctx.prefilter_pack(0, 2, [0], 20, 4)  # a pack outside the single-bin load
        assert e.value.code == -22
        buf, off = _lib._pack(seqs)
        ctx.load_bins(_lib.params(1, 0.93, 58, 68), buf, off, [0, 100, len(seqs)])  # several bins
        with pytest.raises(_lib.UmiclustError) as e:
            ctx.prefilter([0], 20, 4)  # no pack named
        assert e.value.code == -22
        with pytest.raises(_lib.UmiclustError) as e:
            ctx.prefilter_split([0], [10], 10, 4)
        assert e.value.code == -22
        # packs: outside the load, empty, a centroid of bin 1 without the bin's first sequence (100), a centroid and a
        # window before the pack, a block past the pack
        for args in ((1, 2, [100], 120, 4), (2, 1, [], 120, 4), (0, 0, [0], 20, 4), (-1, 2, [0], 20, 4),
                     (0, 2, [0, 101], 120, 4), (0, 2, [101], 120, 4), (1, 1, [0, 100], 120, 4), (1, 1, [100], 104, 4, 2),
                     (0, 1, [0], 98, 4), (0, 2, [0], 248, 4)):
            with pytest.raises(_lib.UmiclustError) as e:
                ctx.prefilter_pack(*args)
            assert e.value.code == -22, args
        g = ctx.prefilter_pack(0, 2, [0, 100], 120, 4)  # ... and what is covered
        assert len(g["ntop"]) == 8
