"""bench.py's output dump (--dump-outputs): names, dtypes, the size budget and the fixed sample."""
import os

import numpy as np

import bench


def _result(rng, n, k, length=64):
    return dict(n_clusters=k, cluster=rng.integers(0, k, n).astype(np.int32),
                strand=rng.integers(0, 2, n).astype(np.uint8), centroid=rng.integers(0, 2, n).astype(np.uint8),
                consensus=["".join(rng.choice(list("ACGT"), length)) for _ in range(k)])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_whole(tmp_path):
    rng = np.random.default_rng(7)
    res = [_result(rng, 1000, 50), _result(rng, 10, 2)]
    bench.dump_outputs(str(tmp_path / "d"), res, prefix="rank1_")
    got = _load(tmp_path / "d")
    assert sorted(got) == ["rank1_" + k for k in ("centroid", "cluster", "consensus", "consensus_length", "n_clusters",
                                                  "strand")]
    assert all(a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got["rank1_cluster"], np.concatenate([r["cluster"] for r in res]))
    assert got["rank1_n_clusters"].tolist() == [50, 2]
    assert got["rank1_consensus_length"].tolist() == [64] * 52
    assert bytes(got["rank1_consensus"].astype(np.uint8)).decode() == "".join(c for r in res for c in r["consensus"])


def test_dump_outputs_wide_values_and_budget(tmp_path, monkeypatch):
    rng = np.random.default_rng(8)
    res = [_result(rng, 400_000, 300)]
    res[0]["cluster"] = res[0]["cluster"].astype(np.int64) + (1 << 24)  # not exact in float32
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4_000_000)
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), res)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert a["cluster"].dtype == np.float64 and a["strand"].dtype == np.float32
    assert sum(x.nbytes for x in a.values()) <= 4_000_000
    assert 0 < a["cluster"].size < 400_000 and a["n_clusters"].tolist() == [300]
    assert all(np.array_equal(a[k], b[k]) for k in a)  # the same positions every time
