"""The four alignment kernels, pair by pair against the CPU oracle, on the edge inputs of tests/align_cases.py under
every scoring set load.cpp validate() accepts (the presets and the corners of its domain, both boundary policies).

 * pk:    k_align_pk (packed 16-bit, one pair per lane), selected for every launch by UMICLUST_BAND=0;
 * band:  k_align_band (groups of 4 or 8 lanes), selected for every launch by UMICLUST_BAND=1<<30;
 * amb:   k_align<QL, true>, which runs a whole call as soon as one sequence of it holds an ambiguous symbol;
 * trace: k_trace_wave (with_ops=True), compared on the ops as well.

tests/test_align_ref_cpu.py shows, without a GPU, that every rule of the operation decides one of these cases.
Bit-exact: score, matches, internal length (and ops) are integers.
"""
import align_cases as A
import numpy as np
import pytest
from umiclust import _lib

pytestmark = pytest.mark.gpu


def _context(kernel, monkeypatch):
    """tunables are read when the context is created"""
    if kernel in A.BAND_ENV:
        monkeypatch.setenv("UMICLUST_BAND", A.BAND_ENV[kernel])
    return _lib.Context(0)


def _check(kernel, s, labels, pairs, r, want):
    """labels[k] names pair k's family (or launch shape); want[k] = (score, matches, internal_len, ops)"""
    got = np.stack([r["score"], r["matches"], r["internal_len"]], axis=1).astype(np.int64)
    exp = np.array([w[:3] for w in want], np.int64).reshape(-1, 3)
    bad = np.flatnonzero((got != exp).any(axis=1)).tolist()
    if kernel == "trace":
        bad = sorted(set(bad) | {k for k, w in enumerate(want) if r["ops"][k] != w[3]})
    if bad:
        lines = [f"kernel {kernel}, scoring {s.name}: {len(bad)} of {len(pairs)} pairs differ from the oracle"]
        for k in bad[:6]:
            g = tuple(int(x) for x in got[k]) + ((r["ops"][k],) if kernel == "trace" else ())
            w = want[k] if kernel == "trace" else want[k][:3]
            lines.append(f"  family {labels[k]}, pair {k}: q={pairs[k][0]} t={pairs[k][1]}\n    got    {g}\n    wanted {w}")
        pytest.fail("\n".join(lines), pytrace=False)


@pytest.mark.parametrize("s", A.ACCEPTED, ids=[s.name for s in A.ACCEPTED])
@pytest.mark.parametrize("kernel", A.KERNELS)
def test_kernel_vs_oracle(kernel, s, monkeypatch):
    """Every case of the kernel in one align_pairs call (one launch per query length 32..112, pairs in case order)."""
    cases = A.kernel_cases(kernel)
    pairs = [(q, t) for _, q, t in cases]
    nb = len(A.base_cases())
    want = A.expected(s, "base", pairs[:nb]) + (A.expected(s, "iupac", pairs[nb:]) if len(pairs) > nb else [])
    assert len(want) == len(pairs)
    with _context(kernel, monkeypatch) as ctx:
        r = ctx.align_pairs(s.lib_params(), [q for q, _ in pairs], [t for _, t in pairs], with_ops=kernel == "trace")
    _check(kernel, s, [f for f, _, _ in cases], pairs, r, want)


@pytest.mark.parametrize("s", A.ACCEPTED, ids=[s.name for s in A.ACCEPTED])
@pytest.mark.parametrize("kernel", ["pk", "band"])
def test_launch_shapes_vs_oracle(kernel, s, monkeypatch):
    """One align_pairs call per shape, all pairs of one query length, so the pair count is the launch size: partial
    and full waves and lane groups, targets of 1 and 112 bases side by side, one target shared by every pair."""
    p = s.lib_params()
    with _context(kernel, monkeypatch) as ctx:
        for name, pairs in A.launch_shapes():
            r = ctx.align_pairs(p, [q for q, _ in pairs], [t for _, t in pairs])
            _check(kernel, s, [name] * len(pairs), pairs, r, A.expected(s, name, pairs))


_Q = "ACGTTGCAAGCTTAGGCATCGATCGGATTACAGGCTA"


@pytest.mark.parametrize("s", A.REFUSED, ids=[s.name for s in A.REFUSED])
def test_refused_scoring_sets(gpu_ctx, s):
    """What the 16-bit cells cannot hold is refused with UMICLUST_EINVAL and a message naming the field, by the probe
    and by load alike; the context stays usable."""
    for call in (lambda: gpu_ctx.align_pairs(s.lib_params(), [_Q], [_Q[3:]]), lambda: gpu_ctx.load(s.lib_params(), [_Q])):
        with pytest.raises(_lib.UmiclustError) as e:
            call()
        assert e.value.code == -22 and s.refused in str(e.value), (s.name, str(e.value))
    ok = A.BY_NAME["preset1_bo1"]
    r = gpu_ctx.align_pairs(ok.lib_params(), [_Q], [_Q[3:]])
    assert (int(r["score"][0]), int(r["matches"][0]), int(r["internal_len"][0])) == A.orc_ref(ok, _Q, _Q[3:])[:3]


def test_validate_line_is_66(gpu_ctx):
    """2 * 112 * mx <= 15000: mx = |match| + |mismatch| = 66 and go + ge = 66 are accepted, 67 is refused."""
    for name in ("m33x33_ext66_bo1", "m0x66_open66_bo0", "m66x0_interior_bo1"):
        s = A.BY_NAME[name]
        assert max(abs(s.match) + abs(s.mismatch), max(a + b for a, b in zip(s.go, s.ge))) == 66
        gpu_ctx.align_pairs(s.lib_params(), [_Q], [_Q])
    for name in ("mx67", "ext67"):
        with pytest.raises(_lib.UmiclustError) as e:
            gpu_ctx.align_pairs(A.BY_NAME[name].lib_params(), [_Q], [_Q])
        assert e.value.code == -22
