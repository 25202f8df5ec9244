"""The fastq_filter drop-in (row f5) on the GPU through the C ABI: the quality kernel against Python
integers, whole files against the restatement in tests/fastq_filter_ref.py (policies O7a-O7d), the guard band at the
threshold, chunk seams, the error paths, host-only records and the reference-shaped wrapper."""
import math
import os

import numpy as np
import pytest
from umiclust import _lib, preprocessing, vsearch_umi_cluster

import fastq_filter_ref as ref

pytestmark = pytest.mark.gpu

EINVAL, EFORMAT = -22, -74
COUNTERS = ("n_input", "n_kept", "n_discarded", "bases_in", "bases_kept", "n_short", "n_long", "n_maxee",
            "n_maxee_rate", "ee_in", "ee_kept")


def _run(ctx, tmp_path, data, name="x", **kw):
    """-> (result dict, kept bytes, discarded bytes, log text)"""
    src = tmp_path / f"{name}.fastq"
    if not src.exists():
        src.write_bytes(data)
    kept, disc, log = tmp_path / f"{name}_kept.fq", tmp_path / f"{name}_disc.fq", tmp_path / f"{name}.log"
    p = _lib.fastq_filter_params(fastq_ascii=kw.get("ascii_", 33), fastq_qmin=kw.get("qmin", 0),
                                 fastq_qmax=kw.get("qmax", 93), fastq_minlen=kw.get("minlen", 1),
                                 fastq_maxlen=kw.get("maxlen", -1), fastq_maxee=kw.get("maxee", -1.0),
                                 fastq_maxee_rate=kw.get("rate", -1.0))
    res = ctx.fastq_filter(p, str(src), str(kept), str(disc), str(log))
    return res, kept.read_bytes(), disc.read_bytes(), log.read_text()


def _same(res, got_kept, got_disc, want):
    want_kept, want_disc, c = want
    assert got_kept == want_kept and got_disc == want_disc
    for k in COUNTERS:
        assert res[k] == c[k], k


# ---- 1. the kernel ----
LENS_DOWN = [15, 31, 63, 255, 1023]                  # each moves the next start down by one (mod 16)
LENS_UP = [1, 17, 33, 65, 257, 1025, 4097, 70001]    # ... up by one
LENS_SAME = [0, 16, 32, 64, 256, 1024]


@pytest.mark.parametrize("ascii_", [33, 64])
def test_kernel_exact(gpu_ctx, ascii_):
    rng = np.random.default_rng(1234 + ascii_)

    def rec(n):
        return (ascii_ + rng.integers(0, 94, n)).astype(np.uint8).tobytes()  # all 94 quality values
    recs = [rec(n) for n in LENS_DOWN] + [b"~" * 6] + [rec(n) for n in LENS_UP] + [b"!"] + [rec(n) for n in LENS_SAME]
    starts = np.cumsum([0] + [len(r) for r in recs])[:-1]
    assert set(int(s) % 16 for s in starts) == set(range(16))
    ee, lo, hi = gpu_ctx.fastq_ee(recs, ascii_)
    _, fx = ref.tables(ascii_, 0, 93)
    for i, r in enumerate(recs):
        assert int(ee[i]) == sum(fx[b] for b in r), (i, len(r))
        assert (int(lo[i]), int(hi[i])) == ((min(r), max(r)) if r else (255, 0)), (i, len(r))
    if ascii_ == 33:
        assert int(ee[5]) == 6 * round(math.pow(10, -93 / 10) * 2 ** 40) and int(ee[14]) == 2 ** 40  # '~' is Q93, '!' is Q0
    else:
        assert int(ee[14]) == 0 and int(lo[14]) == 33  # '!' lies below fastq_ascii 64: adds nothing, shows in qlo


# ---- 2. / 4. file parity and chunk seams ----
SEED = 20261019


@pytest.fixture(scope="module")
def reads():
    data = ref.synth_reads(3000, seed=SEED, max_len=3000)
    return data, {"rate": ref.run(data, minlen=200, rate=0.07),
                  "both": ref.run(data, minlen=200, maxlen=2500, maxee=60.0, rate=0.07)}


def test_file_parity(gpu_ctx, tmp_path, reads):
    data, want = reads
    res, kept, disc, log = _run(gpu_ctx, tmp_path, data, minlen=200, rate=0.07)
    _same(res, kept, disc, want["rate"])
    c = want["rate"][2]
    assert c["n_in_band"] == 0 and res["n_host_rechecked"] == 0
    assert c["n_kept"] > 300 and c["n_maxee_rate"] > 300 and c["n_short"] > 100
    assert f"{c['n_kept']} sequences kept (of which 0 truncated), {c['n_discarded']} sequences discarded." in log
    assert res["n_chunks"] == 1 and res["t_kernel_s"] > 0 and res["t_h2d_s"] > 0
    res, kept, disc, _ = _run(gpu_ctx, tmp_path, data, minlen=200, maxlen=2500, maxee=60.0, rate=0.07)
    _same(res, kept, disc, want["both"])
    c = want["both"][2]
    assert c["n_in_band"] == 0 and res["n_host_rechecked"] == 0
    assert min(c["n_kept"], c["n_short"], c["n_long"], c["n_maxee"], c["n_maxee_rate"]) > 0


def test_chunk_seams(tmp_path, reads, monkeypatch):
    data, want = reads
    monkeypatch.setenv("UMICLUST_FQ_CHUNK", str(128 << 10))
    with _lib.Context(0) as ctx:
        res, kept, disc, _ = _run(ctx, tmp_path, data, minlen=200, rate=0.07)
    _same(res, kept, disc, want["rate"])
    assert res["n_chunks"] >= 20 and res["n_host_rechecked"] == 0


# ---- 3. the threshold ----
@pytest.mark.parametrize("q", [20, 10])
def test_threshold_records_are_decided_by_the_sequential_sum(gpu_ctx, tmp_path, q):
    p, _ = ref.tables()
    recs = []
    for n in range(1, 601):
        recs.append(bytes([33 + q]) * n)
        for d in (-1, 1):  # one base moved to the next quality value: decided on the device
            v = bytearray([33 + q]) * n
            v[n // 2] += d
            recs.append(bytes(v))
    data = b"".join(b"@t%d\n" % i + b"A" * len(r) + b"\n+\n" + r + b"\n" for i, r in enumerate(recs))
    rate = float(p[33 + q])
    want = ref.run(data, rate=rate)
    res, kept, disc, _ = _run(gpu_ctx, tmp_path, data, rate=rate)
    _same(res, kept, disc, want)
    assert want[2]["n_in_band"] == 600 and res["n_host_rechecked"] == 600
    # the sequential double sum puts constant-quality reads on both sides of the threshold
    const_kept = sum(1 for i in range(0, len(recs), 3) if b"@t%d\n" % i in kept)
    assert 0 < const_kept < 600


# ---- 5. error paths ----
def test_quality_below_ascii_is_eformat(gpu_ctx, tmp_path):
    data = ref.synth_reads(100, seed=5, max_len=400, min_len=20)
    lines = data.split(b"\n")
    q = bytearray(lines[4 * 40 + 3])
    q[len(q) // 3] = 32
    lines[4 * 40 + 3] = bytes(q)
    data = b"\n".join(lines)
    src, kept = tmp_path / "bad.fastq", tmp_path / "bad_kept.fq"
    src.write_bytes(data)
    with pytest.raises(_lib.UmiclustError) as e:
        gpu_ctx.fastq_filter(_lib.fastq_filter_params(fastq_qmax=93, fastq_minlen=100, fastq_maxee_rate=0.07), str(src),
                             str(kept))
    assert e.value.code == EFORMAT and "record 40 (read40)" in str(e.value)
    assert kept.read_bytes() == ref.run(data, minlen=100, rate=0.07, stop_at=40)[0]


def test_gzip_magic_is_einval(gpu_ctx, tmp_path):
    src = tmp_path / "z.fastq"
    src.write_bytes(b"\x1f\x8b\x08\x00" + bytes(64))
    with pytest.raises(_lib.UmiclustError) as e:
        gpu_ctx.fastq_filter(_lib.fastq_filter_params(), str(src), str(tmp_path / "o.fq"))
    assert e.value.code == EINVAL and "gzip" in str(e.value)


def test_empty_input(gpu_ctx, tmp_path):
    res, kept, disc, log = _run(gpu_ctx, tmp_path, b"")
    assert (res["n_input"], res["n_kept"], kept, disc) == (0, 0, b"", b"")
    assert "0 sequences kept (of which 0 truncated), 0 sequences discarded." in log


# ---- 6. records evaluated on the host ----
def test_record_longer_than_the_device_limit(gpu_ctx, tmp_path):
    rng = np.random.default_rng(6)
    short = ref.synth_reads(40, seed=66, max_len=300, min_len=1)
    n = (1 << 22) + 1
    q = (33 + np.clip(np.rint(rng.normal(14, 4, n)), 0, 60)).astype(np.uint8).tobytes()
    big = b"@big one\n" + b"A" * n + b"\n+\n" + q + b"\n"
    cut = short.index(b"@read20")
    data = short[:cut] + big + short[cut:]
    for rate in (0.02, 0.2):  # discarded, kept
        want = ref.run(data, minlen=50, rate=rate)
        res, kept, disc, _ = _run(gpu_ctx, tmp_path, data, name=f"big{rate}", minlen=50, rate=rate)
        _same(res, kept, disc, want)
    assert b"@big\n" in kept


# ---- 7. the wrapper ----
def test_wrapper(gpu_ctx, tmp_path, monkeypatch):
    monkeypatch.setitem(vsearch_umi_cluster._CTX, 0, gpu_ctx)
    monkeypatch.delenv("UMICLUST_DEVICE", raising=False)
    lib_dir, out_dir, log_dir = tmp_path / "fastq" / "libA", tmp_path / "out", tmp_path / "logs"
    for d in (lib_dir, out_dir, log_dir):
        d.mkdir(parents=True)
    data = ref.synth_reads(200, seed=9, max_len=2500)
    src = lib_dir / "sample1.trimmed.fastq"
    src.write_bytes(data)
    ret = preprocessing.vsearch_fastq_filtering.remote(str(src), {"libA": str(out_dir)}, {"libA": str(log_dir)}, 0.07,
                                                       1470)
    assert ret == os.path.join(str(out_dir), "sample1_filtered.fastq")
    want_kept, _, c = ref.run(data, minlen=1470, rate=0.07)
    assert open(ret, "rb").read() == want_kept and c["n_kept"] > 0
    log = (log_dir / "sample1_vsearch_fastq_filtering.log").read_text()
    assert f"{c['n_kept']} sequences kept (of which 0 truncated), {c['n_discarded']} sequences discarded." in log
