"""The `seqkit stat -a` tables of the fastq_filter pass (row f5b, policy O8 of DESIGN.md §9a) on the GPU through the C
ABI: k_fastq_stats against Python integers and against k_fastq_ee, whole files against tests/fastq_stats_ref.py and
against the plain filter, chunk seams, a host-only record, the statistics-only pass and the reference-shaped wrapper."""
import os

import numpy as np
import pytest
from umiclust import _lib, preprocessing, vsearch_umi_cluster

import fastq_filter_ref as ref
import fastq_stats_ref as sref

pytestmark = pytest.mark.gpu

COUNTERS = ("n_input", "n_kept", "n_discarded", "bases_in", "bases_kept", "n_short", "n_long", "n_maxee",
            "n_maxee_rate", "n_host_rechecked", "n_chunks", "ee_in", "ee_kept")

# ---- 1. the kernel ----
LENS_DOWN = [15, 31, 63, 255, 1023]                  # each moves the next start down by one (mod 16)
LENS_UP = [1, 17, 33, 65, 257, 1025, 4097, 70001]    # ... up by one
LENS_SAME = [0, 16, 32, 64, 256, 1024]
SEQ_BYTES = np.array([b for b in range(256) if b not in (10, 13)], np.uint8)  # 254 values: no line ends


@pytest.mark.parametrize("ascii_", [33, 64])
def test_kernel_exact(gpu_ctx, ascii_):
    rng = np.random.default_rng(4321 + ascii_)

    def rec(n):  # every quality value, every sequence byte: a neighbour's bytes differ in class from the record's own
        return (SEQ_BYTES[rng.integers(0, len(SEQ_BYTES), n)].tobytes(),
                (ascii_ + rng.integers(0, 94, n)).astype(np.uint8).tobytes())
    q6, q1 = bytes([ascii_ + 93]) * 6, bytes([ascii_])
    recs = [rec(n) for n in LENS_DOWN] + [(b"GcNn-.", q6)] + [rec(n) for n in LENS_UP] + [(b" ", q1)] + \
           [rec(n) for n in LENS_SAME]
    starts = np.cumsum([0] + [len(s) for s, _ in recs])[:-1]
    assert set(int(s) % 16 for s in starts) == set(range(16))
    seqs, quals = [s for s, _ in recs], [q for _, q in recs]
    ee, lo, hi, cnt = gpu_ctx.fastq_record_stats(seqs, quals, ascii_)
    assert cnt.shape == (len(recs), 5) and cnt.dtype == np.uint32
    _, fx = ref.tables(ascii_, 0, 93)
    for i, (s, q) in enumerate(recs):
        assert int(ee[i]) == sum(fx[b] for b in q), (i, len(q))
        assert (int(lo[i]), int(hi[i])) == ((min(q), max(q)) if q else (255, 0)), (i, len(q))
        want = [sum(1 for b in q if b - ascii_ >= 20), sum(1 for b in q if b - ascii_ >= 30),
                sum(1 for b in s if b in b"GCgc"), sum(1 for b in s if b in b"Nn"), sum(1 for b in s if b in b"-. ")]
        assert [int(x) for x in cnt[i]] == want, (i, len(q))
    assert [int(x) for x in cnt[5]] == [6, 6, 2, 2, 2] and [int(x) for x in cnt[14]] == [0, 0, 0, 0, 1]
    assert cnt[:, 2:].sum(axis=0).min() > 200  # every class is met many times
    ee0, lo0, hi0 = gpu_ctx.fastq_ee(quals, ascii_)  # bit-identical to k_fastq_ee on the same input
    assert np.array_equal(ee, ee0) and np.array_equal(lo, lo0) and np.array_equal(hi, hi0)


def test_record_above_the_device_limit_is_erange(gpu_ctx):
    n = (1 << 22) + 1
    with pytest.raises(_lib.UmiclustError) as e:
        gpu_ctx.fastq_record_stats([b"A" * n], [b"I" * n])
    assert e.value.code == -34
    ee, lo, hi, cnt = gpu_ctx.fastq_record_stats([], [])
    assert len(ee) == 0 and cnt.shape == (0, 5)


# ---- 2. / 3. file parity and chunk seams ----
SEED = 20261020


@pytest.fixture(scope="module")
def reads():
    """the 3,000-read input and the restatement's numbers of its two tables under the reference's thresholds"""
    data = ref.synth_reads(3000, seed=SEED, max_len=3000)
    _, _, nb, na = sref.tables(data, "", "", minlen=1470, rate=0.07)
    return data, nb, na


def _same_as_fixture(got, nb, na):
    res, before, after, _, _, in_path, out_path = got
    assert before == sref.table_from_numbers(in_path, nb)
    assert after == sref.table_from_numbers(out_path, na)
    assert res["before"] == nb and res["after"] == na


def _run_stats(ctx, tmp_path, data, name="x", outputs=True, **kw):
    """-> (result dict, before bytes, after bytes, kept bytes, discarded bytes, in path, out path)"""
    src = tmp_path / f"{name}.fastq"
    if not src.exists():
        src.write_bytes(data)
    kept, disc, log = tmp_path / f"{name}_skept.fq", tmp_path / f"{name}_sdisc.fq", tmp_path / f"{name}_s.log"
    before, after = tmp_path / f"{name}_before.txt", tmp_path / f"{name}_after.txt"
    p = _lib.fastq_filter_params(fastq_ascii=kw.get("ascii_", 33), fastq_qmax=93, fastq_minlen=kw.get("minlen", 1),
                                 fastq_maxee_rate=kw.get("rate", -1.0))
    if outputs:
        res = ctx.fastq_filter_stats(p, str(src), str(kept), str(disc), str(log), str(before), str(after))
        return res, before.read_bytes(), after.read_bytes(), kept.read_bytes(), disc.read_bytes(), str(src), str(kept)
    res = ctx.fastq_filter_stats(p, str(src), stats_before_txt=str(before), stats_after_txt=str(after))
    return res, before.read_bytes(), after.read_bytes(), None, None, str(src), "-"


def _same_tables(data, got, **kw):
    res, before, after, _, _, in_path, out_path = got
    tb, ta, nb, na = sref.tables(data, in_path, out_path, **kw)
    assert before == tb, (before, tb)
    assert after == ta, (after, ta)
    assert res["before"] == nb and res["after"] == na


def test_file_parity(gpu_ctx, tmp_path, reads):
    reads, nb, na = reads
    got = _run_stats(gpu_ctx, tmp_path, reads, minlen=1470, rate=0.07)
    _same_as_fixture(got, nb, na)
    res, _, _, kept, disc, in_path, _ = got
    assert res["before"]["num_seqs"] == 3000 and 100 < res["after"]["num_seqs"] < 1500
    assert res["t_kernel_s"] > 0 and res["t_h2d_s"] > 0 and res["n_chunks"] == 1
    # the filter's own outputs and counters are the plain call's
    p = _lib.fastq_filter_params(fastq_qmax=93, fastq_minlen=1470, fastq_maxee_rate=0.07)
    k2, d2 = tmp_path / "plain_kept.fq", tmp_path / "plain_disc.fq"
    plain = gpu_ctx.fastq_filter(p, in_path, str(k2), str(d2), str(tmp_path / "plain.log"))
    assert kept == k2.read_bytes() and disc == d2.read_bytes()
    for k in COUNTERS:
        assert res[k] == plain[k], k
    assert kept == ref.run(reads, minlen=1470, rate=0.07)[0]


def test_chunk_seams(tmp_path, reads, monkeypatch):
    reads, nb, na = reads
    monkeypatch.setenv("UMICLUST_FQ_CHUNK", str(1024))  # the smallest chunk: a record or two in each
    with _lib.Context(0) as ctx:
        got = _run_stats(ctx, tmp_path, reads, minlen=1470, rate=0.07)
    _same_as_fixture(got, nb, na)
    assert got[0]["n_chunks"] >= 1000


def _whole_records(data, limit):
    """the longest prefix of whole records within `limit` bytes"""
    recs, out, size = ref.parse(data), [], 0
    for label, s, q in recs:
        size += len(label) + 2 * len(s) + 6
        if size > limit:
            break
        out.append(b"@" + label + b"\n" + s + b"\n+\n" + q + b"\n")
    return b"".join(out)


def test_fastq_ascii_64_and_classes(gpu_ctx, tmp_path):
    rng = np.random.default_rng(64)
    alphabet = np.frombuffer(b"ACGTacgtNn-. RYKM", np.uint8)
    data = b"".join(b"@c%d\n" % i + alphabet[rng.integers(0, len(alphabet), n)].tobytes() + b"\n+\n" +
                    (64 + rng.integers(0, 63, n)).astype(np.uint8).tobytes() + b"\n"
                    for i, n in enumerate([64, 33, 200, 15, 1, 1000, 257]))
    got = _run_stats(gpu_ctx, tmp_path, data, name="a64", ascii_=64, minlen=20, rate=0.2)
    _same_tables(data, got, ascii_=64, minlen=20, rate=0.2)
    b = got[0]["before"]
    assert min(b["n_gc"], b["sum_n"], b["sum_gap"], b["n_q30"]) > 10


# ---- 4. a record evaluated on the host among device records ----
def test_host_only_record(gpu_ctx, tmp_path):
    rng = np.random.default_rng(6)
    short = ref.synth_reads(40, seed=66, max_len=300, min_len=1)
    n = (1 << 22) + 1
    s = np.frombuffer(b"ACGTNn-", np.uint8)[rng.integers(0, 7, n)].tobytes()
    q = (33 + rng.integers(5, 41, n)).astype(np.uint8).tobytes()
    cut = short.index(b"@read20")
    data = short[:cut] + b"@big one\n" + s + b"\n+\n" + q + b"\n" + short[cut:]
    got = _run_stats(gpu_ctx, tmp_path, data, name="big", minlen=50, rate=0.2)
    _same_tables(data, got, minlen=50, rate=0.2)
    assert got[0]["before"]["max_len"] == n and got[0]["after"]["max_len"] == n


# ---- 5. statistics only ----
def test_stats_only_pass(gpu_ctx, tmp_path, reads):
    data = _whole_records(reads[0], 300000)
    got = _run_stats(gpu_ctx, tmp_path, data, name="only", outputs=False, minlen=1470, rate=0.07)
    _same_tables(data, got, minlen=1470, rate=0.07)
    assert not (tmp_path / "only_skept.fq").exists() and not (tmp_path / "only_s.log").exists()
    assert got[0]["n_kept"] == got[0]["after"]["num_seqs"] > 0


def test_eformat_writes_no_stats_file(gpu_ctx, tmp_path):
    good = ref.synth_reads(20, seed=14, max_len=200, min_len=20)
    src = tmp_path / "bad.fastq"
    src.write_bytes(good + b"@low\nACGT\n+\nII\x1fI\n")
    with pytest.raises(_lib.UmiclustError) as e:
        gpu_ctx.fastq_filter_stats(_lib.fastq_filter_params(fastq_qmax=93), str(src), str(tmp_path / "bad_kept.fq"),
                                   stats_before_txt=str(tmp_path / "b.txt"), stats_after_txt=str(tmp_path / "a.txt"))
    assert e.value.code == -74
    assert not (tmp_path / "b.txt").exists() and not (tmp_path / "a.txt").exists()
    assert (tmp_path / "bad_kept.fq").read_bytes() == ref.run(good)[0]


# ---- 6. the wrapper ----
def test_wrapper(gpu_ctx, tmp_path, monkeypatch):
    monkeypatch.setitem(vsearch_umi_cluster._CTX, 0, gpu_ctx)
    monkeypatch.delenv("UMICLUST_DEVICE", raising=False)
    lib_dir, out_dir, log_dir = tmp_path / "fastq" / "libA", tmp_path / "out", tmp_path / "logs"
    for d in (lib_dir, out_dir, log_dir):
        d.mkdir(parents=True)
    data = ref.synth_reads(200, seed=9, max_len=2500)
    src = lib_dir / "sample1.trimmed.fastq"
    src.write_bytes(data)
    ret = preprocessing.vsearch_fastq_filtering_with_stats.remote(str(src), {"libA": str(out_dir)},
                                                                  {"libA": str(log_dir)}, 0.07, 1470)
    assert ret == os.path.join(str(out_dir), "sample1_filtered.fastq")
    want_kept, _, c = ref.run(data, minlen=1470, rate=0.07)
    assert open(ret, "rb").read() == want_kept and c["n_kept"] > 0
    tb, ta, _, na = sref.tables(data, str(src), ret, minlen=1470, rate=0.07)
    assert (log_dir / "sample1_stats_before_vsearch_filtering.txt").read_bytes() == tb
    assert (log_dir / "sample1_stats_after_vsearch_filtering.txt").read_bytes() == ta
    assert na["num_seqs"] == c["n_kept"]
    log = (log_dir / "sample1_vsearch_fastq_filtering.log").read_text()
    assert f"{c['n_kept']} sequences kept (of which 0 truncated), {c['n_discarded']} sequences discarded." in log
