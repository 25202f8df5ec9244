"""The `seqkit stat -a` tables of the fastq_filter pass (row f5b, policy O8 of DESIGN.md §9a) without a GPU:
tools/fastq_check_main.cpp in stats mode runs the gatherer, the host restatement of k_fastq_stats, the two
accumulators, the histogram walk and the formatter under ASan + UBSan, and both tables are compared byte for byte with
tests/fastq_stats_ref.py.  Also the reader of the table (analysis.py:76-81 restated) and the reference-shaped wrapper.
A sanitizer report fails the test."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
from umiclust import _lib, preprocessing

import fastq_filter_ref as ref
import fastq_stats_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGV = json.load(open(os.path.join(ROOT, "tests", "golden", "argv_fastq_filter.json")))
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
EFORMAT = -74
INTS = ("num_seqs", "sum_len", "min_len", "max_len", "n50", "n50_num", "n_q20", "n_q30", "n_gc", "sum_n", "sum_gap")
DOUBLES = ("avg_len", "q1", "q2", "q3", "q20_pct", "q30_pct", "avg_qual", "gc_pct")


@pytest.fixture(scope="module")
def stats_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("fastq_stats_check")
    b = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ont-tcrconsensus_amd"), "fastq_check",
                        f"SAN_OUT={out}"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    assert "warning" not in b.stderr, b.stderr
    count = [0]

    def run(data, threads=3, chunk=64 << 20, ascii_=33, qmin=0, qmax=93, minlen=1, maxlen=-1, maxee=-1.0, rate=-1.0,
            outputs=True):
        """-> dict(rc, err, before / after: the table's bytes or None, nb / na: the struct's numbers, kept, in_path,
        out_path)"""
        count[0] += 1
        d = out / f"run{count[0]}"
        d.mkdir()
        (d / "in.fq").write_bytes(data)
        files = [d / "kept.fq", d / "disc.fq", d / "log.txt"] if outputs else ["-", "-", "-"]
        r = subprocess.run([str(out / "fastq_check"), "stats", str(d / "in.fq")] + [str(f) for f in files] +
                           [str(d / "before.txt"), str(d / "after.txt")] +
                           [str(a) for a in (threads, chunk, ascii_, qmin, qmax, minlen, maxlen, repr(float(maxee)),
                                             repr(float(rate)))],
                           capture_output=True, text=True, timeout=300, env=SAN_ENV)
        assert r.returncode == 0, r.stderr[-4000:]  # the checker ran ASan- and UBSan-clean
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
        kv = dict(line.split("=", 1) for line in r.stdout.strip("\n").split("\n"))
        res = dict(rc=int(kv["rc"]), err=kv["err"], in_path=str(d / "in.fq"),
                   out_path=str(d / "kept.fq") if outputs else "-", n_chunks=int(kv["n_chunks"]))
        for which, key in (("before", "nb"), ("after", "na")):
            path = d / f"{which}.txt"
            res[which] = path.read_bytes() if path.exists() else None
            nums = {k: int(kv[f"{which}.{k}"]) for k in INTS}
            nums.update({k: float.fromhex(kv[f"{which}.{k}"]) for k in DOUBLES})
            nums["ee_fx"] = (int(kv[f"{which}.ee_fx_hi"]) << 64) | int(kv[f"{which}.ee_fx_lo"])
            nums["type"] = ("DNA", "RNA", "Protein")[int(kv[f"{which}.type"])]
            res[key] = nums
        res["kept"] = (d / "kept.fq").read_bytes() if outputs and (d / "kept.fq").exists() else None
        return res
    return run


def _check(stats_check, data, **kw):
    """both tables and both structs equal the restatement's; returns the checker's result"""
    opts = {k: v for k, v in kw.items() if k not in ("threads", "chunk", "outputs")}
    got = stats_check(data, **kw)
    assert got["rc"] >= 0, got["err"]
    tb, ta, nb, na = sref.tables(data, got["in_path"], got["out_path"], **opts)
    assert got["before"] == tb, (got["before"], tb)
    assert got["after"] == ta, (got["after"], ta)
    assert got["nb"] == nb and got["na"] == na
    assert got["rc"] == na["num_seqs"]
    return got


def _fastq(recs) -> bytes:
    return b"".join(b"@s%d\n" % i + s + b"\n+\n" + q + b"\n" for i, (s, q) in enumerate(recs))


def _rec(rng, n, alphabet=b"ACGT", qlo=0, qhi=60, ascii_=33):
    s = np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()
    return s, (ascii_ + rng.integers(qlo, qhi + 1, n)).astype(np.uint8).tobytes()


LENS = [3, 10, 4, 25, 7, 1, 18, 12, 30]


def test_random_reads_reference_thresholds(stats_check):
    data = ref.synth_reads(3000, seed=20261020, max_len=3000)
    got = _check(stats_check, data, threads=4, minlen=1470, rate=0.07)
    assert got["nb"]["num_seqs"] == 3000 and 100 < got["na"]["num_seqs"] < 1500
    assert got["na"]["min_len"] >= 1470 and got["nb"]["n_q20"] > got["nb"]["n_q30"] > 0
    assert got["nb"]["ee_fx"] > 2 ** 53  # the sum's conversion to double rounds


def test_empty_file(stats_check):
    got = _check(stats_check, b"")
    for t in (got["before"], got["after"]):
        head, row = t.decode().split("\n")[:2]
        assert row.split()[1:] == ["FASTQ", "DNA", "0", "0", "0", "0.0", "0", "0.0", "0.0", "0.0", "0", "0", "0",
                                   "0.00", "0.00", "0.00", "0.00", "0"]


def test_one_record(stats_check):
    rng = np.random.default_rng(1)
    got = _check(stats_check, _fastq([_rec(rng, 41)]))
    nb = got["nb"]
    assert (nb["q1"], nb["q2"], nb["q3"], nb["n50"], nb["n50_num"]) == (41.0, 41.0, 41.0, 41, 1)


@pytest.mark.parametrize("n", range(2, 10))
def test_record_counts_two_to_nine(stats_check, n):
    """even and odd n, even and odd halves; the kept set (minlen 4) has other counts again"""
    rng = np.random.default_rng(100 + n)
    data = _fastq([_rec(rng, ln) for ln in LENS[:n]])
    _check(stats_check, data, threads=2)
    _check(stats_check, data, threads=1, chunk=1024, minlen=4, rate=0.3)


def test_quartiles_and_n50_by_hand(stats_check):
    rng = np.random.default_rng(7)
    got = _check(stats_check, _fastq([_rec(rng, ln) for ln in (1, 2, 3, 4, 5, 6, 7)]))
    nb = got["nb"]  # lower half 1 2 3, upper half 5 6 7; 7 + 6 + 5 = 18 >= 14 is the first at or above half of 28
    assert (nb["q1"], nb["q2"], nb["q3"], nb["n50"], nb["n50_num"], nb["avg_len"]) == (2.0, 4.0, 6.0, 5, 3, 4.0)
    got = _check(stats_check, _fastq([_rec(rng, ln) for ln in (10, 10, 20, 40)]))
    nb = got["nb"]  # 40 >= 40: exactly half counts
    assert (nb["q1"], nb["q2"], nb["q3"], nb["n50"], nb["n50_num"]) == (10.0, 15.0, 30.0, 40, 1)


def test_all_records_the_same_length(stats_check):
    rng = np.random.default_rng(3)
    got = _check(stats_check, _fastq([_rec(rng, 37) for _ in range(11)]), chunk=1024)
    nb = got["nb"]
    assert (nb["min_len"], nb["max_len"], nb["q1"], nb["q2"], nb["q3"], nb["n50"], nb["n50_num"]) == \
        (37, 37, 37.0, 37.0, 37.0, 37, 6)
    got = _check(stats_check, _fastq([(b"", b"")] * 3))  # empty records only: every ratio is 0
    assert (got["nb"]["num_seqs"], got["nb"]["sum_len"], got["nb"]["n50_num"], got["nb"]["avg_qual"]) == (3, 0, 1, 0.0)


def test_no_record_kept(stats_check):
    rng = np.random.default_rng(4)
    got = _check(stats_check, _fastq([_rec(rng, ln) for ln in LENS]), minlen=1000)
    assert got["rc"] == 0 and got["na"]["num_seqs"] == 0 and got["kept"] == b""
    assert got["after"].decode().split("\n")[1].split()[3:] == ["0", "0", "0", "0.0", "0", "0.0", "0.0", "0.0", "0",
                                                                 "0", "0", "0.00", "0.00", "0.00", "0.00", "0"]


def test_composition_classes(stats_check):
    rng = np.random.default_rng(5)
    recs = [_rec(rng, ln, alphabet=b"ACGTacgtNn-. RYKM*") for ln in (64, 33, 200, 15, 1)]
    got = _check(stats_check, _fastq(recs), chunk=1024)
    nb = got["nb"]
    assert min(nb["n_gc"], nb["sum_n"], nb["sum_gap"]) > 10 and nb["type"] == "DNA"
    s = b"".join(r[0] for r in recs)
    assert nb["n_gc"] == sum(s.count(c) for c in (b"G", b"C", b"g", b"c"))
    assert nb["sum_n"] == s.count(b"N") + s.count(b"n") and nb["sum_gap"] == sum(s.count(c) for c in (b"-", b".", b" "))


@pytest.mark.parametrize("first,want", [(b"ACGTNRYKM-acgtn", "DNA"), (b"ACGUacgu", "RNA"), (b"ACGUT", "Protein"),
                                        (b"MKVLAAGIE", "Protein"), (b"", "DNA"), (b"--..", "DNA")])
def test_type_from_the_first_record(stats_check, first, want):
    data = _fastq([(first, b"I" * len(first)), (b"MKVLEEF", b"IIIIIII")])
    got = _check(stats_check, data)
    assert got["nb"]["type"] == want and got["before"].decode().split("\n")[1].split()[2] == want


def test_multi_line_records(stats_check):
    multi = b"@m0 c\nACGT\nACGNAC\n+\nIIII\n@IIII+\n\n@m1\nAC\n+\n@@\n@m2\nAC-TgCGT\n+\n+II\nII\n@II"
    for threads in (1, 3):
        got = _check(stats_check, multi, threads=threads, chunk=1024)
        assert (got["nb"]["num_seqs"], got["nb"]["sum_len"], got["nb"]["sum_n"], got["nb"]["sum_gap"]) == (3, 20, 1, 1)


def test_fastq_ascii_64(stats_check):
    rng = np.random.default_rng(6)
    recs = [_rec(rng, ln, qlo=0, qhi=62, ascii_=64) for ln in (50, 17, 300)]
    got = _check(stats_check, _fastq(recs), ascii_=64, minlen=20, rate=0.2)
    assert 0 < got["nb"]["n_q30"] < got["nb"]["n_q20"] < got["nb"]["sum_len"]


def test_qualities_at_19_20_29_30(stats_check):
    for ascii_ in (33, 64):
        quals = bytes([ascii_ + q for q in (19, 20, 29, 30, 19, 20, 29, 30, 0, 93)])
        got = _check(stats_check, _fastq([(b"ACGTACGTAC", quals)]), ascii_=ascii_)
        assert (got["nb"]["n_q20"], got["nb"]["n_q30"]) == (7, 3)


def test_record_longer_than_the_device_limit(stats_check):
    """2^22 + 1 bases: counted by the host restatement alone, among records that go through the backend"""
    rng = np.random.default_rng(8)
    n = (1 << 22) + 1
    big = _rec(rng, n, alphabet=b"ACGTNn-", qlo=5, qhi=40)
    small = [_rec(rng, ln) for ln in (100, 3000, 257)]
    data = _fastq(small[:2] + [big] + small[2:])
    got = _check(stats_check, data, minlen=200, rate=0.2)
    assert got["nb"]["max_len"] == n and got["na"]["max_len"] == n and got["nb"]["n50"] == n


def test_tables_do_not_depend_on_the_chunk(stats_check):
    data = ref.synth_reads(300, seed=12, max_len=900)
    a = _check(stats_check, data, threads=4, chunk=1024, minlen=300, rate=0.07)
    b = _check(stats_check, data, threads=1, minlen=300, rate=0.07)
    assert a["n_chunks"] > 50 and b["n_chunks"] == 1
    strip = lambda t, p: t.replace(p.encode(), b"F")  # noqa: E731 - the file column holds each run's own path
    assert strip(a["before"], a["in_path"]) == strip(b["before"], b["in_path"])
    assert strip(a["after"], a["out_path"]) == strip(b["after"], b["out_path"])
    assert a["nb"] == b["nb"] and a["na"] == b["na"]


def test_stats_only_pass(stats_check):
    data = ref.synth_reads(50, seed=13, max_len=400)
    got = _check(stats_check, data, minlen=100, rate=0.07, outputs=False)
    assert got["kept"] is None and got["after"].decode().split("\n")[1].split()[0] == "-"


def test_eformat_writes_no_stats_file(stats_check):
    good = ref.synth_reads(20, seed=14, max_len=200, min_len=20)
    for data in (good + b"@bad\nACGTACGT\n+\nIIII\n@after\nAC\n+\nII\n",          # malformed record
                 good + b"@low\nACGT\n+\nII\x1fI\n"):                               # a quality below fastq_ascii
        got = stats_check(data, chunk=1024)
        assert got["rc"] == EFORMAT and got["before"] is None and got["after"] is None
        assert got["kept"] == ref.run(good)[0]  # the filter's own outputs are what they were
        assert got["nb"]["num_seqs"] == 0 and got["na"]["num_seqs"] == 0


# ---- the reader of the table (analysis.py:76-81, without pandas) ----
def _avg_qual_as_the_pipeline_reads_it(text: str) -> float:
    head, row = text.split("\n")[:2]
    names, vals = head.split(), row.split()
    assert len(names) == len(vals)
    return float(vals[names.index("AvgQual")])


def test_reader_contract(stats_check):
    data = ref.synth_reads(200, seed=15, max_len=2000)
    got = _check(stats_check, data, minlen=500, rate=0.07)
    for which, nums in (("before", got["nb"]), ("after", got["na"])):
        text = got[which].decode()
        assert text.count("\n") == 2 and text.endswith("\n")
        assert text.split("\n")[0].split() == sref.COLUMNS and len(sref.COLUMNS) == 19
        want = sref.numbers(ref.parse(data if which == "before" else got["kept"]))["avg_qual"]
        assert _avg_qual_as_the_pipeline_reads_it(text) == float("%.2f" % want)
        assert 5.0 < want < 30.0 and nums["avg_qual"] == want


# ---- the wrapper ----
def test_wrapper_builds_the_reference_argv_and_paths(monkeypatch):
    for call in ARGV["calls"]:
        a, seen = call["args"], []
        monkeypatch.setattr(preprocessing, "run_fastq_filter_stats", lambda *x: seen.append(x))
        monkeypatch.setattr(preprocessing, "run_fastq_filter", lambda argv: pytest.fail("the plain filter ran"))
        ret = preprocessing.vsearch_fastq_filtering_with_stats(a["fastq"], a["out"], a["logs"],
                                                               a["max_ee_rate_base"], a["minimal_length"])
        log = call["argv"][call["argv"].index("--log") + 1]
        stem = log[:-len("_vsearch_fastq_filtering.log")]  # preprocessing.py:117-118: the same directory and name
        assert log.endswith("_vsearch_fastq_filtering.log")
        assert seen == [(call["argv"], stem + "_stats_before_vsearch_filtering.txt",
                         stem + "_stats_after_vsearch_filtering.txt")] and ret == call["ret"]
        assert preprocessing.vsearch_fastq_filtering_with_stats.remote(
            a["fastq"], a["out"], a["logs"], a["max_ee_rate_base"], a["minimal_length"]) == call["ret"]


def test_bindings_are_declared():
    for name in ("umiclust_fastq_filter_stats", "umiclust_fastq_filter_stats_argv", "umiclust_fastq_record_stats"):
        assert name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 9
    assert [k for k, _ in _lib.FastqStats._fields_][:4] == ["num_seqs", "sum_len", "min_len", "max_len"]
