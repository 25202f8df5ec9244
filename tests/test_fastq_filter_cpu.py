"""The fastq_filter drop-in (row f5) without a GPU: the argv the reference builds
(tests/golden/argv_fastq_filter.json, captured from preprocessing.py:129-148), the option grammar (policy O7e), and
the HIP-free host side (ont-tcrconsensus_amd/csrc/fastq_filter.cpp) under ASan + UBSan: tools/fastq_check_main.cpp
runs the indexer, the decision, the band recheck and the writers with the host restatement of the kernel in place of
the device, and its outputs are compared with tests/fastq_filter_ref.py.  A sanitizer report fails the test."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
from umiclust import _lib, preprocessing

import fastq_filter_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGV = json.load(open(os.path.join(ROOT, "tests", "golden", "argv_fastq_filter.json")))
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
EINVAL, EFORMAT = -22, -74


# ---- argv ----
def test_argv_matches_reference():
    assert len(ARGV["calls"]) >= 2
    for call in ARGV["calls"]:
        a, argv = call["args"], call["argv"]
        assert argv[0] == "vsearch"
        filtered, log = argv[argv.index("-fastqout") + 1], argv[argv.index("--log") + 1]
        assert preprocessing.fastq_filter_argv(a["fastq"], filtered, log, a["max_ee_rate_base"],
                                               a["minimal_length"]) == argv
        assert call["ret"] == filtered


def test_wrapper_builds_the_reference_argv_and_return(monkeypatch):
    for call in ARGV["calls"]:
        a, seen = call["args"], []
        monkeypatch.setattr(preprocessing, "run_fastq_filter", lambda argv: seen.append(argv))
        ret = preprocessing.vsearch_fastq_filtering(a["fastq"], a["out"], a["logs"], a["max_ee_rate_base"],
                                                    a["minimal_length"])
        assert seen == [call["argv"]] and ret == call["ret"]
        assert preprocessing.vsearch_fastq_filtering.remote(a["fastq"], a["out"], a["logs"], a["max_ee_rate_base"],
                                                            a["minimal_length"]) == call["ret"]


def test_params_from_reference_argv():
    call = ARGV["calls"][0]
    assert (call["args"]["max_ee_rate_base"], call["args"]["minimal_length"]) == (0.07, 1470)
    for argv in (call["argv"], call["argv"][1:]):  # with and without the leading "vsearch"
        p, paths = _lib.fastq_filter_params_from_argv(argv)
        assert (p.fastq_ascii, p.fastq_qmin, p.fastq_qmax, p.fastq_minlen, p.fastq_maxlen) == (33, 0, 93, 1470, -1)
        assert p.fastq_maxee < 0 and p.fastq_maxee_rate == 0.07
        assert paths == {"in_fastq": call["args"]["fastq"], "fastqout": call["ret"], "fastqout_discarded": None,
                         "log": call["argv"][call["argv"].index("--log") + 1]}
    p, _ = _lib.fastq_filter_params_from_argv(ARGV["calls"][1]["argv"])
    assert (p.fastq_minlen, p.fastq_maxee_rate) == (900, 0.015)


@pytest.mark.parametrize("dash", ["-", "--"])
def test_both_option_spellings(dash):
    argv = ["vsearch", f"{dash}fastq_filter", "a.fq", f"{dash}fastqout", "o.fq", f"{dash}fastqout_discarded", "d.fq",
            f"{dash}fastq_ascii", "64", f"{dash}fastq_qmin", "2", f"{dash}fastq_qmax", "50", f"{dash}fastq_minlen",
            "10", f"{dash}fastq_maxlen", "500", f"{dash}fastq_maxee", "1.5", f"{dash}fastq_maxee_rate", "0.01",
            f"{dash}threads", "8", f"{dash}no_progress", f"{dash}quiet", f"{dash}log", "l.txt"]
    p, paths = _lib.fastq_filter_params_from_argv(argv)
    assert (p.fastq_ascii, p.fastq_qmin, p.fastq_qmax, p.fastq_minlen, p.fastq_maxlen, p.fastq_maxee,
            p.fastq_maxee_rate) == (64, 2, 50, 10, 500, 1.5, 0.01)
    assert paths == {"in_fastq": "a.fq", "fastqout": "o.fq", "fastqout_discarded": "d.fq", "log": "l.txt"}


def test_defaults_are_vsearchs():
    p, _ = _lib.fastq_filter_params_from_argv(["--fastq_filter", "a.fq", "--fastqout", "o.fq"])
    assert (p.fastq_ascii, p.fastq_qmin, p.fastq_qmax, p.fastq_minlen, p.fastq_maxlen) == (33, 0, 41, 1, -1)
    assert p.fastq_maxee < 0 and p.fastq_maxee_rate < 0


@pytest.mark.parametrize("extra", [["--bogus", "1"], ["--fastq_truncqual", "10"], ["--fastq_trunclen", "100"],
                                   ["--fastq_stripleft", "5"], ["--fastaout", "o.fa"], ["--fastq_maxns", "0"],
                                   ["--relabel", "r"], ["--fastq_ascii", "50"], ["--fastq_minlen"], ["stray"],
                                   ["--fastq_maxee", "x"]])
def test_options_outside_o7e_are_einval(extra):
    with pytest.raises(_lib.UmiclustError) as e:
        _lib.fastq_filter_params_from_argv(["vsearch", "--fastq_filter", "a.fq", "--fastqout", "o.fq"] + extra)
    assert e.value.code == EINVAL


@pytest.mark.parametrize("argv", [["vsearch", "--fastqout", "o.fq"], ["vsearch", "--fastq_filter", "a.fq"], ["vsearch"]])
def test_missing_input_or_output_is_einval(argv):
    with pytest.raises(_lib.UmiclustError) as e:
        _lib.fastq_filter_params_from_argv(argv)
    assert e.value.code == EINVAL


# ---- the host side under the sanitizers ----
@pytest.fixture(scope="module")
def fastq_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("fastq_check")
    b = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ont-tcrconsensus_amd"), "fastq_check",
                        f"SAN_OUT={out}"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    assert "warning" not in b.stderr, b.stderr
    count = [0]

    def san(args):
        r = subprocess.run([str(out / "fastq_check")] + [str(a) for a in args], capture_output=True, text=True,
                           timeout=300, env=SAN_ENV)
        assert r.returncode == 0, r.stderr[-4000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
        return r.stdout

    def run(data, threads=3, chunk=1 << 20, ascii_=33, qmin=0, qmax=93, minlen=1, maxlen=-1, maxee=-1.0, rate=-1.0):
        """-> (rc, counters, err, kept bytes, discarded bytes, log text)"""
        count[0] += 1
        d = out / f"run{count[0]}"
        d.mkdir()
        (d / "in.fq").write_bytes(data)
        txt = san(["filter", d / "in.fq", d / "kept.fq", d / "disc.fq", d / "log.txt", threads, chunk, ascii_, qmin,
                   qmax, minlen, maxlen, repr(float(maxee)), repr(float(rate))])
        kv = dict(line.split("=", 1) for line in txt.strip("\n").split("\n"))
        res = {k: (float.fromhex(v) if k.startswith("ee_") else int(v)) for k, v in kv.items() if k not in ("rc", "err")}
        log = (d / "log.txt").read_text() if (d / "log.txt").exists() else None
        files = [(d / f).read_bytes() if (d / f).exists() else None for f in ("kept.fq", "disc.fq")]
        return int(kv["rc"]), res, kv["err"], files[0], files[1], log

    def seams(data):
        count[0] += 1
        path = out / f"seams{count[0]}.fq"
        path.write_bytes(data)
        return san(["seams", path]).split()
    run.seams = seams
    return run


def _check(fastq_check, data, **kw):
    """the checker's outputs and counters equal the restatement's; returns the counters"""
    opts = {k: v for k, v in kw.items() if k not in ("threads", "chunk")}
    want_kept, want_disc, want = ref.run(data, **opts)
    rc, res, err, kept, disc, log = fastq_check(data, **kw)
    assert rc == want["n_kept"], err
    assert kept == want_kept and disc == want_disc
    for k, v in want.items():
        if k != "n_in_band":
            assert res[k] == v, k
    assert res["n_host_rechecked"] == want["n_in_band"]
    assert f"{want['n_kept']} sequences kept (of which 0 truncated), {want['n_discarded']} sequences discarded." in log
    return res


FEW = (b"@r0 first comment\nACGTACGTAC\n+\nIIIIIIIIII\n"
       b"@r1\tx\nACGTACGTACGTACG\n+r1\n@@@@@@@@@@@@@@@\n"       # quality line beginning with '@' (Q31)
       b"@r2\nACGTA\n+\n+++++\n"                                 # ... and with '+' (Q10)
       b"@r3\n\n+\n\n"                                           # an empty record
       b"@r4\nACGTACGTACGTACGTACGTACGTACGTAC\n+\n@+@+@+@+@+@+@+@+@+@+@+@+@+@+@+\n"
       b"@r5\nAC\n+\n!~\n")


def test_seams_every_slice_boundary(fastq_check):
    """windows of every length x 1, 2, 3 and 7 threads: a slice boundary on every byte of every record; the 4-line path
    is never left"""
    got = fastq_check.seams(FEW)
    assert got[:2] == ["seams", "ok"] and "records=6" in got and "fallback=0" in got and "rc=0" in got
    got = fastq_check.seams(FEW[:-1])  # missing final newline
    assert "records=6" in got and "fallback=0" in got
    got = fastq_check.seams(FEW.replace(b"\n", b"\r\n"))
    assert "records=6" in got and "fallback=0" in got
    multi = b"@m0 c\nACGT\nACGTAC\n+\nIIII\n@IIII+\n@m1\nAC\n+\n@@\n@m2\nACGTACGT\n+\n+II\nII\n@II\n"
    got = fastq_check.seams(multi)
    assert "records=3" in got and "rc=0" in got and "fallback=0" not in got


@pytest.mark.parametrize("threads", [1, 2, 3, 7])
def test_small_files_vs_restatement(fastq_check, threads):
    kw = dict(threads=threads, chunk=1024, minlen=3, rate=0.05)
    for data in (FEW, FEW[:-1], FEW.replace(b"\n", b"\r\n")):
        res = _check(fastq_check, data, **kw)
        assert res["n_input"] == 6 and res["n_short"] == 2 and 0 < res["n_kept"] < 4
    multi = b"@m0 c\nACGT\nACGTAC\n+\nIIII\n@IIII+\n\n@m1\nAC\n+\n@@\n@m2\nACGTACGT\n+\n+II\nII\n@II"
    assert _check(fastq_check, multi, threads=threads, chunk=1024, minlen=1, maxee=0.5)["n_input"] == 3


def test_empty_file(fastq_check):
    rc, res, err, kept, disc, log = fastq_check(b"")
    assert (rc, kept, disc) == (0, b"", b"") and res["n_input"] == 0 and res["n_chunks"] == 0
    assert "0 sequences kept (of which 0 truncated), 0 sequences discarded." in log


def test_length_mismatch_is_eformat(fastq_check):
    data = FEW + b"@bad\nACGTACGT\n+\nIIII\n@after\nAC\n+\nII\n"
    for threads in (1, 3):
        rc, res, err, kept, disc, _ = fastq_check(data, threads=threads, chunk=1024)
        assert rc == EFORMAT and "malformed FASTQ" in err
        want_kept, want_disc, want = ref.run(FEW)  # the records before it are written
        assert (kept, disc, res["n_input"]) == (want_kept, want_disc, 6)
    rc, _, err, _, _, _ = fastq_check(b"@r\nACGT\n+\nIIIIII\n")
    assert rc == EFORMAT
    rc, _, err, _, _, _ = fastq_check(b">r\nACGT\n")
    assert rc == EFORMAT


def test_quality_out_of_range_is_eformat(fastq_check):
    recs = ref.synth_reads(100, seed=5, max_len=200, min_len=20)
    lines = recs.split(b"\n")
    q = bytearray(lines[4 * 40 + 3])
    q[len(q) // 2] = 32  # below fastq_ascii, in record 40
    lines[4 * 40 + 3] = bytes(q)
    data = b"\n".join(lines)
    rc, res, err, kept, disc, _ = fastq_check(data, chunk=2048, minlen=50, rate=0.07)
    assert rc == EFORMAT and "record 40 (read40)" in err and "below qmin" in err
    want_kept, want_disc, _ = ref.run(data, minlen=50, rate=0.07, stop_at=40)
    assert (kept, disc) == (want_kept, want_disc)
    # above fastq_qmax with vsearch's default 41
    rc, _, err, _, _, _ = fastq_check(b"@a\nAC\n+\nII\n@b\nAC\n+\nIK\n", qmax=41)
    assert rc == EFORMAT and "record 1 (b)" in err and "above qmax" in err


def test_gzip_magic_is_einval(fastq_check):
    rc, _, err, kept, _, _ = fastq_check(b"\x1f\x8b\x08\x00" + b"\0" * 20)
    assert rc == EINVAL and "gzip" in err and kept is None


def test_random_reads_many_chunks(fastq_check):
    data = ref.synth_reads(400, seed=11, max_len=1200)
    a = _check(fastq_check, data, threads=4, chunk=16 << 10, minlen=200, rate=0.07)
    assert a["n_chunks"] >= 10 and a["n_host_rechecked"] == 0 and a["n_kept"] > 20 and a["n_maxee_rate"] > 20
    b = _check(fastq_check, data, threads=2, chunk=1 << 20, minlen=100, maxlen=1000, maxee=20.0, rate=0.07, ascii_=33)
    assert b["n_chunks"] == 1 and min(b["n_short"], b["n_long"], b["n_maxee"], b["n_maxee_rate"], b["n_kept"]) > 0


def test_threshold_records_are_rechecked(fastq_check):
    """constant-quality reads whose rate equals the threshold: every one lies in the guard band and is decided by the
    host's sequential double sum; a read one quality step away is not"""
    p, _ = ref.tables()
    recs = []
    for q in (20, 10):
        for n in range(1, 301):
            recs.append((b"c%d_%d" % (q, n), bytes([33 + q]) * n))
            if n % 7 == 0:
                for d in (-1, 1):
                    v = bytearray([33 + q]) * n
                    v[n // 2] += d
                    recs.append((b"m%d_%d_%d" % (q, n, d + 1), bytes(v)))
    for q in (20, 10):
        data = b"".join(b"@" + lab + b"\n" + b"A" * len(qs) + b"\n+\n" + qs + b"\n" for lab, qs in recs
                        if lab[1:3] == b"%d" % q)
        res = _check(fastq_check, data, chunk=8192, rate=float(p[33 + q]))
        assert res["n_host_rechecked"] == 300 and res["n_kept"] > 0 and res["n_maxee_rate"] > 0


def test_division_and_product_forms_differ():
    """O7d is ee / len > rate, not ee > rate * len: the two forms disagree on some constant-quality reads, so the
    restatement the tests compare against must be (and is) the division"""
    p, _ = ref.tables()
    differ = 0
    for q in range(1, 42):
        rate = float(p[33 + q])
        for n in range(1, 300):
            ee = ref.ee_seq(p, bytes([33 + q]) * n)
            differ += (ee / n > rate) != (ee > rate * n)
    assert differ > 0
    assert np.isclose(ref.ee_seq(p, b"5" * 10), 10 * 10 ** -2.0)
