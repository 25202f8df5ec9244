"""The consensus alignment filter and the cs-tag census (row f6) without a GPU.

tests/golden/bam_filter/*.json hold what the reference's own filter_consensus_alignments and count_cs_tags left on
each case (tests/golden/make_golden_bam_filter.py).  Here: tests/bam_ref.py (the plain reference of the device scan and
group-by) reproduces every fixture; the formatting half of umiclust.minimap2_align, fed bam_ref's columns, reproduces
every CSV and log byte for byte; and tools/bam_check_main.cpp -- bam_host.cpp under ASan + UBSan -- prints the same
columns as bam_ref and round-trips the BGZF writer.  A sanitizer report fails the test."""
import collections
import glob
import json
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest
from umiclust import _lib, minimap2_align

import bam_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {os.path.basename(p)[:-5]: json.load(open(p))
         for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "bam_filter", "*.json")))}
RUNNING = [k for k, c in CASES.items() if "eformat_record" not in c]
MALFORMED = [k for k, c in CASES.items() if "eformat_record" in c]
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
ERRORS = {"KeyError": KeyError, "ZeroDivisionError": ZeroDivisionError}


def test_fixture_set():
    assert len(CASES) >= 14 and len(MALFORMED) == 2
    for c in CASES.values():
        assert len(c["records"]) <= 400
        assert all(len(t[2]) <= 300 for r in c["records"] for t in r["tags"] if t[0] == "cs" and t[1] == "Z")
    distinct = {t[2] for r in CASES["forced_collision"]["records"] for t in r["tags"] if t[0] == "cs"}
    assert len(distinct) >= 300 and CASES["forced_collision"]["hash_bits"] == 8  # more strings than 8-bit hashes
    assert sorted(c["expect"]["error"][0] for c in CASES.values() if c.get("expect", {}).get("error")) == \
        ["KeyError", "KeyError", "ZeroDivisionError"]


def test_exports_and_abi():
    names = {"umiclust_bam_open", "umiclust_bam_counts", "umiclust_bam_times", "umiclust_bam_columns",
             "umiclust_bam_refs", "umiclust_bam_strings", "umiclust_bam_cs_groups", "umiclust_bam_write",
             "umiclust_bam_close"}
    assert names <= set(_lib.EXPORTS)
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n), n
    assert lib.umiclust_abi_version() == 9


# ---------------------------------------------------------------- bam_ref against the fixtures
@pytest.mark.parametrize("name", RUNNING)
def test_bam_ref_reproduces_the_census(name):
    case, e = CASES[name], CASES[name]["expect"]
    col = bam_ref.Columns(bam_ref.build_raw(case["refs"], case["records"]))
    if e["cs_error"] is None:
        assert [[s, n] for s, n in zip(col.group_strings, col.group_count)] == e["cs_counter"]
        regions = {}
        for i in np.flatnonzero(col.cs_group >= 0):
            regions.setdefault(col.cs[i], {}).setdefault(col.ref_names[col.ref[i]], 0)
            regions[col.cs[i]][col.ref_names[col.ref[i]]] += 1
        assert list(regions) == col.group_strings
        assert [[[r, n] for r, n in v.items()] for v in regions.values()] == e["cs_region_counter"]
        blast = {}
        for i in np.flatnonzero(col.cs_group >= 0):
            x = (int(col.cols[i]) - int(col.nm[i])) / int(col.cols[i])
            blast.setdefault(col.cs[i], {}).setdefault(x, 0)
            blast[col.cs[i]][x] += 1
        assert [[[x, n] for x, n in v.items()] for v in blast.values()] == e["cs_blast_id_counter"]
    assert [int(r) for r in col.group_rep] == [int(np.flatnonzero(col.cs_group == g)[0]) for g in range(len(col.group_rep))]


@pytest.mark.parametrize("name", MALFORMED)
def test_bam_ref_refuses_the_malformed_primary_record(name):
    case = CASES[name]
    with pytest.raises(bam_ref.Malformed) as ei:
        bam_ref.Columns(bam_ref.build_raw(case["refs"], case["records"]))
    assert ei.value.record == case["eformat_record"]


# ---------------------------------------------------------------- the formatting half on bam_ref's columns
def run_drop_in(src, case, tmp_path, monkeypatch, name):
    """filter_consensus_alignments_from on `src` (None: filter_consensus_alignments on the BAM file itself);
    (return or None, error or None, files, kept, inflated output)"""
    calls = []
    monkeypatch.setattr(minimap2_align.subprocess, "run", lambda *a, **k: calls.append(a[0]))
    logs = tmp_path / "logs"
    logs.mkdir()
    fasta = tmp_path / "ref.fa"
    bam_ref.write_fasta(fasta, case["regions"])
    bam = str(tmp_path / (name + ".bam"))
    ret, err = None, None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # numpy's mean / median of an empty list, as in the reference
        try:
            if src is None:
                ret = minimap2_align.filter_consensus_alignments(bam, str(fasta), str(logs), **case["params"])
            else:
                ret = minimap2_align.filter_consensus_alignments_from(src, bam, str(fasta), str(logs), **case["params"])
            ret = os.path.basename(ret)
            assert calls == [["samtools", "index", str(tmp_path / (name + "_filtered.bam"))]]
        except (KeyError, ZeroDivisionError) as e:
            err = [type(e).__name__, [str(a) for a in e.args]]
    files = {f: open(logs / f).read() for f in sorted(os.listdir(logs))}
    stream = bam_ref.check_bgzf(tmp_path / (name + "_filtered.bam"))
    index = {r["name"]: i for i, r in enumerate(case["records"])}
    kept = [index[r.query_name] for r in bam_ref.decode(stream)[2]]
    return ret, err, files, kept, stream


def check_against_fixture(got, case, raw):
    ret, err, files, kept, stream = got
    e = case["expect"]
    assert err == e["error"] and ret == e["return"]
    assert kept == e["kept"]
    assert sorted(files) == sorted(e["files"])
    for f in e["files"]:
        assert files[f] == e["files"][f], f
    keep = np.zeros(len(case["records"]), bool)
    keep[e["kept"]] = True
    assert stream == bam_ref.Columns(raw).expected_stream(keep)


def report_of(e):
    """the three log blocks of minimap2_ont_align (:141-150) from the reference's counters, which the fixture holds in
    their insertion order: the order Counter.most_common breaks ties by"""
    a = collections.Counter(dict(e["cs_counter"]))
    b = {k: collections.Counter(dict(map(tuple, v))) for k, v in zip(a, e["cs_region_counter"])}
    c = {k: collections.Counter(dict(map(tuple, v))) for k, v in zip(a, e["cs_blast_id_counter"])}
    top = a.most_common(40)
    out = ["\nTop 40 most common cs tags:\n"] + [str(t) + "\n" for t in top]
    out.append("\nTop 4 most common regions counted for each of the top 40 most common cs tags:\n")
    out += [str(t[0]) + " " + str(b[t[0]].most_common(4)) + "\n" for t in top]
    out.append("\nTop 4 most common blast identities counted for each of the top 40 most common cs tags:\n")
    out += [str(t[0]) + " " + str(c[t[0]].most_common(4)) + "\n" for t in top]
    return "".join(out)


def check_census(src, case):
    e = case["expect"]
    if e["cs_error"] is not None:
        with pytest.raises(ERRORS[e["cs_error"][0]]) as ei:
            minimap2_align.count_cs_tags(src)
        assert [str(a) for a in ei.value.args] == e["cs_error"][1]
        return
    a, b, c = minimap2_align.count_cs_tags(src)
    assert [[k, v] for k, v in a.items()] == e["cs_counter"]
    assert list(a) == list(b) == list(c)  # the fixture stores the two dicts of Counters without their keys
    assert [[[r, n] for r, n in v.items()] for v in b.values()] == e["cs_region_counter"]
    assert [[[x, n] for x, n in v.items()] for v in c.values()] == e["cs_blast_id_counter"]
    assert minimap2_align.cs_tag_report(src) == report_of(e)


@pytest.mark.parametrize("name", RUNNING)
def test_formatting_half_reproduces_every_file(name, tmp_path, monkeypatch):
    case = CASES[name]
    raw = bam_ref.build_raw(case["refs"], case["records"])
    src = bam_ref.Columns(raw)
    check_against_fixture(run_drop_in(src, case, tmp_path, monkeypatch, name), case, raw)
    check_census(src, case)


def test_the_cut_at_rank_40_follows_first_seen_order():
    e = CASES["grouping"]["expect"]
    counts = [n for _, n in e["cs_counter"]]
    ranked = sorted(range(len(counts)), key=lambda x: (-counts[x], x))
    assert counts[ranked[39]] == counts[ranked[40]]  # ranks 40 and 41 tie: only first-seen order decides
    top = [e["cs_counter"][x][0] for x in ranked[:40]]
    lines = report_of(e).split("\n")
    assert [ln for ln in lines[2:42]] == [str((t, counts[ranked[x]])) for x, t in enumerate(top)]
    half = [k for k, _ in e["cs_counter"]].index("=half")
    assert e["cs_blast_id_counter"][half] == [[0.5, 4], [0.51, 1]]  # (100, 50), (200, 100), (150, 75): one key


# ---------------------------------------------------------------- bam_host.cpp under ASan + UBSan
@pytest.fixture(scope="module")
def bam_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("bam_check")
    b = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ont-tcrconsensus_amd"), "bam_check", f"SAN_OUT={out}"],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    assert "warning" not in b.stderr, b.stderr

    def run(bam, prefix, threads=3, rc=0):
        r = subprocess.run([str(out / "bam_check"), str(bam), str(prefix), str(threads)], capture_output=True, text=True,
                           timeout=300, env=SAN_ENV)
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
        assert r.returncode == rc, (r.stdout[-2000:], r.stderr[-2000:])
        return r.stdout.split("\n")

    return run


def parse_rows(lines):
    rows = {}
    for ln in lines:
        if ln.startswith("rec "):
            head, cs = ln.split(" cs=", 1)
            rows[int(head.split()[1])] = [int(x) for x in head.split()[2:]] + [cs]
    return rows


@pytest.mark.parametrize("name", sorted(CASES))
def test_bam_check_columns_and_writer_roundtrip(bam_check, name, tmp_path):
    case = CASES[name]
    bam = tmp_path / "in.bam"
    raw = bam_ref.write_bam(bam, case["refs"], case["records"], block=4000 if name == "aux_walk" else 60000)
    lines = bam_check(bam, tmp_path / "out", threads=1 if name == "cigar" else 3)
    assert "roundtrip ok" in lines
    assert [ln for ln in lines if ln.startswith("ref ")] == ["ref %s %d" % (n, ln) for n, ln in case["refs"]]
    rows = parse_rows(lines)
    _, start, recs = bam_ref.decode(raw)
    assert len(rows) == len(recs)
    if "eformat_record" in case:
        assert [r for r, v in rows.items() if v[8]] == [case["eformat_record"]]
    else:
        col = bam_ref.Columns(raw)
        for r in range(col.n):
            want = [int(col.cls[r]), int(col.ref[r]), int(col.l_seq[r]), int(col.reference_length[r]), int(col.cols[r]),
                    int(col.nm[r]), int(col.nm_present[r]), len(col.cs[r]) if col.cs[r] is not None else -1, 0,
                    col.cs[r] or ""]
            assert rows[r] == want, r
    # the writer: well-formed BGZF that inflates to the header and the kept records
    assert bam_ref.check_bgzf(str(tmp_path / "out.all.bam")) == raw
    assert bam_ref.check_bgzf(str(tmp_path / "out.alt.bam")) == \
        raw[:start] + b"".join(r.bytes for i, r in enumerate(recs) if i % 2 == 0)


def distinct_record_bam():
    """One hand-built record in which no two fixed fields hold the same value: refID != next_refID, pos != next_pos, an
    odd l_seq, the shortest name (l_read_name = 1) and no CIGAR (n_cigar_op = 0), so that its aux fields would start
    at 36 + 1 + 0 + 4 + 7 = 48 = 4 + block_size.  A reader that takes one field's offset for another's reads another
    number."""
    import struct
    body = struct.pack("<iiBBHHHiiii", 3, 1000, 1, 37, 5000, 0, 0x210, 7, 2, 2000, -300) + b"\0" + \
        bytes([0x12, 0x48, 0x12, 0x40]) + b"\xff" * 7
    assert len(body) == 44
    return bam_ref.build_raw([["r%d" % i, 5000] for i in range(4)], []) + struct.pack("<i", len(body)) + body


@pytest.mark.parametrize("name", sorted(CASES) + ["distinct"])
def test_bam_check_reads_the_fixed_fields_as_bam_ref_does(bam_check, name, tmp_path):
    """The accessors and bam::aux_offset of csrc/bam_record.h (the `fix` lines of bam_check) against bam_ref's decoder,
    which unpacks the fixed part in file order and names no offset: every fixture, and the record above."""
    bam = tmp_path / "in.bam"
    if name == "distinct":
        raw = distinct_record_bam()
        bam_ref.write_bgzf(bam, raw)
    else:
        raw = bam_ref.write_bam(bam, CASES[name]["refs"], CASES[name]["records"])
    lines = bam_check(bam, tmp_path / "out")
    got = {int(ln.split()[1]): [int(x) for x in ln.split()[2:]] for ln in lines if ln.startswith("fix ")}
    recs = bam_ref.decode(raw)[2]
    assert len(recs) >= 1 and sorted(got) == list(range(len(recs)))
    for r, rec in enumerate(recs):
        assert got[r] == rec.fixed, r
    if name == "distinct":
        assert "fields=ok" in lines
        assert recs[0].fixed == [3, 1000, 1, 37, 5000, 0, 0x210, 7, 2, 2000, -300, 48]
        assert len(set(recs[0].fixed)) == 12


@pytest.mark.parametrize("field,value", [("l_read_name", 255), ("l_read_name", 5), ("l_read_name", 0),
                                         ("n_cigar_op", 65535), ("n_cigar_op", 3), ("l_seq", 1000), ("l_seq", 11),
                                         ("l_seq", -1), ("l_seq", 0x7fffffff)])
def test_bam_check_names_the_record_whose_fields_overrun_it(bam_check, tmp_path, field, value):
    """bam::check_record_fields, which umiclust_region_split runs before its kernels (they index the name, the CIGAR
    and the sequence by l_read_name, n_cigar_op and l_seq alone): record 2 of 4 claims a name, a CIGAR or a sequence
    that its block_size does not hold -- by far, and by the smallest step (a record without tags fills its block_size
    exactly: name 4 -> 5, 2 ops -> 3, l_seq 10 -> 11).  CPU only: no such record is ever given to the device."""
    import struct
    recs = [{"name": "a_%d" % i, "flag": 16 * (i & 1), "ref": 0, "cigar": [["M", 6], ["S", 4]], "l_seq": 10,
             "tags": [["NM", "C", 1]] if i == 3 else []} for i in range(4)]
    raw = bytearray(bam_ref.build_raw([["r", 10]], recs))
    p = tmp_path / "ok.bam"
    bam_ref.write_bgzf(p, bytes(raw))
    assert "fields=ok" in bam_check(p, tmp_path / "o")
    o = bam_ref.record_offsets(bytes(raw), bam_ref.parse_header(bytes(raw))[1])[2]
    assert struct.unpack_from("<B", raw, o + 12)[0] == 4 and struct.unpack_from("<H", raw, o + 16)[0] == 2
    assert struct.unpack_from("<i", raw, o + 20)[0] == 10
    struct.pack_into(*{"l_read_name": ("<B", raw, o + 12), "n_cigar_op": ("<H", raw, o + 16),
                       "l_seq": ("<i", raw, o + 20)}[field], value)
    p = tmp_path / "bad.bam"
    bam_ref.write_bgzf(p, bytes(raw))
    lines = bam_check(p, tmp_path / "o")
    msg = [ln for ln in lines if ln.startswith("fields=")]
    assert len(msg) == 1 and msg[0].startswith("fields=BAM record 2: ") and f"{field} {value}" in msg[0], msg


def test_bam_check_refuses_what_is_not_bam(bam_check, tmp_path):
    p = tmp_path / "x.bam"
    p.write_bytes(b"not gzip at all")
    assert any(ln.startswith("err=cannot read BGZF") for ln in bam_check(p, tmp_path / "o", rc=2))
    bam_ref.write_bgzf(p, b"SAM\x01" + b"\0" * 20)
    assert "err=not BAM" in bam_check(p, tmp_path / "o", rc=2)
    raw = bam_ref.build_raw([["r", 10]], [{"name": "a_1", "flag": 0, "ref": 0, "cigar": [["M", 5]], "l_seq": 5, "tags": []}])
    bam_ref.write_bgzf(p, raw[:-3])  # the last record is cut short
    assert any(ln.startswith("err=truncated BAM record 0") for ln in bam_check(p, tmp_path / "o", rc=2))
    bam_ref.write_bgzf(p, raw[:30])  # the header is cut short
    assert any(ln.startswith("err=truncated BAM header") for ln in bam_check(p, tmp_path / "o", rc=2))
