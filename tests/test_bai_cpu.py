"""The .bai index and flagstat (policies O10 and O11) without a GPU.

tools/bai_check_main.cpp -- csrc/bam_index.h (the host restatement of the kernels of bamindex.hip, the finish, the
file's bytes, the flagstat text) under ASan + UBSan -- against tests/bai_ref.py, the plain Python restatement written
from the policy text, on every case of tests/bai_cases.py; the specification's reader contract on the files; and the
flagstat text against lines written by hand.  A sanitizer report fails the test."""
import os
import shutil
import subprocess

import pytest

import bai_cases
import bai_ref
import bam_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def bai_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("bai_check")
    b = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ont-tcrconsensus_amd"), "bai_check", f"SAN_OUT={out}"],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr

    def run(mode, src, tmp):
        bai, fs = tmp / "out.bai", tmp / "out.flagstat"
        for p in (bai, fs):
            if p.exists():
                p.unlink()
        r = subprocess.run([str(out / "bai_check"), mode, str(src), str(bai), str(fs)], capture_output=True, text=True,
                           timeout=300, env=SAN_ENV)
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout.split(), bai.read_bytes() if bai.exists() else None, fs.read_text()
    return run


def test_case_set():
    names = [c.name for c in bai_cases.CASES]
    assert len(set(names)) == len(names) >= 26 and len(bai_cases.REFUSALS) == 4


@pytest.mark.parametrize("case", bai_cases.CASES, ids=repr)
def test_bytes_and_text_equal_the_reference(bai_check, case, tmp_path):
    bai_cases.case_file(tmp_path / "in.case", case)
    words, got, text = bai_check("case", tmp_path / "in.case", tmp_path)
    ref = bai_ref.Index(case.raw, case.keep, case.coff, case.ustart)
    assert ref.first_bad < 0 and words[0] == "ok"
    assert words[1] == "kept=%d" % ref.n_kept and words[2] == "runs=%d" % len(ref.sorted_runs)
    assert words[4] == "windows=%d" % len(ref.linear)
    assert got == ref.bytes
    assert text == bai_ref.flagstat(case.raw, case.keep)[1]
    refs, n_no_coor = bai_ref.parse_bai(got)  # the file reads back as what the reference holds
    assert n_no_coor == ref.n_no_coor and [r["bins"] for r in refs] == ref.bins_of
    assert words[3] == "chunks=%d" % sum(len(c) for r in refs for c in r["bins"].values())
    # the reader contract on the imagined file: the kept stream under the case's block table
    reader = bai_ref.TableReader(bai_ref.kept_stream(case.raw, case.keep), case.coff, case.ustart)
    bai_ref.check_reader_contract(reader, got, ref, bai_cases.query_grid(ref))


def test_the_finish_cases_do_what_they_are_for():
    """the cases named for the finish reach its branches: all of it in bin 0; leaves that stay; one leaf of a parent
    staying while its sibling moves up; neighbours merging in a shared block and not a block later"""
    by = {c.name: bai_ref.Index(c.raw, c.keep, c.coff, c.ustart) for c in bai_cases.CASES if c.name.startswith("alternating")}
    assert set(by["alternating"].bins_of[1]) == {0}
    far, per = by["alternating_far_big_blocks"].bins_of[1], by["alternating_far_block_per_record"].bins_of[1]
    assert any(b >= 4681 for b in far) and any(b >= 4681 for b in per)
    assert sum(map(len, far.values())) < sum(map(len, per.values())) == len(by["alternating_far_block_per_record"].runs)
    half = by["alternating_half_far"].bins_of[1]
    assert any(b >= 4681 for b in half) and any(585 <= b < 4681 for b in half)


@pytest.mark.parametrize("block", [60000, 300, 61])
@pytest.mark.parametrize("case", bai_cases.CASES, ids=repr)
def test_reader_contract_on_a_file(bai_check, case, block, tmp_path):
    """the index of a real BGZF file that holds the case's kept records, and every query of the grid through it finds
    the brute-force set"""
    raw = bai_ref.kept_stream(case.raw, case.keep)
    path = tmp_path / "in.bam"
    bam_ref.write_bgzf(path, raw, block)
    coff, ustart = bai_ref.block_table(path)
    words, got, _ = bai_check("file", path, tmp_path)
    ref = bai_ref.Index(raw, None, coff, ustart)
    assert words[0] == "ok" and got == ref.bytes
    bai_ref.check_reader_contract(bai_ref.BgzfReader(path), got, ref, bai_cases.query_grid(ref))


@pytest.mark.parametrize("name,raw,record,status,hide", bai_cases.REFUSALS, ids=[r[0] for r in bai_cases.REFUSALS])
def test_refusals(bai_check, name, raw, record, status, hide, tmp_path):
    case = bai_cases.Case(name, raw)
    bai_cases.case_file(tmp_path / "in.case", case)
    words, got, _ = bai_check("case", tmp_path / "in.case", tmp_path)
    ref = bai_ref.Index(raw, None, case.coff, case.ustart)
    assert (ref.first_bad, ref.first_status) == (record, status)
    assert words == ["refused", "status=%d" % status, "record=%d" % record] and got is None
    hidden = bai_cases.Case(name + "_hidden", raw, keep=hide)
    bai_cases.case_file(tmp_path / "in.case", hidden)
    words, got, _ = bai_check("case", tmp_path / "in.case", tmp_path)
    assert words[0] == "ok" and got == bai_ref.Index(raw, hide, hidden.coff, hidden.ustart).bytes


def test_flagstat_text_by_hand(bai_check, tmp_path):
    """the 16 lines in samtools >= 1.13's order -- line 7 (from 0) is "primary mapped", which
    filter_and_split_reads_by_region_old reads -- with the four percentages and their N/A forms"""
    R = bai_cases.rec
    raw = bai_cases.stream(bai_cases.REFS3, [
        R("a", 0, 1, "10M", flag=0x1 | 0x2 | 0x40, next_ref=0), R("b", 0, 2, "10M", flag=0x1 | 0x80 | 0x8, next_ref=0),
        R("c", 0, 3, "10M", flag=0x100), R("d", 0, 4, "10M", flag=0x4), R("e", 0, 5, "10M", flag=0x1 | 0x200, mapq=5, next_ref=1),
        R("f", 0, 6, "10M", flag=0x800 | 0x400), R("g", 0, 7, "10M", flag=0)])
    want = ("6 + 1 in total (QC-passed reads + QC-failed reads)\n4 + 1 primary\n1 + 0 secondary\n1 + 0 supplementary\n"
            "1 + 0 duplicates\n0 + 0 primary duplicates\n5 + 1 mapped (83.33% : 100.00%)\n"
            "3 + 1 primary mapped (75.00% : 100.00%)\n2 + 1 paired in sequencing\n1 + 0 read1\n1 + 0 read2\n"
            "1 + 0 properly paired (50.00% : 0.00%)\n1 + 1 with itself and mate mapped\n1 + 0 singletons (50.00% : 0.00%)\n"
            "0 + 1 with mate mapped to a different chr\n0 + 1 with mate mapped to a different chr (mapQ>=5)\n")
    case = bai_cases.Case("hand", raw)
    bai_cases.case_file(tmp_path / "in.case", case)
    _, _, text = bai_check("case", tmp_path / "in.case", tmp_path)
    assert text == want == bai_ref.flagstat(raw)[1]
    assert text.splitlines()[7].split(" + ")[0] == "3"
    none = bai_cases.Case("hand_none", raw, keep=[0] * 7)
    bai_cases.case_file(tmp_path / "in.case", none)
    _, _, text = bai_check("case", tmp_path / "in.case", tmp_path)
    lines = text.splitlines()
    assert lines[0] == "0 + 0 in total (QC-passed reads + QC-failed reads)"
    assert lines[6] == "0 + 0 mapped (N/A : N/A)" and lines[7] == "0 + 0 primary mapped (N/A : N/A)"
    assert lines[11] == "0 + 0 properly paired (N/A : N/A)" and lines[13] == "0 + 0 singletons (N/A : N/A)"
    assert text == bai_ref.flagstat(raw, [0] * 7)[1]
