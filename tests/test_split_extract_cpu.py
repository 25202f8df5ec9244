"""Row f4+f1 without a device: the plain reference of the fused call (tests/split_extract_ref.py) on
hand-derived records, the shares of its seeded read generator, and the library's new symbols.  The GPU comparison is
tests/test_gpu_split_extract.py."""
import os
import random
import shutil
import subprocess

import pytest
import split_extract_ref as ref
from umiclust import _lib, minimap2_align
from umiclust import region_split as rs

import bam
import extract as oex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
REGIONS = [("TRBV_a", 60), ("TRBV_b", 80)]


def _rec(name, flag, ref_id, seq, span=None):
    return dict(name=name, flag=flag, ref=ref_id, pos=0, cigar=[("M", span or REGIONS[ref_id][1])], seq=seq)


def test_sequence_less_record_is_the_text_none():
    """The case of the issue: a kept record without a sequence is `None` to the UMI search, and N equals A and T."""
    text, n = oex.extract_records([("x;strand=+", "None")], 73, 68, 0, "A", "T")
    assert n == 1 and text == ">x;strand=+;umi_fwd_dist=0;umi_rev_dist=0;umi_fwd_seq=N;umi_rev_seq=N;seq=None\nNN\n"
    out = ref.compose(REGIONS, REGIONS, {"TRBV_a": 0, "TRBV_b": 0}, [_rec("x", 0, 0, "")], 0.95, 73, 68, 73, 68, 0, "A", "T")
    assert out[3] == {"region_cluster0_detected_umis.fasta": text} and out[4] == {0: 1}


def test_composition_on_hand_derived_records():
    """Two clusters; a reverse read stored reverse-complemented with a non-ACGT base inside its 5' UMI; a read without
    UMIs; a cluster whose only read has none (an empty file); a short read (dropped by the split)."""
    fwd, rev = "ACGTAC", "TTGGAA"
    plus = "ACGTAC" + "CCCCCCCC" + "TTGGAA"
    minus = "ACNTAC" + "GGGG" + "TTGGAA"  # distance 0: N equals G
    records = [_rec("plus", 0, 0, plus), _rec("minus", 16, 0, ref.stored(minus, True)), _rec("none", 0, 0, "C" * 30),
               _rec("lonely", 16, 1, "G" * 40), _rec("short", 0, 0, plus, span=10)]
    counts, per_cluster, detected, files, umis, kept = ref.compose(
        REGIONS, REGIONS, {"TRBV_a": 3, "TRBV_b": 1}, records, 0.95, 73, 68, 10, 8, 1, fwd, rev)
    assert counts == dict(unmapped=0, primary=5, short=1, long=0) and per_cluster == {3: 3, 1: 1}
    assert [nm for nm, _ in kept] == ["plus;strand=+", "minus;strand=-", "none;strand=+", "lonely;strand=-"]
    assert files == {
        "region_cluster3_detected_umis.fasta":
            f">plus;strand=+;umi_fwd_dist=0;umi_rev_dist=0;umi_fwd_seq=ACGTAC;umi_rev_seq=TTGGAA;seq={plus}\nACGTACTTGGAA\n"
            f">minus;strand=-;umi_fwd_dist=0;umi_rev_dist=0;umi_fwd_seq=ACNTAC;umi_rev_seq=TTGGAA;seq={minus}\nTTCCAAGTANGT\n",
        "region_cluster1_detected_umis.fasta": ""}
    assert umis == {3: 2, 1: 0} and detected == {"TRBV_a", "TRBV_b"}


@pytest.mark.parametrize("name,rid,strand,combined", [
    ("a;b", "a", "+", "ACGTACTTGGAA"),             # the read name ends at the first ';'
    ("a=b", "a=b", "+", "ACGTACTTGGAA"),
    ("strand=", "strand=", ";", "TTCCAAGTACGT"),    # between the name's "strand=" and the appended one: ';'
    ("x;strand=-", "x", "-;", "TTCCAAGTACGT"),      # '-;' is not '+': the reverse-complement branch, on a + record
    ("qstrand=+", "qstrand=+", "+;", "TTCCAAGTACGT"),
])
def test_names_with_separators(name, rid, strand, combined):
    """What the two-step path prints for a query name that itself holds ';' or 'strand=' (both legal in SAM)."""
    seq = "ACGTAC" + "CCCC" + "TTGGAA"
    files = ref.compose(REGIONS, REGIONS, {"TRBV_a": 0, "TRBV_b": 0}, [_rec(name, 0, 0, seq)], 0.95, 73, 68, 10, 8, 0,
                        "ACGTAC", "TTGGAA")[3]
    assert files["region_cluster0_detected_umis.fasta"] == (
        f">{rid};strand={strand};umi_fwd_dist=0;umi_rev_dist=0;umi_fwd_seq=ACGTAC;umi_rev_seq=TTGGAA;seq={seq}\n"
        f"{combined}\n")


def test_key_error_comes_before_any_extraction():
    records = [_rec("ok", 0, 0, "A" * 60), _rec("passes", 0, 1, "A" * 80)]
    with pytest.raises(KeyError) as e:
        ref.compose(REGIONS, REGIONS, {"TRBV_a": 0}, records, 0.95, 73, 68, 10, 8, 0, "A", "T")
    assert e.value.args[0] == "TRBV_b"


@pytest.mark.parametrize("a5,a3,k", [(40, 36, 3), (73, 68, 3), (33, 30, 2)])
def test_generator_shares(a5, a3, k):
    """The planted reads at the three settings the GPU tests use: at least 30 % with both UMIs, at least 30 % without,
    both strands, every distance 0..k.  Conditions on the inputs, asserted by split_extract_ref.conditions."""
    rng = random.Random(11)
    regions = [("TRBV_%d" % i, 300) for i in range(4)]
    records = ref.planted_records(rng, 700, regions, a5, a3, k)
    out = ref.compose(regions, regions, {nm: i // 2 for i, (nm, _) in enumerate(regions)}, records, 0.9, 200, 200, a5, a3, k)
    assert sum(out[1].values()) == 700 == len(out[5])
    n, strands, dists = ref.conditions(out[3], 700, k)
    assert n == sum(out[4].values())


def test_host_formatter_under_asan_and_ubsan(tmp_path):
    """bam::forward_text and bam::format_umi_record -- the host restatement of k_bam_emit_umi, and the formatter of the
    records whose name holds "strand=" -- in a stand-alone program built with ASan + UBSan, against oracle/extract.py:
    both strands, odd and even lengths, all 16 base codes, a record without a sequence, names with ';' and 'strand=',
    names of 1 and 254 bytes, a3 = 0 and windows longer than the read."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    b = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ont-tcrconsensus_amd"), "umi_text_check",
                        f"SAN_OUT={tmp_path}"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0 and "warning" not in b.stderr, b.stderr
    rng = random.Random(3)
    fwd, rev = "ACNTAC", "TTBGAA"
    names = ["n", "d" * 254, "a;b", ";", "strand=", "x;strand=-", "strand=+strand=-", "s" * 200 + "strand=", "a=b"]
    for a5, a3 in ((12, 10), (9, 0), (300, 300)):
        records = [_rec("none", 16 * (i % 2), 0, "") for i in range(2)]
        for i in range(60):
            alpha = bam.SEQ_CODES if i % 5 == 0 else "ACGT"
            text = (ref._instance(rng, fwd, rng.randint(0, 2), "ACGT") + "".join(rng.choices(alpha, k=rng.randint(0, 9)))
                    + ref._instance(rng, rev, rng.randint(0, 2), "ACGT"))
            records.append(_rec(names[i % len(names)], 16 * (i % 2), 0, ref.stored(text, i % 2 == 1)))
        bam.write_bam(str(tmp_path / "in.bam"), REGIONS, records)
        entries = [(f"{s.query_name};strand={'-' if s.is_reverse else '+'}", f"{s.get_forward_sequence()}")
                   for s in ref.segments(REGIONS, records)]
        res, want = [], ""
        for name, seq in entries:
            w3 = seq[-a3:]
            h5, h3 = oex.hw_locate(fwd, seq[:a5], 1), oex.hw_locate(rev, w3, 1)
            res += list(h5 or (-1, -1, -1)) + list(h3 or (-1, -1, -1))
            want += oex.extract_records([(name, seq)], a5, a3, 1, fwd, rev)[0]
        (tmp_path / "res.txt").write_text(" ".join(str(v) for v in res))
        r = subprocess.run([str(tmp_path / "umi_text_check"), str(tmp_path / "in.bam"), str(tmp_path / "res.txt"), str(a3),
                            str(tmp_path / "out.txt")], capture_output=True, text=True, timeout=300, env=SAN_ENV)
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
        assert r.returncode == 0, r.stderr[-2000:]
        texts, _, got = (tmp_path / "out.txt").read_text().partition("--\n")
        assert texts.split("\n")[:-1] == [seq for _, seq in entries]
        assert got == want and want.count(">") > 20 and ";strand=-;;umi_fwd_dist=" in want


def test_exports_and_signatures():
    names = {"umiclust_region_split_extract", "umiclust_bam_split_extract"}
    assert names <= set(_lib.EXPORTS)
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n), n
    assert callable(_lib.Context.region_split_extract) and callable(_lib.BamSession.split_extract)
    assert callable(rs.filter_split_and_extract_umis) and callable(rs.filter_split_and_extract_umis_by_region_from)
    assert callable(minimap2_align.filter_consensus_alignments_split_and_extract)
