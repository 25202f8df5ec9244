"""SURVEY.md §8f row f4 test infrastructure on CPU: the BAM writer/reader of oracle/bam.py round-trips the
fixture records (tests/golden/region_split/*.json hold the reference's own outputs for them,
tests/golden/make_golden_region_split.py)."""
import glob
import json
import os

import bam
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "region_split")
ERRORS = {"KeyError": KeyError, "ZeroDivisionError": ZeroDivisionError}


def error_class(case):
    """The exception the reference raised on this fixture: the prefix of its `error` string."""
    return ERRORS[case["error"].split(":")[0]]


def cases():
    return [json.load(open(p)) for p in sorted(glob.glob(os.path.join(GOLD, "*.json")))]


@pytest.mark.parametrize("case", cases(), ids=[c["name"] for c in cases()])
def test_bam_round_trip(tmp_path, case):
    p = str(tmp_path / "x.bam")
    bam.write_bam(p, [tuple(r) for r in case["refs"]], case["records"])
    refs, recs = bam.read_bam(p)
    assert [list(r) for r in refs] == [list(r) for r in case["refs"]]
    assert len(recs) == len(case["records"])
    for a, r in zip(recs, case["records"]):
        assert a.query_name == r["name"] and a.flag == r["flag"] and a.reference_id == r["ref"]
        assert (a.query_sequence or "") == r["seq"]
        assert [("MIDNSHP=X"[op], ln) for op, ln in a.cigartuples] == [tuple(x) for x in r["cigar"]]


def test_fixtures_cover_the_branches():
    cs = {c["name"]: c for c in cases()}
    assert cs["unknown_reference"]["error"].startswith("KeyError")
    nc = cs["no_cigar"]
    assert nc["error"] is None and any(r["flag"] == 16 and not r["cigar"] for r in nc["records"])
    assert cs["append_existing"]["out_files"][next(iter(cs["append_existing"]["pre_existing"]))].startswith(">old")
    flags = {r["flag"] & 0x914 for c in cs.values() for r in c["records"]}
    assert {0, 4, 16, 256, 2048} <= flags | {x & ~16 for x in flags}
    assert len(cs) >= 17 and all(os.path.getsize(os.path.join(GOLD, n + ".json")) <= 470000 for n in cs)

    def kept(c):
        """name -> (strand, printed sequence) of the records in the fixture's output files"""
        out = {}
        for text in c["out_files"].values():
            lines = text.split("\n")
            for head, seq in zip(lines[0:-1:2], lines[1::2]):
                name, strand = head[1:].rsplit(";strand=", 1)
                out[name] = (strand, seq)
        return out

    # names that need a second, third and fourth trip of a 64-lane loop, on both strands
    k = kept(cs["name_lengths"])
    assert {(len(n), s) for n, (s, _) in k.items()} == {(ln, s) for ln in (1, 63, 64, 65, 128, 254) for s in "+-"}
    # every CIGAR op; kept records whose span comes from N, = or X alone; hard clips at both ends; only I / S
    c = cs["cigar_ops"]
    k = kept(c)
    assert {op for r in c["records"] for op, _ in r["cigar"]} == set("MIDNSHP=X")
    for only in "N=X":
        assert any(r["name"] in k and {op for op, _ in r["cigar"]} & set("MDN=X") == {only} for r in c["records"])
    assert any(r["name"] in k and r["cigar"][0][0] == "H" and r["cigar"][-1][0] == "H" for r in c["records"])
    only_is = [r for r in c["records"] if {op for op, _ in r["cigar"]} <= set("IS")]
    assert only_is and not any(r["name"] in k for r in only_is)
    assert "shorter overlap than minimal region overlap: 33.33\n" in next(iter(c["log_files"].values()))  # 8 of 24
    # all 16 sequence codes printed on both strands, at lengths on either side of 64, odd and even
    c = cs["iupac_seq"]
    k = kept(c)
    assert {(len(q), s) for s, q in k.values()} >= {(ln, s) for ln in (1, 2, 63, 64, 65, 127) for s in "+-"}
    for strand in "+-":
        assert set("".join(q for s, q in k.values() if s == strand)) == set(bam.SEQ_CODES)
    assert k["table_r"][1] == (bam.SEQ_CODES * 2)[::-1].translate(str.maketrans("ACGT", "TGCA"))
    # kept primary records without a stored sequence, on both strands
    c = cs["kept_without_seq"]
    k = kept(c)
    no_seq = {r["name"]: r["flag"] for r in c["records"] if not r["seq"]}
    assert {k[n] for n in no_seq if n in k} == {("+", "None"), ("-", "None")} and "no_seq_short" not in k
    # a KeyError for a region that the reference FASTA holds: the cluster lookup, after the earlier records' files
    c = cs["no_cluster"]
    missing = c["error"][len("KeyError: '"):-1]
    assert c["error"] == f"KeyError: '{missing}'" and missing in dict(map(tuple, c["regions"])) and missing not in c["clusters"]
    at = next(i for i, r in enumerate(c["records"]) if r["name"] == "c_passes")
    assert sorted(kept(c)) == ["a0", "a1", "b0", "b1"] and len(c["records"]) > at + 1
    assert any(c["refs"][r["ref"]][0] == missing for r in c["records"][:at])  # its short and long records do not raise
    assert cs["no_primary"]["error"] == "ZeroDivisionError: division by zero" and cs["no_primary"]["out_files"] == {}
    assert all(r["flag"] & 0x904 for r in cs["no_primary"]["records"])
    # the threshold fixtures: the reference keeps the three reads that a fused multiply-add of the bound drops as long
    from make_golden_region_split import fused_flips
    edges = [c for n, c in cs.items() if n.startswith("threshold_edges_")]
    assert {(c["minimal_region_overlap"], c["max_softclip_5_end"] + c["max_softclip_3_end"], ln) for c in edges
            for _, ln in c["regions"]} == {(0.93, 141, 400), (0.93, 141, 100), (0.93, 20, 1900), (0.95, 141, 500),
                                           (1.0, 0, 300), (0.5, 20, 640)}
    flips = []
    for c in edges:
        k = kept(c)
        for nm, ln in c["regions"]:
            assert [f"{nm}_span{d:+d}" in k for d in (-1, 0, 1, 2)] == [False, True, True, True]
            assert [f"{nm}_query{d:+d}" in k for d in (-1, 0, 1)] == [True, True, False]
            lens = [len(r["seq"]) for r in c["records"] if r["name"].startswith(nm + "_query")]
            assert lens == [lens[1] - 1, lens[1], lens[1] + 1]
        for ln, q in fused_flips(c):
            flips.append((ln, q))
            assert any(len(seq) == q for _, seq in k.values())  # kept by the reference
    assert sorted(flips) == [(100, 248), (400, 569), (1900, 2053)]


@pytest.mark.parametrize("case", cases(), ids=[c["name"] for c in cases()])
def test_oracle_restatement_vs_reference_fixtures(case):
    """oracle/region_split.py (the f4 checker and CPU baseline) reproduces the reference's files and counts."""
    import region_split as ors
    recs = [bam.AlignedSegment([tuple(r) for r in case["refs"]], r["ref"], r["pos"], r["flag"], r["name"],
                               [("MIDNSHP=X".index(op), ln) for op, ln in r["cigar"]], r["seq"] or None)
            for r in case["records"]]
    lengths = {nm: ln for nm, ln in case["regions"]}
    kw = dict(minimal_region_overlap=case["minimal_region_overlap"], max_softclip_5_end=case["max_softclip_5_end"],
              max_softclip_3_end=case["max_softclip_3_end"])
    if case["error"] and error_class(case) is KeyError:
        with pytest.raises(KeyError) as e:
            ors.split_records(recs, lengths, case["clusters"], **kw)
        assert f"KeyError: {e.value}" == case["error"]
        return
    counts, per_cluster, texts, _ = ors.split_records(recs, lengths, case["clusters"], **kw)
    want = {fn: t[len(case["pre_existing"].get(fn, "")):] for fn, t in case["out_files"].items()}
    assert {f"region_cluster{k}.fasta": t for k, t in texts.items()} == want
    if case["error"]:  # the record loop itself ran through: the log's percentages divide by the primary count
        assert error_class(case) is ZeroDivisionError and counts["primary"] == 0 and not case["log_files"]
        return
    log = next(iter(case["log_files"].values()))
    assert f"Total # primary alignments in bam file: {counts['primary']}\n" in log
