"""The round-2 region split, the precision census and the UMI count CSV (rows f4b, f6b and f7) without
a GPU.

tests/golden/by_region, precision and count hold what the reference's own filter_and_split_reads_by_region,
estimate_precision_at_num_subreads and write_region_umi_counts_to_csv left on each case (tests/golden/
make_golden_by_region.py, make_golden_precision.py, make_golden_count.py).  Here the Python halves of the drop-ins run
on tests/split_ref.py's plain-Python session, which implements split() and name_suffix() from their definitions, and
must reproduce every file, log, printed line, return value and exception.  The helpers are shared with
tests/test_gpu_round2.py, which puts the real session in the stand-in's place."""
import ast
import glob
import gzip
import json
import os
import warnings

import numpy as np
import pytest
from make_golden_region_split import fused_flips, write_inputs
from umiclust import _lib, count, minimap2_align
from umiclust import region_split as rs
from umiclust import vsearch_umi_cluster as _v

import bam_ref
import split_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BY_REGION = {os.path.basename(p)[:-5]: json.load(open(p)) for p in sorted(glob.glob(os.path.join(GOLD, "by_region", "*.json")))}
PRECISION = {os.path.basename(p)[:-5]: json.load(open(p)) for p in sorted(glob.glob(os.path.join(GOLD, "precision", "*.json")))}
COUNT = {os.path.basename(p)[:-5]: json.load(open(p)) for p in sorted(glob.glob(os.path.join(GOLD, "count", "*.json")))}
ERRORS = {"KeyError": KeyError, "ZeroDivisionError": ZeroDivisionError, "ValueError": ValueError,
          "RuntimeError": RuntimeError, "IndexError": IndexError}
SET_LINE = "missing/non-detected regions from reference: "


def norm_log(text):
    """The last line prints a Python set, whose order depends on string hashing: compare it as a set."""
    out = []
    for line in text.splitlines():
        if line.startswith(SET_LINE):
            out.append((SET_LINE, frozenset(ast.literal_eval(line[len(SET_LINE):]) or ())))
        else:
            out.append(line)
    return out


def read_dir(d):
    return {fn: open(os.path.join(d, fn)).read() for fn in sorted(os.listdir(d))}


# ---------------------------------------------------------------- by region
def by_region_kw(case):
    return dict(minimal_region_overlap=case["minimal_region_overlap"], max_softclip_5_end=case["max_softclip_5_end"],
                max_softclip_3_end=case["max_softclip_3_end"])


def check_by_region(case, tmp_path, call):
    """call(bam_path, ref_fa, logs, out, **kw) runs one form of the drop-in on the case's inputs; its return value or
    exception, the FASTA files and the log must be the reference's"""
    bam_path, ref_fa, _, out, logs = write_inputs(case, str(tmp_path))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # numpy's median of an empty list, as in the reference
        if case["error"]:
            exc = ERRORS[case["error"].split(":")[0]]
            with pytest.raises(exc) as e:
                call(bam_path, ref_fa, logs, out, **by_region_kw(case))
            assert f"{exc.__name__}: {e.value}" == case["error"]
        else:
            ret = call(bam_path, ref_fa, logs, out, **by_region_kw(case))
            assert sorted(os.path.relpath(p, str(tmp_path)) for p in ret) == case["result"]
    assert read_dir(out) == case["out_files"]
    assert {fn: norm_log(t) for fn, t in read_dir(logs).items()} == {fn: norm_log(t) for fn, t in case["log_files"].items()}


def standin(bam_path):
    return split_ref.Session(gzip.decompress(open(bam_path, "rb").read()))


@pytest.mark.parametrize("keep", ["none", "ones"])
@pytest.mark.parametrize("name", sorted(BY_REGION))
def test_by_region_python_half_on_the_standin_session(name, keep, tmp_path):
    def call(bam_path, ref_fa, logs, out, **kw):
        src = standin(bam_path)
        return rs.filter_and_split_reads_by_region_from(src, None if keep == "none" else np.ones(src.n, np.uint8), bam_path,
                                                        ref_fa, logs, out, **kw)
    check_by_region(BY_REGION[name], tmp_path, call)


@pytest.mark.parametrize("name", ["small", "unknown_reference", "no_primary"])
def test_by_region_file_form_opens_a_session(name, tmp_path, monkeypatch):
    monkeypatch.setattr(_v, "context", lambda device=None: split_ref.Context())
    check_by_region(BY_REGION[name], tmp_path, rs.filter_and_split_reads_by_region)


def test_by_region_fixtures_cover_the_issue():
    cs = BY_REGION
    assert len(cs["many_regions"]["regions"]) >= 30
    assert sum(nm.endswith(rs.NEGATIVE_CONTROL_SUFFIXES) for nm, _ in cs["many_regions"]["regions"]) >= 3
    pre = cs["append_existing"]["pre_existing"]
    assert len(pre) == 1 and all(fn.startswith("region_TRBV") and cs["append_existing"]["out_files"][fn].startswith(t)
                                 and len(cs["append_existing"]["out_files"][fn]) > len(t) for fn, t in pre.items())
    assert cs["unknown_reference"]["error"] == "KeyError: 'not_in_reference'" and cs["unknown_reference"]["out_files"]
    assert cs["refid_minus1"]["error"] == "KeyError: None" and len(cs["refid_minus1"]["out_files"]) == 2
    assert cs["no_primary"]["error"] == "ZeroDivisionError: division by zero" and not cs["no_primary"]["out_files"]
    none_kept = cs["none_kept"]
    assert none_kept["error"] is None and none_kept["result"] == [] and not none_kept["out_files"]
    assert "are not too long: nan\n" in next(iter(none_kept["log_files"].values()))
    assert sum(t.count("\nNone\n") for t in cs["kept_without_seq"]["out_files"].values()) == 3
    for strand in "+-":
        seqs = "".join(t.split("\n")[i + 1] for t in cs["iupac_seq"]["out_files"].values()
                       for i, ln in enumerate(t.split("\n")) if ln.endswith(";strand=" + strand))
        assert set(seqs) == set(split_ref.SEQ_CODES)
    lens = {len(ln) - len(";strand=+") - 1 for t in cs["name_lengths"]["out_files"].values() for ln in t.split("\n")
            if ln.startswith(">")}
    assert lens == {1, 63, 64, 65, 128, 254}
    edges = [c for n, c in cs.items() if n.startswith("threshold_edges_")]
    assert sorted(f for c in edges for f in fused_flips(c)) == [(100, 248), (400, 569), (1900, 2053)]
    for c in edges:  # the reference keeps the read exactly at the bound, which a fused multiply-add drops
        kept = {len(ln) for t in c["out_files"].values() for ln in t.split("\n")[1::2]}
        assert all(q in kept for _, q in fused_flips(c))
    small = next(iter(cs["small"]["log_files"].values())).split("\n")  # a mixed draw: short, long and kept records
    assert all(float(small[k].rsplit(": ", 1)[1]) > 5 for k in (1, 2, 3)) and len(cs["small"]["out_files"]) == 6
    assert all(os.path.getsize(os.path.join(GOLD, "by_region", n + ".json")) <= 40000 and len(c["records"]) <= 500
               for n, c in cs.items())
    assert all(fn.startswith("region_") and not fn.startswith("region_cluster") for c in cs.values() for fn in c["out_files"])


def test_keep_mask_is_the_file_of_the_kept_records(tmp_path):
    """Splitting a session under keep equals splitting a BAM that holds only the kept records."""
    case = BY_REGION["small"]
    rng = np.random.default_rng(5)
    keep = (rng.random(len(case["records"])) < 0.6).astype(np.uint8)
    sub = dict(case, records=[r for r, k in zip(case["records"], keep) if k])
    dirs = []
    for tag, c, k in (("masked", case, keep), ("subset", sub, None)):
        d = tmp_path / tag
        bam_path, ref_fa, _, out, logs = write_inputs(c, str(d))
        ret = rs.filter_and_split_reads_by_region_from(standin(bam_path), k, bam_path, ref_fa, logs, out, **by_region_kw(c))
        dirs.append((sorted(os.path.relpath(p, str(d)) for p in ret), read_dir(out),
                     {fn: norm_log(t) for fn, t in read_dir(logs).items()}))
    assert dirs[0] == dirs[1] and dirs[0][1]


# ---------------------------------------------------------------- precision
def check_precision(case, name, tmp_path, capsys, call):
    """call(bam_path, fasta, logs, **params); the CSV, the printed lines and the exception must be the reference's"""
    logs = tmp_path / "logs"
    logs.mkdir()
    fasta = tmp_path / "ref.fa"
    bam_ref.write_fasta(fasta, case["regions"])
    bam_path = str(tmp_path / (name + ".bam"))
    bam_ref.write_bam(bam_path, case["refs"], case["records"])
    e, err = case["expect"], None
    capsys.readouterr()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # numpy's mean / median of an empty list, as in the reference
        try:
            assert call(bam_path, str(fasta), str(logs), **case["params"]) is None
        except tuple(ERRORS.values()) as x:
            err = [type(x).__name__, [str(a) if a is not None else None for a in x.args]]
    assert err == e["error"]
    assert capsys.readouterr().out == e["stdout"]
    assert read_dir(logs) == e["files"]


@pytest.mark.parametrize("name", sorted(PRECISION))
def test_precision_python_half_on_the_standin_session(name, tmp_path, capsys):
    def call(bam_path, fasta, logs, **params):
        return minimap2_align.estimate_precision_at_num_subreads_from(standin(bam_path), bam_path, fasta, logs, **params)
    check_precision(PRECISION[name], name, tmp_path, capsys, call)


def test_precision_file_form_opens_a_session(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(_v, "context", lambda device=None: split_ref.Context())
    check_precision(PRECISION["tails"], "tails", tmp_path, capsys, minimap2_align.estimate_precision_at_num_subreads)


def test_precision_fixtures_cover_the_issue():
    names = [r["name"] for r in PRECISION["tails"]["records"]]
    status = {n: split_ref.name_suffix(n)[1] for n in names}
    assert [n for n in names if n.endswith(("_1", "_007"))] and "12345" in names
    assert {len(n.split("_")[-1]) for n in names if status[n]} >= {1, 3, 5, 18}
    assert [n for n in names if len(n.split("_")[-1]) == 19 and n.split("_")[-1].isdigit() and not status[n]]
    assert [n for n in names if n.endswith("_+5") and not status[n]]
    csv_text = next(iter(PRECISION["tails"]["expect"]["files"].values()))
    assert "\n9,0.0\n" in csv_text and "\n1,0.5\n" in csv_text  # mapped and never written: fillna(0)
    assert [PRECISION[k]["expect"]["error"][0] for k in ("tail_empty", "tail_nondigit", "tail_no_underscore")] == ["ValueError"] * 3
    for k in ("nothing_above_threshold", "no_primary"):  # the final division, after the CSV and four printed lines
        e = PRECISION[k]["expect"]
        assert e["error"][0] == "ZeroDivisionError" and len(e["files"]) == 1 and e["stdout"].count("\n") == 4
    assert PRECISION["zero_columns"]["expect"] == {"error": ["ZeroDivisionError", ["division by zero"]], "stdout": "", "files": {}}
    assert PRECISION["unknown_ref"]["expect"]["error"] == ["KeyError", ["not_in_fasta"]]
    eq = PRECISION["identity_equals_threshold"]
    assert eq["params"]["blast_id_threshold"] == 0.99 == (200 - 2) / 200 and eq["expect"]["stdout"].startswith("2 4\n")
    assert PRECISION["overlap_below_one"]["params"]["minimal_region_overlap"] < 1 and "minimal_region_overlap" not in eq["params"]


# ---------------------------------------------------------------- filter + split on one session
def fused_and_two_step(case, tmp_path, monkeypatch):
    """filter_consensus_alignments_and_split, and filter_consensus_alignments followed by
    filter_and_split_reads_by_region on the filtered BAM it wrote: per form the list, the region files, the logs
    directory (the split log among it) and the filtered BAM's stream, which must all be equal"""
    monkeypatch.setattr(minimap2_align.subprocess, "run", lambda *a, **k: None)  # samtools index
    got = []
    for tag in ("fused", "two_step"):
        d = tmp_path / tag
        for sub in ("logs", "fa"):
            (d / sub).mkdir(parents=True)
        bam_ref.write_fasta(d / "ref.fa", case["regions"])
        bam_ref.write_bam(d / "cons.bam", case["refs"], case["records"])
        args = (str(d / "cons.bam"), str(d / "ref.fa"), str(d / "logs"), case["params"]["blast_id_threshold"])
        kw = dict(minimal_region_overlap=case["params"]["minimal_region_overlap"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # numpy's mean / median of an empty list, as in the reference
            if tag == "fused":
                filtered, fastas = minimap2_align.filter_consensus_alignments_and_split(*args, str(d / "fa"), **kw)
            else:
                filtered = minimap2_align.filter_consensus_alignments(*args, **kw)
                fastas = rs.filter_and_split_reads_by_region(filtered, str(d / "ref.fa"), str(d / "logs"), str(d / "fa"),
                                                             **kw)
        assert filtered == str(d / "cons_filtered.bam")
        got.append((sorted(os.path.relpath(p, str(d)) for p in fastas), read_dir(d / "fa"),
                    {fn: norm_log(t) for fn, t in read_dir(d / "logs").items()}, bam_ref.check_bgzf(filtered)))
    assert got[0] == got[1]
    assert "cons_filtered_filter_and_split_reads_by_region.err" in got[0][2]
    assert sum(t.count(">") for t in got[0][1].values()) == len(case["expect"]["kept"]) > 0
    return got[0]


FUSED_CASES = ["big_output", "grouping"]  # of tests/golden/bam_filter: one region in several BGZF blocks; three regions


@pytest.mark.parametrize("name", FUSED_CASES)
def test_filter_and_split_equals_the_two_steps(name, tmp_path, monkeypatch):
    monkeypatch.setattr(_v, "context", lambda device=None: split_ref.Context())
    case = json.load(open(os.path.join(GOLD, "bam_filter", name + ".json")))
    lists = fused_and_two_step(case, tmp_path, monkeypatch)[0]
    assert lists == sorted("fa/region_%s.fasta" % n for n in {case["refs"][case["records"][k].get("ref", 0)][0]
                                                               for k in case["expect"]["kept"]})


# ---------------------------------------------------------------- count.py
def run_count(case, tmp_path):
    paths = []
    for rel, text in case["files"]:
        p = tmp_path / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(text)
        paths.append(str(p))
    out = tmp_path / "counts"
    out.mkdir()
    return paths, out


@pytest.mark.parametrize("name", sorted(COUNT))
def test_count_against_the_reference(name, tmp_path):
    case, e = COUNT[name], COUNT[name]["expect"]
    paths, out = run_count(case, tmp_path)
    if e["error"]:
        for call in (lambda: count.umi_counter(smolecule_filtered_fa_list=paths),
                     lambda: count.write_region_umi_counts_to_csv(paths, str(out), region_name=case["region_name"])):
            with pytest.raises(ERRORS[e["error"][0]]) as ei:
                call()
            assert [str(a).replace(str(tmp_path), "{tmp}") for a in ei.value.args] == e["error"][1]
        assert os.listdir(out) == []
        return
    assert [[k, v] for k, v in count.umi_counter(smolecule_filtered_fa_list=paths).items()] == e["counter"]
    assert count.write_region_umi_counts_to_csv(paths, str(out), region_name=case["region_name"]) is None
    assert read_dir(out) == {"umi_consensus_counts.csv": e["csv"]}


def test_count_task_forms_and_missing_file(tmp_path):
    p = tmp_path / "a.fa"
    p.write_text(">x\nAC\n>y\nGT\n")
    assert count.count_sequences_in_fasta.remote(str(p)) == 2 == count.count_sequences_in_fasta(str(p))
    with pytest.raises(RuntimeError) as e:
        count.count_sequences_in_fasta.remote(str(tmp_path / "absent.fa"))
    absent = str(tmp_path / "absent.fa")
    assert str(e.value) == (f"Exception occurred while processing {absent}: Error processing {absent}: "
                            f"grep: {absent}: No such file or directory")
    assert {c["expect"]["error"][0] for c in COUNT.values() if c["expect"]["error"]} == {"RuntimeError", "IndexError"}


# ---------------------------------------------------------------- the library's symbols
def test_exports_and_abi():
    names = {"umiclust_bam_split", "umiclust_bam_name_suffix"}
    assert names <= set(_lib.EXPORTS)
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n), n
    assert lib.umiclust_abi_version() == 9
