"""Generate tests/golden/count/*.json from the REFERENCE itself (run where the reference is present): inputs and
outputs of write_region_umi_counts_to_csv and umi_counter (ont_tcr_consensus/count.py:23-51).

The reference's functions run with the installed pandas and `grep`; `ray` is not installed and is replaced by a
stand-in whose remote tasks run in-process.  A fixture holds data only: the FASTA files (paths relative to a scratch
directory and their text), the order of the list, region_name, and the CSV's text, the counter or the exception text
(with the scratch directory written as {tmp}).

Usage: python tests/golden/make_golden_count.py  (requires /root/reference)
"""
from __future__ import annotations

import importlib.util
import json
import os
import shutil
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = "/root/reference/ont_tcr_consensus/count.py"
OUT = os.path.join(HERE, "count")


def load_reference():
    ray = types.ModuleType("ray")

    class _Task:
        def __init__(self, fn):
            self._fn = fn

        def remote(self, *a, **kw):
            return self._fn(*a, **kw)

    ray.remote = lambda *a, **k: _Task(a[0]) if a and callable(a[0]) else _Task
    ray.get = lambda values: values
    sys.modules["ray"] = ray
    spec = importlib.util.spec_from_file_location("reference_count", REFERENCE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fasta(n, tail_newline=True):
    text = "".join(">umi%d;x=%d\nACGT%s\n" % (i, i, "A>C" * (i % 3)) for i in range(n))  # a '>' inside a line is no record
    return text if tail_newline else text[:-1]


def cases():
    return {
        "basic": dict(files=[["smolecule/region_TRBV1_1/a.fa", fasta(3)], ["smolecule/region_TRBV20_4_v_n/b.fa", fasta(120)],
                             ["smolecule/region_TRAV7/c.fa", fasta(1, tail_newline=False)],
                             ["smolecule/region_last_header_only/d.fa", fasta(2) + ">no_newline"]], region_name="TCR"),
        "quoting": dict(files=[["x/region_A,B/a.fa", fasta(2)], ["x/region_say \"hi\"/b.fa", fasta(4)],
                               ["x/region_ spaced /c.fa", fasta(5)]], region_name="region, name"),
        "same_region_twice": dict(files=[["x/region_R1/a.fa", fasta(2)], ["x/region_R2/b.fa", fasta(3)],
                                         ["x/region_R1/c.fa", fasta(7)]], region_name="TCR"),
        "region_in_two_components": dict(files=[["x/region_outer/region_inner/a.fa", fasta(2)]], region_name="TCR"),
        "empty_list": dict(files=[], region_name="TCR"),
        "no_header_line": dict(files=[["x/region_R1/a.fa", fasta(2)], ["x/region_R2/b.fa", "ACGT\nAC>GT\n"],
                                      ["x/region_R3/c.fa", fasta(1)]], region_name="TCR"),
        "empty_file": dict(files=[["x/region_R1/a.fa", ""]], region_name="TCR"),
        "no_region_in_dirname": dict(files=[["x/plain/a.fa", fasta(2)]], region_name="TCR"),
    }


def write_files(case, tmp):
    paths = []
    for rel, text in case["files"]:
        p = os.path.join(tmp, rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "w") as fh:
            fh.write(text)
        paths.append(p)
    os.makedirs(os.path.join(tmp, "counts"), exist_ok=True)
    return paths, os.path.join(tmp, "counts")


def run_case(mod, case):
    tmp = tempfile.mkdtemp()
    try:
        paths, out = write_files(case, tmp)
        expect = {"error": None, "csv": None, "counter": None}
        try:
            expect["counter"] = [[k, v] for k, v in mod.umi_counter(smolecule_filtered_fa_list=paths).items()]
            assert mod.write_region_umi_counts_to_csv(paths, out, region_name=case["region_name"]) is None
            expect["csv"] = open(os.path.join(out, "umi_consensus_counts.csv")).read()
        except Exception as e:
            expect["error"] = [type(e).__name__, [str(a).replace(tmp, "{tmp}") for a in e.args]]
        assert os.listdir(out) == (["umi_consensus_counts.csv"] if expect["csv"] is not None else [])
        case["expect"] = expect
    finally:
        shutil.rmtree(tmp)
    return case


def main():
    mod = load_reference()
    os.makedirs(OUT, exist_ok=True)
    for name, case in cases().items():
        case = run_case(mod, case)
        with open(os.path.join(OUT, name + ".json"), "w") as fh:
            json.dump(case, fh, indent=None, separators=(",", ":"))
            fh.write("\n")
        print(name, case["expect"])


if __name__ == "__main__":
    main()
