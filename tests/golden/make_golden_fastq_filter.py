"""Generate tests/golden/argv_fastq_filter.json from the REFERENCE itself (run here, not on the GPU box): the exact
`vsearch --fastq_filter` argv that vsearch_fastq_filtering builds
(/root/reference/ont_tcr_consensus/preprocessing.py:104-159, argv :129-148) and the path it returns.

`ray` is not installed: ray.remote is a pass-through decorator.  subprocess.run records its arguments and runs
nothing (the function's seqkit calls are recorded too and left out of the fixture).  The function opens its seqkit
statistics files for writing, so it runs inside a temporary directory with relative paths.  Only data is written.

Usage: python tests/golden/make_golden_fastq_filter.py  (requires /root/reference)
"""
from __future__ import annotations

import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (the stubs and the module loader)

CASES = [
    # max_ee_rate_base and minimal_length of the reference's run_config.json
    dict(fastq="fastq/libA/reads_trimmed.fastq", out={"libA": "out/libA"}, logs={"libA": "logs/libA"},
         max_ee_rate_base=0.07, minimal_length=1470),
    dict(fastq="fastq/lib_B/barcode07.pass.fastq", out={"lib_B": "out/b"}, logs={"lib_B": "logs/b"},
         max_ee_rate_base=0.015, minimal_length=900),
]


def main():
    make_golden._stub_modules()
    captured = []
    real_run = subprocess.run
    cwd = os.getcwd()
    calls = []
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        subprocess.run = lambda argv, *a, **k: captured.append(list(argv))
        try:
            mod = make_golden._load("preprocessing")
            for c in CASES:
                for d in list(c["out"].values()) + list(c["logs"].values()):
                    os.makedirs(d, exist_ok=True)
                captured.clear()
                ret = mod.vsearch_fastq_filtering(c["fastq"], c["out"], c["logs"], c["max_ee_rate_base"],
                                                  c["minimal_length"])
                argv = [a for a in captured if a and a[0] == "vsearch"]
                assert len(argv) == 1
                calls.append(dict(args=c, argv=argv[0], ret=ret))
        finally:
            subprocess.run = real_run
            os.chdir(cwd)
    with open(os.path.join(HERE, "argv_fastq_filter.json"), "w") as fh:
        json.dump(dict(calls=calls), fh, indent=1)
    print(f"wrote {len(calls)} argv lists")


if __name__ == "__main__":
    main()
