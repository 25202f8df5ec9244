"""Generate tests/golden/by_region/*.json from the REFERENCE itself (run where the reference is present, not on the
GPU box): inputs and outputs of filter_and_split_reads_by_region (ont_tcr_consensus/region_split.py:336-435, SURVEY.md
§8f row f4b), the round-2 split of the filtered consensus BAM into one FASTA per reference name.

Built like make_golden_region_split.py, whose record builders, input writer and pysam stand-in (oracle/bam.py) are
imported from it: a fixture holds data only (records, reference regions, parameters, output files, the log, the
returned paths or the exception text).  The `clusters` a builder adds are not read by this function.

Usage: python tests/golden/make_golden_by_region.py  (requires /root/reference)
"""
from __future__ import annotations

import json
import os
import random
import shutil
import sys
import tempfile
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_region_split as f4  # noqa: E402  (puts oracle/ on sys.path)
import bam  # noqa: E402
import make_golden  # noqa: E402


def refid_minus1_case(rng):
    """A mapped primary record without a reference (refID -1): reference_name is None and the length lookup raises
    KeyError(None), after the files of the records before it."""
    records = [f4._rec("a0", 0, 0, f4._cigar(60, 60), f4._seq(rng, 60)),
               f4._rec("unmapped_no_ref", 4, -1, [], f4._seq(rng, 40)),  # counted as unmapped, never looked up
               f4._rec("b0", 16, 1, f4._cigar(59, 61), f4._seq(rng, 61)),
               f4._rec("no_ref", 0, -1, f4._cigar(60, 60), f4._seq(rng, 60)),
               f4._rec("a_never", 0, 0, f4._cigar(60, 60), f4._seq(rng, 60))]
    return f4._case("refid_minus1", f4.DEFAULT_REGIONS, records)


def none_kept_case(rng):
    """Primary records, every one too short or too long: no file, and the median of an empty list in the log."""
    records = [f4._rec(f"s{i}", 16 * (i & 1), i % 2, f4._cigar(50 + i % 6, 60), f4._seq(rng, 60)) for i in range(6)]
    records += [f4._rec(f"l{i}", 16 * (i & 1), i % 2, f4._cigar(60, 205 + i), f4._seq(rng, 205 + i)) for i in range(4)]
    return f4._case("none_kept", f4.DEFAULT_REGIONS, records)


class ShortDraws(random.Random):
    """make_case draws region lengths with randint(300, 700), unaligned reads with randint(50, 300) and clips with
    randint(0, 90) and (0, 80): a tenth of each, with softclip allowances of 7 and 6, keeps the mixture of short, long
    and kept reads at a tenth of the bytes.  The hand-built cases below keep the default allowances."""

    def randint(self, a, b):
        return super().randint(a // 10, b // 10) if b >= 80 else super().randint(a, b)


def cases():
    rng = ShortDraws(20261101)
    out = [f4.make_case(rng, "small", 6, 100, s5=7, s3=6), f4.make_case(rng, "many_regions", 32, 100, s5=7, s3=6),
           f4.make_case(rng, "append_existing", 5, 60, s5=7, s3=6),
           f4.make_case(rng, "unknown_reference", 5, 60, s5=7, s3=6, unknown_ref=True)]
    assert sum(nm.endswith(("_v_n", "cdr3j_n", "full_n")) for nm, _ in out[1]["regions"]) >= 3
    for r in out[3]["records"][:20]:  # the unknown reference comes after records whose files are written
        r["ref"] = r["ref"] % len(out[3]["regions"]) if r["ref"] >= 0 else -1
    first = out[2]["regions"][0][0]
    out[2]["pre_existing"] = {f"region_{first}.fasta": ">old;strand=+\nACGT\n"}  # this function appends as well
    hand = random.Random(20261102)
    # hand_cases asserts the three fused-multiply-add flips (100/248, 400/569, 1900/2053) of its threshold-edge rows,
    # which the two 0.93 cases hold; the cluster lookup of no_cluster is not part of this function
    keep = ("name_lengths", "iupac_seq", "kept_without_seq", "threshold_edges_093", "threshold_edges_093_tight", "no_primary")
    out += [c for c in f4.hand_cases(hand) if c["name"] in keep]
    out += [refid_minus1_case(hand), none_kept_case(hand)]
    return out


def run_reference(mod, case):
    tmp = tempfile.mkdtemp(prefix="br_")
    try:
        bam_path, ref_fa, _, out, logs = f4.write_inputs(case, tmp)
        res = dict(case)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # numpy's median of an empty list
            try:
                ret = mod.filter_and_split_reads_by_region(
                    bam_file=bam_path, reference=ref_fa, logs_dir=logs, region_fasta_out_dir=out,
                    minimal_region_overlap=case["minimal_region_overlap"],
                    max_softclip_5_end=case["max_softclip_5_end"], max_softclip_3_end=case["max_softclip_3_end"])
                res["result"] = sorted(os.path.relpath(p, tmp) for p in ret)
                res["error"] = None
            except Exception as e:  # KeyError: an unknown region; ZeroDivisionError: the log without primaries
                res["result"] = None
                res["error"] = f"{type(e).__name__}: {e}"
        res["out_files"] = {fn: open(os.path.join(out, fn)).read() for fn in sorted(os.listdir(out))}
        res["log_files"] = {fn: open(os.path.join(logs, fn)).read() for fn in sorted(os.listdir(logs))}
        return res
    finally:
        shutil.rmtree(tmp)


def main():
    make_golden._stub_modules()
    sys.modules["pysam"].AlignmentFile = bam.AlignmentFile
    mod = make_golden._load("region_split")
    od = os.path.join(HERE, "by_region")
    os.makedirs(od, exist_ok=True)
    for c in cases():
        r = run_reference(mod, c)
        with open(os.path.join(od, c["name"] + ".json"), "w") as fh:
            json.dump(r, fh, indent=None, separators=(",", ":"), sort_keys=True)
            fh.write("\n")
        print(c["name"], len(c["records"]), r["result"] and len(r["result"]), r["error"], list(r["log_files"]))


if __name__ == "__main__":
    main()
