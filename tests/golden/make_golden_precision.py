"""Generate tests/golden/precision/*.json from the REFERENCE itself (run where the reference is present, not on the GPU
box): inputs and outputs of estimate_precision_at_num_subreads (ont_tcr_consensus/minimap2_align.py:362-435, SURVEY.md
§8f row f6b).

Built like make_golden_bam_filter.py, whose reference loader (the pysam stand-in of tests/bam_ref.py, the installed
pandas and numpy) and record builders are imported from it.  A fixture holds data only: records, references, regions,
parameters, the CSV's text, what the function printed and the exception it raised.

Usage: python tests/golden/make_golden_precision.py  (requires /root/reference)
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import shutil
import sys
import tempfile
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_bam_filter as f6  # noqa: E402  (puts tests/ and the package on sys.path)
import bam_ref  # noqa: E402

OUT = os.path.join(HERE, "precision")
REGIONS = f6.REGIONS  # lengths 200, 300, 250


def rec(name, ref=0, nm=0, cigar=None, flag=0, l_seq=None, tags=None):
    """good_cigar(L): reference_length L + 7, l_seq L + 13, cols L: passes overlap 1.0, blast identity (L - nm) / L"""
    r = f6.rec(0, ref, cigar or f6.good_cigar(REGIONS[ref][1]), [("NM", "C", nm)] if tags is None else tags, flag=flag,
               l_seq=l_seq)
    r["name"] = name
    return r


DIGITS18, DIGITS19 = "123456789012345678", "1234567890123456789"


def case_tails():
    """every tail int() accepts: plain, leading zeros, 18 and 19 digits, a name of digits only, a sign, and names with
    more than one "_"; the counts 1 and 7 are mapped more often than written, 9 is mapped and never written"""
    names = ["a_1", "b_1", "c_007", "d_7", "e_" + DIGITS18, "f_" + DIGITS19, "12345", "g_+5", "h_5", "i_x_y_12",
             "_3", "j__4", "k_9", "l_9", "m_0", "n_00", "o_-2", "p_ 6", "q_1_000"]
    recs = [rec(nm, ref=i % 3, nm=(2 if nm in ("b_1", "d_7", "k_9", "l_9") else 0)) for i, nm in enumerate(names)]
    recs.append(rec("unmapped_x", flag=4))       # never parsed
    recs.append(rec("secondary_y", flag=0x100))
    recs.append(rec("short_8", cigar=[("M", 150)]))   # mapped, dropped as short
    recs.append(rec("long_8", l_seq=600))             # mapped, dropped as too long
    return dict(records=recs, params=dict())


def case_bad_tail(name):
    recs = [rec("ok_7"), rec("ok_8", ref=1), rec(name, ref=2), rec("after_9")]
    return dict(records=recs, params=dict())


def case_nothing_above_threshold():
    recs = [rec("r%d_%d" % (i, 1 + i % 5), ref=i % 3, nm=i % 2) for i in range(12)]
    return dict(records=recs, params=dict())  # num_subreads_threshold 6: the final division is 0 / 0


def case_identity_equals_threshold():
    """region 200: cols 200, NM 2 gives 198 / 200 == 0.99 (kept by >=), NM 3 gives 0.985"""
    recs = [rec("r%d_%d" % (i, 5 + i % 4), nm=2 + i % 2) for i in range(10)]
    assert (200 - 2) / 200 == 0.99
    return dict(records=recs, params=dict(blast_id_threshold=0.99, num_subreads_threshold=7))


def case_overlap_below_one():
    recs = []
    for i in range(40):
        L = REGIONS[i % 3][1]
        kind = i % 5
        cigar = [("M", int(L * 0.9) - 1 + (i % 2))] if kind == 3 else None   # span on either side of L * 0.9
        l_seq = int(L * 1.1 + 141) + (i % 2) if kind == 4 else None          # l_seq on either side of the bound
        recs.append(rec("r%d_%d" % (i, 2 + i % 9), ref=i % 3, nm=i % 4, cigar=cigar, l_seq=l_seq,
                        flag=(0x800 if i == 17 else 0)))
    return dict(records=recs, params=dict(minimal_region_overlap=0.9, blast_id_threshold=0.995, num_subreads_threshold=4))


def case_no_primary():
    recs = [rec("r%d_%d" % (i, 6 + i), flag=(4, 0x100, 0x800, 0x104)[i % 4]) for i in range(6)]
    return dict(records=recs, params=dict())


def case_unknown_ref():
    recs = [rec("r%d_%d" % (i, 6 + i), ref=i % 3) for i in range(8)]
    recs[5]["ref"] = 3
    return dict(records=recs, refs=REGIONS + [["not_in_fasta", 400]], params=dict())


def case_nm_missing():
    recs = [rec("r%d_%d" % (i, 6 + i)) for i in range(5)]
    recs[3]["tags"] = []
    return dict(records=recs, params=dict())


def case_zero_columns():
    """a CIGAR of N alone spans the region and has no M / I / D column: calculate_blast_id divides by zero"""
    recs = [rec("r0_6"), rec("r1_7", cigar=[("N", 200)], l_seq=0), rec("r2_8")]
    return dict(records=recs, params=dict())


def cases():
    return {"tails": case_tails(), "tail_empty": case_bad_tail("trailing_"), "tail_nondigit": case_bad_tail("z_x9"),
            "tail_no_underscore": case_bad_tail("nounderscore"), "nothing_above_threshold": case_nothing_above_threshold(),
            "identity_equals_threshold": case_identity_equals_threshold(), "overlap_below_one": case_overlap_below_one(),
            "no_primary": case_no_primary(), "unknown_ref": case_unknown_ref(), "nm_missing": case_nm_missing(),
            "zero_columns": case_zero_columns()}


def run_case(mod, name, case):
    case.setdefault("refs", REGIONS)
    case.setdefault("regions", REGIONS)
    tmp = tempfile.mkdtemp()
    try:
        logs = os.path.join(tmp, "logs")
        os.mkdir(logs)
        bam = os.path.join(tmp, name + ".bam")
        bam_ref.write_bam(bam, case["refs"], case["records"])
        fasta = os.path.join(tmp, "ref.fa")
        bam_ref.write_fasta(fasta, case["regions"])
        expect = {"error": None}
        printed = io.StringIO()
        with warnings.catch_warnings(), contextlib.redirect_stdout(printed):
            warnings.simplefilter("ignore")  # numpy's mean / median of an empty list
            try:
                assert mod.estimate_precision_at_num_subreads(bam, fasta, logs, **case["params"]) is None
            except Exception as e:
                expect["error"] = [type(e).__name__, [str(a) if a is not None else None for a in e.args]]
        expect["stdout"] = printed.getvalue()
        expect["files"] = {f: open(os.path.join(logs, f)).read() for f in sorted(os.listdir(logs))}
        case["expect"] = expect
    finally:
        shutil.rmtree(tmp)
    return case


def main():
    mod = f6.load_reference()
    os.makedirs(OUT, exist_ok=True)
    for name, case in cases().items():
        case = run_case(mod, name, case)
        with open(os.path.join(OUT, name + ".json"), "w") as fh:
            json.dump(case, fh, indent=None, separators=(",", ":"))
            fh.write("\n")
        e = case["expect"]
        print(name, len(case["records"]), "records; error", e["error"], "files", list(e["files"]), repr(e["stdout"]))


if __name__ == "__main__":
    main()
