"""Measurement tool for DESIGN.md §9c (rows f6 + f4b): wall-clock time of filter_consensus_alignments_and_split (one
session) next to filter_consensus_alignments followed by filter_and_split_reads_by_region on the filtered BAM it wrote
(two sessions), on one seeded synthetic consensus BAM.  Not a gate and not part of bench.py.

    python tools/round2_split_bench.py [records = 20000] [--out DIR]

The input: `records` draws (seed 20261103) from 2,000 template records shaped like consensus alignments -- 1,500-base
reads on 100 regions of 1,500, NM 0..12, a cs:Z string of 10 to 80 bytes, a trailing _<subreads> in the name; one in
ten unmapped, secondary or clipped short -- written as BGZF by tests/bam_ref.py.  `samtools index` is not run.  Prints
one JSON line with the median of five runs of either path."""
import json
import os
import random
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ont-tcrconsensus_amd"), os.path.join(ROOT, "tests")]
import bam_ref  # noqa: E402

REGIONS = [["TRBV%d" % r, 1500] for r in range(100)]


def build(n, seed, path):
    rng = random.Random(seed)
    templates = []
    for t in range(2000):
        kind = rng.random()
        cigar = [["S", rng.randrange(0, 60)], ["M", 1500 if kind > 0.04 else 1200], ["S", 20]]
        flag = 4 if kind > 0.98 else 0x100 if kind > 0.96 else 16 * rng.randrange(2)
        cs = "".join(rng.choice([":%d" % rng.randrange(3, 900), "*ag", "*ct", "+a", "-t"]) for _ in range(rng.randrange(3, 20)))
        templates.append(bam_ref.encode_record(
            {"name": "cons%05d_%d" % (t, rng.randrange(1, 40)), "flag": flag, "ref": rng.randrange(100), "cigar": cigar,
             "tags": [["NM", "i", rng.choice([0, 0, 0, 1, 2, 5, 12])], ["tp", "A", "P"], ["cs", "Z", cs]]}))
    raw = bam_ref.build_raw(REGIONS, []) + b"".join(rng.choice(templates) for _ in range(n))
    bam_ref.write_bgzf(path, raw, block=0xff00)
    return len(raw)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 20000
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else tempfile.mkdtemp()
    os.makedirs(out, exist_ok=True)
    path, fasta = os.path.join(out, "cons.bam"), os.path.join(out, "ref.fa")
    nbytes = build(n, 20261103, path)
    bam_ref.write_fasta(fasta, REGIONS)
    from umiclust import minimap2_align, region_split
    minimap2_align.subprocess.run = lambda *a, **k: None  # samtools index
    res = {"records": n, "inflated_bytes": nbytes, "file_bytes": os.path.getsize(path)}
    kw = dict(minimal_region_overlap=0.9975)
    times = {"fused_s": [], "two_step_s": []}
    for run in range(6):  # the first run of either path also creates the context and loads the kernels: dropped
        for tag in times:
            logs, fa = os.path.join(out, "logs"), os.path.join(out, "fa")
            for d in (logs, fa):
                shutil.rmtree(d, ignore_errors=True)
                os.mkdir(d)
            t0 = time.perf_counter()
            if tag == "fused_s":
                filtered, lst = minimap2_align.filter_consensus_alignments_and_split(path, fasta, logs, 0.995, fa, **kw)
            else:
                filtered = minimap2_align.filter_consensus_alignments(path, fasta, logs, 0.995, **kw)
                lst = region_split.filter_and_split_reads_by_region(filtered, fasta, logs, fa, **kw)
            if run:
                times[tag].append(time.perf_counter() - t0)
            res["region_files"] = len(lst)
            res["kept_records"] = sum(open(p).read().count(">") for p in lst)
            res["filtered_bam_bytes"] = os.path.getsize(filtered)
    for tag, v in times.items():
        res[tag + "_runs"] = [round(x, 4) for x in v]
        res[tag] = round(statistics.median(v), 4)
    if "--out" not in sys.argv:
        shutil.rmtree(out)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
