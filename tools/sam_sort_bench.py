"""Measurement tool for DESIGN.md §9f: the wall time of umiclust_sam_open on seeded synthetic SAM text and the five
HIP-event times of umiclust_sam_info (upload, lines + measure, sort, encode, copy back), next to umiclust_bam_open of
the equal BAM -- the file umiclust_bam_write leaves with every record of that session kept.  Not a gate and not part of
bench.py.

    python tools/sam_sort_bench.py [records = 100000] [--out DIR] [--keep] [--bam-only FILE] [--package DIR]

The input is the record mix of tools/bam_scan_bench.py rendered as SAM (seed 20261020): `records` draws from 8,000
template alignments -- 1,500-base reads with qualities, 7 CIGAR operations, 9 short aux tags (one of type f) and a cs:Z
string of 40 to 600 bytes, on 100 references at 200 positions, both strands, some unmapped, secondary or supplementary
-- in random order, so the sort has all of its work.  5 opens, the first as warm-up.  Prints one JSON line.
--keep leaves the SAM and the BAM in DIR.  --bam-only FILE times umiclust_bam_open of FILE alone (5 opens), and
--package DIR imports the umiclust package from DIR: together the way to time the same file on another commit's build."""
import json
import os
import random
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --package DIR: the directory that holds the umiclust package to import (another commit's build)
sys.path[:0] = [sys.argv[sys.argv.index("--package") + 1] if "--package" in sys.argv
                else os.path.join(ROOT, "ont-tcrconsensus_amd")]

SEED = 20261020


def build(n, path):
    rng = random.Random(SEED)
    refs = [("TRBV%d" % r, 1500) for r in range(100)]
    ops = [":%d" % k for k in range(3, 60)] + ["*ag", "*ct", "*ga", "+a", "-t", "+gg", "-ca"]
    templates = []
    for t in range(8000):
        cs = ""
        want = rng.randrange(40, 600)
        while len(cs) < want:
            cs += rng.choice(ops)
        cigar = "%dS400M%dI700M2D390M20S" % (rng.randrange(1, 60), rng.randrange(1, 4))
        flag = rng.choice([0, 0, 0, 0, 0, 0, 16, 16, 4, 0x100, 0x800])
        seq = "".join(rng.choices("ACGT", k=1500))
        qual = "".join(rng.choices("+5?IS", k=1500))
        aux = ["NM:i:%d" % rng.randrange(0, 40), "ms:i:2900", "AS:i:2890", "nn:i:0", "tp:A:P", "cm:i:250", "s1:i:1400",
               "de:f:0.0%d" % rng.randrange(10, 99), "rl:i:0", "cs:Z:" + cs]
        templates.append(("read%07d_%d" % (t, rng.randrange(1, 30)), flag, refs[rng.randrange(100)][0], cigar, seq, qual,
                          "\t".join(aux)))
    common = templates[:50]
    with open(path, "w") as fh:
        fh.write("@HD\tVN:1.6\tSO:unsorted\tGO:query\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
                 + "@PG\tID:minimap2\tPN:minimap2\n")
        for _ in range(n):
            name, flag, ref, cigar, seq, qual, aux = rng.choice(common) if rng.random() < 0.25 else rng.choice(templates)
            fh.write("\t".join([name, str(flag), ref, str(rng.randrange(1, 201)), "60", cigar, "*", "0", "0", seq, qual,
                                aux]) + "\n")
    return os.path.getsize(path)


def time_bam_open(ctx, _lib, path):
    opens, runs = [], []
    for _ in range(5):
        t1 = time.perf_counter()
        ctx._check(_lib.lib().umiclust_bam_open(ctx._h, os.fspath(path).encode(), 64), "bam_open")
        opens.append(time.perf_counter() - t1)
        with _lib.BamSession(ctx) as s:
            runs.append(dict(s.times))
            n = s.n
    return {"bam_records": n, "bam_file_bytes": os.path.getsize(path), "bam_open_s_runs": opens,
            "bam_open_s": statistics.median(opens[1:]), "bam_open_s_spread": max(opens[1:]) - min(opens[1:]),
            "bam_inflate_s": statistics.median(r["inflate_s"] for r in runs[1:]),
            "bam_device_s": statistics.median(r["device_s"] for r in runs[1:])}


def main():
    from umiclust import _lib
    if "--bam-only" in sys.argv:
        print(json.dumps(time_bam_open(_lib.Context(0), _lib, sys.argv[sys.argv.index("--bam-only") + 1])))
        return
    n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 100000
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else tempfile.mkdtemp()
    os.makedirs(out, exist_ok=True)
    sam, bam = os.path.join(out, "synth_%d.sam" % n), os.path.join(out, "synth_%d.bam" % n)
    t0 = time.time()
    res = {"records": n, "text_bytes": build(n, sam), "build_s": round(time.time() - t0, 2)}
    print(json.dumps(res), flush=True)
    import numpy as np
    ctx = _lib.Context(0)
    opens, infos = [], []
    for k in range(5):
        t1 = time.perf_counter()
        ctx._check(_lib.lib().umiclust_sam_open(ctx._h, sam.encode(), 64), "sam_open")
        opens.append(time.perf_counter() - t1)  # the C call alone: the first open is the warm-up
        with _lib.BamSession(ctx) as s:
            infos.append(dict(s.sam_info(), scan_s=s.times["device_s"]))
            if k == 4:
                t1 = time.perf_counter()
                res["written"] = s.write(np.ones(s.n, np.uint8), bam)
                res["write_s"] = round(time.perf_counter() - t1, 3)
    res["sam_open_s_runs"] = opens
    res["sam_open_s"] = statistics.median(opens[1:])
    res["sam_open_s_spread"] = max(opens[1:]) - min(opens[1:])
    for key in ("upload_s", "measure_s", "sort_s", "encode_s", "copy_back_s", "scan_s"):
        warm = [i[key] for i in infos[1:]]
        res[key] = statistics.median(warm)
        res[key + "_spread"] = max(warm) - min(warm)
    res["f_values"], res["lines"] = infos[0]["f_values"], infos[0]["lines"]
    res.update(time_bam_open(ctx, _lib, bam))
    if "--keep" not in sys.argv:
        os.remove(sam), os.remove(bam)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
