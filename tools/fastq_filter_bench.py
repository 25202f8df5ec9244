"""Throughput of the fastq_filter drop-in (row f5) on a synthetic library FASTQ (measurement aid).

Writes a 4-line FASTQ of about --gb GB to --dir (default /dev/shm): reads of --len bases (1,500), 16-character labels,
per-read mean quality uniform in Q8-Q25 with Gaussian spread 5 (as tests/fastq_filter_ref.synth_reads); one block of
32,768 seeded records is repeated under distinct labels.  Runs the reference's argv
(preprocessing.fastq_filter_argv, max_ee_rate_base 0.07, minimal_length 1470) through the library once to warm up and
--runs (3) times, and writes one JSON file (--out, default profiles/fastq_filter/bench.json): the input size, per run
the wall time, input GB/s and the result struct (counters and phase times), and whether the kernel's summed HIP-event
time stayed below the summed host-to-device copy time of the same chunks.  If a `vsearch` binary is on PATH the same
argv is timed with it once; otherwise the JSON says it is absent.  Needs a GPU: there is no CPU fallback.

With --stats (row f5b) the same process then runs the same argv on the same file through
umiclust_fastq_filter_stats_argv, which also writes the two `seqkit stat -a` tables: the JSON (default
profiles/fastq_filter/bench_stats.json) holds the plain runs as above and, under "stats", the runs with the tables,
their phase sums, the added host-to-device time, and whether k_fastq_stats's summed HIP-event time stayed below the
summed host-to-device copy time of the same chunks.  seqkit, like vsearch, is only timed if a binary is on PATH.

    python tools/fastq_filter_bench.py [--gb 2.0] [--runs 3] [--stats] [--out FILE]
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ont-tcrconsensus_amd"))
from umiclust import _lib, preprocessing  # noqa: E402

BLOCK = 32768


def write_input(path: str, gb: float, length: int, seed: int) -> tuple[int, int]:
    rng = np.random.default_rng(seed)
    rec = 1 + 16 + 1 + length + 3 + length + 1
    a = np.empty((BLOCK, rec), np.uint8)
    a[:, 0] = ord("@")
    label = np.array([list(b"r%02d_%012d" % (0, i)) for i in range(BLOCK)], np.uint8)
    a[:, 1:17] = label
    a[:, 17] = 10
    a[:, 18:18 + length] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (BLOCK, length))]
    a[:, 18 + length:21 + length] = np.frombuffer(b"\n+\n", np.uint8)
    mean = rng.uniform(8, 25, (BLOCK, 1))
    q = np.clip(np.rint(rng.normal(0.0, 5.0, (BLOCK, length)) + mean), 0, 60).astype(np.uint8) + 33
    a[:, 21 + length:21 + 2 * length] = q
    a[:, rec - 1] = 10
    reps = max(1, int(round(gb * 1e9 / a.size)))
    with open(path, "wb") as fh:
        for r in range(reps):
            a[:, 2] = ord("0") + r // 10 % 10  # distinct labels per repetition
            a[:, 3] = ord("0") + r % 10
            fh.write(a.tobytes())
    return reps * BLOCK, reps * a.size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=2.0)
    ap.add_argument("--len", type=int, default=1500)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--out", default=None)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--stats", action="store_true", help="also time the pass that writes the seqkit tables")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "fastq_filter", "bench_stats.json" if args.stats else "bench.json")
    work = os.path.join(args.dir, f"umiclust_fq_bench_{os.getpid()}")
    os.makedirs(work, exist_ok=True)
    try:
        src = os.path.join(work, "library.fastq")
        t0 = time.time()
        n, size = write_input(src, args.gb, args.len, args.seed)
        print(f"wrote {n} reads, {size / 1e9:.2f} GB in {time.time() - t0:.1f} s", flush=True)
        argv = preprocessing.fastq_filter_argv(src, os.path.join(work, "filtered.fastq"), os.path.join(work, "f.log"),
                                               0.07, 1470)
        out = dict(input_bytes=size, reads=n, read_length=args.len, argv=argv[3:-1], runs=[],
                   io_threads=os.environ.get("UMICLUST_IO_THREADS"), fq_chunk=os.environ.get("UMICLUST_FQ_CHUNK"))
        with _lib.Context(0) as ctx:
            for i in range(args.runs + 1):
                t0 = time.perf_counter()
                r = ctx.fastq_filter_argv(argv)
                dt = time.perf_counter() - t0
                print(f"run {i}{' (warm-up)' if i == 0 else ''}: {dt:.3f} s, {size / dt / 1e9:.2f} GB/s, kernel "
                      f"{r['t_kernel_s'] * 1e3:.2f} ms, h2d {r['t_h2d_s'] * 1e3:.2f} ms", flush=True)
                if i > 0:
                    out["runs"].append(dict(wall_s=dt, input_gb_per_s=size / dt / 1e9, result=r))
            if args.stats:
                txt = [os.path.join(work, "stats_before.txt"), os.path.join(work, "stats_after.txt")]
                st = out["stats"] = dict(runs=[])
                for i in range(args.runs + 1):
                    t0 = time.perf_counter()
                    r = ctx.fastq_filter_stats_argv(argv, *txt)
                    dt = time.perf_counter() - t0
                    print(f"stats run {i}{' (warm-up)' if i == 0 else ''}: {dt:.3f} s, {size / dt / 1e9:.2f} GB/s, "
                          f"kernel {r['t_kernel_s'] * 1e3:.2f} ms, h2d {r['t_h2d_s'] * 1e3:.2f} ms", flush=True)
                    if i > 0:
                        r["before"]["ee_fx"] = str(r["before"]["ee_fx"])  # beyond a JSON reader's integers
                        r["after"]["ee_fx"] = str(r["after"]["ee_fx"])
                        st["runs"].append(dict(wall_s=dt, input_gb_per_s=size / dt / 1e9, result=r))
                st["tables"] = [open(t).read() for t in txt]
        out["input_gb_per_s_median"] = float(np.median([x["input_gb_per_s"] for x in out["runs"]]))
        k = sum(x["result"]["t_kernel_s"] for x in out["runs"])
        h = sum(x["result"]["t_h2d_s"] for x in out["runs"])
        out.update(kernel_s_sum=k, h2d_s_sum=h, kernel_below_h2d=bool(k < h),
                   kernel_qual_gb_per_s=sum(x["result"]["bases_in"] for x in out["runs"]) / k / 1e9,
                   h2d_gb_per_s=sum(x["result"]["bases_in"] for x in out["runs"]) / h / 1e9)
        if args.stats:
            st = out["stats"]
            sk = sum(x["result"]["t_kernel_s"] for x in st["runs"])
            sh = sum(x["result"]["t_h2d_s"] for x in st["runs"])
            phases = ("t_read_s", "t_h2d_s", "t_kernel_s", "t_write_s")
            st.update(input_gb_per_s_median=float(np.median([x["input_gb_per_s"] for x in st["runs"]])),
                      wall_s_median=float(np.median([x["wall_s"] for x in st["runs"]])),
                      kernel_s_sum=sk, h2d_s_sum=sh, kernel_below_h2d=bool(sk < sh), h2d_s_added=sh - h,
                      phase_s_per_run={k: sum(x["result"][k] for x in st["runs"]) / len(st["runs"]) for k in phases})
            out["wall_s_median"] = float(np.median([x["wall_s"] for x in out["runs"]]))
            out["phase_s_per_run"] = {k: sum(x["result"][k] for x in out["runs"]) / len(out["runs"]) for k in phases}
            out["seqkit"] = shutil.which("seqkit")
            if out["seqkit"]:
                t0 = time.perf_counter()
                rc = subprocess.run([out["seqkit"], "stat", "-a", src], stdout=subprocess.DEVNULL).returncode
                out["seqkit_run"] = dict(returncode=rc, wall_s=time.perf_counter() - t0)
            else:
                print("no seqkit binary on PATH: the reference's two passes are not measured")
        vs = shutil.which("vsearch")
        out["vsearch"] = vs
        if vs:
            vargv = list(argv)
            vargv[-1] = os.path.join(work, "filtered_vsearch.fastq")
            t0 = time.perf_counter()
            rc = subprocess.run(vargv).returncode
            dt = time.perf_counter() - t0
            out["vsearch_run"] = dict(returncode=rc, wall_s=dt, input_gb_per_s=size / dt / 1e9)
        else:
            print("no vsearch binary on PATH: the reference's rate is not measured")
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
        brief = {k: v for k, v in out.items() if k != "runs"}
        if args.stats:
            brief["stats"] = {k: v for k, v in out["stats"].items() if k != "runs"}
        print(json.dumps(brief))
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
