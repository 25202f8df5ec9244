"""Measurement tool for DESIGN.md §9h: the .bai index and flagstat of a session on the device, on the seeded synthetic
SAM text of tools/sam_sort_bench.py.  Not a gate and not part of bench.py.

    python tools/bam_index_bench.py [records = 50000] [--out DIR] [--bai-check PROGRAM]

The session is opened from the text (umiclust_sam_open), then, 5 times each with the first as warm-up:
  - umiclust_bam_write, and umiclust_bam_write_index to the same place: the difference is what the index costs a
    pipeline that writes the BAM anyway; umiclust_bam_index_info gives the HIP-event seconds of the upload, the kernels
    and the copies back, and the host's finish with the file;
  - umiclust_bam_flagstat;
  - umiclust_bam_index_file on the written BAM (`samtools index`: the file inflated on the device first);
  - the host restatement over the written file -- tools/bai_check_main.cpp built without sanitizers (`make bai_check
    BAI_SAN=`, or --bai-check PROGRAM), which inflates with zlib and runs bai::build_host on one thread: the only path
    to the same two files without this feature, standing in for `samtools index`, which is absent.
The device's .bai and the host's are compared byte for byte.  Prints one JSON line."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ont-tcrconsensus_amd"), os.path.join(ROOT, "tools")]


def med(xs):
    return statistics.median(xs[1:])


def main():
    import numpy as np
    import sam_sort_bench
    from umiclust import _lib
    n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 50000
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else tempfile.mkdtemp()
    os.makedirs(out, exist_ok=True)
    if "--bai-check" in sys.argv:
        bai_check = sys.argv[sys.argv.index("--bai-check") + 1]
    else:
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ont-tcrconsensus_amd"), "bai_check", "BAI_SAN=",
                        f"SAN_OUT={out}"], check=True)
        bai_check = os.path.join(out, "bai_check")
    sam, bam = os.path.join(out, "in.sam"), os.path.join(out, "sorted.bam")
    res = {"records": n, "sam_bytes": sam_sort_bench.build(n, sam)}
    t_write, t_both, t_flag, t_file, t_host, infos = [], [], [], [], [], []
    with _lib.Context(0) as ctx:
        with ctx.sam_open(sam) as s:
            keep = np.ones(s.n, np.uint8)
            for _ in range(5):
                t0 = time.perf_counter()
                s.write(keep, bam)
                t_write.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                s.write(keep, bam, index=True)
                t_both.append(time.perf_counter() - t0)
                infos.append(s.index_info())
                t0 = time.perf_counter()
                _, text = s.flagstat()
                t_flag.append(time.perf_counter() - t0)
            flag_info = s.index_info()
        device_bai = open(bam + ".bai", "rb").read()
        for _ in range(5):
            t0 = time.perf_counter()
            ctx.bam_index_file(bam, os.path.join(out, "file.bai"))
            t_file.append(time.perf_counter() - t0)
        file_info = ctx.bam_index_info()
    for _ in range(5):
        t0 = time.perf_counter()
        r = subprocess.run([bai_check, "file", bam, os.path.join(out, "host.bai"), os.path.join(out, "host.flagstat")],
                           capture_output=True, text=True, check=True)
        t_host.append(time.perf_counter() - t0)
    assert r.stdout.startswith("ok"), r.stdout
    res.update(bam_bytes=os.path.getsize(bam), bai_bytes=len(device_bai),
               bai_equal_host=device_bai == open(os.path.join(out, "host.bai"), "rb").read(),
               bai_equal_index_file=device_bai == open(os.path.join(out, "file.bai"), "rb").read(),
               flagstat_equal_host=text == open(os.path.join(out, "host.flagstat")).read(),
               write_s=med(t_write), write_index_s=med(t_both), index_added_s=med(t_both) - med(t_write),
               flagstat_s=med(t_flag), index_file_s=med(t_file), host_restatement_s=med(t_host),
               write_index_runs=t_both, host_runs=t_host)
    for k in ("kept", "runs", "chunks", "windows"):
        res[k] = infos[-1][k]
    for k in ("upload_s", "kernel_s", "copy_back_s", "finish_s"):
        res["index_" + k] = statistics.median(i[k] for i in infos[1:])
        res["index_file_" + k] = file_info[k]
        res["flagstat_" + k] = flag_info[k]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
