"""Measurement tool for DESIGN.md §9g: the wall time of umiclust_bam_write on two sessions -- the 200,000-record BAM
of tools/bam_scan_bench.py with the primary records kept, and the 100,000-record SAM session of
tools/sam_sort_bench.py with every record kept -- 5 writes each, the first as warm-up; where the library has it, the
split of umiclust_bam_write_info (upload, kernels, copy back by HIP events, the host's gather + CRC32) and the block
kinds; the written file's size, and with --refs the size of zlib level 1 over the same 0xff00-byte blocks.  Not a gate
and not part of bench.py.

    python tools/bgzf_write_bench.py --out DIR [--package DIR2] [--refs] [--small]

The inputs are built into DIR once and reused, so that a second run with --package DIR2 (the directory that holds
another commit's umiclust package) times the same files in the same visit.  --small: 20,000 and 10,000 records.
Prints one JSON line."""
import gzip
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = sys.argv[sys.argv.index("--package") + 1] if "--package" in sys.argv else os.path.join(ROOT, "ont-tcrconsensus_amd")
sys.path[:0] = [os.path.join(ROOT, "tools")]
import bam_scan_bench  # noqa: E402
import sam_sort_bench  # noqa: E402
sys.path[:0] = [PACKAGE]  # (after the two tools, which put their own first)


def level1_size(path):
    """zlib level 1 over the 0xff00-byte blocks of the stream that `path` inflates to, framed, EOF block included"""
    raw = gzip.decompress(open(path, "rb").read())
    total = 28
    for i in range(0, len(raw), 0xff00):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        total += 26 + len(c.compress(raw[i:i + 0xff00]) + c.flush())
    return len(raw), total


def time_writes(_lib, s, keep, path, res, key):
    import numpy as np
    L, h = _lib.lib(), s._ctx._h
    keep = np.ascontiguousarray(keep, np.uint8)
    walls, infos = [], []
    for _ in range(5):
        t1 = time.perf_counter()
        k = L.umiclust_bam_write(h, keep.ctypes.data_as(_lib.C.POINTER(_lib.C.c_uint8)), path.encode())
        walls.append(time.perf_counter() - t1)  # the C call alone: the first write is the warm-up
        assert k == int(keep.sum()), k
        if hasattr(s, "write_info"):
            infos.append(s.write_info())
    res[key + "_written"] = int(keep.sum())
    res[key + "_write_s_runs"] = walls
    res[key + "_write_s"] = statistics.median(walls[1:])
    res[key + "_write_s_spread"] = max(walls[1:]) - min(walls[1:])
    res[key + "_file_bytes"] = os.path.getsize(path)
    if infos:
        for f in ("upload_s", "kernel_s", "copy_back_s", "gather_crc_s"):
            res[key + "_" + f] = statistics.median(i[f] for i in infos[1:])
        res[key + "_info"] = {f: infos[-1][f] for f in ("blocks", "device_blocks", "stored", "fixed", "dynamic",
                                                         "host_blocks", "batches", "compressed_bytes")}
    if "--refs" in sys.argv:
        res[key + "_stream_bytes"], res[key + "_level1_bytes"] = level1_size(path)
        if infos and res[key + "_kernel_s"] > 0:
            res[key + "_kernel_bytes_per_s"] = res[key + "_stream_bytes"] / res[key + "_kernel_s"]
    os.remove(path)


def main():
    out = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(out, exist_ok=True)
    nb, ns = (20000, 10000) if "--small" in sys.argv else (200000, 100000)
    bam, sam = os.path.join(out, "synth_%d.bam" % nb), os.path.join(out, "synth_%d.sam" % ns)
    t0 = time.time()
    if not os.path.exists(bam):
        bam_scan_bench.build(nb, 20261019, bam)
    if not os.path.exists(sam):
        sam_sort_bench.build(ns, sam)
    res = {"package": PACKAGE, "bam_records": nb, "sam_records": ns, "build_s": round(time.time() - t0, 2),
           "env": {k: v for k, v in os.environ.items() if k.startswith("UMICLUST_BGZF")}}
    print(json.dumps(res), flush=True)
    import numpy as np
    from umiclust import _lib
    ctx = _lib.Context(0)
    with ctx.bam_open(bam) as s:
        time_writes(_lib, s, s.cls == 2, os.path.join(out, "w_%d_bam.bam" % os.getpid()), res, "bam")
    ctx._check(_lib.lib().umiclust_sam_open(ctx._h, sam.encode(), 64), "sam_open")
    with _lib.BamSession(ctx) as s:
        time_writes(_lib, s, np.ones(s.n, np.uint8), os.path.join(out, "w_%d_sam.bam" % os.getpid()), res, "sam")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
