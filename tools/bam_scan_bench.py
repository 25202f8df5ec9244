"""Measurement tool for DESIGN.md §9b and §9e (row f6): the device time of scan + group + verify (HIP events, through
umiclust_bam_times), the inflate time and the wall time of umiclust_bam_open on a seeded synthetic BAM, next to a
device-to-device copy of the same inflated bytes timed in the same process; where the library has it, the BGZF inflate
kernel alone (umiclust_bgzf_inflate, HIP events) and the session's inflate_info.  Not a gate and not part of bench.py.

    python tools/bam_scan_bench.py [records = 200000] [--out DIR]

The input: `records` draws (seed 20261019) from 8,000 template records shaped like raw-read alignments -- 1,500-base
reads, 7 CIGAR operations, 9 short aux tags and a cs:Z string of 40 to 600 bytes; a quarter of the draws come from 50
of the templates -- written as BGZF by tests/bam_ref.py.  Prints one JSON line; --no-gpu only builds the input."""
import json
import os
import random
import statistics
import struct
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ont-tcrconsensus_amd"), os.path.join(ROOT, "tests")]
import bam_ref  # noqa: E402


def build(n, seed, path):
    rng = random.Random(seed)
    refs = [["TRBV%d" % r, 1500] for r in range(100)]
    ops = [":%d" % k for k in range(3, 60)] + ["*ag", "*ct", "*ga", "+a", "-t", "+gg", "-ca"]
    templates = []
    for t in range(8000):  # 8000 distinct cs strings of 40..600 bytes; a quarter of the records share 50 of them
        cs = ""
        want = rng.randrange(40, 600)
        while len(cs) < want:
            cs += rng.choice(ops)
        cig = [["S", rng.randrange(0, 60)], ["M", 400], ["I", rng.randrange(1, 4)], ["M", 700], ["D", 2], ["M", 390], ["S", 20]]
        flag = rng.choice([0, 0, 0, 0, 0, 0, 16, 16, 4, 0x100, 0x800])
        r = {"name": "read%07d_%d" % (t, rng.randrange(1, 30)), "flag": flag, "ref": rng.randrange(100), "cigar": cig,
             "l_seq": 1500, "tags": [["NM", "i", rng.randrange(0, 40)], ["ms", "i", 2900], ["AS", "i", 2890], ["nn", "i", 0],
                                      ["tp", "A", "P"], ["cm", "i", 250], ["s1", "i", 1400], ["de", "f", 0.01],
                                      ["rl", "i", 0], ["cs", "Z", cs]]}
        templates.append(bam_ref.encode_record(r))
    common = templates[:50]
    parts = [bam_ref.build_raw(refs, [])]
    for _ in range(n):
        parts.append(rng.choice(common) if rng.random() < 0.25 else rng.choice(templates))
    raw = b"".join(parts)
    with open(path, "wb") as fh:
        for i in range(0, len(raw), 0xff00):
            d = raw[i:i + 0xff00]
            c = zlib.compressobj(1, zlib.DEFLATED, -15)
            comp = c.compress(d) + c.flush()
            fh.write(struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(comp) + 25) + comp +
                     struct.pack("<II", zlib.crc32(d) & 0xffffffff, len(d)))
        fh.write(bam_ref.EOF_BLOCK)
    return len(raw)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 200000
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else tempfile.mkdtemp()
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "synth_%d.bam" % n)
    t0 = time.time()
    nbytes = build(n, 20261019, path)
    res = {"records": n, "inflated_bytes": nbytes, "file_bytes": os.path.getsize(path), "build_s": round(time.time() - t0, 2)}
    print(json.dumps(res), flush=True)
    if "--no-gpu" in sys.argv:
        os.remove(path)
        return
    import torch
    from umiclust import _lib
    ctx = _lib.Context(0)
    runs = []
    opens = []
    for _ in range(5):
        t1 = time.perf_counter()
        ctx._check(_lib.lib().umiclust_bam_open(ctx._h, path.encode(), 64), "bam_open")
        opens.append(time.perf_counter() - t1)  # the C call alone: the first open is the warm-up
        with _lib.BamSession(ctx) as s:
            runs.append(dict(s.times))
            if hasattr(s, "inflate_info"):
                res["inflate_info"] = s.inflate_info()
            res["groups"], res["reruns"] = s.n_cs_groups, s.n_hash_reruns
            t1 = time.time()
            k = s.write((s.cls == 2).astype("uint8"), os.path.join(out, "synth_filtered.bam"))
            res["write_s"], res["written"] = round(time.time() - t1, 3), k
    os.remove(os.path.join(out, "synth_filtered.bam"))
    a = torch.empty(nbytes, dtype=torch.uint8, device="cuda").random_(0, 255)
    b = torch.empty_like(a)
    copies = []
    for _ in range(12):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        copies.append(e0.elapsed_time(e1) * 1e-3)
    if hasattr(ctx, "bgzf_inflate"):  # the kernel alone, on the same file
        data, k = open(path, "rb").read(), []
        for _ in range(5):
            ctx.bgzf_inflate(data)
            k.append(dict(ctx.bgzf_times))
        res["bgzf_kernel_s_runs"] = [r["kernel_s"] for r in k]
        res["bgzf_kernel_s"] = statistics.median(r["kernel_s"] for r in k[1:])
        res["bgzf_h2d_s"] = statistics.median(r["h2d_s"] for r in k[1:])
        res["bgzf_d2h_s"] = statistics.median(r["d2h_s"] for r in k[1:])
    os.remove(path)
    warm = runs[1:]
    res["open_s_runs"] = opens
    res["open_s"] = statistics.median(opens[1:])
    res["open_s_spread"] = max(opens[1:]) - min(opens[1:])
    res["inflate_s_runs"] = [r["inflate_s"] for r in runs]
    res["device_s_runs"] = [r["device_s"] for r in runs]
    res["device_s"] = statistics.median(r["device_s"] for r in warm)
    res["inflate_s"] = statistics.median(r["inflate_s"] for r in warm)
    res["h2d_s"] = statistics.median(r["h2d_s"] for r in warm)
    res["d2d_copy_s_runs"] = copies
    res["d2d_copy_s"] = statistics.median(copies[2:])
    res["ratio_device_over_copy"] = res["device_s"] / res["d2d_copy_s"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
