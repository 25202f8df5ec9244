"""LDS bank load of k_fastq_ee's table reads for ONT-like qualities (measurement aid, not product code).

The 256-entry u64 table is read with ds_read_b64: entry b lies on banks 2b and 2b + 1 (mod 64), so entries b and b + 32
share a bank pair; lanes conflict within a 32-lane group, equal addresses broadcast.  Lane l of a wave holds the 16-byte
slot l of a read and instruction j looks up byte j of every lane's slot, so a group's 32 bytes are every 16th base of
one read.  Qualities as tests/fastq_filter_ref.synth_reads: per-read mean uniform in Q8-Q25, Gaussian spread 5.
An access costs the largest number of distinct entries on one bank pair.

    python tools/fastq_bank_sim.py [reads]
"""
import json
import sys

import numpy as np


def main():
    reads = int(sys.argv[1]) if len(sys.argv) > 1 else 400
    rng = np.random.default_rng(3)
    hist = {}
    for _ in range(reads):
        q = np.clip(np.rint(rng.normal(rng.uniform(8, 25), 5.0, 1536)), 0, 60).astype(int) + 33
        slots = q.reshape(-1, 16)[:64]  # the read's first wave load: lane l holds slot l
        for half in (0, 32):
            for j in range(16):
                c = int(np.bincount(np.unique(slots[half:half + 32, j]) % 32, minlength=32).max())
                hist[c] = hist.get(c, 0) + 1
    n = sum(hist.values())
    print(json.dumps(dict(group_accesses=n, mean_cycles=sum(k * v for k, v in hist.items()) / n,
                          share_by_cycles={k: v / n for k, v in sorted(hist.items())})))


if __name__ == "__main__":
    main()
