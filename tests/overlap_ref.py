"""Plain reference of the region-vs-region UMI overlap join (row f3; test infrastructure, no GPU, no numpy).

join() restates the operation of umiclust_overlap_regions on the flat sequence list and region_start with dicts:
byte-equal sequences form a class, and for regions a < b
    total[a, b]    = sum over classes of c_a * c_b        (c_r = the class's sequences in region r)
    maxcount[a, b] = max over classes with c_a > 0 of c_b
both kept sparse (absent = 0).  counts() is the two-set form (umiclust_overlap_counts).

hash64() restates the kernel's 64-bit hash (k_ov_hash of csrc/overlap.hip): the seed xor the length times the
golden-ratio constant, FNV-1a over the bytes, the two-multiply mixer, and all-ones (the table's empty key) remapped to
all-ones minus one.  With it the probe's hash[] is compared exactly and cases are built for chosen home slots
(tests/overlap_cases.py); a change of the kernel's hash shows up as that comparison failing, not as a case that
silently stops reaching its path.
"""
from __future__ import annotations

M64 = (1 << 64) - 1
SEEDS = (0x243f6a8885a308d3, 0x13198a2e03707344, 0xa4093822299f31d0, 0x082efa98ec4e6c89)  # tried in this order
SMALL_BUCKET = 32   # buckets of more members go to the workgroup kernel (kOvSmallBucket)
SCAN_BLOCK = 1024   # slot counts per scan block (kOvScan)
SCAN_CHUNK = 256    # block sums scanned at a time by k_ov_scan_top


def hash64(seq: bytes, seed: int = SEEDS[0]) -> int:
    h = seed ^ ((len(seq) * 0x9e3779b97f4a7c15) & M64)
    for b in seq:
        h = ((h ^ b) * 0x100000001b3) & M64
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & M64
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & M64
    h ^= h >> 33
    return h - 1 if h == M64 else h


def table_slots(n: int) -> int:
    """m: the smallest power of two that is >= 1024 and >= 2 n"""
    m = 1024
    while m < 2 * n:
        m *= 2
    return m


def scan_blocks(n: int) -> int:
    """nb: the block sums k_ov_scan_top scans, 256 at a time"""
    return table_slots(n) // SCAN_BLOCK


def join(seqs, region_start) -> dict:
    """seqs: the flat list (bytes); region r = seqs[region_start[r]:region_start[r + 1]]"""
    nreg = len(region_start) - 1
    assert region_start[0] == 0 and region_start[nreg] == len(seqs)
    region = [None] * len(seqs)
    for r in range(nreg):
        for i in range(region_start[r], region_start[r + 1]):
            region[i] = r
    classes = {}
    for i, s in enumerate(seqs):
        classes.setdefault(s, []).append(i)
    rep = [classes[s][0] for s in seqs]
    size = [len(classes[s]) for s in seqs]
    total, maxcount = {}, {}
    for idx in classes.values():
        per = {}
        for i in idx:
            per[region[i]] = per.get(region[i], 0) + 1
        held = sorted(per)
        for x, a in enumerate(held):
            for b in held[x + 1:]:
                total[a, b] = total.get((a, b), 0) + per[a] * per[b]
                maxcount[a, b] = max(maxcount.get((a, b), 0), per[b])
    return dict(region=region, classes=classes, rep=rep, size=size, total=total, maxcount=maxcount)


def counts(set1, set2) -> list:
    """per set-1 sequence, the number of byte-equal set-2 sequences"""
    c2 = {}
    for s in set2:
        c2[s] = c2.get(s, 0) + 1
    return [c2.get(s, 0) for s in set1]
