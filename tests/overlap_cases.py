"""The smallest inputs at which the region overlap join (csrc/overlap.hip, row f3) can go wrong (test infrastructure,
no GPU).

Each case is a list of regions (lists of byte strings) with the path it was built for; tests/test_overlap_ref_cpu.py
asserts by the case's name that it still reaches that path, tests/test_gpu_overlap_kernels.py runs every case through
umiclust_overlap_probe and compares every array.  Nothing here is a recorded answer: the sequences that need chosen
home slots or chosen 8-bit hashes are found with the restated hash (overlap_ref.hash64) by a seeded search when this
module is imported (about a tenth of a second).

Where the kernels take another path, and the case that stands there:
  k_ov_hash        the binary search over region_start: one region, empty regions first, last and three in a row,
                   region boundaries at sequence 255 / 256 / 257 (the thread-block seam); sequences of length 0, 1, 4000
  k_ov_insert      linear probing past the table's end (probe_wrap), 8-bit hashes (collide_*)
  k_ov_verify      byte comparison: a last byte, a prefix, bytes >= 0x80, letter case
  k_ov_scan_*      nb = 1, 2 and 512 block sums (scan_n1, scan_n513, scan_n131073: two chunks of k_ov_scan_top)
  k_ov_pairs       buckets of 1, 2, 31, 32 members, in several regions and in one (the early return)
  k_ov_pairs_big   buckets of 33, 64, 257 members; 1, 255, 256, 257 non-empty regions; regions up to 4095
"""
from __future__ import annotations

import random
from dataclasses import dataclass
from functools import cached_property

import overlap_ref as R

BUCKET_SIZES = (1, 2, 31, 32, 33, 64, 257)
SEAM_REGIONS = 320   # regions of the compaction cases
CAP_REGIONS = 4096   # UMICLUST_OVERLAP_MAX_REGIONS
CAP_MUST_HOLD = (0, 255, 256, 4094, 4095)
WRAP_HOMES = (1022, 1023)


@dataclass(frozen=True)
class Case:
    name: str
    regions: tuple       # of tuples of bytes
    pins: str
    hash_bits: int = 64  # of the first table pass
    passes: int = 1      # table passes expected

    @cached_property
    def flat(self):
        return [s for r in self.regions for s in r]

    @cached_property
    def region_start(self):
        rs = [0]
        for r in self.regions:
            rs.append(rs[-1] + len(r))
        return rs


def _case(name, regions, pins, **kw):
    return Case(name, tuple(tuple(s if isinstance(s, bytes) else s.encode() for s in r) for r in regions), pins, **kw)


def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n)).encode()


def _distinct(rng, k, n=20):
    out = set()
    while len(out) < k:
        out.add(_rand(rng, n))
    return sorted(out)


def _region_cases():
    rng = random.Random(101)
    pool = _distinct(rng, 12)
    pick = lambda k: [rng.choice(pool) for _ in range(k)]  # noqa: E731
    seam = [rng.choice(pool) for _ in range(257)]
    return [
        _case("regions_one", [pick(40)], "nregions = 1: the binary search has nothing to halve, no pair exists"),
        _case("regions_n0", [[], [], []], "n = 0 in 3 regions: no kernel runs, every output is zero"),
        _case("regions_empty_edges", [[], [], pick(9), pick(7), [], [], [], pick(8), pick(5), [], []],
              "two leading, two trailing and three consecutive middle empty regions"),
        _case("regions_one_nonempty", [[], [], [], [], pick(30), [], [], [], []],
              "every region empty but one"),
        _case("regions_block_seam", [seam[:255], seam[255:256], seam[256:257], []],
              "n = 257 with region boundaries at 255, 256 and 257: the second thread block of k_ov_hash holds one "
              "sequence, the regions change at the block's last and first thread"),
    ]


def _sequence_cases():
    rng = random.Random(102)
    a, b, c = _distinct(rng, 3, 24)
    long_ = _rand(rng, 4000)
    hi = bytes(rng.randrange(0x80, 0x100) for _ in range(16))
    return [
        _case("seq_empty_strings", [[a, b"", b], [c, a], [b"", b, b""]],
              "empty strings in two regions beside non-empty ones: a class like any other, no byte is read"),
        _case("seq_length_1", [[b"A", b"C", b"A"], [b"G", b"A"], [b"C", b"T", b"C"]], "sequences of one byte"),
        _case("seq_last_byte", [[a[:-1] + b"A", a[:-1] + b"C", b], [a[:-1] + b"C", a[:-1] + b"G"], [a[:-1] + b"A"]],
              "sequences that differ only in the last byte"),
        _case("seq_prefix", [[a, a[:-1], a[:1]], [a + b"A", a[:-1]], [a[:1], a, b""]],
              "sequences that are prefixes of one another, down to the empty one"),
        _case("seq_high_bytes", [[hi, hi[:-1] + bytes([hi[-1] ^ 0x80]), b"\xff" * 8], [b"\xff" * 8, hi, b"\x80"],
                                 [b"\x80", b"\x00", hi]],
              "bytes >= 0x80 (the hash reads them unsigned) and a zero byte"),
        _case("seq_letter_case", [[a, a.lower()], [a.lower(), b], [b.lower(), a]],
              "lower and upper case of the same letters are different sequences"),
        _case("seq_long_4000", [[long_, a], [long_[:-1] + b"N", b], [long_]],
              "a 4,000-byte sequence twice, and once with another last byte"),
    ]


def _bucket_regions(sizes, nreg, spread, seed):
    """distinct UMIs with exactly `sizes` copies: dealt over the regions, or all copies of one UMI in one region"""
    rng = random.Random(seed)
    umis = _distinct(rng, len(sizes))
    regions = [[] for _ in range(nreg)]
    for k, (u, c) in enumerate(zip(umis, sizes)):
        for x in range(c):
            regions[(k + x) % nreg if spread else k % nreg].append(u)
    for r in regions:
        rng.shuffle(r)
    return regions


def _bucket_cases():
    return [
        _case("bucket_sizes_spread", _bucket_regions(BUCKET_SIZES, 5, True, 103),
              "UMIs with exactly 1, 2, 31, 32, 33, 64 and 257 copies over 5 regions: 32 stays with k_ov_pairs, 33 is "
              "the first bucket handed to k_ov_pairs_big"),
        _case("bucket_sizes_one_region", _bucket_regions(BUCKET_SIZES, 3, False, 104),
              "the same sizes with all copies of a UMI in one region: the early return of k_ov_pairs, one non-empty "
              "region (no pair) in k_ov_pairs_big"),
    ]


def _seam_case(k):
    """one UMI in exactly k of 320 regions, 1..3 times each; small UMIs beside it"""
    rng = random.Random(200 + k)
    art, *small = _distinct(rng, 9)
    held = sorted(rng.sample(range(SEAM_REGIONS), k))
    regions = [[] for _ in range(SEAM_REGIONS)]
    for x, r in enumerate(held):
        regions[r] += [art] * (1 + (x * 7 + r) % 3)
    for u in small:
        for r in rng.sample(range(SEAM_REGIONS), 3):
            regions[r].append(u)
    for r in regions:
        rng.shuffle(r)
    return _case(f"compact_{k}", regions,
                 f"one UMI in exactly {k} of {SEAM_REGIONS} regions, 1..3 times each: the compaction of k_ov_pairs_big "
                 "across its chunks of 256 regions")


def _cap_case():
    rng = random.Random(105)
    art, edge, *pool = _distinct(rng, 2002)
    regions = [[] for _ in range(CAP_REGIONS)]
    held = sorted(set(CAP_MUST_HOLD) | set(rng.sample(range(CAP_REGIONS), 40)))
    for x, r in enumerate(held):
        regions[r] += [art] * (1 + x % 3)
    regions[17].append(edge)
    regions[CAP_REGIONS - 1] += [edge, edge]
    regions[CAP_REGIONS - 1].append(pool[0])
    regions[CAP_REGIONS - 2].append(pool[0])
    for _ in range(4900):
        regions[rng.randrange(CAP_REGIONS)].append(rng.choice(pool))
    for r in regions:
        rng.shuffle(r)
    return _case("region_cap_4096", regions,
                 "4,096 regions (the cap of one join, the size of the LDS arrays of k_ov_pairs_big): one UMI in more "
                 "than 32 regions that include 0, 255, 256, 4094 and 4095, small buckets that touch region 4095")


def _count_cases():
    rng = random.Random(106)
    x, y, z = _distinct(rng, 3)
    shared = _distinct(rng, 500)
    r0 = shared + shared[:50]
    r1 = shared + shared[450:]
    rng.shuffle(r0)
    rng.shuffle(r1)
    return [
        _case("count_3000_by_2000", [[x] * 3000, [y, z], [x] * 2000],
              "one UMI 3,000 times in one region and 2,000 times in another: total 6,000,000, maxcount 2,000"),
        _case("count_contended_cell", [r0, r1],
              "500 distinct UMIs shared by the same two regions: 500 atomic adds and maxima on one cell"),
        _case("count_asymmetric", [[x] * 5, [x], [y], [y] * 5],
              "c_a = 5 against c_b = 1 and its mirror: maxcount is the larger region's count only from its side"),
    ]


def _scan_cases():
    rng = random.Random(107)
    pool = _distinct(rng, 200)
    n513 = [rng.choice(pool) for _ in range(513)]
    big = [str(i % 40000).encode() for i in range(131073)]
    cuts = [0, 18000, 36001, 54003, 72000, 90500, 110000, 131073]
    return [
        _case("scan_n1", [[], [pool[0]], []], "n = 1: m = 1,024 slots, one scan block"),
        _case("scan_n513", [n513[:200], n513[200:400], n513[400:]], "n = 513: m = 2,048 slots, two scan blocks"),
        _case("scan_n131073", [big[a:b] for a, b in zip(cuts, cuts[1:])],
              "n = 131,073 short decimal strings in 7 regions: m = 524,288 slots, 512 block sums, the second chunk of "
              "k_ov_scan_top and its carry"),
    ]


def _wrap_case():
    """distinct 20-mers homed (hash & 1023 under the first seed) at the table's last two slots and at its first 16"""
    rng = random.Random(108)
    last, first = [], []
    for s in _distinct(rng, 9000):
        home = R.hash64(s) & 1023
        if home in WRAP_HOMES:
            last.append(s)
        elif home < 16 and len(first) < 60:
            first.append(s)
    assert len(last) >= 10, len(last)
    seqs = last + first + last[:6] + first[:10]
    rng.shuffle(seqs)
    k = len(seqs) // 3
    return _case("probe_wrap", [seqs[:k], seqs[k:2 * k], seqs[2 * k:]],
                 "n <= 512 (m = 1,024): at least 10 distinct sequences homed at slots 1022 and 1023, whose probes wrap "
                 "to slot 0, where sequences homed at 0..15 already sit")


def _collision_cases():
    rng = random.Random(109)
    many = _distinct(rng, 320)
    seqs = many + [rng.choice(many) for _ in range(200)]
    rng.shuffle(seqs)
    regions = [seqs[:150], seqs[150:330], [], seqs[330:]]
    few, seen = [], set()
    for s in _distinct(rng, 40):
        if R.hash64(s) & 0xff not in seen and len(few) < 5:
            seen.add(R.hash64(s) & 0xff)
            few.append(s)
    return [
        _case("collide_8bit", regions, "more than 256 distinct sequences under 8-bit hashes: the first pass collides, "
              "the second seed with all 64 bits is exact", hash_bits=8, passes=2),
        _case("collide_64bit", regions, "the same input with all 64 bits: one pass, the same outputs"),
        _case("collide_8bit_distinct", [few + few[:2], few[1:4], few[3:] + few[:1]],
              "5 distinct sequences whose 8-bit hashes differ: the masked first pass is accepted", hash_bits=8),
    ]


CASES = (_region_cases() + _sequence_cases() + _bucket_cases() + [_seam_case(k) for k in (255, 256, 257)] +
         [_cap_case()] + _count_cases() + _scan_cases() + [_wrap_case()] + _collision_cases())
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
_REF = {}


def ref(case) -> dict:
    """overlap_ref.join of one case, computed once and shared by the tests (never modified)"""
    if case.name not in _REF:
        _REF[case.name] = R.join(case.flat, case.region_start)
    return _REF[case.name]


def _two_set_cases():
    rng = random.Random(110)
    a, b, c, d = _distinct(rng, 4)
    return {
        "two_n1_zero": ([], [a, b, a]),
        "two_n2_zero": ([a, b, a], []),
        "two_both_zero": ([], []),
        "two_absent": ([a, b, c], [a, a, c, d]),
        "two_40_by_3": ([a] * 40 + [b], [c, a, d, a, a, b]),
        "two_empty_strings": ([b"", a, b""], [b"", b, b"", b""]),
    }


TWO_SET_CASES = _two_set_cases()
