"""The overlap join's reference and case list (tests/overlap_ref.py, tests/overlap_cases.py), checked without a GPU.

 * the reference equals the CPU oracle (oracle/overlap.py: overlap_counts, and count_single_umi_overlaps pair by pair
   on the small cases) and reproduces the reference implementation's own outputs (tests/golden/overlap);
 * every case reaches the path it is named after: the bucket-size multiset, the non-empty regions of the big bucket,
   m and nb, the home slots of the wrap case, the 8-bit hashes of the collision cases, asserted from the case's data
   and the restated hash, not from a recorded answer.  A case that stops reaching its path fails here instead of
   passing silently in tests/test_gpu_overlap_kernels.py.
"""
import itertools
import random
from collections import Counter

import overlap as oracle
import overlap_cases as C
import overlap_ref as R
import pytest
from test_overlap_cpu import _golden

IDS = [c.name for c in C.CASES]
ref = C.ref  # the reference of one case, computed once and shared (never modified)


def sizes(case):
    """the multiset of bucket sizes: copies per distinct sequence"""
    return Counter(len(v) for v in ref(case)["classes"].values())


def held_regions(case, seq):
    """the regions that hold seq, with their counts"""
    return {r: reg.count(seq) for r, reg in enumerate(case.regions) if seq in reg}


def biggest(case):
    return max(ref(case)["classes"], key=lambda s: len(ref(case)["classes"][s]))


def test_hash_restatement_known_values():
    """hand-computable corners of the restated hash: the empty string skips the byte loop, the length is mixed in"""
    def mix(h):
        h ^= h >> 33
        h = (h * 0xff51afd7ed558ccd) & R.M64
        h ^= h >> 33
        h = (h * 0xc4ceb9fe1a85ec53) & R.M64
        return h ^ (h >> 33)
    for seed in R.SEEDS:
        assert R.hash64(b"", seed) == mix(seed)
        one = ((seed ^ 0x9e3779b97f4a7c15) ^ 0x41) * 0x100000001b3 & R.M64
        assert R.hash64(b"A", seed) == mix(one)
    assert R.hash64(b"A") != R.hash64(b"a") != R.hash64(b"AA")
    assert len({R.hash64(b"ACGT", s) for s in R.SEEDS}) == 4
    assert [R.table_slots(n) for n in (0, 1, 512, 513, 131072, 131073)] == [1024, 1024, 1024, 2048, 262144, 524288]


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_reference_equals_oracle(case):
    r = ref(case)
    regs = [list(x) for x in case.regions]
    nreg, n = len(regs), len(case.flat)
    assert r["region"] == [a for a, reg in enumerate(regs) for _ in reg]
    flat = case.flat
    assert all(flat[i] == flat[j] and j <= i for i, j in enumerate(r["rep"]))
    assert all(a < b and v > 0 for (a, b), v in r["total"].items()) and set(r["total"]) == set(r["maxcount"])
    if nreg <= 16:
        pairs = list(itertools.combinations(range(nreg), 2))
    else:  # every pair the reference reports, and a sample of those it does not
        rng = random.Random(case.name)
        pairs = sorted(set(r["total"]) | {tuple(sorted(rng.sample(range(nreg), 2))) for _ in range(2000)})
    for a, b in pairs:
        c = oracle.overlap_counts(regs[a], regs[b])
        assert r["total"].get((a, b), 0) == sum(c) and r["maxcount"].get((a, b), 0) == (max(c) if c else 0), (a, b)
        if n <= 600:  # the literal pairwise scan
            assert c == [oracle.count_single_umi_overlaps(u, regs[b], 2) for u in regs[a]]
    # all pairs at once: sum over a < b of c_a c_b per class = ((sum c)^2 - sum c^2) / 2
    want = 0
    for idx in r["classes"].values():
        per = Counter(r["region"][i] for i in idx)
        want += (len(idx) ** 2 - sum(v * v for v in per.values())) // 2
    assert sum(r["total"].values()) == want


@pytest.mark.parametrize("name", list(C.TWO_SET_CASES))
def test_two_set_reference_equals_oracle(name):
    s1, s2 = C.TWO_SET_CASES[name]
    got = R.counts(s1, s2)
    assert got == oracle.overlap_counts(s1, s2) == [oracle.count_single_umi_overlaps(u, s2, 2) for u in s1]
    want = {"two_n1_zero": [], "two_n2_zero": [0, 0, 0], "two_both_zero": [], "two_absent": [2, 0, 1],
            "two_40_by_3": [3] * 40 + [1], "two_empty_strings": [3, 0, 3]}
    assert got == want[name]


@pytest.mark.parametrize("fx", _golden(), ids=[c["name"] for c in _golden()])
def test_reference_reproduces_golden_fixtures(fx):
    """the TSV rows, the warnings and the result list of the reference implementation, rendered from join()"""
    regs = [[s.encode() for s in reg["seqs"]] for reg in fx["regions"]]
    names = [reg["name"] for reg in fx["regions"]]
    rs = [0]
    for reg in regs:
        rs.append(rs[-1] + len(reg))
    r = R.join([s for reg in regs for s in reg], rs)
    tsv, warn, result, error = "region_1\tregion_2\tumi_overlap_count\n", "", [], False
    for a, b in itertools.combinations(range(len(regs)), 2):
        if not regs[a]:
            error = True
            continue
        t = r["total"].get((a, b), 0)
        if r["maxcount"].get((a, b), 0) > 1:
            warn += f"WARNING: there are UMIs from {names[a]} that match more than 1 UMI within {names[b]}\n"
        if t:
            tsv += f"{names[a]}\t{names[b]}\t{t}\n"
        result.append(bool(t))
    files = {"regions_w_overlapping_umis.tsv": tsv}
    if warn:
        files["region_region_umi_comparison.stderr"] = warn
    assert files == fx["files"]
    assert error == bool(fx["error"]) and (error or result == fx["result"])


# ------------------------------------------------------------------ the path of every case, by name
def _p_regions_one(c):
    assert len(c.regions) == 1 and len(c.flat) > 1 and max(sizes(c)) > 1 and not ref(c)["total"]


def _p_n0(c):
    assert len(c.regions) == 3 and not c.flat and R.table_slots(0) == 1024


def _p_empty_edges(c):
    empty = [not r for r in c.regions]
    assert empty[:3] == [True, True, False] and empty[-3:] == [False, True, True]
    assert any(empty[i:i + 3] == [True] * 3 and not empty[i - 1] and not empty[i + 3] for i in range(3, len(empty) - 5))
    assert ref(c)["total"]  # the regions on both sides of the empty ones share sequences


def _p_one_nonempty(c):
    assert sum(1 for r in c.regions if r) == 1 and c.regions[0] == () == c.regions[-1] and max(sizes(c)) > 1


def _p_block_seam(c):
    assert c.region_start == [0, 255, 256, 257, 257] and len(c.flat) == 257
    t = ref(c)["total"]
    assert (0, 1) in t and (0, 2) in t  # sequences 255 and 256 are each equal to one of the first block


def _p_empty_strings(c):
    h = held_regions(c, b"")
    assert len(h) == 2 and sum(h.values()) == 3 and all(any(s for s in c.regions[r]) for r in h)


def _p_length_1(c):
    assert all(len(s) == 1 for s in c.flat) and ref(c)["total"]


def _p_last_byte(c):
    d = sorted(ref(c)["classes"])
    assert sum(1 for a, b in itertools.combinations(d, 2) if len(a) == len(b) and a[:-1] == b[:-1]) >= 3
    assert ref(c)["total"]


def _p_prefix(c):
    d = sorted(ref(c)["classes"])
    assert sum(1 for a, b in itertools.combinations(d, 2) if b.startswith(a)) >= 6 and b"" in d


def _p_high_bytes(c):
    assert sum(1 for s in ref(c)["classes"] if s and min(s) >= 0x80) >= 3 and b"\x00" in c.flat
    assert ref(c)["total"]


def _p_letter_case(c):
    d = ref(c)["classes"]
    pairs = [s for s in d if s != s.lower() and s.lower() in d]
    assert len(pairs) == 2
    # each region pair's total counts equal spellings only
    assert ref(c)["total"] == {(0, 1): 1, (0, 2): 1}


def _p_long(c):
    d = ref(c)["classes"]
    long_ = [s for s in d if len(s) == 4000]
    assert sorted(len(d[s]) for s in long_) == [1, 2] and long_[0][:-1] == long_[1][:-1]
    assert ref(c)["total"] == {(0, 2): 1}


def _p_bucket_spread(c):
    assert sizes(c) == Counter(C.BUCKET_SIZES)
    assert R.SMALL_BUCKET in C.BUCKET_SIZES and R.SMALL_BUCKET + 1 in C.BUCKET_SIZES
    for s, idx in ref(c)["classes"].items():
        assert len(held_regions(c, s)) == min(len(idx), len(c.regions))


def _p_bucket_one_region(c):
    assert sizes(c) == Counter(C.BUCKET_SIZES) and not ref(c)["total"]
    assert all(len(held_regions(c, s)) == 1 for s in ref(c)["classes"])


def _p_compact(c):
    k = int(c.name.split("_")[1])
    art = biggest(c)
    h = held_regions(c, art)
    assert len(c.regions) == C.SEAM_REGIONS >= 300 and len(h) == k
    assert set(h.values()) == {1, 2, 3} and sum(h.values()) > R.SMALL_BUCKET
    assert min(h) < 256 < max(h) and sum(1 for r in h if r > 255) >= 10
    assert sum(1 for r in h if r < 256) < k  # the second chunk of 256 regions adds to the first's compacted list
    assert len({ref(c)["maxcount"][a, b] for a, b in itertools.combinations(sorted(h), 2)}) == 3
    assert sorted(sizes(c).elements())[-2] <= R.SMALL_BUCKET  # the only big bucket


def _p_cap(c):
    assert len(c.regions) == C.CAP_REGIONS == 4096 and 4900 <= len(c.flat) <= 5100
    art = biggest(c)
    h = held_regions(c, art)
    assert len(h) > 32 and set(C.CAP_MUST_HOLD) <= set(h) and sum(h.values()) > R.SMALL_BUCKET
    small = [s for s in set(c.regions[-1]) if 2 <= len(ref(c)["classes"][s]) <= R.SMALL_BUCKET and
             len(held_regions(c, s)) >= 2]
    assert len(small) >= 2
    t = ref(c)["total"]
    assert (0, 4095) in t and (4094, 4095) in t and (17, 4095) in t and t[17, 4095] >= 2


def _p_3000(c):
    assert ref(c)["total"] == {(0, 2): 6000000} and ref(c)["maxcount"] == {(0, 2): 2000}
    assert max(sizes(c)) == 5000


def _p_contended(c):
    r = ref(c)
    shared = [s for s in r["classes"] if len(held_regions(c, s)) == 2]
    assert len(c.regions) == 2 and len(shared) == 500 == len(r["classes"])
    assert r["total"] == {(0, 1): 400 + 2 * 50 + 2 * 50} and r["maxcount"] == {(0, 1): 2}


def _p_asymmetric(c):
    r = ref(c)
    assert r["total"] == {(0, 1): 5, (2, 3): 5} and r["maxcount"] == {(0, 1): 1, (2, 3): 5}


def _p_scan(c):
    n, m, nb = {"scan_n1": (1, 1024, 1), "scan_n513": (513, 2048, 2), "scan_n131073": (131073, 524288, 512)}[c.name]
    assert len(c.flat) == n and R.table_slots(n) == m and R.scan_blocks(n) == nb
    if n == 131073:
        assert nb == 2 * R.SCAN_CHUNK and R.scan_blocks(n - 1) == R.SCAN_CHUNK and len(c.regions) == 7
        assert c.flat[:3] == [b"0", b"1", b"2"] and sizes(c) == Counter({3: 40000 - 11073, 4: 11073})
        assert len(ref(c)["total"]) >= 10  # of the 21 region pairs


def _p_wrap(c):
    assert len(c.flat) <= 512 and R.table_slots(len(c.flat)) == 1024
    home = {s: R.hash64(s, R.SEEDS[0]) & 1023 for s in ref(c)["classes"]}
    assert sum(1 for h in home.values() if h in C.WRAP_HOMES) >= 10
    assert sum(1 for h in home.values() if h < 16) >= 16 and set(home.values()) <= set(C.WRAP_HOMES) | set(range(16))
    # at most two of the sequences homed at the last two slots fit there: the others wrap to the table's start, past the
    # sequences homed at 0..15 (linear probing fills the same set of slots in whatever order the keys arrive)
    assert len({R.hash64(s) for s in home}) == len(home) and len(ref(c)["total"]) == 3
    table = {}
    for s in sorted(home):
        x = home[s]
        while x in table:
            x = (x + 1) & 1023
        table[x] = s
    wrapped = sum(1 for x, s in table.items() if x < home[s])
    assert wrapped >= 8 and set(table) == {1022, 1023} | set(range(len(table) - 2))  # one run across the table's end


def _p_collide(c):
    d = list(ref(c)["classes"])
    low = {R.hash64(s, R.SEEDS[0]) & 0xff for s in d}
    if c.name == "collide_8bit_distinct":
        assert (c.hash_bits, c.passes) == (8, 1) and len(d) == 5 == len(low) and ref(c)["total"]
    else:
        assert len(d) >= 300 and len(d) > 256 >= len(low)  # two of them share an 8-bit hash, whatever the hash
        assert (c.hash_bits, c.passes) == ((8, 2) if c.name == "collide_8bit" else (64, 1))
        assert c.regions == C.BY_NAME["collide_8bit"].regions
        assert len({R.hash64(s, R.SEEDS[1]) for s in d}) == len(d)  # the second seed is accepted


PROPERTY = {"regions_one": _p_regions_one, "regions_n0": _p_n0, "regions_empty_edges": _p_empty_edges,
            "regions_one_nonempty": _p_one_nonempty, "regions_block_seam": _p_block_seam,
            "seq_empty_strings": _p_empty_strings, "seq_length_1": _p_length_1, "seq_last_byte": _p_last_byte,
            "seq_prefix": _p_prefix, "seq_high_bytes": _p_high_bytes, "seq_letter_case": _p_letter_case,
            "seq_long_4000": _p_long, "bucket_sizes_spread": _p_bucket_spread,
            "bucket_sizes_one_region": _p_bucket_one_region, "compact_255": _p_compact, "compact_256": _p_compact,
            "compact_257": _p_compact, "region_cap_4096": _p_cap, "count_3000_by_2000": _p_3000,
            "count_contended_cell": _p_contended, "count_asymmetric": _p_asymmetric, "scan_n1": _p_scan,
            "scan_n513": _p_scan, "scan_n131073": _p_scan, "probe_wrap": _p_wrap, "collide_8bit": _p_collide,
            "collide_64bit": _p_collide, "collide_8bit_distinct": _p_collide}


def test_every_case_has_a_property():
    assert set(PROPERTY) == set(C.BY_NAME)
    assert all(c.hash_bits == 64 and c.passes == 1 for c in C.CASES if not c.name.startswith("collide_8bit"))


@pytest.mark.parametrize("name", IDS)
def test_case_property(name):
    PROPERTY[name](C.BY_NAME[name])
