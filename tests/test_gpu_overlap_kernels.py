"""The region overlap join (csrc/overlap.hip, row f3) stage by stage: every array umiclust_overlap_probe copies out,
on every case of tests/overlap_cases.py, against tests/overlap_ref.py.

Everything compared here is integer data: equal or wrong, and no case is left out.  The probe runs the production
sequence (the table passes with the member lists, then the region pairs), so what is checked is what
umiclust_overlap_regions computes from; the same regions through that entry point must give identical matrices.
tests/test_overlap_ref_cpu.py shows that the reference equals the CPU oracle and that each case reaches the path it is
named after.

Not covered: the remap of an all-ones hash to all-ones minus one (all-ones is the table's empty key).  No real input
is known to hash to it and none can be found by search, so the branch is restated in overlap_ref.hash64 and left
unforced; hash_bits < 64 cannot produce it either (the masked value is below all-ones).
"""
import numpy as np
import overlap_cases as C
import overlap_ref as R
import pytest
from umiclust import _lib

pytestmark = pytest.mark.gpu

IDS = [c.name for c in C.CASES]


def _dense(sparse, nreg, dtype):
    out = np.zeros((nreg, nreg), dtype)
    for (a, b), v in sparse.items():
        out[a, b] = v
    return out


def _check(case, got):
    """every output of one probe call against the reference"""
    r = C.ref(case)
    flat, n, nreg = case.flat, len(case.flat), len(case.regions)
    m = R.table_slots(n)
    assert (got["m"], got["passes"]) == (m, case.passes)
    assert got["seed"] == R.SEEDS[case.passes - 1]
    # hash: the restated one under the accepted seed; a first pass that was accepted kept hash_bits of it
    keep = (1 << case.hash_bits) - 1 if case.passes == 1 else R.M64
    h_of = {s: R.hash64(s, got["seed"]) & keep for s in r["classes"]}
    assert np.array_equal(got["hash"], np.array([h_of[s] for s in flat], np.uint64))
    assert np.array_equal(got["region"], np.array(r["region"], np.int32))
    # slots: equal iff byte-equal; the representative is the lowest equal index
    slot, cnt, start, members = got["slot"], got["cnt"], got["start"], got["members"]
    assert len(cnt) == m and len(start) == m + 1
    assert n == 0 or (slot.min() >= 0 and slot.max() < m)
    slot_of = {}
    for s, idx in r["classes"].items():
        assert (slot[idx] == slot[idx[0]]).all(), s
        slot_of[s] = int(slot[idx[0]])
    assert len(set(slot_of.values())) == len(slot_of)
    assert np.array_equal(got["rep_of"], np.array(r["rep"], np.int64))
    # counts and their scan, entry for entry
    assert np.array_equal(cnt[slot], np.array(r["size"], np.uint32))
    assert int(cnt.sum(dtype=np.int64)) == n and int(np.count_nonzero(cnt)) == len(r["classes"])
    want_start = np.zeros(m + 1, np.int64)
    np.cumsum(cnt, dtype=np.int64, out=want_start[1:])
    assert np.array_equal(start.astype(np.int64), want_start) and int(start[m]) == n
    # members: every slot's list is its index set; k_ov_pairs leaves the buckets of 2..32 ascending
    assert np.array_equal(np.sort(members), np.arange(n, dtype=np.uint32))
    for s, idx in r["classes"].items():
        t = slot_of[s]
        mine = members[start[t]:start[t + 1]].tolist()
        assert sorted(mine) == idx, s
        if 2 <= len(idx) <= R.SMALL_BUCKET:
            assert mine == idx, (s, "not ascending")
    # the hand-over: exactly the slots with more than 32 members, once each
    big = got["big"].tolist()
    assert sorted(big) == np.flatnonzero(cnt > R.SMALL_BUCKET).tolist()
    assert sorted(big) == sorted(t for s, t in slot_of.items() if len(r["classes"][s]) > R.SMALL_BUCKET)
    # what ov_find relies on: no empty slot between a sequence's home and its slot, cyclically
    occupied = cnt > 0
    for s, t in slot_of.items():
        x = h_of[s] & (m - 1)
        while x != t:
            assert occupied[x], (s, x, t)
            x = (x + 1) & (m - 1)
    # the matrices
    assert np.array_equal(got["total"], _dense(r["total"], nreg, np.int64))
    assert np.array_equal(got["maxcount"], _dense(r["maxcount"], nreg, np.int32))
    return slot_of, h_of


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_probe_vs_reference(gpu_ctx, case):
    got = gpu_ctx.overlap_probe(case.regions, case.hash_bits)
    slot_of, h_of = _check(case, got)
    total, maxc = gpu_ctx.overlap_regions(case.regions)
    assert np.array_equal(total, got["total"]) and np.array_equal(maxc, got["maxcount"])
    if case.name == "probe_wrap":  # all but two of the sequences homed at the table's last two slots sit past its end
        last = [s for s in slot_of if h_of[s] & 1023 in C.WRAP_HOMES]
        assert sum(1 for s in last if slot_of[s] < 1022) >= len(last) - 2 >= 8
    if case.name == "collide_64bit":  # the same matrices as the run that collided first
        again = gpu_ctx.overlap_probe(case.regions, 8)
        assert again["passes"] == 2 and np.array_equal(again["total"], got["total"])
        assert np.array_equal(again["maxcount"], got["maxcount"]) and np.array_equal(again["rep_of"], got["rep_of"])


@pytest.mark.parametrize("name", list(C.TWO_SET_CASES))
def test_two_set_counts_vs_reference(gpu_ctx, name):
    s1, s2 = C.TWO_SET_CASES[name]
    assert gpu_ctx.overlap_counts(s1, s2).tolist() == R.counts(s1, s2)


def test_public_entries_after_a_smaller_join(gpu_ctx):
    """the wrap case and the n = 131,073 case through umiclust_overlap_regions and umiclust_overlap_counts on a context
    that has just run a smaller join: tables, counters and lists start from a clean state in every call"""
    small = C.BY_NAME["bucket_sizes_spread"]
    for name in ("probe_wrap", "scan_n131073"):
        case = C.BY_NAME[name]
        r = C.ref(case)
        gpu_ctx.overlap_regions(small.regions)
        total, maxc = gpu_ctx.overlap_regions(case.regions)
        assert np.array_equal(total, _dense(r["total"], len(case.regions), np.int64))
        assert np.array_equal(maxc, _dense(r["maxcount"], len(case.regions), np.int32))
        gpu_ctx.overlap_counts(small.regions[0], small.regions[1])
        s1, s2 = case.regions[0], case.regions[-1]
        assert gpu_ctx.overlap_counts(s1, s2).tolist() == R.counts(s1, s2)
        assert int(gpu_ctx.overlap_counts(s1, s2).sum()) == r["total"].get((0, len(case.regions) - 1), 0)


def test_probe_refusals(gpu_ctx):
    case = C.BY_NAME["regions_empty_edges"]
    n = len(case.flat)
    for caps in ((n - 1, 1024, 1), (n, 1023, 1)):
        with pytest.raises(_lib.UmiclustError) as e:
            gpu_ctx.overlap_probe(case.regions, 64, caps)
        assert e.value.code == -34
    big = C.BY_NAME["bucket_sizes_spread"]
    with pytest.raises(_lib.UmiclustError) as e:
        gpu_ctx.overlap_probe(big.regions, 64, (len(big.flat), 1024, 2))  # three large buckets
    assert e.value.code == -34
    for bits in (0, 65):
        with pytest.raises(_lib.UmiclustError) as e:
            gpu_ctx.overlap_probe(case.regions, bits)
        assert e.value.code == -22
    # region boundaries that do not span [0, n], or decrease: refused before anything is launched
    buf, off = _lib._pack(case.flat)
    for rs in ([0, 5, n - 1], [1, 5, n], [0, 9, 5, n]):
        rs = np.array(rs, np.int64)
        info = np.zeros(3, np.uint64)
        rc = _lib.lib().umiclust_overlap_probe(gpu_ctx._h, buf.ctypes.data, _lib._i64(off), n, _lib._i64(rs),
                                               len(rs) - 1, 64, n, 1024, 1, *([None] * 11), info.ctypes.data)
        assert rc == -22 and not info.any()
    _check(case, gpu_ctx.overlap_probe(case.regions))  # the context still works
