"""The cases of the .bai index and flagstat tests -- TEST INFRASTRUCTURE ONLY.

A case is a Case: the uncompressed BAM stream, a keep mask (None: every record) and a block table, synthetic here so
that a few hundred bytes put records on every kind of block seam and a few hundred records spread over gigabytes of
imagined compressed file.  CASES are accepted; REFUSALS carry the status and the record the index must name.
Coordinates cost no data: long spans are N operations, and the header's references are 2^29 long.
"""
from __future__ import annotations

import struct

import bam_ref

L29 = 1 << 29


def rec(name, ref, pos, cigar, flag=0, mapq=60, next_ref=-1, l_seq=None):
    r = dict(name=name, ref=ref, pos=pos, cigar=cigar, flag=flag)
    if l_seq is not None:
        r["l_seq"] = l_seq
    b = bytearray(bam_ref.encode_record(r))
    b[13] = mapq
    b[24:28] = struct.pack("<i", next_ref)
    return bytes(b)


def stream(refs, records) -> bytes:
    return bam_ref.build_raw(refs, []) + b"".join(records)


def sizes_of(raw):
    start = bam_ref.parse_header(raw)[1]
    return start, [4 + struct.unpack_from("<i", raw, o)[0] for o in bam_ref.record_offsets(raw, start)]


def table(raw, keep, kind, arg=None, cgap=100):
    """(coff, ustart) over the kept stream.  kind "even": a block every `arg` bytes; "pattern": blocks of the sizes in
    `arg`, over and over; "records": a block ends where the header and every kept record end.  Block b sits at
    compressed offset b * cgap; the EOF block is last."""
    start, sizes = sizes_of(raw)
    kept = [s for r, s in enumerate(sizes) if keep is None or keep[r]]
    total = start + sum(kept)
    ustart, at, k = [], 0, 0
    if kind == "records":
        for s in [start] + kept:
            while s > 0:  # a record longer than a block can be: cut every 0xff00
                ustart.append(at)
                at += min(s, 0xff00)
                s -= min(s, 0xff00)
    else:
        pattern = [arg] if kind == "even" else arg
        while at < total:
            ustart.append(at)
            at = min(total, at + pattern[k % len(pattern)])
            k += 1
    ustart.append(total)
    return [b * cgap for b in range(len(ustart))], ustart


class Case:
    def __init__(self, name, raw, keep=None, kind="even", arg=4096, cgap=100):
        self.name, self.raw, self.keep = name, raw, keep
        self.coff, self.ustart = table(raw, keep, kind, arg, cgap)

    def __repr__(self):
        return self.name


REFS3 = [("chrA", L29), ("chrB", L29), ("chrC", 100000)]


def _boundaries():
    out = []
    for k in (14, 17, 20, 23, 26):
        B = 1 << k
        out += [(B - 10, "10M"), (B - 10, "11M"), (B - 1, "1M"), (B - 1, "2M"), (B, "5M"), (B - 40, "20M20N1M"),
                (B + 1, "3=")]
    out.append((L29 - 5, "5M"))      # end = 2^29 exactly
    out.append((L29 - 1, "1X"))
    out.sort(key=lambda x: x[0])
    return stream(REFS3, [rec("b%d" % i, 0, p, c) for i, (p, c) in enumerate(out)])


def _cigars():
    W = 1 << 14
    return stream(REFS3, [
        rec("nocigar", 0, 5 * W + 7, ""),
        rec("clips", 0, 5 * W + 9, "5S3H2I1P2S"),
        rec("ops", 0, 5 * W + 100, "3M2N4=5X1D"),
        rec("three_windows", 0, 5 * W + 200, "10M%dN10M" % (2 * W)),  # windows 5, 6, 7; 0..4 are empty
        rec("placed_unmapped", 0, 12 * W + 1, "10M", flag=4),        # windows 8..11 are empty
        rec("later", 0, 12 * W + 50, "10M"),
        rec("other_ref", 2, 0, "50M"),
        rec("nowhere1", -1, -1, "", flag=4, l_seq=10),
        rec("nowhere2", -1, -1, "", flag=4, l_seq=3),
    ])


def _alternating():
    """260 records in one window's neighbourhood whose bin flips at kept-record indices 1, 2, 3, 4 (A B A B), 63, 64,
    65, 255, 256 and 257"""
    B = 4 << 14
    flips, leaf, recs = {1, 2, 3, 4, 63, 64, 65, 255, 256, 257}, True, []
    for j in range(260):
        if j in flips:
            leaf = not leaf
        recs.append(rec("a%d" % j, 1, B - 200 + j // 2, "10M" if leaf else "5M300N5M"))
    return stream(REFS3, recs)


def _three_refs():
    recs = []
    for t in range(3):
        recs += [rec("r%d_%d" % (t, i), t, 1000 * i + 17 * t, "%dM" % (20 + i)) for i in range(6)]
    return stream(REFS3, recs)


def _big():
    """one record of more than 0xff00 bytes between small ones; with 0xff00-byte blocks it spans three blocks"""
    return stream(REFS3, [rec("s0", 0, 10, "10M"), rec("big", 0, 20, "90000M"), rec("s1", 0, 30, "10M"),
                          rec("s2", 1, 5, "8M")])


def _multiple_of_block():
    """a stream of exactly 2 * 0xff00 bytes: the last record ends on the last block's end"""
    head = [rec("m0", 0, 1, "10M"), rec("m1", 0, 2, "40000M")]
    base = len(stream(REFS3, head))
    for name in ("f", "ff", "fff", "ffff"):
        for l_seq in range(0, 80000):
            need = 2 * 0xff00 - base - (36 + len(name) + 1 + 4 + (l_seq + 1) // 2 + l_seq)
            if need == 0:
                return stream(REFS3, head + [rec(name, 0, 3, "1M", l_seq=l_seq)])
            if need < 0:
                break
    raise AssertionError("no filler fits")


FLAGS = [1 << b for b in range(12)] + [0x1 | 0x2, 0x1 | 0x4, 0x1 | 0x8, 0x1 | 0x40, 0x1 | 0x80, 0x1 | 0x2 | 0x4,
                                       0x1 | 0x8 | 0x4, 0x100 | 0x800, 0x200 | 0x100, 0x200 | 0x800, 0x200 | 0x1 | 0x2,
                                       0x200 | 0x4, 0x200 | 0x400, 0x1 | 0x400, 0]


def _flags():
    recs = [rec("f%d" % i, 0, 10 * i, "10M", flag=f, next_ref=0) for i, f in enumerate(FLAGS)]
    n = len(recs)
    recs += [rec("mate4", 0, 10 * n, "10M", flag=0x1, mapq=4, next_ref=1),
             rec("mate5", 0, 10 * n + 1, "10M", flag=0x1, mapq=5, next_ref=1),
             rec("mate5_qc", 0, 10 * n + 2, "10M", flag=0x1 | 0x200, mapq=5, next_ref=2),
             rec("mate_same", 0, 10 * n + 3, "10M", flag=0x1, mapq=30, next_ref=0)]
    return stream(REFS3, recs)


def _many_refs():
    refs = [("ref%d" % i, L29 if i % 2 else 1000 + i) for i in range(300)]
    return stream(refs, [rec("x0", 0, 5, "10M"), rec("x1", 150, 1 << 20, "10M100N5M"), rec("x2", 150, (1 << 20) + 5, "3M"),
                         rec("x3", 299, L29 - 20, "20M")])


def _refs_with_a_zero_byte(nref):
    """nref - 1 = 256 or 512: the largest reference number has no bit where the smaller ones differ.  Records on
    references 1, 2 and nref - 1, two bins on each, so that the runs sorted by bin alone would interleave the
    references"""
    refs = [("z%d" % i, L29) for i in range(nref)]
    recs = []
    for t in (1, 2, nref - 1):
        recs += [rec("z%d_a" % t, t, 5 + t, "10M"), rec("z%d_b" % t, t, 20000 + t, "10M"),
                 rec("z%d_c" % t, t, 40000, "5M20000N5M"), rec("z%d_d" % t, t, 40001 + t, "3M")]
    return stream(refs, recs)


def _build():
    empty, one = stream(REFS3, []), stream(REFS3, [rec("only", 1, 70000, "25M")])
    nocoor = stream(REFS3, [rec("u%d" % i, -1, -1, "", flag=4, l_seq=5) for i in range(3)])
    bounds, cigars, alt, three, big = _boundaries(), _cigars(), _alternating(), _three_refs(), _big()
    hdr = bam_ref.parse_header(cigars)[1]
    n3 = 18
    cases = [
        Case("empty", empty), Case("one", one), Case("nocoor_only", nocoor), Case("many_refs", _many_refs()),
        Case("boundaries", bounds), Case("boundaries_far", bounds, kind="even", arg=64, cgap=0x8000),
        Case("cigars", cigars), Case("cigars_seams_3_1_0", cigars, kind="pattern", arg=[3, 1, 0, 50, 0, 0, 7]),
        Case("cigars_block_per_record", cigars, kind="records"),
        Case("cigars_header_over_blocks", cigars, kind="even", arg=max(1, hdr // 3)),
        Case("alternating", alt),  # every bin under 64 KiB: all of it merges up to bin 0
        Case("alternating_far_big_blocks", alt, kind="even", arg=2000, cgap=0x10000),  # neighbours share blocks: merge
        Case("alternating_far_block_per_record", alt, kind="records", cgap=0x10000),   # a block later: no merge
        Case("alternating_half_far", alt, kind="even", arg=300, cgap=0x1000),  # one leaf stays, its short sibling goes up
        Case("alternating_every_second", alt, keep=[j % 2 for j in range(260)], kind="even", arg=300, cgap=0x1000),
        Case("three_refs", three),
        Case("keep_drop_first_of_ref", three, keep=[0 if r == 6 else 1 for r in range(n3)], kind="records"),
        Case("keep_drop_last_of_ref", three, keep=[0 if r == 11 else 1 for r in range(n3)], kind="even", arg=77),
        Case("keep_drop_whole_ref", three, keep=[0 if 6 <= r < 12 else 1 for r in range(n3)], kind="even", arg=50),
        Case("keep_every_second", three, keep=[r % 2 for r in range(n3)], kind="pattern", arg=[1, 0, 33]),
        Case("keep_none", three, keep=[0] * n3),
        Case("big_record", big, kind="even", arg=0xff00, cgap=20000),
        Case("big_record_two_blocks", big, kind="even", arg=0xff00 + 0x80, cgap=30000),
        Case("multiple_of_block", _multiple_of_block(), kind="even", arg=0xff00, cgap=0xfff0),
        Case("refs_257", _refs_with_a_zero_byte(257)),
        Case("refs_513", _refs_with_a_zero_byte(513), kind="even", arg=90, cgap=0x9000),
        Case("flags", _flags()),
        Case("flags_every_second", _flags(), keep=[j % 2 for j in range(len(FLAGS) + 4)]),
    ]
    return cases


CASES = _build()


def _refusals():
    U, R = 1, 2  # bai_ref.UNSORTED, bai_ref.RANGE
    pos_back = stream(REFS3, [rec("p0", 0, 100, "10M"), rec("p1", 0, 200, "10M"), rec("p2", 0, 199, "10M"),
                              rec("p3", 1, 5, "10M")])
    tid_back = stream(REFS3, [rec("t0", 1, 100, "10M"), rec("t1", 0, 200, "10M"), rec("t2", 2, 1, "10M")])
    after_nocoor = stream(REFS3, [rec("n0", 0, 1, "10M"), rec("n1", -1, -1, "", flag=4, l_seq=4), rec("n2", 2, 9, "10M")])
    too_far = stream(REFS3, [rec("e0", 0, 1, "10M"), rec("e1", 0, L29 - 5, "6M"), rec("e2", 1, 3, "10M")])
    # (stream, the first refused record, its status, the keep mask that hides the defect)
    return [("pos_decreasing", pos_back, 2, U, [1, 1, 0, 1]), ("tid_decreasing", tid_back, 1, U, [1, 0, 1]),
            ("placed_after_unplaced", after_nocoor, 2, U, [1, 0, 1]), ("end_past_2_29", too_far, 1, R, [1, 0, 1])]


REFUSALS = _refusals()


def case_file(path, case) -> None:
    """the input of `bai_check case`"""
    keep = bytes(case.keep) if case.keep is not None else b""
    with open(path, "wb") as fh:
        fh.write(struct.pack("<qqq", len(case.raw), len(keep) if case.keep is not None else -1, len(case.coff)))
        fh.write(case.raw + keep + struct.pack("<%dq" % len(case.coff), *case.coff)
                 + struct.pack("<%dq" % len(case.ustart), *case.ustart))


def query_grid(idx):
    """(tid, beg, end) per reference with records: every touched window's edges +-1, every record's own span, the
    whole reference and an empty stretch"""
    out = []
    for t in sorted(set(x for x in idx.tid if x >= 0)):
        spans = [(idx.w0[j], idx.w1[j]) for j in range(idx.n_kept) if idx.tid[j] == t]
        edges = sorted({w << 14 for a, b in spans for w in (a, b, b + 1)})
        for e in edges:
            out += [(t, max(0, e - 1), e), (t, e, e + 1), (t, max(0, e - 1), e + 1)]
        out += [(t, idx.beg[j], idx.end[j]) for j in range(idx.n_kept) if idx.tid[j] == t]
        out += [(t, 0, L29), (t, (3 << 26) + 12345, (3 << 26) + 12346)]
    return sorted(set(out))
