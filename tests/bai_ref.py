"""Plain Python reference for the .bai index and flagstat (policies O10 and O11) -- TEST
INFRASTRUCTURE ONLY.  Written from the policy text and the SAM specification §5, not from csrc/bam_index.h.

- block_table(path): coff / ustart of every block of a BGZF file, the EOF block (or the file's end) last;
- Index(raw, keep, coff, ustart): every array the device leaves (per kept record bin, windows, virtual offsets, status;
  the runs before and after the sort; per reference n_intv, the linear index, mapped / unmapped), the finish, and
  .bytes, the file;
- parse_bai(bytes): the file read back;
- query(reader, refs, tid, beg, end): the specification's reader -- reg2bins, the linear index's lower bound, chunks
  with v <= min_off skipped -- walking the records through a BGZF file (BgzfReader) or through a stream under a
  synthetic block table (TableReader); brute(idx, tid, beg, end) is the set it must find;
- flagstat(raw, keep): the 32 counters and the text.
"""
from __future__ import annotations

import os
import struct
import zlib

import numpy as np

import bam_ref

META_BIN = 37450
OK, UNSORTED, RANGE, BADREF = 0, 1, 2, 3
LABELS = [ln.rstrip("\n") for ln in open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                                      "flagstat_lines.txt"))]


# ---------------------------------------------------------------- the block table and virtual offsets
def block_table(path):
    data = open(path, "rb").read()
    coff, ustart, o, u, last = [], [], 0, 0, 0
    while o < len(data):
        bsize = struct.unpack_from("<H", data, o + 16)[0] + 1
        last = struct.unpack_from("<I", data, o + bsize - 4)[0]
        coff.append(o), ustart.append(u)
        u += last
        o += bsize
    if not coff or last:
        coff.append(len(data)), ustart.append(u)
    return coff, ustart


def voffset(p, coff, ustart):
    """of stream position p > 0: inside the block that holds byte p - 1, or the start of the block after it"""
    b = max(x for x in range(len(ustart)) if ustart[x] <= p - 1)
    if b + 1 >= len(ustart) or p < ustart[b + 1]:
        return (coff[b] << 16) | (p - ustart[b])
    return coff[b + 1] << 16


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def reg2bins(beg, end):
    end -= 1
    bins = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        bins += range(first + (beg >> shift), first + (end >> shift) + 1)
    return bins


class Rec:
    def __init__(self, raw, off):
        self.off = off
        self.size = 4 + struct.unpack_from("<i", raw, off)[0]
        (self.tid, self.beg, lrn, self.mapq, _b, ncig, self.flag, _l, self.next_tid) = struct.unpack_from(
            "<iiBBHHHii", raw, off + 4)
        rlen = 0
        if not (self.flag & 4) and ncig:
            for v in struct.unpack_from("<%dI" % ncig, raw, off + 36 + lrn):
                if (v & 15) in (0, 2, 3, 7, 8):
                    rlen += v >> 4
        self.end = self.beg + (rlen or 1)


def kept_records(raw, keep=None):
    start = bam_ref.parse_header(raw)[1]
    offs = bam_ref.record_offsets(raw, start)
    return start, [(r, Rec(raw, o)) for r, o in enumerate(offs) if keep is None or keep[r]]


# ---------------------------------------------------------------- the index
class Index:
    def __init__(self, raw, keep, coff, ustart):
        refs, _ = bam_ref.parse_header(raw)
        nref = self.nref = len(refs)
        start, recs = kept_records(raw, keep)
        self.first_bad, self.first_status = -1, OK
        self.tid, self.bin, self.w0, self.w1, self.u, self.v, self.status = [], [], [], [], [], [], []
        self.beg, self.end = [], []
        self.mapped, self.unmapped, self.n_intv = [0] * nref, [0] * nref, [0] * nref
        self.n_no_coor, pos, prev = 0, start, None
        for r, R in recs:
            st = OK
            if R.tid >= nref:
                st = BADREF
            elif R.tid >= 0 and (R.beg < 0 or R.end > 1 << 29):
                st = RANGE
            if st == OK and prev is not None:
                if (R.tid & 0xffffffff) < (prev.tid & 0xffffffff) or (R.tid == prev.tid and R.tid >= 0 and R.beg < prev.beg):
                    st = UNSORTED
            if st and self.first_bad < 0:
                self.first_bad, self.first_status = r, st
            ok = 0 <= R.tid < nref and st != RANGE
            self.tid.append(R.tid), self.status.append(st)
            self.beg.append(R.beg), self.end.append(R.end)
            self.bin.append(reg2bin(R.beg, R.end) if ok else 0)
            self.w0.append(R.beg >> 14 if ok else 0), self.w1.append((R.end - 1) >> 14 if ok else 0)
            self.u.append(voffset(pos, coff, ustart)), self.v.append(voffset(pos + R.size, coff, ustart))
            pos += R.size
            prev = R
            if R.tid < 0:
                self.n_no_coor += 1
            elif R.tid < nref:
                if R.flag & 4:
                    self.unmapped[R.tid] += 1
                else:
                    self.mapped[R.tid] += 1
                if ok:
                    self.n_intv[R.tid] = max(self.n_intv[R.tid], self.w1[-1] + 1)
        self.n_kept, self.total = len(recs), pos
        self.runs, self.sorted_runs, self.linear, self.bytes = [], [], [], None
        if self.first_bad >= 0:
            return
        for j in range(self.n_kept):
            if self.tid[j] < 0:
                continue
            if j and self.tid[j] == self.tid[j - 1] and self.bin[j] == self.bin[j - 1]:
                self.runs[-1][3] = self.v[j]
            else:
                self.runs.append([self.tid[j], self.bin[j], self.u[j], self.v[j]])
        self.sorted_runs = sorted(self.runs, key=lambda x: (x[0], x[1]))  # stable
        self.linear_of = []
        for t in range(nref):
            lin = [None] * self.n_intv[t]
            for j in range(self.n_kept):
                if self.tid[j] == t:
                    for w in range(self.w0[j], self.w1[j] + 1):
                        lin[w] = self.u[j] if lin[w] is None else min(lin[w], self.u[j])
            for w in range(len(lin) - 2, -1, -1):
                if lin[w] is None:
                    lin[w] = lin[w + 1]
            self.linear_of.append(lin)
            self.linear += lin
        self.bins_of = [self._finish(t) for t in range(nref)]
        self.bytes = self._serialise()

    def _finish(self, t):
        bins = {}
        for tid, b, u, v in self.sorted_runs:
            if tid == t:
                bins.setdefault(b, []).append((u, v))
        for level in (5, 4, 3, 2, 1):
            lo, hi = ((1 << 3 * level) - 1) // 7, ((1 << 3 * (level + 1)) - 1) // 7
            for b in sorted(x for x in bins if lo <= x < hi):
                c = sorted(bins[b], key=lambda x: x[0])
                if (c[-1][1] >> 16) - (c[0][0] >> 16) < 0x10000:
                    bins.setdefault((b - 1) >> 3, []).extend(c)
                    del bins[b]
        out = {}
        for b in sorted(bins):
            c = sorted(bins[b], key=lambda x: x[0])
            merged = [list(c[0])]
            for u, v in c[1:]:
                if merged[-1][1] >> 16 >= u >> 16:
                    merged[-1][1] = max(merged[-1][1], v)
                else:
                    merged.append([u, v])
            out[b] = [tuple(x) for x in merged]
        return out

    def _serialise(self):
        out = [b"BAI\x01", struct.pack("<i", self.nref)]
        for t in range(self.nref):
            mine = [j for j in range(self.n_kept) if self.tid[j] == t]
            if not mine:
                out.append(struct.pack("<ii", 0, 0))
                continue
            bins = self.bins_of[t]
            out.append(struct.pack("<i", len(bins) + 1))
            for b in sorted(bins):
                out.append(struct.pack("<Ii", b, len(bins[b])))
                out += [struct.pack("<QQ", u, v) for u, v in bins[b]]
            out.append(struct.pack("<IiQQQQ", META_BIN, 2, self.u[mine[0]], self.v[mine[-1]], self.mapped[t],
                                   self.unmapped[t]))
            out.append(struct.pack("<i", self.n_intv[t]))
            out += [struct.pack("<Q", x) for x in self.linear_of[t]]
        out.append(struct.pack("<Q", self.n_no_coor))
        return b"".join(out)


def parse_bai(data: bytes):
    assert data[:4] == b"BAI\x01"
    nref, o = struct.unpack_from("<i", data, 4)[0], 8
    refs = []
    for _ in range(nref):
        nbin = struct.unpack_from("<i", data, o)[0]
        o += 4
        bins, meta = {}, None
        for _ in range(nbin):
            b, nch = struct.unpack_from("<Ii", data, o)
            o += 8
            chunks = [struct.unpack_from("<QQ", data, o + 16 * k) for k in range(nch)]
            o += 16 * nch
            if b == META_BIN:
                meta = chunks
            else:
                bins[b] = chunks
        nintv = struct.unpack_from("<i", data, o)[0]
        o += 4
        refs.append(dict(bins=bins, meta=meta, linear=list(struct.unpack_from("<%dQ" % nintv, data, o))))
        o += 8 * nintv
    n_no_coor = struct.unpack_from("<Q", data, o)[0]
    assert o + 8 == len(data)
    return refs, n_no_coor


# ---------------------------------------------------------------- the specification's reader
class BlockReader:
    """records by virtual offset: block(coff) gives (the block's bytes, the next block's offset) or None past the end"""

    def read(self, voff, n):
        """(n bytes from voff on, the virtual offset after them as bgzf_tell gives it); (None, None) past the end"""
        coff, within = voff >> 16, voff & 0xffff
        out = b""
        while len(out) < n:
            blk = self.block(coff)
            if blk is None:
                return None, None
            payload, nxt = blk
            take = payload[within:within + n - len(out)]
            out += take
            within += len(take)
            if within >= len(payload):  # the block is used up: the position is the next block's start
                coff, within = nxt, 0
        return out, (coff << 16) | within


class BgzfReader(BlockReader):
    """over a BGZF file (blocks inflated on demand)"""

    def __init__(self, path):
        self.data = open(path, "rb").read()
        self.cache = {}

    def block(self, coff):
        if coff >= len(self.data):
            return None
        if coff not in self.cache:
            bsize = struct.unpack_from("<H", self.data, coff + 16)[0] + 1
            self.cache[coff] = (zlib.decompress(self.data[coff + 18:coff + bsize - 8], -15), coff + bsize)
        return self.cache[coff]


class TableReader(BlockReader):
    """over an uncompressed stream cut by a block table (coff, ustart): the imagined file of a synthetic case"""

    def __init__(self, stream, coff, ustart):
        assert len(stream) == ustart[-1]
        self.stream, self.coff, self.ustart = stream, coff, ustart
        self.at = {c: b for b, c in enumerate(coff)}

    def block(self, coff):
        b = self.at[coff]  # KeyError: an offset that is no block's start
        if b + 1 >= len(self.coff):
            return None
        return self.stream[self.ustart[b]:self.ustart[b + 1]], self.coff[b + 1]


def kept_stream(raw, keep=None) -> bytes:
    start, recs = kept_records(raw, keep)
    return raw[:start] + b"".join(raw[R.off:R.off + R.size] for _, R in recs)


def query(reader, refs, tid, beg, end):
    """(virtual offset, tid, beg, end) of every record the reader reaches that overlaps [beg, end); refs =
    parse_bai(...)[0]"""
    ref = refs[tid]
    lin = ref["linear"]
    min_off = 0 if not lin else lin[min(beg >> 14, len(lin) - 1)]
    chunks = sorted(c for b in reg2bins(beg, end) for c in ref["bins"].get(b, []) if c[1] > min_off)
    found = []
    for u, v in chunks:
        at = u
        while at < v:
            head, nxt = reader.read(at, 4)
            if head is None:
                break
            body, nxt = reader.read(nxt, struct.unpack("<i", head)[0])
            R = Rec(head + body, 0)
            if R.tid != tid or R.beg >= end:
                break
            if R.end > beg:
                found.append((at, R.tid, R.beg, R.end))
            at = nxt
    return sorted(set(found))


def brute(idx, tid, beg, end):
    """the same set straight from the records of an Index"""
    return sorted((idx.u[j], tid, idx.beg[j], idx.end[j]) for j in range(idx.n_kept)
                  if idx.tid[j] == tid and idx.beg[j] < end and idx.end[j] > beg)


def check_reader_contract(reader, bai: bytes, idx, grid) -> None:
    refs = parse_bai(bai)[0]
    for tid, beg, end in grid:
        assert query(reader, refs, tid, beg, end) == brute(idx, tid, beg, end), (tid, beg, end)


# ---------------------------------------------------------------- flagstat
def flagstat(raw, keep=None):
    c = [0] * 32
    for _, R in kept_records(raw, keep)[1]:
        f, w = R.flag, 1 if R.flag & 0x200 else 0

        def add(row):
            c[2 * row + w] += 1
        add(0)
        if f & 0x100:
            add(2)
        elif f & 0x800:
            add(3)
        else:
            add(1)
            if f & 0x1:
                add(8)
                if f & 0x2 and not f & 0x4:
                    add(11)
                if f & 0x40:
                    add(9)
                if f & 0x80:
                    add(10)
                if f & 0x8 and not f & 0x4:
                    add(13)
                if not f & 0x4 and not f & 0x8:
                    add(12)
                    if R.next_tid != R.tid:
                        add(14)
                        if R.mapq >= 5:
                            add(15)
            if not f & 0x4:
                add(7)
            if f & 0x400:
                add(5)
        if not f & 0x4:
            add(6)
        if f & 0x400:
            add(4)
    return c, flagstat_text(c)


def flagstat_text(c) -> str:
    def pct(n, total):
        return "%.2f%%" % (float(np.float32(n) / np.float32(total)) * 100.0) if total else "N/A"
    of = {6: 0, 7: 1, 11: 8, 13: 8}
    out = []
    for k in range(16):
        line = "%d + %d %s" % (c[2 * k], c[2 * k + 1], LABELS[k])
        if k in of:
            d = of[k]
            line += " (%s : %s)" % (pct(c[2 * k], c[2 * d]), pct(c[2 * k + 1], c[2 * d + 1]))
        out.append(line + "\n")
    return "".join(out)
