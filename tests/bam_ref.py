"""Plain Python reference for the BAM scan, the cs group-by and the BAM writer (row f6) -- TEST
INFRASTRUCTURE ONLY.

- write_bam / build_raw: a BAM writer with aux tags of every type (A c C s S i I f Z H B, plus raw bytes for the
  malformed cases);
- decode / columns: the record decoder, the aux walk, cols (M/I/D), reference_length (M/D/N/=/X, 0 -> 1) and NM, and
  the cs strings grouped with a dict (first-seen order);
- Columns: the attributes umiclust.minimap2_align's formatting half reads, filled from this reference;
- check_bgzf: every member passes gzip (CRC checked), every payload is <= 0xff00 bytes, the EOF block is last;
- pysam_standin(): a module object with AlignmentFile / AlignedSegment (get_tag, has_tag, cigartuples, query_name,
  query_length = l_seq, reference_name, reference_length, the flag properties, and "wb" files whose write re-emits the
  record's bytes) for running the reference's own functions where pysam is absent.
"""
from __future__ import annotations

import gzip
import re
import struct
import types
import zlib

import numpy as np

CIGAR_OPS = "MIDNSHP=X"
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
PACK = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}
INT_TYPES = "cCsSiI"
HEADER_TEXT = b"@HD\tVN:1.6\tSO:coordinate\n"


class Malformed(Exception):
    def __init__(self, record, what):
        super().__init__("record %d: %s" % (record, what))
        self.record = record


# ---------------------------------------------------------------- writer
def encode_tag(tag, ty, value) -> bytes:
    if ty == "raw":
        return bytes.fromhex(value)
    head = tag.encode() + ty.encode()
    if ty == "A":
        return head + value.encode()
    if ty in PACK:
        return head + struct.pack(PACK[ty], value)
    if ty in "ZH":
        return head + value.encode() + b"\0"
    if ty == "B":
        sub, vals = value
        return head + sub.encode() + struct.pack("<I", len(vals)) + b"".join(struct.pack(PACK[sub], v) for v in vals)
    raise ValueError(ty)


def encode_record(r) -> bytes:
    """r: dict with name, cigar (SAM text such as "4S186M2I", or [[op, len]]), tags [[tag, type, value]] and, where they
    differ from the defaults, flag (0), ref (0), pos (0) and l_seq (the read bases the CIGAR consumes)."""
    name = r["name"].encode() + b"\0"
    ops = r["cigar"]
    if isinstance(ops, str):
        ops = [(op, int(ln)) for ln, op in re.findall(r"(\d+)([MIDNSHP=X])", ops)]
    lseq = r["l_seq"] if "l_seq" in r else sum(ln for op, ln in ops if op in "MIS=X")
    cig = b"".join(struct.pack("<I", (ln << 4) | CIGAR_OPS.index(op)) for op, ln in ops)
    codes = [(1, 2, 4, 8)[i & 3] for i in range(lseq)]
    packed = bytes(((codes[i] << 4) | (codes[i + 1] if i + 1 < lseq else 0)) for i in range(0, lseq, 2))
    body = struct.pack("<iiBBHHHiiii", r.get("ref", 0), r.get("pos", 0), len(name), 60, 4680, len(ops), r.get("flag", 0), lseq,
                       -1, -1, 0) + name + cig + packed + b"\xff" * lseq
    body += b"".join(encode_tag(*t) for t in r.get("tags", []))
    return struct.pack("<i", len(body)) + body


def build_raw(refs, records) -> bytes:
    raw = bytearray(b"BAM\x01")
    raw += struct.pack("<i", len(HEADER_TEXT)) + HEADER_TEXT + struct.pack("<i", len(refs))
    for name, ln in refs:
        nb = name.encode() + b"\0"
        raw += struct.pack("<i", len(nb)) + nb + struct.pack("<i", ln)
    for r in records:
        raw += encode_record(r)
    return bytes(raw)


def bgzf_block(data: bytes) -> bytes:
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    comp = c.compress(data) + c.flush()
    hdr = struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(comp) + 25)
    return hdr + comp + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data))


def write_bgzf(path, raw: bytes, block: int = 60000) -> None:
    with open(path, "wb") as fh:
        for i in range(0, len(raw), block):
            fh.write(bgzf_block(raw[i:i + block]))
        fh.write(EOF_BLOCK)


def write_bam(path, refs, records, block: int = 60000) -> bytes:
    raw = build_raw(refs, records)
    write_bgzf(path, raw, block)
    return raw


def write_fasta(path, regions) -> None:
    with open(path, "w") as fh:
        for name, ln in regions:
            fh.write(">%s\n%s\n" % (name, "ACGT" * (ln // 4) + "ACGT"[:ln % 4]))


# ---------------------------------------------------------------- BGZF checker
def check_bgzf(path) -> bytes:
    """the inflated stream of a BGZF file, after checking its form block by block"""
    data = open(path, "rb").read()
    assert data.endswith(EOF_BLOCK), "no EOF block at the end"
    out, o, sizes = [], 0, []
    while o < len(data):
        assert data[o:o + 4] == b"\x1f\x8b\x08\x04", "block %d: not a gzip member with an extra field" % len(sizes)
        xlen = struct.unpack_from("<H", data, o + 10)[0]
        assert xlen == 6 and data[o + 12:o + 16] == b"BC\x02\x00", "block %d: no BC extra field" % len(sizes)
        bsize = struct.unpack_from("<H", data, o + 16)[0] + 1
        member = data[o:o + bsize]
        assert len(member) == bsize
        payload = gzip.decompress(member)  # checks CRC32 and ISIZE
        assert len(payload) <= 0xff00, "block %d: payload of %d bytes" % (len(sizes), len(payload))
        assert struct.unpack_from("<I", member, bsize - 4)[0] == len(payload)
        out.append(payload)
        sizes.append(len(payload))
        o += bsize
    assert o == len(data) and sizes[-1] == 0
    assert all(s > 0 for s in sizes[:-1]), "an empty block before the EOF block"
    return b"".join(out)


# ---------------------------------------------------------------- decoder
def parse_header(raw: bytes):
    assert raw[:4] == b"BAM\x01"
    lt = struct.unpack_from("<i", raw, 4)[0]
    o = 8 + lt
    nref = struct.unpack_from("<i", raw, o)[0]
    o += 4
    refs = []
    for _ in range(nref):
        ln = struct.unpack_from("<i", raw, o)[0]
        refs.append((raw[o + 4:o + 4 + ln - 1].decode(), struct.unpack_from("<i", raw, o + 4 + ln)[0]))
        o += 8 + ln
    return refs, o


def record_offsets(raw: bytes, start: int):
    offs, o = [], start
    while o < len(raw):
        offs.append(o)
        o += 4 + struct.unpack_from("<i", raw, o)[0]
    assert o == len(raw)
    return offs


def walk_aux(raw: bytes, o: int, end: int, record: int):
    """[(tag, type, value, value offset)] of the aux fields in raw[o:end]; Malformed on a defect"""
    tags = []
    while o < end:
        if o + 3 > end:
            raise Malformed(record, "tag header past the record end")
        tag, ty = raw[o:o + 2].decode("latin-1"), chr(raw[o + 2])
        v = o + 3
        if ty in FIXED:
            if v + FIXED[ty] > end:
                raise Malformed(record, "field past the record end")
            val = chr(raw[v]) if ty == "A" else struct.unpack_from(PACK[ty], raw, v)[0]
            tags.append((tag, ty, val, v))
            o = v + FIXED[ty]
        elif ty == "B":
            if v + 5 > end:
                raise Malformed(record, "array header past the record end")
            sub, cnt = chr(raw[v]), struct.unpack_from("<I", raw, v + 1)[0]
            if sub not in PACK:
                raise Malformed(record, "unknown array subtype")
            size = struct.calcsize(PACK[sub])
            if v + 5 + size * cnt > end:
                raise Malformed(record, "array past the record end")
            tags.append((tag, ty, (sub, list(struct.unpack_from("<%d%s" % (cnt, PACK[sub][1]), raw, v + 5))), v))
            o = v + 5 + size * cnt
        elif ty in "ZH":
            z = raw.find(b"\0", v, end)
            if z < 0:
                raise Malformed(record, "string without NUL")
            tags.append((tag, ty, raw[v:z].decode("ascii"), v))
            o = z + 1
        else:
            raise Malformed(record, "unknown type byte %r" % ty)
    return tags


class Record:
    def __init__(self, raw: bytes, off: int, index: int, refs):
        self.raw, self.off, self.index, self._refs = raw, off, index, refs
        bs = struct.unpack_from("<i", raw, off)[0]
        self.end = off + 4 + bs
        (self.ref, self.pos, lrn, mapq, bin_, ncig, self.flag, self.l_seq, next_ref, next_pos, tlen) = \
            struct.unpack_from("<iiBBHHHiiii", raw, off + 4)
        p = off + 36
        self.query_name = raw[p:p + lrn - 1].decode()
        p += lrn
        self.cigar = [(v & 15, v >> 4) for v in struct.unpack_from("<%dI" % ncig, raw, p)]
        self.aux = p + 4 * ncig + (self.l_seq + 1) // 2 + self.l_seq
        # the fixed fields in file order, then where the aux fields start within the record
        self.fixed = [self.ref, self.pos, lrn, mapq, bin_, ncig, self.flag, self.l_seq, next_ref, next_pos, tlen,
                      self.aux - off]
        self.bytes = raw[off:self.end]

    @property
    def cls(self):
        return 0 if self.flag & 4 else 1 if self.flag & 0x900 else 2

    @property
    def reference_length(self):
        return sum(ln for op, ln in self.cigar if op in (0, 2, 3, 7, 8)) or 1  # htslib bam_endpos: 0 -> 1

    @property
    def cols(self):
        return sum(ln for op, ln in self.cigar if op in (0, 1, 2))

    def tags(self):
        return walk_aux(self.raw, self.aux, self.end, self.index)


def decode(raw: bytes):
    refs, start = parse_header(raw)
    return refs, start, [Record(raw, o, i, refs) for i, o in enumerate(record_offsets(raw, start))]


class Columns:
    """The per-record columns and the cs groups of a BAM, as the device session reports them.  Raises Malformed for
    the first primary record whose aux fields are malformed, or whose NM is no integer / cs no Z string."""

    def __init__(self, raw: bytes):
        self.raw = raw
        refs, self.header_end, self.records = decode(raw)
        self.ref_names = [n for n, _ in refs]
        self.ref_lengths = np.array([ln for _, ln in refs], np.int64)
        n = self.n = len(self.records)
        self.cls = np.array([r.cls for r in self.records], np.int8)
        self.ref = np.array([r.ref for r in self.records], np.int32)
        self.l_seq = np.array([r.l_seq for r in self.records], np.int32)
        self.reference_length = np.array([r.reference_length for r in self.records], np.int64)
        self.cols = np.array([r.cols for r in self.records], np.int64)
        self.nm, self.nm_present = np.zeros(n, np.int64), np.zeros(n, np.uint8)
        self.cs_group = np.full(n, -1, np.int32)
        self.cs = [None] * n
        groups = {}  # cs string -> group id, first-seen order
        self.group_count, self.group_rep = [], []
        for i, r in enumerate(self.records):
            if r.cls != 2:
                continue  # the reference never reads the tags of the other records
            seen = set()
            for tag, ty, val, _ in r.tags():
                if tag in seen:
                    continue  # the first field of a tag is the one bam_aux_get finds
                seen.add(tag)
                if tag == "NM":
                    if ty not in INT_TYPES:
                        raise Malformed(i, "NM is no integer")
                    self.nm[i], self.nm_present[i] = val, 1
                elif tag == "cs":
                    if ty != "Z":
                        raise Malformed(i, "cs is no Z string")
                    self.cs[i] = val
                    if val not in groups:
                        groups[val] = len(groups)
                        self.group_count.append(0)
                        self.group_rep.append(i)
                    self.cs_group[i] = groups[val]
                    self.group_count[groups[val]] += 1
        self.group_strings = list(groups)

    def query_names(self, idx):
        return [self.records[int(i)].query_name for i in idx]

    def cs_strings(self, idx):
        return [self.cs[int(i)] or "" for i in idx]

    def expected_stream(self, keep) -> bytes:
        return self.raw[:self.header_end] + b"".join(r.bytes for r, k in zip(self.records, keep) if k)

    def write(self, keep, path) -> int:
        write_bgzf(path, self.expected_stream(keep), block=0xff00)
        return int(np.count_nonzero(np.asarray(keep)))


# ---------------------------------------------------------------- pysam stand-in
class AlignedSegment:
    def __init__(self, rec: Record):
        self._r = rec
        self.query_name, self.flag, self.reference_id = rec.query_name, rec.flag, rec.ref

    is_unmapped = property(lambda s: bool(s.flag & 0x4))
    is_secondary = property(lambda s: bool(s.flag & 0x100))
    is_supplementary = property(lambda s: bool(s.flag & 0x800))
    query_length = property(lambda s: s._r.l_seq)
    reference_name = property(lambda s: s._r._refs[s.reference_id][0] if s.reference_id >= 0 else None)
    cigartuples = property(lambda s: list(s._r.cigar) if s._r.cigar else None)

    @property
    def reference_length(self):
        return None if self.is_unmapped else self._r.reference_length

    def _first(self, tag):
        for t, ty, val, _ in self._r.tags():
            if t == tag:
                return ty, val
        return None

    def has_tag(self, tag):
        return self._first(tag) is not None

    def get_tag(self, tag):
        hit = self._first(tag)
        if hit is None:
            raise KeyError("tag '%s' not present" % tag)
        return hit[1]


class AlignmentFile:
    def __init__(self, path, mode="rb", template=None):
        self._mode, self._path = mode, path
        if mode == "rb":
            self._raw = gzip.decompress(open(path, "rb").read())
            _, self._start, recs = decode(self._raw)
            self._segs = [AlignedSegment(r) for r in recs]
        else:
            assert mode == "wb" and template is not None
            self._out = bytearray(template._raw[:template._start])

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
        return False

    def close(self):
        if self._mode == "wb" and self._out is not None:
            write_bgzf(self._path, bytes(self._out), block=0xff00)
            self._out = None

    def __iter__(self):
        return iter(self._segs)

    def write(self, seg):
        self._out += seg._r.bytes


def pysam_standin():
    m = types.ModuleType("pysam")
    m.AlignmentFile, m.AlignedSegment = AlignmentFile, AlignedSegment
    m.libcalignedsegment = types.SimpleNamespace(AlignedSegment=AlignedSegment)
    return m
