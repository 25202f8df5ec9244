"""Plain Python reference for the SAM-text open (policy O9) -- TEST INFRASTRUCTURE ONLY.

encode(sam_text) -> (raw, roff): the inflated BAM that `samtools sort` of the text holds, written from the SAM
specification (§1.4 the mandatory fields, §1.5 the aux fields, §4.2 the BAM layout, §5.3 reg2bin) and the rules the issue
of §9f lists, independently of csrc/sam_text.h: str.split, int(), struct.pack and sorted(..., key=...) (Python's sort is
stable).  Refused is raised for what the library refuses, with the code's name, the 1-based line and the field.  The
bytes decode with bam_ref.decode.
"""
from __future__ import annotations

import struct

SEQ_CODES = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"
FIELDS = ["QNAME", "FLAG", "RNAME", "POS", "MAPQ", "CIGAR", "RNEXT", "PNEXT", "TLEN", "SEQ", "QUAL"]


class Refused(Exception):
    def __init__(self, code, line, field, what=""):
        super().__init__("%s line %d: %s: %s" % (code, line, field, what))
        self.code, self.line, self.field = code, line, field


def _digits(s: bytes, most=10) -> bool:
    return 0 < len(s) <= most and all(48 <= b <= 57 for b in s)


def header(lines):
    """(BAM text, [(name, length)]) of the '@' lines (each without its '\\n')"""
    out, refs, have_hd = [], [], False
    for no, line in enumerate(lines, 1):
        f = line.split(b"\t")
        if f[0] == b"@HD" and not have_hd:
            have_hd = True
            kept = [x for x in f[1:] if not x.startswith(b"GO:")]
            kept = [b"SO:coordinate" if x.startswith(b"SO:") else x for x in kept]
            if b"SO:coordinate" not in kept:
                kept.append(b"SO:coordinate")
            line = b"\t".join([b"@HD"] + kept)
        if f[0] == b"@SQ":
            sn = [x[3:] for x in f[1:] if x.startswith(b"SN:")]
            ln = [x[3:] for x in f[1:] if x.startswith(b"LN:")]
            if not sn or not ln or not sn[0] or not _digits(ln[0]) or not 1 <= int(ln[0]) <= 2 ** 31 - 1:
                raise Refused("EFORMAT", no, "@SQ")
            if sn[0] in [n for n, _ in refs]:
                raise Refused("EFORMAT", no, "@SQ", "duplicate")
            refs.append((sn[0], int(ln[0])))
        out.append(line + b"\n")
    text = b"".join(out)
    if not have_hd:
        text = b"@HD\tVN:1.6\tSO:coordinate\n" + text
    return text, refs


def reg2bin(beg, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def _aux(field: bytes, no):
    if len(field) < 5 or field[2:3] != b":" or field[4:5] != b":":
        raise Refused("EFORMAT", no, "aux")
    tag, ty, val = field[:2], field[3:4], field[5:]
    if ty == b"A":
        if len(val) != 1:
            raise Refused("EFORMAT", no, "aux")
        return tag + b"A" + val
    if ty == b"i":
        body = val[1:] if val[:1] == b"-" else val
        if not _digits(body):
            raise Refused("EFORMAT", no, "aux")
        v = int(val)
        if not -2 ** 31 <= v <= 2 ** 32 - 1:
            raise Refused("EFORMAT", no, "aux")
        if v < 0:
            code = "c" if v >= -128 else "s" if v >= -32768 else "i"
        else:
            code = "C" if v <= 255 else "S" if v <= 65535 else "I"
        return tag + code.encode() + struct.pack("<" + {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}[code], v)
    if ty == b"f":
        if not val:
            raise Refused("EFORMAT", no, "aux")
        return tag + b"f" + struct.pack("<f", float(val))
    if ty in (b"Z", b"H"):
        return tag + ty + val + b"\0"
    raise Refused("EFORMAT", no, "aux", "type %r" % ty)


def record(line: bytes, no, tid_of):
    """(sort key, record bytes with block_size) of one record line"""
    if not line:
        raise Refused("EFORMAT", no, "line", "empty")
    f = line.split(b"\t")
    if len(f) < 11:
        raise Refused("EFORMAT", no, "line", "fewer than 11 fields")
    for k in range(11):
        if not f[k]:
            raise Refused("EFORMAT", no, FIELDS[k], "empty")
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
    if len(qname) > 254:
        raise Refused("EFORMAT", no, "QNAME")

    def number(text, field, top, signed=False):
        body = text[1:] if signed and text[:1] == b"-" else text
        if not _digits(body) or not (-top - 1 if signed else 0) <= int(text) <= top:
            raise Refused("EFORMAT", no, field)
        return int(text)

    def ref_id(name, field, same=None):
        if name == b"*":
            return -1
        if name == b"=" and same is not None:
            return same
        if name not in tid_of:
            raise Refused("EFORMAT", no, field, "unknown reference name '%s'" % name.decode("latin-1"))
        return tid_of[name]

    flag = number(flag, "FLAG", 65535)
    tid = ref_id(rname, "RNAME")
    pos = number(pos, "POS", 2 ** 31 - 1) - 1
    mapq = number(mapq, "MAPQ", 255)
    ops = []
    if cigar != b"*":
        run = b""
        for b in cigar:
            ch = bytes([b])
            if ch.isdigit():
                run += ch
                continue
            if ch.decode("latin-1") not in CIGAR_OPS or not _digits(run, 9) or not 1 <= int(run) <= 2 ** 28 - 1:
                raise Refused("EFORMAT", no, "CIGAR")
            ops.append((CIGAR_OPS.index(ch.decode()), int(run)))
            run = b""
        if run:
            raise Refused("EFORMAT", no, "CIGAR")
        if len(ops) > 65535:
            raise Refused("ERANGE", no, "CIGAR")
    ntid = ref_id(rnext, "RNEXT", same=tid)
    npos = number(pnext, "PNEXT", 2 ** 31 - 1) - 1
    tlen = number(tlen, "TLEN", 2 ** 31 - 1, signed=True)
    bases = b"" if seq == b"*" else seq
    if qual == b"*":
        quals = b"\xff" * len(bases)
    else:
        if len(qual) != len(bases):
            raise Refused("EFORMAT", no, "QUAL")
        quals = bytes((b - 33) & 0xff for b in qual)
    codes = [SEQ_CODES.index(chr(b).upper()) if chr(b).upper() in SEQ_CODES else 15 for b in bases]
    packed = bytes((codes[i] << 4) | (codes[i + 1] if i + 1 < len(codes) else 0) for i in range(0, len(codes), 2))
    rlen = sum(ln for op, ln in ops if op in (0, 2, 3, 7, 8)) if not flag & 4 and ops else 1
    bin_ = reg2bin(pos, pos + (rlen or 1)) & 0xffff
    aux = b"".join(_aux(x, no) for x in f[11:])
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(qname) + 1, mapq, bin_, len(ops), flag, len(bases), ntid, npos, tlen)
    body += qname + b"\0" + b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in ops) + packed + quals + aux
    if len(body) + 4 > 2 ** 31 - 1:
        raise Refused("ERANGE", no, "line")
    key = (tid if tid >= 0 else 2 ** 32, pos + 1, (flag >> 4) & 1)
    return key, struct.pack("<i", len(body)) + body


def split(sam_text: bytes):
    """(header lines, record lines): a last line without '\\n' is a line, an empty line stays (and is refused)"""
    lines = sam_text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    n = 0
    while n < len(lines) and lines[n].startswith(b"@"):
        n += 1
    return lines[:n], lines[n:]


def encode(sam_text):
    """(raw, roff) of the coordinate-sorted BAM of `sam_text` (bytes or str); Refused for what the library refuses"""
    if isinstance(sam_text, str):
        sam_text = sam_text.encode("latin-1")
    head, lines = split(sam_text)
    text, refs = header(head)
    tid_of = {name: k for k, (name, _) in enumerate(refs)}
    raw = bytearray(b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs)))
    for name, ln in refs:
        raw += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", ln)
    recs = [record(line, len(head) + k + 1, tid_of) for k, line in enumerate(lines)]
    roff = []
    for _, rec in sorted(recs, key=lambda kr: kr[0]):
        roff.append(len(raw))
        raw += rec
    return bytes(raw), roff
