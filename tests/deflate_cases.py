"""The inputs of the DEFLATE encoder's tests (tests/test_bgzf_deflate_cpu.py, tests/test_gpu_bgzf_deflate.py), seeded:
the smallest shapes at which the encoder of csrc/deflate.h can go wrong.  Each case is a byte string that the encoder
cuts into 0xff00-byte blocks.  Built once per process and never changed."""
import fractions
import functools
import heapq
import random
import struct

import bam_ref
from inflate_cases import EOF_BLOCK, SEED  # noqa: F401

BLOCK = 0xff00


def bam_shaped():
    refs = [["regA", 760], ["regB", 720], ["regC", 700]]
    recs = []
    for i in range(300):
        ref = i % 3
        ln = refs[ref][1] - (i % 7) * (i % 3)
        recs.append({"name": "read%d_%d" % (i, 1 + i % 9), "flag": (0, 16, 0, 0x100)[i % 4], "ref": ref, "pos": i % 5,
                     "cigar": "%dS%dM%dI%dM" % (i % 4 + 1, ln // 2, i % 3 + 1, ln - ln // 2),
                     "tags": [["NM", "i", i % 11], ["cs", "Z", ":%d*ag:%d" % (10 + i % 13, 20 + i % 5)]]})
    return bam_ref.build_raw(refs, recs)


def fibonacci_text(k=14, fillers=32, each=1900):
    """Literal counts 1, 2, 3, 5, 8, ... over 14 symbols (the end-of-block symbol is the other 1 of the sequence), so
    that the unlimited Huffman depth exceeds 15 -- under 32 filler symbols of 1,900 each, placed so that no 4 bytes of
    the text occur twice.  A Fibonacci text alone repeats its 4-byte strings (its entropy is 2.2 bits a symbol), the
    tokeniser then finds matches and the literal counts are no longer Fibonacci; the fillers are each more frequent
    than the whole chain, so they leave its depth alone and add theirs on top (20 in all, huffman_depth below)."""
    rng = random.Random(SEED + 7)
    counts, a, b = [], 1, 2
    for _ in range(k):
        counts.append(a)
        a, b = b, a + b
    return no_repeat_order([s for s, n in enumerate(counts) for _ in range(n)] +
                           [k + f for f in range(fillers) for _ in range(each)], rng)


def no_repeat_order(pool, rng, window=200):
    """the byte values of `pool` in an order in which no 4 bytes occur twice, so that the tokeniser finds no match and
    the literal counts are the pool's"""
    for attempt in range(50):  # the last few bytes may find no place: shuffle again
        left = list(pool)
        rng.shuffle(left)
        out, seen = bytearray(), set()
        while left:
            for tries in range(400):
                j = len(left) - 1 - (rng.randrange(min(len(left), window)) if tries else 0)
                g = bytes(out[-3:]) + bytes([left[j]])
                if len(g) < 4 or g not in seen:
                    break
            else:
                break
            seen.add(g)
            out.append(left[j])
            left[j] = left[-1]
            left.pop()
        if not left:
            return bytes(out)
    raise AssertionError("no order without a repeated 4-byte string")


def code_length_plan():
    """symbols per code length 2..12 of a complete code: Fibonacci numbers, plus the few symbols that bring the Kraft
    sum to 1"""
    n = {2: 1, 3: 1, 4: 2, 5: 3, 6: 5, 7: 8, 8: 13, 9: 21, 10: 34, 11: 55, 12: 89}
    rest = 1 - sum(fractions.Fraction(c, 2 ** l) for l, c in n.items())
    for l in range(1, 13):
        if rest >= fractions.Fraction(1, 2 ** l):
            n[l] = n.get(l, 0) + 1
            rest -= fractions.Fraction(1, 2 ** l)
    assert rest == 0
    return n


def code_length_text():
    """4,095 literals whose counts are powers of two, 2^(12 - l) for a symbol of code_length_plan()'s length l (the
    end-of-block symbol is one of the rarest), so that the Huffman code has exactly those lengths; the number of codes
    per length then follows Fibonacci numbers, and the code-length code over them needs more than 7 bits.  No four
    adjacent byte values have the same length (no repeat symbol 16 thins the counts) and no 4 bytes occur twice."""
    rng = random.Random(SEED + 8)
    lens = [l for l, c in code_length_plan().items() for _ in range(c)]
    lens.remove(12)
    lens += [0] * (256 - len(lens))
    while True:
        rng.shuffle(lens)
        if not any(lens[i] == lens[i + 1] == lens[i + 2] == lens[i + 3] for i in range(253)):
            break
    return no_repeat_order([v for v, l in enumerate(lens) if l for _ in range(2 ** (12 - l))], rng)


def huffman_depth(counts) -> int:
    """the longest code of an unlimited Huffman code of the counts"""
    h = [(c, i, 0) for i, c in enumerate(counts)]
    heapq.heapify(h)
    n = len(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        n += 1
        heapq.heappush(h, (a[0] + b[0], n, max(a[2], b[2]) + 1))
    return h[0][2]


def hash4(b: bytes) -> int:
    """the tokeniser's hash of 4 bytes (csrc/deflate.h hash4)"""
    return (int.from_bytes(b, "little") * 2654435761 & 0xffffffff) >> 20


def far_repeat(rng, dist):
    """300 random bytes, filler, and the same 300 bytes again `dist` after the first.  The tokeniser keeps one
    candidate per hash value, so the filler is chosen byte by byte to leave the hash values of the 300 bytes' 4-byte
    strings alone: the candidate of every position of the second copy is then the first copy's."""
    blk = bytes(rng.randrange(256) for _ in range(300))
    keep = {hash4(blk[i:i + 4]) for i in range(297)}
    out = bytearray(blk)
    while len(out) < dist:
        c = rng.randrange(256)
        if hash4(bytes(out[-3:]) + bytes([c])) not in keep:
            out.append(c)
    for i in range(1, 4):  # the 4-byte strings across the seam
        assert hash4(bytes(out[-i:]) + blk[:4 - i]) not in keep
    return bytes(out) + blk + b"tail"


@functools.lru_cache(maxsize=None)
def cases():
    """name -> bytes, in a fixed order"""
    rng = random.Random(SEED + 5)

    def rnd(n):
        return bytes(rng.randrange(256) for _ in range(n))

    def text(n):  # compressible: words over a small alphabet
        words = [bytes(rng.choice(b"ACGTN:*=") for _ in range(rng.randrange(3, 12))) for _ in range(40)]
        out = bytearray()
        while len(out) < n:
            out += rng.choice(words)
        return bytes(out[:n])

    c = {}
    for n in (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 257, 258, 259, 260, 0xfeff, 0xff00):
        c[f"len_{n}"] = text(n)
    c["zeros"] = b"\0" * BLOCK
    for period in (1, 2, 3, 7, 63, 64, 65, 257, 258, 259):  # matches that overlap themselves and start inside a step
        c[f"period_{period}"] = (rnd(period) * (3000 // period + 2))[:3000 + period]
    # the only repeat at distance exactly 32768, and at 32769 (which is no match)
    c["dist_32768"] = far_repeat(random.Random(SEED + 6), 32768)
    c["dist_32769"] = far_repeat(random.Random(SEED + 6), 32769)
    c["random"] = rnd(BLOCK)
    c["all_bytes"] = bytes(range(256))
    c["one_value"] = b"\xa5" * 5000
    c["two_values"] = bytes(rng.choice(b"\x00\xff") for _ in range(5000))
    c["bam"] = bam_shaped()
    c["fibonacci"] = fibonacci_text()
    c["code_lengths"] = code_length_text()
    c["three_blocks_text"] = text(3 * BLOCK + 17)
    c["three_blocks_random"] = rnd(3 * BLOCK + 17)
    c["everything"] = b"".join(c.values())  # the seams between the cases fall inside blocks
    return c


def n_blocks(data: bytes) -> int:
    return -(-len(data) // BLOCK)


def write_case_file(path, datas) -> None:
    """what tools/deflate_check_main.cpp reads: u32 count, then per case u32 bytes and the bytes"""
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(datas)))
        for d in datas:
            fh.write(struct.pack("<I", len(d)) + d)


def members(data: bytes):
    """the gzip members of a BGZF byte string"""
    out, o = [], 0
    while o < len(data):
        assert data[o:o + 4] == b"\x1f\x8b\x08\x04" and data[o + 10:o + 16] == b"\x06\0BC\x02\0", o
        bsize = struct.unpack_from("<H", data, o + 16)[0] + 1
        out.append(data[o:o + bsize])
        o += bsize
    assert o == len(data)
    return out
