"""The BGZF blocks of the DEFLATE decoder's tests (tests/test_bgzf_inflate_cpu.py, tests/test_gpu_bgzf_inflate.py),
seeded.  Python's zlib is the reference throughout: the expected bytes come from zlib.decompressobj(-15), and a block
counts as accepted exactly when that object reaches eof with exactly ISIZE bytes out of decompress(payload, ISIZE + 1)
-- the host reader's rule (io::inflate_bgzf: Z_STREAM_END with avail_out == 0, input left over ignored).

valid()    name -> (payload, data): one DEFLATE stream each, every encoding, flush and match shape the decoder has a path for
damaged()  a list of Block: per valid payload of at least 8 bytes 24 single-bit flips (a third in the first 48 bytes, a
           third anywhere, a third in the last 16), truncations by 1, by 2 and by half, ISIZE - 1 and ISIZE + 1
Both are built once per process and never changed."""
import collections
import functools
import random
import struct
import zlib

SEED = 20261020
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
Block = collections.namedtuple("Block", "name kind payload isize expect")  # expect: zlib's bytes, None = rejected


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=(), flush=zlib.Z_FULL_FLUSH):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, prev = b"", 0
    for f in flush_at:
        out += c.compress(data[prev:f]) + c.flush(flush)
        prev = f
    return out + c.compress(data[prev:]) + c.flush()


def reference(payload: bytes, isize: int):
    """zlib's bytes where the host reader accepts the block, else None"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload, isize + 1)
    except zlib.error:
        return None
    return out if d.eof and len(out) == isize else None


def frame(payload: bytes, isize: int, crc: int = 0) -> bytes:
    """one BGZF block around a DEFLATE stream (the CRC32 is never checked)"""
    bsize = len(payload) + 26
    assert bsize <= 65536, bsize
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", bsize - 1) + payload +
            struct.pack("<II", crc, isize))


@functools.lru_cache(maxsize=None)
def valid():
    rng = random.Random(SEED)

    def reads(n):
        return bytes(rng.choice(b"ACGT") for _ in range(n))

    def recordish(n):  # record-like bytes: binary header, name, ACGT run, 0xff run
        out = bytearray()
        while len(out) < n:
            out += (bytes(rng.randrange(256) for _ in range(36)) + b"read%07d\0" % rng.randrange(10 ** 7) +
                    reads(200)[:rng.randrange(50, 200)] + b"\xff" * rng.randrange(1, 300))
        return bytes(out[:n])

    cases = {"empty_stored": (deflate(b"", 0), b""), "one_byte_fixed": (deflate(b"A", 6, zlib.Z_FIXED), b"A")}
    for n in (1, 63, 64, 65, 257, 258, 259, 4096, 0xff00, 65536):
        d = recordish(n)
        cases[f"dyn_{n}"] = (deflate(d, 6), d)
        cases[f"fixed_{n}"] = (deflate(d, 6, zlib.Z_FIXED), d)
        if n <= 0xff00:  # 65536 stored bytes do not fit a block
            cases[f"stored_{n}"] = (deflate(d, 0), d)
    d = recordish(30000)
    cases["huffman_only"] = (deflate(d, 6, zlib.Z_HUFFMAN_ONLY), d)
    cases["level1"] = (deflate(d, 1), d)
    cases["level9"] = (deflate(d, 9), d)
    cases["full_flush_x3"] = (deflate(d, 6, flush_at=(1, 9999, 20000)), d)
    cases["sync_flush_x3"] = (deflate(d, 6, flush_at=(7, 10000, 29999), flush=zlib.Z_SYNC_FLUSH), d)
    for period in (1, 2, 3, 7, 63, 64, 65, 257, 258, 259):  # overlapping matches of every alignment
        d = (reads(period) * (70000 // period + 1))[:60000]
        cases[f"period_{period}"] = (deflate(d, 9), d)
    blk = bytes(rng.randrange(256) for _ in range(300))
    d = blk + bytes(rng.randrange(256) for _ in range(32768 - 300)) + blk + b"tail"
    cases["dist_32768"] = (deflate(d, 9), d)
    d = b"\0" * 65536
    cases["zeros_65536"] = (deflate(d, 9), d)
    for k, (c, d) in cases.items():
        assert len(c) + 26 <= 65536, k
    return cases


def valid_blocks():
    return [Block(k, "valid", c, len(d), reference(c, len(d))) for k, (c, d) in valid().items()]


@functools.lru_cache(maxsize=None)
def damaged():
    rng = random.Random(SEED + 1)
    out = []
    for k, (c, d) in valid().items():
        if len(c) < 8:
            continue
        for j in range(24):
            b = bytearray(c)
            if j % 3 == 0:
                pos = rng.randrange(min(len(b), 48))  # headers and code lengths
            elif j % 3 == 1:
                pos = rng.randrange(len(b))
            else:
                pos = len(b) - 1 - rng.randrange(min(len(b), 16))  # the end-of-block area
            b[pos] ^= 1 << rng.randrange(8)
            out.append(Block(f"{k}/flip{j}@{pos}", "flip", bytes(b), len(d), reference(bytes(b), len(d))))
        for cut in (1, 2, len(c) // 2):
            out.append(Block(f"{k}/cut{cut}", "cut", c[:-cut], len(d), reference(c[:-cut], len(d))))
        out.append(Block(f"{k}/isize-1", "isize", c, len(d) - 1, reference(c, len(d) - 1)))
        out.append(Block(f"{k}/isize+1", "isize", c, len(d) + 1, reference(c, len(d) + 1)))
    return tuple(out)


def bgzf_file(blocks) -> bytes:
    """the blocks framed one after another, and the 28-byte EOF block"""
    return b"".join(frame(b.payload, b.isize) for b in blocks) + EOF_BLOCK


def write_case_file(path, blocks) -> None:
    """what tools/inflate_check_main.cpp reads: per block `u32 payload bytes, u32 ISIZE, u32 accepted`, the payload,
    then zlib's ISIZE bytes where accepted"""
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(blocks)))
        for b in blocks:
            fh.write(struct.pack("<III", len(b.payload), b.isize, int(b.expect is not None)) + b.payload)
            if b.expect is not None:
                fh.write(b.expect)
