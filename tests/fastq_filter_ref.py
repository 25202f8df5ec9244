"""Python restatement of the fastq_filter drop-in's policies O7a-O7d, for the tests to compare against.

Nothing here is shared with the library: records are parsed line by line, the expected error is the left-to-right
double sum of pow(10, -q/10) (numpy's cumsum adds sequentially), the decision is the four checks in vsearch's order,
and the fixed-point sum uses Python integers.
"""
from __future__ import annotations

import math

import numpy as np

FX_SHIFT = 40


class Malformed(ValueError):
    def __init__(self, msg, records):
        super().__init__(msg)
        self.records = records  # the records before the malformed one


def parse(data: bytes) -> list[tuple[bytes, bytes, bytes]]:
    """O7a: (label, sequence, quality) per record; multi-line records joined, '\\r' stripped at line ends."""
    lines = [x[:-1] if x.endswith(b"\r") else x for x in data.split(b"\n")]
    if lines and lines[-1] == b"":
        lines.pop()
    out, i = [], 0
    while i < len(lines):
        if lines[i] == b"":
            i += 1
            continue
        if not lines[i].startswith(b"@"):
            raise Malformed("no @", out)
        hdr = lines[i][1:]
        cut = min([k for k in (hdr.find(b" "), hdr.find(b"\t")) if k >= 0] or [len(hdr)])
        label = hdr[:cut]
        i += 1
        seq = []
        while i < len(lines) and not lines[i].startswith(b"+"):
            seq.append(lines[i])
            i += 1
        if i >= len(lines):
            raise Malformed("no +", out)
        i += 1
        s = b"".join(seq)
        q = b""
        while i < len(lines) and len(q) < len(s):
            q += lines[i]
            i += 1
        if len(q) != len(s):
            raise Malformed("length mismatch", out)
        out.append((label, s, q))
    return out


def tables(ascii_=33, qmin=0, qmax=93):
    """(p, fx) indexed by the raw byte; 0 outside [qmin, qmax]"""
    p = np.zeros(256, np.float64)
    fx = [0] * 256
    for b in range(max(0, ascii_ + qmin), min(255, ascii_ + qmax) + 1):
        q = b - ascii_
        p[b] = math.pow(10.0, -q / 10.0)
        fx[b] = round(p[b] * 2 ** FX_SHIFT)
    return p, fx


def ee_seq(p: np.ndarray, qual: bytes) -> float:
    """O7c: the left-to-right double sum"""
    if not qual:
        return 0.0
    return float(np.cumsum(p[np.frombuffer(qual, np.uint8)])[-1])


def ee_fx(fx: list[int], qual: bytes) -> int:
    return sum(fx[b] for b in qual)


def decide(n: int, ee: float, minlen=1, maxlen=-1, maxee=-1.0, rate=-1.0) -> int:
    """O7d: 0 kept, 1 short, 2 long, 3 maxee, 4 maxee_rate"""
    if n < minlen:
        return 1
    if maxlen >= 0 and n > maxlen:
        return 2
    if maxee >= 0 and ee > maxee:
        return 3
    if rate >= 0 and n > 0 and ee / n > rate:
        return 4
    return 0


def in_band(n: int, efx: int, minlen=1, maxlen=-1, maxee=-1.0, rate=-1.0) -> bool:
    """the guard band of DESIGN.md §9a around each given threshold, for records the length checks let through"""
    if n < minlen or (maxlen >= 0 and n > maxlen):
        return False
    ee = efx * 2.0 ** -FX_SHIFT
    base = n * 2.0 ** -41 + 2 * n * 2.0 ** -53 * ee
    if maxee >= 0:
        if abs(ee - maxee) <= base + 4 * 2.0 ** -52 * maxee:
            return True
        if ee > maxee:
            return False
    if rate >= 0 and n > 0:
        thr = rate * n
        return abs(ee - thr) <= base + 4 * 2.0 ** -52 * thr
    return False


def run(data: bytes, ascii_=33, qmin=0, qmax=93, minlen=1, maxlen=-1, maxee=-1.0, rate=-1.0, stop_at=None):
    """The whole step on a file's bytes: (kept bytes, discarded bytes, counters).  stop_at: only records [0, stop_at)."""
    p, fx = tables(ascii_, qmin, qmax)
    recs = parse(data)[:stop_at]
    kept, disc = [], []
    c = dict(n_input=0, n_kept=0, n_discarded=0, bases_in=0, bases_kept=0, n_short=0, n_long=0, n_maxee=0,
             n_maxee_rate=0, n_in_band=0, ee_in=0.0, ee_kept=0.0)
    names = [None, "n_short", "n_long", "n_maxee", "n_maxee_rate"]
    for label, s, q in recs:
        n = len(s)
        why = decide(n, ee_seq(p, q), minlen, maxlen, maxee, rate)
        efx = ee_fx(fx, q)
        e = float(efx) * 2.0 ** -FX_SHIFT
        c["n_in_band"] += in_band(n, efx, minlen, maxlen, maxee, rate)
        c["n_input"] += 1
        c["bases_in"] += n
        c["ee_in"] += e
        rec = b"@" + label + b"\n" + s + b"\n+\n" + q + b"\n"
        if why == 0:
            kept.append(rec)
            c["n_kept"] += 1
            c["bases_kept"] += n
            c["ee_kept"] += e
        else:
            disc.append(rec)
            c["n_discarded"] += 1
            c[names[why]] += 1
    return b"".join(kept), b"".join(disc), c


def synth_reads(n: int, seed: int, max_len=3000, min_len=0) -> bytes:
    """n seeded reads, lengths min_len..max_len, Gaussian qualities around a per-read mean of Q8-Q25, labels followed
    by comments after a space or a tab"""
    rng = np.random.default_rng(seed)
    out = []
    acgt = np.frombuffer(b"ACGT", np.uint8)
    for i in range(n):
        ln = int(rng.integers(min_len, max_len + 1))
        mean = rng.uniform(8, 25)
        q = np.clip(np.rint(rng.normal(mean, 5.0, ln)), 0, 60).astype(np.uint8) + 33
        s = acgt[rng.integers(0, 4, ln)]
        sep = [b"", b" runid=7 ch=%d" % i, b"\tstart_time=2024"][i % 3]
        out.append(b"@read%d" % i + sep + b"\n" + s.tobytes() + b"\n+\n" + q.tobytes() + b"\n")
    return b"".join(out)
