"""Python restatement of policy O8: the `seqkit stat -a` table of a list of parsed FASTQ
records, for the tests to compare against.

Nothing here is shared with the library.  The records come from fastq_filter_ref.parse; the length statistics are read
off a sorted list of the lengths (the library walks a histogram); the counts and the expected-error sum are Python
integers (numpy only counts how often each byte value occurs in a record); the text is built with Python's own number
formatting.
"""
from __future__ import annotations

import math

import numpy as np

import fastq_filter_ref as ref

COLUMNS = ["file", "format", "type", "num_seqs", "sum_len", "min_len", "avg_len", "max_len", "Q1", "Q2", "Q3",
           "sum_gap", "N50", "N50_num", "Q20(%)", "Q30(%)", "AvgQual", "GC(%)", "sum_n"]
DNA = set(b"ACGTRYSWKMBDHVN")


def seq_type(seq: bytes) -> str:
    """O8f, from one record's letters"""
    letters = set(bytes(seq).upper()) & set(range(ord("A"), ord("Z") + 1))
    if letters <= DNA:
        return "DNA"
    if ord("U") in letters and ord("T") not in letters:
        return "RNA"
    return "Protein"


def median(v: list[int]) -> float:
    n = len(v)
    return float(v[n // 2]) if n % 2 else (v[n // 2 - 1] + v[n // 2]) / 2


def numbers(recs, ascii_=33) -> dict:
    """O8c-O8f of (label, sequence, quality) records"""
    _, fx = ref.tables(ascii_, 0, 93)
    n = len(recs)
    d = dict(type=seq_type(recs[0][1]) if recs else "DNA", num_seqs=n, sum_len=0, min_len=0, max_len=0, avg_len=0.0,
             q1=0.0, q2=0.0, q3=0.0, sum_gap=0, n50=0, n50_num=0, n_q20=0, n_q30=0, n_gc=0, sum_n=0, ee_fx=0,
             q20_pct=0.0, q30_pct=0.0, avg_qual=0.0, gc_pct=0.0)
    if n == 0:
        return d
    lens = sorted(len(s) for _, s, _ in recs)
    total = sum(lens)
    d.update(sum_len=total, min_len=lens[0], max_len=lens[-1], avg_len=total / n)
    h = n // 2
    d["q2"] = median(lens)
    d["q1"] = median(lens[:h]) if h else float(lens[0])
    d["q3"] = median(lens[n - h:]) if h else float(lens[0])
    cum = 0
    for k, ln in enumerate(reversed(lens)):
        cum += ln
        if 2 * cum >= total:
            d["n50"], d["n50_num"] = ln, k + 1
            break
    for _, s, q in recs:  # per byte value: how often it occurs (Python integers from here on)
        qn = [int(c) for c in np.bincount(np.frombuffer(q, np.uint8), minlength=256)]
        d["n_q20"] += sum(c for b, c in enumerate(qn) if b - ascii_ >= 20)
        d["n_q30"] += sum(c for b, c in enumerate(qn) if b - ascii_ >= 30)
        d["ee_fx"] += sum(c * fx[b] for b, c in enumerate(qn))
        d["n_gc"] += sum(s.count(bytes([b])) for b in b"GCgc")
        d["sum_n"] += sum(s.count(bytes([b])) for b in b"Nn")
        d["sum_gap"] += sum(s.count(bytes([b])) for b in b"-. ")
    if total > 0:
        d["q20_pct"] = 100.0 * d["n_q20"] / total
        d["q30_pct"] = 100.0 * d["n_q30"] / total
        d["gc_pct"] = 100.0 * d["n_gc"] / total
        if d["ee_fx"] > 0:
            d["avg_qual"] = 0.0 - 10.0 * math.log10(math.ldexp(float(d["ee_fx"]), -ref.FX_SHIFT) / total)
    return d


def table(path: str, recs, ascii_=33) -> bytes:
    """O8a / O8b: the two lines of the table"""
    return table_from_numbers(path, numbers(recs, ascii_))


def table_from_numbers(path: str, d: dict) -> bytes:
    vals = [path, "FASTQ", d["type"], f"{d['num_seqs']:,}", f"{d['sum_len']:,}", f"{d['min_len']:,}",
            f"{d['avg_len']:,.1f}", f"{d['max_len']:,}", f"{d['q1']:,.1f}", f"{d['q2']:,.1f}", f"{d['q3']:,.1f}",
            f"{d['sum_gap']:,}", f"{d['n50']:,}", f"{d['n50_num']:,}", f"{d['q20_pct']:.2f}", f"{d['q30_pct']:.2f}",
            f"{d['avg_qual']:.2f}", f"{d['gc_pct']:.2f}", f"{d['sum_n']:,}"]
    head, data = [], []
    for k, (name, v) in enumerate(zip(COLUMNS, vals)):
        w = max(len(name), len(v))
        head.append(name.ljust(w) if k < 3 else name.rjust(w))
        data.append(v.ljust(w) if k < 3 else v.rjust(w))
    return ("  ".join(head) + "\n" + "  ".join(data) + "\n").encode()


def tables(data: bytes, in_path: str, out_path: str, ascii_=33, qmin=0, qmax=93, minlen=1, maxlen=-1, maxee=-1.0,
           rate=-1.0):
    """(before table, after table, numbers before, numbers after) of a file's bytes under the filter's options: the
    records read and the records policy O7d keeps"""
    recs = ref.parse(data)
    p, _ = ref.tables(ascii_, qmin, qmax)
    kept = [r for r in recs if ref.decide(len(r[1]), ref.ee_seq(p, r[2]), minlen, maxlen, maxee, rate) == 0]
    return table(in_path, recs, ascii_), table(out_path, kept, ascii_), numbers(recs, ascii_), numbers(kept, ascii_)
