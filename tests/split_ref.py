"""Plain Python reference for the region split and the name suffix on a BAM session (rows f4b / f6b)
-- TEST INFRASTRUCTURE ONLY.

Session(raw) is bam_ref.Columns (the decoded records and the session's columns) with the two methods of
_lib.BamSession that the round-2 drop-ins call, written from their definitions in include/umiclust.h:
  - split(keep, names, lengths, buckets, bucket_paths, overlap, s5, s3): walks the records in BAM order with the
    reference's own Python comparisons, appends `>{name};strand={+|-}` + forward sequence per kept record, raises
    KeyError(name) at the first primary record without a region or a bucket;
  - name_suffix(): (value, status) of the tail after the last "_".
split_texts is the same walk without files: what each bucket would be appended with.
"""
from __future__ import annotations

import gzip
import os

import numpy as np

import bam_ref

SEQ_CODES = "=ACMGRSVTWYHKDBN"
_COMP = str.maketrans("ACGT", "TGCA")


def forward_sequence(rec) -> str:
    """what the reference prints for a record: the stored bases, reverse-complemented (A C G T only) on the reverse
    strand; `None` for a record that stores none"""
    if rec.l_seq <= 0:
        return "None"
    p = rec.aux - rec.l_seq - (rec.l_seq + 1) // 2
    sb = rec.raw[p:p + (rec.l_seq + 1) // 2]
    seq = "".join(SEQ_CODES[(sb[i // 2] >> (4 * (1 - i % 2))) & 15] for i in range(rec.l_seq))
    return seq[::-1].translate(_COMP) if rec.flag & 16 else seq


def name_suffix(name: str):
    """(value, status): status 1 and the decimal value when the tail is 1..18 ASCII digits, else (0, 0)"""
    tail = name.split("_")[-1]
    if 1 <= len(tail) <= 18 and all(c in "0123456789" for c in tail):
        return int(tail), 1
    return 0, 0


def split_texts(col, keep, names, lengths, buckets, nbuckets, overlap, s5, s3):
    """(counts[4], reads per bucket, detected[len(names)], text per bucket, missing name or None)"""
    length_of = dict(zip(names, lengths))
    bucket_of = dict(zip(names, buckets))
    region_of = {n: r for r, n in enumerate(names)}
    counts = [0, 0, 0, 0]
    per_bucket, detected, texts = [0] * nbuckets, [0] * len(names), [[] for _ in range(nbuckets)]
    for r, rec in enumerate(col.records):
        if keep is not None and not keep[r]:
            continue
        if rec.flag & 4:
            counts[0] += 1
            continue
        if rec.flag & 0x900:
            continue
        counts[1] += 1
        name = col.ref_names[rec.ref] if 0 <= rec.ref < len(col.ref_names) else None
        if name not in length_of:
            return counts, per_bucket, detected, ["".join(t) for t in texts], str(name)
        if rec.reference_length < length_of[name] * overlap:
            counts[2] += 1
            continue
        if rec.l_seq > length_of[name] * (2 - overlap) + (s5 + s3):
            counts[3] += 1
            continue
        b = bucket_of[name]
        if b < 0:
            return counts, per_bucket, detected, ["".join(t) for t in texts], name
        per_bucket[b] += 1
        detected[region_of[name]] = 1
        texts[b].append(">%s;strand=%s\n%s\n" % (rec.query_name, "-" if rec.flag & 16 else "+", forward_sequence(rec)))
    return counts, per_bucket, detected, ["".join(t) for t in texts], None


class Session(bam_ref.Columns):
    def split(self, keep, names, lengths, buckets, bucket_paths, overlap, s5, s3):
        counts, per_bucket, detected, texts, missing = split_texts(self, keep, names, lengths, buckets,
                                                                   len(bucket_paths), overlap, s5, s3)
        for path, text in zip(bucket_paths, texts):
            if text:
                with open(os.fspath(path), "a") as fh:
                    fh.write(text)
        if missing is not None:
            raise KeyError(missing)
        return np.array(counts, np.int64), np.array(per_bucket, np.int64), np.array(detected, np.uint8)

    def name_suffix(self):
        pairs = [name_suffix(r.query_name) for r in self.records]
        return np.array([v for v, _ in pairs], np.int64), np.array([s for _, s in pairs], np.uint8)

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        pass


class Context:
    """stands in for the process's device context where a CPU test runs a drop-in's file form: bam_open alone"""

    def bam_open(self, bam_file, hash_bits=64):
        with open(bam_file, "rb") as fh:
            return Session(gzip.decompress(fh.read()))
