"""The plain reference of the fused region split + UMI extraction (row f4+f1) and its seeded inputs.

TEST INFRASTRUCTURE ONLY.  The reference is a composition of two pieces that reference-made fixtures already pin:
oracle/region_split.split_records (the record loop of region_split.py:219-333) feeds, cluster by cluster, the FASTA
entries it would have written to oracle/extract.extract_records (extract_umis.py:189-267); a record without a sequence
is the text None, as print() writes it.  The inputs are reads with planted UMIs (planted_records), so that the comparison
cannot pass on files with nothing found: conditions() states what a test asserts of them.
"""
import re

import bam
import extract as oex
import region_split as ors

UMI_FWD = "TTTVVVVTTVVVVTTVVVVTTVVVVTTT"
UMI_REV = "AAABBBBAABBBBAABBBBAABBBBAAA"
IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "M": "AC", "R": "AG", "W": "AT", "S": "CG", "Y": "CT", "K": "GT",
         "V": "ACG", "H": "ACT", "D": "AGT", "B": "CGT", "N": "ACGT"}
WIDE = "ACGTNRYMK"
_COMP = str.maketrans("ACGT", "TGCA")


def stored(forward: str, reverse: bool) -> str:
    """the sequence a BAM record stores for a read whose forward text is `forward`"""
    return forward[::-1].translate(_COMP) if reverse else forward


def _instance(rng, pattern, edits, alpha):
    """an instance of the IUPAC pattern with `edits` random substitutions, deletions or insertions"""
    s = [rng.choice(IUPAC[ch]) for ch in pattern]
    for _ in range(edits):
        kind = rng.randrange(3)
        if kind == 0 and s:
            s[rng.randrange(len(s))] = rng.choice(alpha)
        elif kind == 1 and s:
            del s[rng.randrange(len(s))]
        else:
            s.insert(rng.randint(0, len(s)), rng.choice(alpha))
    return "".join(s)


def planted_read(rng, a5, a3, k, fwd=UMI_FWD, rev=UMI_REV):
    """5' flank, an edited instance of fwd, a middle, an edited instance of rev, 3' flank: the forward text of a read"""
    alpha = WIDE if rng.random() < 0.15 else "ACGT"
    run = lambda n: "".join(rng.choices(alpha, k=n))  # noqa: E731
    return (run(rng.choice([0, 1, rng.randint(0, a5)])) + _instance(rng, fwd, rng.randint(0, k + 2), alpha)
            + run(rng.choice([0, 3, rng.randint(0, 120)])) + _instance(rng, rev, rng.randint(0, k + 2), alpha)
            + run(rng.choice([0, 1, rng.randint(0, a3)])))


def planted_records(rng, n, regions, a5, a3, k, fwd=UMI_FWD, rev=UMI_REV, prefix="p"):
    """n records with planted UMIs, each spanning its whole region (so that it is never short) on either strand; the
    reverse ones are stored reverse-complemented, as an aligner stores them"""
    out = []
    for i in range(n):
        ref = rng.randrange(len(regions))
        reverse = rng.random() < 0.5
        out.append(dict(name="%s%d" % (prefix, i), flag=16 * reverse, ref=ref, pos=0, cigar=[("M", regions[ref][1])],
                        seq=stored(planted_read(rng, a5, a3, k, fwd, rev), reverse)))
    return out


def segments(refs, records):
    return [bam.AlignedSegment(refs, r["ref"], r["pos"], r["flag"], r["name"],
                               [(bam.CIGAR_OPS.index(op), ln) for op, ln in r["cigar"]], r["seq"] or None)
            for r in records]


def fasta_entries(text):
    """(name, sequence) of the two-line records split_records builds"""
    lines = text.split("\n")
    assert lines[-1] == "" and len(lines) % 2 == 1
    return [(lines[i][1:], lines[i + 1]) for i in range(0, len(lines) - 1, 2)]


def compose(refs, regions, clusters, records, ov, s5, s3, a5, a3, k, fwd=UMI_FWD, rev=UMI_REV):
    """The two reference loops one after the other.  Returns (counts, reads per cluster, detected regions, {file name:
    text}, {cluster: records written}, the kept entries); split_records' KeyError propagates, before any extraction."""
    counts, per_cluster, texts, detected = ors.split_records(segments(refs, records), dict(regions), clusters, ov, s5, s3)
    files, umis, kept = {}, {}, []
    for c, text in texts.items():
        entries = fasta_entries(text)
        kept += entries
        files["region_cluster%d_detected_umis.fasta" % c], umis[c] = oex.extract_records(entries, a5, a3, k, fwd, rev)
    return counts, per_cluster, detected, files, umis, kept


_FIELDS = re.compile(r"^>(.*);strand=(.*);umi_fwd_dist=(\d+);umi_rev_dist=(\d+);umi_fwd_seq=", re.S)


def conditions(files, n_kept, k):
    """What the inputs must be for a comparison to mean something: at least 30 % of the kept reads with both UMIs and
    at least 30 % without, both strands at least 40 % of the found, every distance 0..k present.  Returns the counts."""
    found = [_FIELDS.match(rec) for text in files.values() for rec in re.findall(r">[^\n]*\n[^\n]*\n", text)]
    assert all(found)
    n = len(found)
    strands = {s: sum(m.group(2) == s for m in found) for s in "+-"}
    dists = {int(m.group(g)) for m in found for g in (3, 4)}
    assert 0.3 * n_kept <= n <= 0.7 * n_kept, (n, n_kept)
    assert min(strands.values()) >= 0.4 * n, strands
    assert dists >= set(range(k + 1)), dists
    return n, strands, dists
