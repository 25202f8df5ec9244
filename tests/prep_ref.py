"""What the load kernel (K1, k_prep_wave) has to produce, in plain Python (test infrastructure, no GPU).

K1 is the first kernel of every clustering call: DUST masking, the 4-bit codes of both strands, the ascending unique
8-mers of both strands, and three things that steer later code -- the batch's "some symbol is not A, C, G, T or U" bit
(the aligner family), the number of records whose output differs from their input, and which records those are (the
cluster-file writer's three branches).  prep() restates all of it on oracle/pyref.py's c4 and revcomp; its DUST and
k-mer loops are pyref.dust / pyref.kmers with one switch per rule added (tests/test_prep_ref_cpu.py shows that with no
switch they equal pyref and the C oracle on every case of tests/prep_cases.py, and that a flipped switch changes the
output of at least one case, so a kernel with exactly that mistake fails tests/test_gpu_prep.py).

The output of a record, as vsearch's dust() and the oracle define it: under qmask_dust every letter upper-cased, then
the letters of each masked interval lower-cased (a byte that is no letter has no case and stays as it is, masked or
not); without qmask_dust the input bytes.  A k-mer window is dropped when one of its output characters is lower-case.
"""
from __future__ import annotations

import numpy as np
from pyref import c4, revcomp

MAX_LEN = 112
CODE_WORDS = 14  # MAX_LEN / 8 nibbles per u32
K = 8

# One switch per rule.  Every switch at its default is the operation; one switch flipped is what a kernel with exactly
# that mistake computes.
RULES = ("best_ge",            # v > bestv made >= (the last of tied (start, end) pairs wins instead of the first)
         "level_ge",           # bestv > 20 made >= 20
         "l1_minus",           # l1 = l - 8: the window's last start is lost
         "l1_plus",            # l1 = l - 6: one more start (tests/test_prep_ref_cpu.py: it cannot reach 21)
         "step31", "step33",   # windows every 31 / 33 residues instead of 32
         "end_exclusive",      # the masked interval's last position left out
         "kwin7", "kwin9",     # a k-mer dropped for a masked position among its first 7 / its 8 and the next one
         "minus_unmirrored",   # the minus strand's k-mers dropped by the plus strand's mask positions
         "u_not_t",            # U read as an unknown symbol
         "no_upper_unmasked",  # under qmask_dust, unmasked lower-case input left lower-case
         "ambig_from_input")   # the ambiguity bit from the input bytes instead of the output bytes


def _c2(ch):
    u = ch.upper()
    return "ACGT".index(u) if u in "ACGT" else (3 if u == "U" else 0)


def _is_letter(ch):
    return "A" <= ch <= "Z" or "a" <= ch <= "z"


def windows(seq, rules=()):
    """wo() of every DUST window of seq: dicts with i0, l, bestv, besti, bestj (window-relative, the pair wo() returns)
    and ties, every (i, j) that reaches bestv, in wo()'s order."""
    c2 = [_c2(ch) for ch in seq]
    step = 31 if "step31" in rules else 33 if "step33" in rules else 32
    out = []
    for i0 in range(0, len(seq), step):
        L = min(64, len(seq) - i0)
        l1 = L - 3 + 1 - 5 + ("l1_plus" in rules) - ("l1_minus" in rules)
        if l1 < 0:
            continue
        words, w = [], 0
        for j in range(L):
            w = ((w << 2) | c2[i0 + j]) & 63
            words.append(w)
        bestv = besti = bestj = 0
        scored = []
        for i in range(l1):
            counts = [0] * 64
            tot = 0
            for j in range(2, L - i):
                x = words[i + j]
                if counts[x]:
                    tot += counts[x]
                    v = 10 * tot // j
                    scored.append((v, i, j))
                    if v >= bestv if "best_ge" in rules else v > bestv:
                        bestv, besti, bestj = v, i, j
                counts[x] += 1
        out.append(dict(i0=i0, l=L, bestv=bestv, besti=besti, bestj=bestj,
                        ties=[(i, j) for v, i, j in scored if v == bestv]))
    return out


def intervals(seq, rules=()):
    """the masked intervals [lo, hi] (inclusive, record positions), one per window whose best score passes the level"""
    out = []
    for w in windows(seq, rules):
        if w["bestv"] >= 20 if "level_ge" in rules else w["bestv"] > 20:
            lo = w["i0"] + w["besti"]
            out.append((lo, lo + w["bestj"] - ("end_exclusive" in rules)))
    return out


def mask_bits(seq, rules=(), rec=None):
    """per position: a letter of rec (default seq) inside a masked interval of seq"""
    m = [False] * len(seq)
    for lo, hi in intervals(seq, rules):
        for j in range(lo, hi + 1):
            m[j] = _is_letter((rec or seq)[j])
    return m


def dust(seq, rules=(), m=None):
    m = mask_bits(seq, rules) if m is None else m
    keep = "no_upper_unmasked" in rules
    return "".join(ch.lower() if b else (ch if keep else ch.upper()) for ch, b in zip(seq, m))


def kmer_code(w):
    code = 0
    for ch in w:
        code = code * 4 + _c2(ch)
    return code


def kmer_lists(seq, mask, rules=()):
    """(plus, minus): the ascending unique 8-mer codes of seq and of its reverse complement; a k-mer is dropped when
    the mask covers one of its positions (mask: per position of seq, or None)"""
    n = len(seq)
    w = 7 if "kwin7" in rules else 9 if "kwin9" in rules else K
    out = []
    for st, s in enumerate((seq, revcomp(seq))):
        got = set()
        for x in range(n - K + 1):
            if mask is not None:
                if st == 0 or "minus_unmirrored" in rules:
                    cover = range(x, min(n, x + w))
                else:  # strand position y is record position n - 1 - y: the window mirrored, widened the same way
                    cover = range(max(0, n - 1 - x - (w - 1)), n - x)
                if any(mask[j] for j in cover):
                    continue
            got.add(kmer_code(s[x:x + K]))
        out.append(sorted(got))
    return out[0], out[1]


def pack_codes(seq):
    """the 14 code words of one strand: nibble t of word w is c4 of position 8 w + t, 0 past the record"""
    words = [0] * CODE_WORDS
    for p, ch in enumerate(seq):
        words[p // 8] |= c4(ch) << (4 * (p % 8))
    return words


def prep(records, dust_on=1, rules=()):
    """K1's outputs for a batch of ASCII records (str), in the order given."""
    assert all(r in RULES for r in rules), rules
    n = len(records)
    masked, kmers = [], []
    codes = np.zeros((n, 2, CODE_WORDS), np.uint32)
    lens = np.zeros(n, np.uint8)
    nk = np.zeros((n, 2), np.int32)
    changed = np.zeros(n, np.uint8)
    ambig = 0
    for i, rec in enumerate(records):
        assert len(rec) <= MAX_LEN and all(ord(ch) < 128 for ch in rec)
        # U not read as T: every U stands as a symbol outside the alphabet (code 0 in both maps, its own complement)
        seq = rec.replace("U", "\x01").replace("u", "\x01") if "u_not_t" in rules else rec
        m = mask_bits(seq, rules, rec) if dust_on else None
        out = dust(rec, rules, m) if dust_on else rec
        coded = "".join("\x01" if s == "\x01" else o for s, o in zip(seq, out))
        masked.append(out)
        kp, km = kmer_lists(coded, m, rules)
        kmers.append([kp, km])
        nk[i] = len(kp), len(km)
        codes[i, 0] = pack_codes(coded)
        codes[i, 1] = pack_codes(revcomp(coded))
        lens[i] = len(rec)
        changed[i] = out != rec
        ambig |= any(c4(ch) not in (1, 2, 4, 8) for ch in (seq if "ambig_from_input" in rules else coded))
    return dict(masked=masked, codes=codes, lens=lens, kmers=kmers, nk=nk, changed=changed,
                n_changed=int(changed.sum()), ambig=int(ambig))
