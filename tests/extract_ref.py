"""Brute-force definition of what oracle/extract.py::hw_locate returns -- TEST INFRASTRUCTURE ONLY.

hw_locate is the checker of the GPU Myers kernels (row f1); this pins it from the definition, sharing no code
with it (own equality, own Levenshtein, no HW/SHW dynamic program):
  distance = the smallest plain Levenshtein distance, under eq, between the pattern and any substring
             w[s:e+1] of the window, the empty substring included (which costs len(pattern));
  end      = the first e at which a substring ending there (or the empty one) attains it;
  start    = the smallest s with lev(pattern, w[s:end+1]) equal to it.
None when the window is empty or the distance exceeds k.  O(n^2) Levenshtein calls: short windows only.
"""
from __future__ import annotations

# what each ambiguity code of the reference's additionalEqualities stands for (extract_umis.py:26-87)
CODES = {"M": "AC", "R": "AG", "W": "AT", "S": "CG", "Y": "CT", "K": "GT", "V": "ACG", "H": "ACT", "D": "AGT",
         "B": "CGT", "N": "ACGT"}


def _one_way(a: str, b: str) -> bool:
    if a in CODES:
        return b in CODES[a]
    if a.upper() in CODES:  # a lowercase code stands for lowercase bases only
        return b in CODES[a.upper()].lower()
    return a in "acgt" and b == a.upper()  # a base equals itself in the other case


def eq(a: str, b: str) -> bool:
    return a == b or _one_way(a, b) or _one_way(b, a)


def lev(p: str, t: str) -> int:
    """Plain edit distance (unit costs) between the whole of p and the whole of t."""
    d = {(i, 0): i for i in range(len(p) + 1)}
    d.update({(0, j): j for j in range(len(t) + 1)})
    for i in range(1, len(p) + 1):
        for j in range(1, len(t) + 1):
            d[i, j] = min(d[i - 1, j] + 1, d[i, j - 1] + 1, d[i - 1, j - 1] + (not eq(p[i - 1], t[j - 1])))
    return d[len(p), len(t)]


def locate(pattern: str, w: str, k: int):
    if not w:
        return None
    per_end = [min([len(pattern)] + [lev(pattern, w[s:e + 1]) for s in range(e + 1)]) for e in range(len(w))]
    best = min(per_end)
    if best > k:
        return None
    end = per_end.index(best)
    return best, min(s for s in range(end + 1) if lev(pattern, w[s:end + 1]) == best), end
