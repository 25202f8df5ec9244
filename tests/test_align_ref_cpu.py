"""The alignment reference behind tests/test_gpu_align_kernels.py, checked without a GPU.

 * oracle/pyref.py (nw + trim_id: Gotoh DP in Python integers, settable scoring) equals the C oracle on score, matches,
   internal length and ops, under every scoring set the library accepts, on a subset of every family of
   tests/align_cases.py that includes 112 x 112;
 * every rule of the operation decides at least one case each kernel is given: pyref.nw / trim_id have one switch per
   rule, and a flipped switch changes (score, matches, internal length) of a case of every kernel's set and the ops of
   a case of k_trace_wave's.  A kernel with exactly that mistake therefore fails the GPU test.
"""
import align_cases as A
import pyref
import pytest


def _subset():
    """every family at the shortest query length, a thinned query length 57 (8 lanes, 7 virtual rows), the IUPAC
    family's shortest, and 112 x 112 of ties, no_diagonal and identical"""
    out, seen = [], {}
    for f, q, t in A.kernel_cases("amb"):
        n = seen.get((f, len(q)), 0)
        seen[(f, len(q))] = n + 1
        if len(q) == 32 and (f != "target_lengths" or n % 3 == 0 or len(t) < 4):
            out.append((f, q, t))
        elif len(q) == 57 and f in ("ties", "ends") and n % 4 == 0:
            out.append((f, q, t))
        elif len(q) == 112 and len(t) >= 111 and f in ("ties", "no_diagonal", "identical"):
            out.append((f, q, t))
    return out


SUBSET = _subset()


def test_subset_covers_every_family_and_the_largest_pair():
    assert {f for f, _, _ in SUBSET} == {f for f, _, _ in A.kernel_cases("amb")}
    assert any(len(q) == 112 and len(t) == 112 for _, q, t in SUBSET)


@pytest.mark.parametrize("s", A.ACCEPTED, ids=[s.name for s in A.ACCEPTED])
def test_pyref_equals_oracle(s):
    for f, q, t in SUBSET:
        got, want = A.py_ref(s, q, t), A.orc_ref(s, q, t)
        assert got == want, (s.name, f, q, t, got, want)


# ------------------------------------------------------------------ one switch per rule
def _small(kernel):
    """the kernel's cases at the three shortest query lengths (every family is built per length), cheapest first"""
    c = [(f, q, t) for f, q, t in A.kernel_cases(kernel) if len(q) <= 34]
    return sorted(c, key=lambda x: len(x[1]) * len(x[2]))


_BASE = {}


def _base(s, q, t):
    k = (s.name, q, t)
    if k not in _BASE:
        _BASE[k] = A.py_ref(s, q, t)
    return _BASE[k]


_WITNESS = {}


def _witness(rule, kernel, field):
    """the first (scoring, family, q, t) of the kernel's cases whose `field` of the result the flipped rule changes"""
    pick = (lambda r: r[:3]) if field == "summary" else (lambda r: r[3])
    cases = _small(kernel)
    have = _WITNESS.get((rule, field))
    if have and (have[1], have[2], have[3]) in set(cases):
        return have
    for s in A.ACCEPTED:
        for f, q, t in cases:
            if pick(A.py_ref(s, q, t, (rule,))) != pick(_base(s, q, t)):
                _WITNESS[(rule, field)] = (s, f, q, t)
                return _WITNESS[(rule, field)]
    return None


REACHABLE = [r for r in pyref.RULES if r != "no_single_run"]


@pytest.mark.parametrize("kernel", A.KERNELS)
@pytest.mark.parametrize("rule", REACHABLE)
def test_every_rule_decides_a_case_of_every_kernel(rule, kernel):
    w = _witness(rule, kernel, "summary")
    assert w is not None, f"no case of {kernel} notices the rule {rule} flipped"
    s, f, q, t = w
    assert A.py_ref(s, q, t, (rule,))[:3] != A.orc_ref(s, q, t)[:3]


@pytest.mark.parametrize("rule", pyref.NW_RULES)
def test_every_dp_rule_decides_the_ops_of_a_trace_case(rule):
    """the trimming rules read the ops and cannot change them; every rule of the DP and the backtrack does"""
    w = _witness(rule, "trace", "ops")
    assert w is not None, f"no case of trace shows the rule {rule} flipped in its ops"
    s, f, q, t = w
    assert A.py_ref(s, q, t, (rule,))[3] != A.orc_ref(s, q, t)[3]


def test_single_run_rule_is_out_of_reach():
    """align_trim's `left >= cols` rule (a one-run alignment is trimmed once) needs an alignment that is a single gap
    run, i.e. an empty query or target.  A path between two non-empty sequences holds a diagonal move or both a D and an
    I run, and align_pairs takes queries from 32 and targets from 1 base.  So no input can show this rule: dropping it
    changes no case, which is asserted here instead of a witness.  The all-gap alignments of no_diagonal under
    preset 1 still end at internal length 0, as leading run + trailing run = columns."""
    s = A.BY_NAME["preset1_bo1"]
    allgap = 0
    for f, q, t in _small("trace"):
        r = A.py_ref(s, q, t)
        assert A.py_ref(s, q, t, ("no_single_run",)) == r == A.orc_ref(s, q, t)
        ops = r[3]
        assert ops[0] == "M" or len(ops.lstrip(ops[0])) > 0  # a leading gap run never is the whole alignment
        allgap += "M" not in ops and r[2] == 0
    assert allgap > 0
