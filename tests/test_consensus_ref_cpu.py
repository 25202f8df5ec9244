"""The consensus reference checks itself (tests/consensus_ref.py): msa_ref at its defaults equals the oracle's Python
restatement on every case and the C oracle's consensus on clustered synthetic UMIs, every rule switch changes the
expected bytes of some case (so tests/test_gpu_consensus.py would catch a kernel with that mistake), and the given-ops
cases are what they claim to be.  No GPU."""
import consensus_ref as R
import orc
import pytest
from umiclust import synth

ALL = list(R.TRACED) + list(R.GIVEN)


def _expected(name):
    return [(name, 1, 1)] if name in R.GIVEN else [(name, pr, bo) for pr, bo in R.SCORINGS]


@pytest.mark.parametrize("name", ALL)
def test_default_rules_equal_pyref(name):
    seqs, clusters, strands, _ = R.case(name)
    for key in _expected(name):
        cigars, want = R.expected(*key)
        assert want == R.pyref_consensus(seqs, clusters, strands, cigars), key


@pytest.mark.parametrize("kind,mix", [("short", 0.0), ("short", 0.4), ("long", 0.3)])
def test_reference_equals_c_oracle_on_clustered_umis(kind, mix):
    """clusters of the C oracle, their CIGARs rebuilt by its aligner: msa_ref gives msa_consensus's bytes"""
    if kind == "short":
        seqs = synth.make_umis(40, seed=61, max_reads=600, orient_mix=mix, error_rate=0.03).as_list()
        p = orc.params(1, 0.93, 58, 68)
    else:
        seqs = synth.make_umis(6, seed=62, max_reads=500, orient_mix=mix, mean_reads=1500.0, error_rate=0.15,
                               split=(0.0, 0.5, 0.5), max_edits=4, pattern_fwd=synth.UMI_FWD_LONG,
                               pattern_rev=synth.UMI_REV_LONG).as_list()
        p = orc.params(1, 0.80, 80, 110)
    o = orc.cluster(p, seqs)
    clusters, strands = R.clusters_of(o)
    assert sum(map(len, clusters)) == o["stats"]["kept"] and max(map(len, clusters)) > 3
    assert (not mix) or any(any(st) for st in strands)
    cigars = [[""] + [orc.align(p, q, seqs[m[0]])["cigar"] for q in qs[1:]]
              for m, qs in zip(clusters, R.oriented(seqs, clusters, strands))]
    assert any("D" in c or "I" in c for cg in cigars for c in cg)
    assert R.reference(seqs, clusters, strands, cigars) == o["consensus"]
    assert R.pyref_consensus(seqs, clusters, strands, cigars) == o["consensus"]


@pytest.mark.parametrize("rule", R.RULES)
def test_every_rule_is_discriminated(rule):
    """flipping the rule changes the expected consensus of at least one cluster of some case"""
    changed = []
    for name in ALL:
        seqs, clusters, strands, _ = R.case(name)
        cigars, want = R.expected(name)
        if R.reference(seqs, clusters, strands, cigars, **{rule: False}) != want:
            changed.append(name)
    assert changed, rule
    assert any(name in R.GIVEN for name in changed), (rule, changed)  # also where the ops are not the aligner's


@pytest.mark.parametrize("name", list(R.GIVEN))
def test_given_ops_pass_the_entry_points_checks(name):
    seqs, clusters, _, cigars = R.case(name)
    for m, cg in zip(clusters, cigars):
        for r, ops in zip(m[1:], cg[1:]):
            assert R.ops_valid(ops, len(seqs[m[0]]), len(seqs[r])), (name, m[0], r, ops)
    assert not R.ops_valid("MMX", 3, 3) and not R.ops_valid("MM", 3, 2) and not R.ops_valid("MMD", 2, 2)
    assert not R.ops_valid("I" * 113 + "D" * 112, 113, 112) and R.ops_valid("I" * 112 + "D" * 112, 112, 112)


def test_cases_stay_small_and_in_range():
    total = 0
    for name in ALL:
        seqs, clusters, strands, cigars = R.case(name)
        assert all(1 <= len(s) <= R.MAX_LEN for s in seqs), name
        assert all(1 <= len(m) <= 600 for m in clusters), name
        flat = [r for m in clusters for r in m]
        assert len(set(flat)) == len(flat) and all(0 <= r < len(seqs) for r in flat), name
        assert [len(s) for s in strands] == [len(m) for m in clusters] and all(s[0] == 0 for s in strands), name
        assert (cigars is None) == (name in R.TRACED)
        total += len(flat)
    assert total < 6000


def test_traced_cases_have_the_shapes_they_are_named_for():
    def member_lens(name):
        seqs, clusters, _, _ = R.case(name)
        return [len(seqs[r]) for m in clusters for r in m[1:]], [len(seqs[m[0]]) for m in clusters]
    for L in (33, 64, 65, 72, 112):
        assert max(map(len, R.case(f"maxl{L}")[0])) == L
    for name in ("maxl33", "maxl64", "short_vs_long"):  # an empty second launch
        assert max(member_lens(name)[0]) <= R.TW_SPLIT, name
    assert min(member_lens("long_only")[0]) > R.TW_SPLIT  # an empty first launch
    for name in ("maxl65", "maxl72", "maxl112", "edges", "many"):  # both launches
        ml = member_lens(name)[0]
        assert min(ml) <= R.TW_SPLIT < max(ml), name
    ml, cl = member_lens("short_vs_long")
    assert min(cl) > R.TW_SPLIT and max(cl) == R.MAX_LEN
    ml, cl = member_lens("edges")
    assert {1, 2, 63, 64, 65, 111, 112} <= set(ml) and {1, 2, 63, 64, 65, 111, 112} <= set(cl)
    seqs, clusters, strands, _ = R.case("edges")
    same = [(seqs[m[0]], seqs[r]) for m in clusters for r, st in zip(m[1:], strands[clusters.index(m)][1:]) if not st]
    assert sum(c == q and set(c) <= set("ACGT") for c, q in same) >= 5          # the all-M shortcut
    assert sum(len(c) == len(q) and sum(a != b for a, b in zip(c, q)) == 1 and "N" in q for c, q in same) >= 5
    assert sum(len(c) == len(q) and sum(a != b for a, b in zip(c, q)) == 1 and "R" in q for c, q in same) >= 5
    assert sum(len(c) == len(q) and sum(a != b for a, b in zip(c, q)) == 1 and set(q) <= set("ACGT")
               for c, q in same) >= 5
    assert sorted(len(m) for m in R.case("sizes")[1]) == [1, 2, 3, 255, 256, 257, 513]
    assert len(R.case("many")[1]) >= 300
    assert sum(sum(st) for st in R.case("minus_indels")[2]) >= 30
    # the aligner puts indels near both ends of minus-strand members
    ends = [0, 0]
    for al, st in zip(R.oracle_alignments("minus_indels", 1, 1), R.case("minus_indels")[2]):
        for a, s in zip(al[1:], st[1:]):
            ops = R.expand(a["cigar"])
            if s and set(ops[:6]) & set("DI"):
                ends[0] += 1
            if s and set(ops[-6:]) & set("DI"):
                ends[1] += 1
    assert min(ends) >= 5, ends


def test_limit_cases_have_the_widths_they_claim():
    def widths(name):
        seqs, clusters, _, cigars = R.case(name)
        return [R.msa_width(seqs, m, dict(zip(m[1:], cg[1:]))) for m, cg in zip(clusters, cigars)]
    seqs, clusters, _, _ = R.case("cons224")
    assert widths("cons224") == [224] and [len(c) for c in R.expected("cons224")[1]] == [R.CONS_CAP]
    assert widths("msa2048")[0] == R.MSA_COLS and widths("msa2049")[0] == R.MSA_COLS + 1
    for name in ("msa2048", "msa2049"):  # the oracle sizes generously and answers both: the centroid
        seqs, clusters, _, _ = R.case(name)
        assert R.expected(name)[1][0] == seqs[clusters[0][0]]
    # best == gaps and best == gaps - 1 both occur among the columns of best_vs_gaps
    seqs, clusters, strands, cigars = R.case("best_vs_gaps")
    want = R.expected("best_vs_gaps")[1]
    strict = R.reference(seqs, clusters, strands, cigars, emit_on_equal=False)
    assert sum(len(a) - len(b) for a, b in zip(want, strict)) >= 3
