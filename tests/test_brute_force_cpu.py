"""The independent log-space evaluator (tests/brute_force.py) on the CPU: tied to the committed golden vectors, checked
for self-consistency, and used to pin the CPU oracle on every configuration of tests/brute_cases.py -- unequal category
weights, 1 .. 16 categories, +I, IUPAC codes and gap runs in the reference tips, trees deep enough to rescale in both
scaler modes, a 1700-site window, branch lengths from 1e-6 to 12 (drawn from [1e-8, 20]).  tests/test_gpu_brute_force.py runs the device
against the same evaluator on the same inputs.

Bound of every comparison with the oracle: 1e-8, the bound of test_oracle_golden.py for the golden files.  Measured
(tree lnL, preplacement table, lnL at the optimiser's returned lengths; test_oracle_against_brute_force prints them):
at most 1.5e-11 in groups D, A and S, 1.1e-10 in L (1700 sites), 9.7e-10 in Xshort -- branches of 1e-6, where
exp(lambda r t) through the oracle's eigenbasis cancels to 1e-16 absolute on off-diagonal entries of 1e-6; expm does
not, so the difference is the oracle's."""
import numpy as np
import pytest

import brute_cases as bc
from brute_force import BruteForce
from gen_golden import DEFAULT_BL
from golden_util import load_case
from oracle_lib import Oracle

TOL = 1e-8
GOLDEN_CASES = ["dna8_gtr_g_default", "dna8_gtr_fu_g4", "dna8_gtr_fu_i_g4", "aa8_protgtr_g4"]


# ---- 1. ties to the committed fixtures ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_reproduces_the_golden_vectors(name):
    g = load_case(name)
    labels, seqs = [a for a, _ in g["msa"]], [b for _, b in g["msa"]]
    bf = BruteForce(g["newick"], labels, seqs, g["states"], g["subst"], g["freqs"], g["gamma_rates"],
                    pinv=g.get("pinv", 0.0))
    assert bf.B == len(g["branch_lengths"]) and np.array_equal(bf.lengths, g["branch_lengths"])
    if "invariant_state" in g and bf.pinv > 0.0:
        assert bf.invariant_state.tolist() == g["invariant_state"]
    for b in range(bf.B):
        assert abs(bf.tree_lnl(b) - g["tree_lnl"]) < TOL
    qs = [q["seq"] for q in g["queries"]]
    assert np.max(np.abs(bf.preplace(qs) - np.array(g["preplace"]))) < TOL
    n = 0
    for qi, row in enumerate(g["thorough"]):
        for b, e in enumerate(row):
            assert abs(bf.score_at(b, qs[qi], e["pendant"], e["distal"]) - e["lnl"]) < TOL, (qi, b)
            n += 1
    assert n == len(qs) * bf.B


# ---- 2. self-consistency -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["D5", "S4"])
def test_tree_lnl_is_the_same_on_every_branch(name):
    bf = bc.brute(name)
    l = np.array([bf.tree_lnl(b) for b in range(bf.B)])
    assert np.all(np.isfinite(l))
    assert np.max(np.abs(l - l[0])) < 1e-9 * abs(l[0])
    if name == "S4":
        assert l[0] / bf.W < -256 * np.log(2)          # 2^-256 per site: the device and the oracle do rescale here


def test_score_at_the_starting_lengths_is_the_preplacement_value():
    c, bf = bc.case("D6"), bc.brute("D6")
    pre = bf.preplace(c["reads"])
    for b in (0, 7, bf.B - 1):
        for q in (0, 4, len(c["reads"]) - 1):
            assert abs(bf.score_at(b, c["reads"][q], DEFAULT_BL, bf.lengths[b] / 2) - pre[q, b]) < 1e-10


# ---- 3. pins the oracle ------------------------------------------------------------------------------------------------
def oracle_of(c, rate_scalers=False):
    return Oracle(c["newick"], c["labels"], c["seqs"], c["states"], c["subst"], c["freqs"], c["rates"],
                  weights=c["weights"], pinv=c["pinv"], rate_scalers=rate_scalers)


def differences(c, o, bf):
    """largest |oracle - brute force| of: tree lnL on three branches, the preplacement table, lnL at the lengths the
    oracle's optimiser returns on the configuration's pairs"""
    assert o.B == bf.B
    assert max(abs(o.branch_info(b)[0] - bf.lengths[b]) for b in range(bf.B)) == 0.0      # same edge numbering
    tree = max(abs(o.tree_lnl(b) - bf.tree_lnl(b)) for b in (0, bf.B // 2, bf.B - 1))
    pre = float(np.max(np.abs(o.preplace(c["reads"]) - bf.preplace(c["reads"]))))
    pb, ps = bc.pair_lists(c, bf.B)
    tl, tp, td = o.thorough(pb, ps, c["reads"])
    assert np.all(np.isfinite(tl)) and np.all(tp > 0) and np.all(td >= 0) and np.all(td <= bf.lengths[pb])
    thor = float(np.max(np.abs(tl - bf.score_pairs(pb, ps, c["reads"], tp, td))))
    return {"tree": tree, "preplace": pre, "thorough": thor}


@pytest.mark.parametrize("name", bc.NAMES)
def test_oracle_against_brute_force(name):
    c, bf = bc.case(name), bc.brute(name)
    for rs in sorted({v["rate_scalers"] for v in c["variants"]}):
        d = differences(c, oracle_of(c, rate_scalers=rs), bf)
        print("%s rate_scalers=%d: max |oracle - brute force| tree %.3g preplace %.3g thorough %.3g"
              % (name, rs, d["tree"], d["preplace"], d["thorough"]))
        assert max(d.values()) < TOL, d


def test_inputs_reach_the_paths_they_are_meant_for():
    from gen_golden import valid_range
    for name in ("S4", "S20"):
        bf = bc.brute(name)
        assert bf.tree_lnl(0) / bf.W < -256 * np.log(2)
    assert max(valid_range(r)[1] for r in bc.case("L")["reads"]) > 1536
    assert {65, 96, 129, 160} <= {valid_range(r)[1] for r in bc.case("D5")["reads"]}
    for name in bc.NAMES:
        c = bc.case(name)
        amb = bc.AMBIG[c["states"]]
        assert all(sum(ch in amb for ch in s) >= 6 for s in c["seqs"])
        assert any("-" * 20 in s for s in c["seqs"])
        assert abs(np.sum(c["rates"] * c["weights"]) - 1.0) < 1e-12 and abs(np.sum(c["weights"]) - 1.0) < 1e-12
    assert bc.brute("Xlong").lengths.max() > 10.0 and bc.brute("Xshort").lengths.min() < 1e-6


# ---- 4. teeth ------------------------------------------------------------------------------------------------------------
def test_swapped_category_weights_are_noticed():
    """two weights of a +R model exchanged in the brute force's input alone: the comparison of section 3 fails by far"""
    c = bc.case("D5")
    w = np.array(c["weights"])
    w[[0, 4]] = w[[4, 0]]                                                   # the mutation
    bf = BruteForce(c["newick"], c["labels"], c["seqs"], c["states"], c["subst"], c["freqs"], c["rates"], weights=w,
                    pinv=c["pinv"])
    d = differences(c, oracle_of(c), bf)
    assert min(d.values()) > 1e-3, d


def test_dropped_log_factors_are_noticed():
    """the rescaling ladder without the per-(site, category) log factors: tree lnL is non-finite or off by more than 1"""
    class NoLogFactors(BruteForce):
        @staticmethod
        def _normalise(acc):
            acc, logf = BruteForce._normalise(acc)
            return acc, np.zeros_like(logf)                                 # the mutation

    c = bc.case("S4")
    bad = NoLogFactors(c["newick"], c["labels"], c["seqs"], c["states"], c["subst"], c["freqs"], c["rates"],
                       weights=c["weights"], pinv=c["pinv"])
    good = bc.brute("S4").tree_lnl(0)
    got = bad.tree_lnl(0)
    assert not np.isfinite(got) or abs(got - good) > 1.0


# ---- 5. the golden generator is unchanged by Model's new argument ----------------------------------------------------------
def test_golden_model_default_weights_are_equal():
    from gen_golden import Model
    m = Model(4, [1.0] * 6, [0.25] * 4, 0.5)
    assert np.array_equal(m.weights, np.full(4, 0.25))
    w = [0.1, 0.2, 0.3, 0.4]
    assert np.array_equal(Model(4, [1.0] * 6, [0.25] * 4, 0.5, weights=w).weights, w)
