"""Where the branch-length optimiser ENDS, checked on the CPU against an optimiser that shares no arithmetic with it.

BruteForce.optimise (tests/brute_force.py) drives the recollected control flow of the two rules (sliding, --raxml-blo)
with derivatives from Q^k expm products on log-factored partials; its end points on the configurations
brute_cases.OPT_NAMES are committed under tests/golden/endpoints (tests/gen_endpoints.py).  This file
  1. runs the C oracle (oracle/epa_oracle.c: sumtable in the eigenbasis, scaler counts, padded categories) against every
     fixture, by the rule of tests/endpoints_util.py with the oracle's lnL bound 1e-8, in both scaler modes on the ladders;
  2. recomputes two pairs per configuration and mode with optimise (the files are what the code gives today) and checks
     that the files obey their own thinning rule;
  3. ties optimise to the older generator: the `thorough` entries of the four golden files (gen_golden.thorough);
  4. shows the comparison has teeth: optimise with +I left out of the derivative's l0, or with uniform weights in the
     derivative, breaks the rule on T4I / T4;
  5. asserts from window lengths alone that the inputs reach every span class of the Newton kernels.
tests/test_gpu_endpoints.py applies the same rule to the device.

Measured, oracle against fixtures, per configuration and rule (test_oracle_against_fixtures prints these lines; on
the ladders both scaler modes give the same figures): largest |dlnL|, relative pendant and relative distal difference
(floor 1e-3), and the pairs off the fixture's end point.  Every read is on four branches, so the lists are short, the
allowance n // 100 is 0 and every pair must agree; rounds and reverts equal the fixtures' sums everywhere.

                 pairs   sliding                        --raxml-blo                    not agreeing
    T4              56   1.4e-12  9.8e-14  1.5e-13      1.6e-12  9.9e-15  8.3e-14      0 / 0
    T4 MIN 1e-06    56   9.1e-13  1.1e-13  1.4e-13      1.4e-12  1.1e-14  8.5e-14      0 / 0
    T4I             56   1.6e-12  1.5e-11  1.3e-13      1.4e-12  1.5e-11  7.5e-14      0 / 0
    M               44   4.6e-11  6.7e-14  6.3e-13      7.8e-11  9.7e-15  5.8e-13      0 / 0
    MI              44   4.6e-11  5.4e-13  1.9e-13      5.4e-11  4.8e-14  3.5e-13      0 / 0
    AL              24   1.3e-11  7.8e-13  1.8e-12      1.5e-11  7.9e-13  1.7e-12      0 / 0
    AL384           16   1.2e-11  3.6e-13  1.6e-12      1.2e-11  3.7e-13  1.4e-12      0 / 0
    D1              56   2.5e-12  9.9e-13  6.3e-14      2e-12    9.9e-13  6.6e-14      0 / 0
    D2              56   1.3e-12  1.5e-11  6.4e-14      1.4e-12  4e-11    7.3e-14      0 / 0
    D3              56   1.8e-12  6.1e-11  9.2e-14      1.7e-12  6.1e-11  8.4e-14      0 / 0
    D5              56   2.7e-12  1.3e-10  1.1e-13      1.4e-12  1.3e-10  1.4e-13      0 / 0
    D6              56   2e-12    1.5e-10  6.8e-14      1.8e-12  1.5e-10  5e-13        0 / 0
    D7              56   2.5e-12  3.1e-11  1e-13        1.4e-12  3e-11    1.6e-13      0 / 0
    D9              56   5e-12    6.6e-11  2.7e-13      3.2e-12  6.6e-11  3.1e-13      0 / 0
    D13             56   2e-12    1e-10    1.2e-13      1.1e-12  1e-10    1.2e-13      0 / 0
    D16             56   3.2e-12  1e-10    9e-14        1.5e-12  1e-10    3.6e-13      0 / 0
    A1              48   5.7e-12  6.9e-13  1.1e-12      3.8e-12  7.5e-13  8e-14        0 / 0
    A2              48   5.1e-12  7.3e-13  1e-12        4.3e-12  6.9e-13  6.4e-14      0 / 0
    A3              48   6.4e-12  2e-12    7.5e-13      6.1e-12  2.1e-12  1.6e-12      0 / 0
    A4              48   4.1e-12  6.3e-13  1.1e-12      3.8e-12  7e-13    7.9e-14      0 / 0
    A6              48   6.8e-12  5.5e-13  1.6e-12      4.4e-12  5.9e-13  6.4e-14      0 / 0
    A8              48   8.9e-12  1.7e-12  1.4e-12      6.4e-12  1.9e-12  1.6e-12      0 / 0
    A9              48   1.2e-11  1.9e-10  2.7e-12      8.2e-12  1.9e-10  1.3e-13      0 / 0
    S4              32   7.3e-12  5.2e-11  9.1e-12      5.5e-12  5.5e-11  6.7e-11      0 / 0
    S20             24   8.2e-12  1.7e-10  1.3e-14      9.1e-12  1.7e-10  7.7e-11      0 / 0
    L               16   1.1e-10  4e-14    1.2e-13      5.5e-11  4.1e-14  1.4e-13      0 / 0
    Xlong           32   3.4e-13  6.8e-11  3.7e-14      3.4e-13  7.4e-11  1.4e-11      0 / 0
    Xshort           8   6e-10    1.7e-11  0            5.7e-10  1.5e-11  3.2e-15      0 / 0

The oracle's margin where the likelihood is flattest is measured on ALL 360 candidate pairs of S4 by
test_s4_every_candidate_pair_oracle_margin: 2 pairs off under the sliding rule, 1 under --raxml-blo, allowance 3.

Teeth (pairs on which the mutant leaves the fixture, and its largest |dlnL| against the allowance of 1e-4):
    T4I, +I missing from the derivative's l0:   51 of 56 (5.8) sliding,  52 of 56 (2.3) --raxml-blo
    T4,  uniform weights in the derivative:     52 of 56 (0.39) sliding, 52 of 56 (0.019) --raxml-blo
"""
import os

import numpy as np
import pytest

import brute_cases as bc
import endpoints_util as eu
import gen_endpoints
from brute_force import BruteForce
from gen_golden import valid_range
from golden_util import load_case
from oracle_lib import Oracle

ORACLE_LNL_TOL = 1e-8                   # the oracle's bound in test_brute_force_cpu.py
GOLDEN_CASES = ["dna8_gtr_g_default", "dna8_gtr_fu_g4", "dna8_gtr_fu_i_g4", "aa8_protgtr_g4"]


def split_key(key):
    mode, mn = key.split("@")
    return mode, float(mn)


def oracle_of(c, mode, min_branch, rate_scalers=False):
    o = Oracle(c["newick"], c["labels"], c["seqs"], c["states"], c["subst"], c["freqs"], c["rates"],
               weights=c["weights"], pinv=c["pinv"], rate_scalers=rate_scalers)
    o.set_raxml_blo(mode == "raxml")
    o.set_blo(min_branch=min_branch)
    return o


# ---- 1. the oracle against every fixture ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.OPT_NAMES)
def test_oracle_against_fixtures(name):
    c, bf, g = bc.case(name), bc.brute(name), eu.load(name)
    keys = {bc.endpoint_key(v["mode"], v["min_branch"]) for v in bc.opt_variants(name)}
    assert set(g["modes"]) == keys
    for key in sorted(keys):
        e = g["modes"][key]
        mode, mn = split_key(key)
        for rs in sorted({v["rate_scalers"] for v in bc.opt_variants(name)}):
            o = oracle_of(c, mode, mn, rate_scalers=rs)
            assert o.B == bf.B and all(o.branch_info(b)[0] == bf.lengths[b] for b in range(bf.B))
            lnl, pen, dis = o.thorough(e["branch"], e["read"], c["reads"])
            st = eu.measure(e, lnl, pen, dis, bf.lengths, ORACLE_LNL_TOL)
            print(eu.line(name, key + (" rs" if rs else ""), st), st["other_pairs"] or "")
            eu.compare(e, lnl, pen, dis, bf.lengths, ORACLE_LNL_TOL)
            if st["other"] == 0:
                assert o.last_stats["rounds"] == int(e["rounds"].sum())
                assert o.last_stats["reverts"] == int(e["reverted"].sum())


# ---- 2. the files are fresh and obey their thinning rule -----------------------------------------------------------------
@pytest.mark.parametrize("name", bc.OPT_NAMES)
def test_fixtures_are_fresh(name):
    c, bf, g = bc.case(name), bc.brute(name), eu.load(name)
    assert os.path.getsize(os.path.join(eu.DIR, name + ".json")) < 64 * 1024
    pairs = gen_endpoints.thinned_pairs(name)
    assert g["thinning"] == gen_endpoints.RULE
    need = gen_endpoints.must_have(bf)
    assert any(not bf.brs[b].kids for b in need) and {int(np.argmin(bf.lengths)), int(np.argmax(bf.lengths))} <= set(need)
    for key, e in g["modes"].items():
        assert list(zip(e["branch"].tolist(), e["read"].tolist())) == pairs
        for q in range(len(c["reads"])):
            mine = set(e["branch"][e["read"] == q].tolist())
            assert len(mine) >= 4 and set(need) <= mine, (key, q)
        mode, mn = split_key(key)
        rows = np.array([len(pairs) // 3, 2 * len(pairs) // 3])
        r = [bf.optimise(int(e["branch"][i]), c["reads"][int(e["read"][i])], mode=mode, min_branch=mn) for i in rows]
        st = eu.compare(e, [x["lnl"] for x in r], [x["pendant"] for x in r], [x["distal"] for x in r], bf.lengths,
                        ORACLE_LNL_TOL, rows=rows)
        assert st["other"] == 0
        assert [x["rounds"] for x in r] == e["rounds"][rows].tolist()
        assert [x["reverted"] for x in r] == e["reverted"][rows].tolist()


def test_s4_every_candidate_pair_oracle_margin():
    """the flattest input of the set (every branch 0.9, 48 random columns) on ALL its candidate pairs, optimise computed
    here instead of read from the thinned file: how much of the rule's allowance the C oracle itself uses.  Measured:
    sliding 2 of 360 pairs ((162, 5), (261, 3)), --raxml-blo 1 of 360 ((162, 5)), allowance 3; their lnL equals optimise's to 3.4e-9"""
    c, bf = bc.case("S4"), bc.brute("S4")
    pb, ps = bc.pair_lists(c, bf.B)
    for mode in ("sliding", "raxml"):
        r = [bf.optimise(int(b), c["reads"][int(q)], mode=mode) for b, q in zip(pb, ps)]
        e = {"branch": pb, "read": ps, "lnl": np.array([x["lnl"] for x in r]),
             "pendant": np.array([x["pendant"] for x in r]), "distal": np.array([x["distal"] for x in r])}
        lnl, pen, dis = oracle_of(c, mode, 1e-4).thorough(pb, ps, c["reads"])
        st = eu.compare(e, lnl, pen, dis, bf.lengths, ORACLE_LNL_TOL)
        print(eu.line("S4", mode + ", all", st), st["other_pairs"])
        assert st["n"] == 360 and st["cap"] == 3


# ---- 3. optimise against the older generator's thorough entries -------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_optimise_reproduces_the_golden_thorough_entries(name):
    g = load_case(name)
    labels, seqs = [a for a, _ in g["msa"]], [b for _, b in g["msa"]]
    bf = BruteForce(g["newick"], labels, seqs, g["states"], g["subst"], g["freqs"], g["gamma_rates"],
                    pinv=g.get("pinv", 0.0))
    n = 0
    for qi, row in enumerate(g["thorough"]):
        for b, e in enumerate(row):
            r = bf.optimise(b, g["queries"][qi]["seq"])
            assert abs(r["lnl"] - e["lnl"]) < 1e-7, (qi, b, r, e)
            assert abs(r["pendant"] - e["pendant"]) < 1e-7 * max(1.0, e["pendant"]), (qi, b, r, e)
            assert abs(r["distal"] - e["distal"]) < 1e-7, (qi, b, r, e)
            assert (r["rounds"], r["reverted"]) == (e["rounds"], bool(e["reverted"])), (qi, b, r, e)
            n += 1
    assert n == len(g["queries"]) * bf.B


# ---- 4. teeth --------------------------------------------------------------------------------------------------------------
def mutant_breaks_the_rule(name, cls):
    """optimise of the mutated class on the fixture's pairs -> {key: pairs off the fixture}; asserts that the rule breaks
    under every mode of the file (with the device's lnL bound, the wider of the two)"""
    c, g = bc.case(name), eu.load(name)
    bad = cls(c["newick"], c["labels"], c["seqs"], c["states"], c["subst"], c["freqs"], c["rates"],
              weights=c["weights"], pinv=c["pinv"])
    off = {}
    for key in ("sliding@0.0001", "raxml@0.0001"):
        e = g["modes"][key]
        mode, mn = split_key(key)
        r = [bad.optimise(int(b), c["reads"][int(q)], mode=mode, min_branch=mn) for b, q in zip(e["branch"], e["read"])]
        st = eu.measure(e, [x["lnl"] for x in r], [x["pendant"] for x in r], [x["distal"] for x in r],
                        bad.lengths, 1e-6)
        print(eu.line(name, key, st))
        assert st["broken"] and st["max_dlnl_other"] > eu.FLAT_LNL_TOL, st
        off[key] = st["other"]
    return off


def test_teeth_invariant_term():
    """+I left out of l0 in the derivative ONLY (the score keeps it): the mutant leaves the fixture on 51 of 56 pairs
    under the sliding rule and on 52 of 56 under --raxml-blo (allowance 0), lnL up to 5.8 / 2.3 away (allowance 1e-4)"""
    class NoInvariantInDerivative(BruteForce):
        def _deriv_log_cinv(self, sl):
            return np.full(len(self.log_cinv[sl]), -np.inf)                 # the mutation

    off = mutant_breaks_the_rule("T4I", NoInvariantInDerivative)
    assert min(off.values()) > len(eu.load("T4I")["modes"]["sliding@0.0001"]["lnl"]) // 2


def test_teeth_uniform_weights():
    """equal category weights in the derivative ONLY: the mutant leaves the fixture on 52 of 56 pairs under
    either rule (allowance 0), lnL up to 0.39 / 0.019 away (allowance 1e-4)"""
    class UniformWeightsInDerivative(BruteForce):
        def _deriv_logw(self):
            return np.full(self.c, -np.log(self.c))                         # the mutation

    off = mutant_breaks_the_rule("T4", UniformWeightsInDerivative)
    assert min(off.values()) > len(eu.load("T4")["modes"]["sliding@0.0001"]["lnl"]) // 2


# ---- 5. the inputs reach the paths they are meant for ------------------------------------------------------------------------
def span_class(states, span):
    """the class table of the thorough kernels, restated: 20 states 0 .. 3 by 64 / 128 / 192; nucleotides by 64-site
    chunks per lane 1, 2, 3, 4, 6, 8, 12, 16, 24 (0 .. 8), 9 beyond, 10 / 11 the half-chunk tails 65 .. 96 / 129 .. 160"""
    if states != 4:
        return 0 if span <= 64 else 1 if span <= 128 else 2 if span <= 192 else 3
    if 64 < span <= 96:
        return 10
    if 128 < span <= 160:
        return 11
    nch = (span + 63) // 64
    for cls, top in enumerate((1, 2, 3, 4, 6, 8, 12, 16, 24)):
        if nch <= top:
            return cls
    return 9


def test_inputs_reach_the_paths_they_are_meant_for():
    spans = lambda name: {valid_range(r)[1] for r in bc.case(name)["reads"]}         # noqa: E731
    for name in ("T4", "T4I"):
        assert {span_class(4, n) for n in spans(name)} == {0, 1, 2, 3, 10, 11}
        assert bc.case(name)["pinv"] == (0.2 if name == "T4I" else 0.0)
    for name in ("M", "MI"):
        assert {span_class(4, n) for n in spans(name)} == {3, 4, 5, 6, 7, 8}
        assert set(bc.M_READS) == spans(name)                                  # both sides of every step
    dna = set().union(*(spans(n) for n in bc.OPT_NAMES if bc.case(n)["states"] == 4))
    assert {span_class(4, n) for n in dna} == set(range(12))                  # 9: L's windows beyond 1536 sites
    # 20 states, class 3: ONE thorough call is dispatched by its longest window (launch_thorough: bound = the call's
    # max_span), and both test files pass all reads of a configuration in one call.  Up to 384 residues with four
    # categories the matrix-core kernel runs, under both rules; beyond, the lane-per-site kernel with its slab under the
    # sliding rule and the general kernel under --raxml-blo.
    al, al384 = spans("AL"), spans("AL384")
    assert {span_class(20, n) for n in al | al384} == {3} and len(bc.case("AL384")["rates"]) == 4
    assert max(al384) == 384 and min(al384) > 256                             # the whole call on the last MFMA window
    assert max(al) > 384 and min(al) <= 384                                   # the whole call beyond it
    aa = set().union(*(spans(n) for n in bc.OPT_NAMES if bc.case(n)["states"] == 20))
    assert {span_class(20, n) for n in aa} == {0, 1, 2, 3}
    for name in ("T4", "T4I", "M", "MI", "AL", "AL384"):
        c = bc.case(name)
        assert len(c["rates"]) == 4 and np.ptp(c["weights"]) > 0.05
        assert abs(np.sum(c["rates"] * c["weights"]) - 1.0) < 1e-12 and abs(np.sum(c["weights"]) - 1.0) < 1e-12
    # every read of every fixture is on a tip branch, the shortest and the longest branch: test_fixtures_are_fresh
