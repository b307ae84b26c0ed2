"""The host side of the marginal likelihood (epa_dev_marginal_like): the quadrature helpers, the choice of the default
rule, the restatement of tests/marginal_ref.py itself and what the executable refuses.  Nothing here needs a GPU."""
import math

import numpy as np
import pytest
from numpy.polynomial.laguerre import laggauss
from numpy.polynomial.legendre import leggauss

import brute_cases as bc
import epa_ng_amd as epa
import marginal_ref as mr
import rescore_util as ru
from test_rescore_cpu import MSA, QUERY, TREE

QUAD_TOL = 1e-10


def test_quadrature_helpers_against_numpy():
    """K = 1 .. 64, nodes relatively, log weights absolutely, against numpy's leggauss (mapped to [0, 1]) and laggauss.
    Largest differences measured: Legendre nodes 1.4e-13, log weights 2.2e-12; Laguerre nodes 5.7e-14, log weights
    8.6e-12 (numpy's Laguerre weights stay normal numbers up to K = 64: none is left out); the moments
    sum w_j t_j^m = m!, m < 6, hold to 6.8e-13 relatively.  100 x the largest of these is 8.6e-10, above the cap: the
    bound is the cap, 1e-10 -- both sides are fp64 Newton-polished roots, anything worse is a bug."""
    worst = dict(leg_nodes=0.0, leg_logw=0.0, lag_nodes=0.0, lag_logw=0.0, moments=0.0)
    left_out = 0
    for K in range(1, 65):
        x, w = leggauss(K)
        x, w = (x + 1.0) / 2.0, w / 2.0
        n, lw = epa.quadrature_legendre01(K)
        assert n.shape == lw.shape == (K,) and np.all(np.diff(n) > 0) and n[0] > 0.0 and n[-1] < 1.0
        worst["leg_nodes"] = max(worst["leg_nodes"], float(np.max(np.abs(n - x) / x)))
        worst["leg_logw"] = max(worst["leg_logw"], float(np.max(np.abs(lw - np.log(w)))))
        assert abs(float(np.exp(lw).sum()) - 1.0) < 1e-14
        x, w = laggauss(K)
        n, lw = epa.quadrature_laguerre(K)
        assert n.shape == lw.shape == (K,) and np.all(np.diff(n) > 0) and n[0] > 0.0 and np.all(np.isfinite(lw))
        worst["lag_nodes"] = max(worst["lag_nodes"], float(np.max(np.abs(n - x) / x)))
        normal = w >= np.finfo(np.float64).tiny
        left_out += int((~normal).sum())
        worst["lag_logw"] = max(worst["lag_logw"], float(np.max(np.abs(lw[normal] - np.log(w[normal])))))
        assert abs(float(np.exp(lw).sum()) - 1.0) < 1e-14
        for m in range(min(6, 2 * K)):      # a K-node rule is exact up to degree 2K - 1
            got = float(np.sum(np.exp(lw + m * np.log(n))))
            worst["moments"] = max(worst["moments"], abs(got / math.factorial(m) - 1.0))
    print("\nquadrature helpers against numpy, K = 1 .. 64: %s; %d Laguerre weights below the normal range left to the moments"
          % (", ".join("%s %.3g" % kv for kv in worst.items()), left_out))
    for key, value in worst.items():
        assert value < QUAD_TOL, (key, value)
    # the smallest node at K = 5 that the GPU tests' pendant bound rests on
    assert abs(epa.quadrature_laguerre(5)[0][0] - 0.2636) < 1e-4


@pytest.mark.parametrize("K", [0, 65, 1000])
def test_quadrature_helpers_refuse_node_counts_outside_1_to_64(K):
    for fn in (epa.quadrature_legendre01, epa.quadrature_laguerre):
        with pytest.raises(epa.EpaError) as e:
            fn(K)
        assert e.value.code == -1
    with pytest.raises(epa.EpaError):
        epa.posterior_rule(0.1, Kx=K)
    with pytest.raises(epa.EpaError):
        epa.posterior_rule(0.1, Kp=K)


def test_posterior_rule():
    x, xw, p, pw = epa.posterior_rule(0.25)
    assert x.shape == xw.shape == (8,) and p.shape == pw.shape == (16,)
    t, tw = epa.quadrature_laguerre(16)
    assert np.array_equal(p, 0.25 * t) and np.array_equal(pw, tw) and np.array_equal(x, epa.quadrature_legendre01(8)[0])
    x, xw, p, pw = epa.posterior_rule(1.0, Kx=3, Kp=5)
    assert x.shape == (3,) and p.shape == (5,)
    # the exponential prior's mean through the rule
    assert abs(float(np.sum(np.exp(pw) * p)) - 1.0) < 1e-12
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            epa.posterior_rule(bad)


@pytest.mark.parametrize("name", ["D5", "A4"])
def test_default_rule_is_converged(name):
    """BruteForce marginals with the project's rules (8, 16) and (16, 32), prior mean = mean branch length, at branches
    {0, B // 2, B - 1} x reads {0, 1}, differ by less than 1e-6.  Measured: D5 1.1e-14, A4 1.0e-08."""
    c, bf = bc.case(name), bc.brute(name)
    mu = float(np.mean(bf.lengths))
    small, large = epa.posterior_rule(mu), epa.posterior_rule(mu, Kx=16, Kp=32)
    worst = 0.0
    for b in (0, bf.B // 2, bf.B - 1):
        for q in (0, 1):
            m = [mr.combine(mr.brute_grid(bf, c["reads"][q], b, r[0], r[2]), r[1], r[3]) for r in (small, large)]
            worst = max(worst, abs(m[0] - m[1]))
            assert abs(m[0] - m[1]) < 1e-6, (b, q, m)
    print("\n%s: max |M(8, 16) - M(16, 32)| %.3g" % (name, worst))


def test_combine_of_a_constant_grid():
    x, xw, p, pw = epa.posterior_rule(0.05, Kx=3, Kp=5)
    for cst in (0.0, -1234.5):
        got = mr.combine(np.full((3, 5), cst), xw, pw)
        assert abs(got - cst) < 1e-12          # the rule's weights sum to 1
    xw2, pw2 = np.log([0.5, 2.0]), np.log([1.0, 3.0, 0.25])
    got = mr.combine(np.full((2, 3), -7.0), xw2, pw2)
    assert abs(got - (-7.0 + math.log(2.5 * 4.25))) < 1e-12


# ---- what the executable refuses before any device is touched

def refused(tmp_path, extra, message, rescore=True):
    out = tmp_path / "out"
    out.mkdir()
    jp = tmp_path / "in.jplace"
    jp.write_text('{"tree": "unused;", "placements": [{"p": [[3, -1000.0, 1.0, 0.01, 0.1]], "n": ["Rat"]}], "version": 3, '
                  '"fields": ["edge_num", "likelihood", "like_weight_ratio", "distal_length", "pendant_length"]}')
    r = ru.run_cli(TREE, MSA, QUERY, out, (["--rescore", jp] if rescore else []) + list(extra))
    assert r.returncode == 1, r.stdout + r.stderr
    assert message in r.stderr, r.stderr
    assert "no HIP device" not in r.stderr
    assert not (out / "epa_result.jplace").exists()
    return r


def test_posterior_without_rescore(tmp_path):
    r = refused(tmp_path, ["--posterior"], "--rescore out.jplace --posterior", rescore=False)
    assert "place first" in r.stderr


@pytest.mark.parametrize("value", ["0", "-0.5", "nan", "inf", "abc"])
def test_prior_mean_must_be_positive_and_finite(tmp_path, value):
    refused(tmp_path, ["--posterior", "--prior-mean", value], "--prior-mean")


@pytest.mark.parametrize("value", ["0,16", "8,0", "65,16", "8,65", "8", "8,16,4", "-1,16", "a,b"])
def test_posterior_nodes_outside_1_to_64(tmp_path, value):
    r = refused(tmp_path, ["--posterior", "--posterior-nodes", value], "--posterior-nodes")
    assert "1 .. 64" in r.stderr


@pytest.mark.parametrize("extra", [["--prior-mean", "0.1"], ["--posterior-nodes", "4,8"]])
def test_sub_flags_need_posterior(tmp_path, extra):
    r = refused(tmp_path, extra, "--posterior")
    assert "need" in r.stderr


def test_help_names_the_flags():
    import subprocess
    from epa_ng_amd import hostlib
    text = subprocess.run([hostlib.cli_exe(), "--help"], capture_output=True, text=True, timeout=60).stdout
    for flag in ("--posterior ", "--prior-mean", "--posterior-nodes", "marginal_like", "post_prob"):
        assert flag in text
