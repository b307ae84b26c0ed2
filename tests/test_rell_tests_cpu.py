"""The specification of epa_dev_rell_tests (include/epa_dev.h) restated in numpy (tests/rell_tests_ref.py): the
restatement against itself on matrices made by hand, the reason for centring the SH test at the observed lnL, the
restatement against plain multinomial resampling with numpy's own generator on brute-force site rows, and what the
executable refuses.  No device.

Measured here, on the input of the statistical tests (22 reads of 30 sites x 3 branches, R = 4096):
  mean over the replicates of s_k against L_k: largest |mean - L| / standard error 1.74 (bound 6)
  restatement (Philox) against default_rng, |difference| / six_sigma bound: elw 0.138, p_sh 0.23 (66 values each);
  all 22 reads have a p_sh strictly inside (0, 1)
  classic SH (centred at the mean of the replicates) against the exact centre on the same default_rng resamples:
  largest difference of a p-value 0.0271 (111 counts of 4096); no threshold is set for this one: the replicates' mean
  misses L by a standard error of the score, and the difference shrinks like 1 / sqrt(R).
"""
import subprocess

import numpy as np

import rell_ref as rr
import rell_tests_ref as rt
import rescore_util as ru
from epa_ng_amd import hostlib
from test_rescore_cpu import MSA, QUERY, TREE


def test_restatement_on_hand_made_matrices():
    R, n_q = 257, 13
    rng = np.random.RandomState(5)
    rows = rng.uniform(-9.0, -1.0, (5, n_q))
    branch = [3, 1, 4, 1, 5]
    j = rt.draws(n_q, R, 7, 3)
    s = rt.query_stats(rows, j, branch)
    # the weights of a replicate add up to 1, the best score has the largest weight
    assert np.all(np.abs(s["w"].sum(axis=1) - 1.0) < 1e-14)
    assert np.array_equal(np.argmax(s["w"], axis=1), np.argmax(s["score"], axis=1))
    # the observed lnL is the row's sequential sum; its arg-max has T = 0 and t >= 0: p_sh = 1
    assert np.allclose(s["L"], rows.sum(axis=1), rtol=0, atol=1e-12)
    groups = {0: [0, 1, 2, 3, 4]}
    out = rt.rell_tests(rows, [n_q], groups, [7], R, 3, branch)
    top = int(np.argmax(out["L"]))
    assert out["sh"][top] == R and np.all((out["sh"] >= 0) & (out["sh"] <= R))
    assert abs(out["elw"].sum() - 1.0) < 1e-12 and np.all(out["elw"] > 0)
    # support is rell_ref's count
    assert np.array_equal(out["wins"], rr.rell_counts(rows, [n_q], groups, [7], R, 3, branch))
    # two queries are independent of each other; seed and stream id select the replicates
    rows2 = rng.uniform(-9.0, -1.0, (7, n_q))
    groups2 = {0: [0, 3], 1: [1, 2, 4, 5, 6]}
    br2 = [3, 1, 4, 1, 5, 9, 2]
    both = rt.rell_tests(rows2, [n_q, 7], groups2, [0, 1], R, 9, br2)
    assert np.array_equal(both["wins"], rr.rell_counts(rows2, [n_q, 7], groups2, [0, 1], R, 9, br2))
    alone = rt.rell_tests(rows2, [n_q, 7], {1: groups2[1]}, [0, 1], R, 9, br2)
    for key in ("wins", "elw", "sh"):
        assert np.array_equal(alone[key][groups2[1]], both[key][groups2[1]])
    other = rt.rell_tests(rows2, [n_q, 7], groups2, [5, 1], R, 9, br2)
    assert np.array_equal(other["elw"][groups2[1]], both["elw"][groups2[1]])
    assert not np.array_equal(other["elw"][groups2[0]], both["elw"][groups2[0]])
    assert not np.array_equal(rt.rell_tests(rows2, [n_q, 7], groups2, [0, 1], R, 10, br2)["elw"], both["elw"])
    # one entry larger at every site: it takes all support, nearly all weight, and the other is rejected in most replicates
    low = rng.uniform(-9.0, -1.0, n_q)
    out = rt.rell_tests(np.stack([low, low + 0.5]), [n_q], {0: [0, 1]}, [0], R, 1, [0, 1])
    assert out["wins"].tolist() == [0, R] and out["elw"][1] > 0.99 and out["sh"].tolist() == [0, R]
    # identical rows share the weight (no tie rule) and are never rejected; support follows RELL's tie rule
    out = rt.rell_tests(np.stack([low, low, low]), [n_q], {0: [0, 1, 2]}, [0], R, 1, [5, 2, 2])
    assert np.all(np.abs(out["elw"] - 1.0 / 3.0) < 1e-14) and out["sh"].tolist() == [R, R, R]
    assert out["wins"].tolist() == [0, R, 0]


def test_span_zero_and_single_entry():
    R = 65
    out = rt.rell_tests(np.zeros((3, 4)), [0], {0: [0, 1, 2]}, [3], R, 1, [9, 1, 4])
    assert out["wins"].tolist() == [0, R, 0]                       # every score is 0.0: the smaller branch id
    assert np.all(np.abs(out["elw"] - 1.0 / 3.0) < 1e-14) and out["sh"].tolist() == [R, R, R]
    assert np.array_equal(out["L"], np.zeros(3))
    rows = np.random.RandomState(1).uniform(-5.0, -1.0, (1, 9))
    out = rt.rell_tests(rows, [9], {0: [0]}, [0], R, 1, [2])
    assert out["wins"].tolist() == [R] and out["elw"].tolist() == [1.0] and out["sh"].tolist() == [R]


def test_observed_lnl_is_the_mean_of_the_resampled_score():
    """what justifies centring at L: E[s_k] = sum_d E[row[j_d]] = n_q * mean(row) = L_k; over STAT_R replicates the mean
    of s_k lies within six standard errors of L_k for every entry"""
    s = rr.stat_input()
    Q = len(s["reads"])
    worst = 0.0
    for q in range(Q):
        st = rt.query_stats(s["rows"][3 * q:3 * q + 3], rt.draws(rr.STAT_SPAN, rr.STAT_R, q, 1), s["branch"][3 * q:3 * q + 3])
        se = st["score"].std(axis=0, ddof=1) / np.sqrt(rr.STAT_R)
        worst = max(worst, float(np.max(np.abs(st["score"].mean(axis=0) - st["L"]) / se)))
    print("\nmean of s_k against L_k over %d replicates: largest |mean - L| / standard error %.3g" % (rr.STAT_R, worst))
    assert worst <= 6.0


def test_restatement_against_multinomial_resampling():
    """a mean of R values in [0, 1] with expectation p has variance at most p (1 - p) / R, so the binomial bound of
    rell_ref.six_sigma holds for elw as it does for the proportion p_sh"""
    s = rr.stat_input()
    cpu = rt.stat_tests()
    Q = len(s["reads"])
    out = rt.rell_tests(s["rows"], [rr.STAT_SPAN] * Q, rt.group_by_query(s["seq"]), list(range(Q)), rr.STAT_R, 1, s["branch"])
    elw, p_sh = out["elw"], out["sh"] / float(rr.STAT_R)
    assert np.all(np.abs(elw.reshape(Q, 3).sum(1) - 1.0) < 1e-12)
    assert np.all(p_sh.reshape(Q, 3).max(1) == 1.0)
    # the input is not vacuous: at least a third of the queries have a p-value strictly inside (0, 1)
    inside = int(np.sum(np.any((p_sh.reshape(Q, 3) > 0.0) & (p_sh.reshape(Q, 3) < 1.0), axis=1)))
    r_elw = np.abs(elw - cpu["elw"]) / rt.six_sigma(elw, cpu["elw"], rr.STAT_R)
    r_sh = np.abs(p_sh - cpu["p_sh"]) / rt.six_sigma(p_sh, cpu["p_sh"], rr.STAT_R)
    classic = float(np.max(np.abs(cpu["p_sh_classic"] - cpu["p_sh"])))
    print("\n%d values of %d reads: max |restatement - default_rng| / bound: elw %.3g, p_sh %.3g; %d reads with a p_sh in "
          "(0, 1); classic (mean-centred) SH against the exact centre on the same resamples: largest difference %.3g"
          % (len(elw), Q, r_elw.max(), r_sh.max(), inside, classic))
    assert 3 * inside >= Q
    assert np.all(r_elw <= 1.0) and np.all(r_sh <= 1.0)


# ---- the executable: refused before any device is touched, named by --help

def refused(tmp_path, extra, rescore):
    out = tmp_path / "out"
    out.mkdir()
    jp = tmp_path / "in.jplace"
    jp.write_text('{"tree": "unused;", "placements": [{"p": [[3, -1000.0, 1.0, 0.01, 0.1]], "n": ["Rat"]}], "version": 3, '
                  '"fields": ["edge_num", "likelihood", "like_weight_ratio", "distal_length", "pendant_length"]}')
    r = ru.run_cli(TREE, MSA, QUERY, out, (["--rescore", jp] if rescore else []) + list(extra))
    assert r.returncode == 1, r.stdout + r.stderr
    assert "no HIP device" not in r.stderr and "outside the placement hot path" not in r.stderr, r.stderr
    assert not (out / "epa_result.jplace").exists()
    return r


def test_rell_tests_needs_rescore_and_rell(tmp_path):
    for tag, extra, rescore in (("a", ["--rell-tests"], True), ("b", ["--rell-tests"], False),
                                ("c", ["--rell-tests", "--posterior"], True)):
        sub = tmp_path / tag
        sub.mkdir()
        r = refused(sub, extra, rescore)
        assert "--rell-tests" in r.stderr and "--rescore out.jplace --rell N" in r.stderr, r.stderr


def test_rell_inside_a_placement_run_stays_refused(tmp_path):
    r = refused(tmp_path, ["--rell", "100", "--rell-tests"], False)
    assert "--rescore out.jplace --rell N" in r.stderr and "place first" in r.stderr


def test_help_names_the_flag_and_the_fields():
    text = subprocess.run([hostlib.cli_exe(), "--help"], capture_output=True, text=True, timeout=60).stdout
    for word in ("--rell-tests", '"elw"', '"p_sh"'):
        assert word in text
