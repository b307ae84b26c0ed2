"""The specification of epa_dev_rell_kh (include/epa_dev.h) restated in numpy (tests/rell_kh_ref.py): the restatement
against cases worked by hand, the invariants that tie it to the SH test of rell_tests_ref, the restatement against plain
multinomial resampling with numpy's own generator on brute-force site rows, and what the executable refuses.  No device.

Measured here, on the input of the statistical tests (22 reads of 30 sites x 3 branches, R = 4096):
  restatement (Philox) against default_rng, |difference| / six_sigma bound: p_kh 0.356, p_wkh 0.41, p_wsh 0.418 (66 values each)
  the best row of a query gets 1.0 in all three by the rule of the specification; tested against the row nearest below
  it instead (CONSEL's convention) its p_wkh would be 0.655 .. 0.970 and its p_wsh 0.781 .. 0.996 over the 22 reads
"""
import subprocess

import numpy as np

import rell_kh_ref as rk
import rell_ref as rr
import rell_tests_ref as rt
from epa_ng_amd import hostlib
from test_rell_tests_cpu import refused

X0 = np.array([-1.0, -2.0, -3.0, -4.0])
X1 = np.array([-2.0, -2.0, -2.0, -5.0])


def by_hand_k2(x_best, x_other, j):
    """K = 2 written as scalar loops: the replicates in which the other row is not rejected by KH"""
    L_b = L_o = 0.0
    for site in range(len(x_best)):
        L_b += x_best[site]
        L_o += x_other[site]
    count = 0
    for r in range(j.shape[0]):
        s_b = s_o = 0.0
        for d in range(j.shape[1]):
            s_b += x_best[j[r, d]]
            s_o += x_other[j[r, d]]
        count += ((s_b - L_b) - (s_o - L_o)) >= (L_b - L_o)
    return count


def test_two_rows_by_hand():
    R, sid, seed = 257, 7, 3
    j = rk.draws(4, R, sid, seed)
    s = rk.query_stats(np.stack([X0, X1]), j, [5, 2])
    # d = x1 - x0 = (-1, 0, 1, -1): a = -1, m = -0.25, q = 0.5625 + 0.0625 + 1.5625 + 0.5625 = 2.75, every step exact
    w = 1.0 / np.sqrt(2.75)
    assert s["w"].tolist() == [[0.0, w], [w, 0.0]] and s["ok"].tolist() == [[False, True], [True, False]]
    assert s["L"].tolist() == [-10.0, -11.0] and s["best"] == 0 and s["opp"].tolist() == [-1, 0]
    assert np.isnan(s["T"][0]) and s["T"][1] == 1.0 * w               # the best row has no opponent
    kh = by_hand_k2(X0, X1, j)
    assert 0 < kh < R
    assert s["kh"].tolist() == [R, kh]
    # the worse row's opponent is the best row: weighted KH is KH; one opponent: weighted SH scales both sides by w
    assert s["wkh"][1] == kh and s["wsh"][1] >= kh
    # the best row is never rejected
    assert s["wkh"][0] == R and s["wsh"][0] == R
    # through the entry point of the restatement, rows longer than the span, entries of two queries interleaved
    rows = [np.concatenate([X0, [9.0]]), np.zeros(5), np.concatenate([X1, [9.0]]), np.zeros(5)]
    out = rk.rell_kh(rows, [4, 0], {0: [0, 2], 1: [1, 3]}, [sid, 1], R, seed, [5, 0, 2, 0])
    assert out["kh"].tolist() == [R, R, kh, R] and out["best"].tolist() == [True, True, False, False]
    assert out["L"].tolist() == [-10.0, 0.0, -11.0, 0.0]


def test_duplicated_row_is_skipped():
    R = 300
    j = rk.draws(4, R, 0, 1)
    # the two copies alone: no opponent, nothing is rejected
    s = rk.query_stats(np.stack([X0, X0]), j, [4, 1])
    assert not s["ok"].any() and s["best"] == 1 and s["opp"].tolist() == [-1, -1]
    assert s["kh"].tolist() == [R, R] and s["wkh"].tolist() == [R, R] and s["wsh"].tolist() == [R, R]
    # with a third row: the pair of copies is skipped; the best row and its copy get 1 in all three tests
    s = rk.query_stats(np.stack([X0, X1, X0]), j, [4, 1, 4])
    assert s["ok"].tolist() == [[False, True, False], [True, False, True], [False, True, False]]
    assert s["best"] == 0 and s["opp"].tolist() == [-1, 0, -1]              # row 1's opponents tie: the smaller index
    assert s["kh"][0] == R and s["kh"][2] == R and 0 < s["kh"][1] < R
    assert s["wkh"][0] == s["wkh"][2] == R and s["wsh"][0] == s["wsh"][2] == R and 0 < s["wkh"][1] <= s["wsh"][1] < R
    # a row with the best row's L that is NOT a copy of it keeps its opponents
    x2 = X0[[1, 0, 3, 2]]
    t = rk.query_stats(np.stack([X0, X1, x2]), j, [4, 1, 4])
    assert t["L"][2] == t["L"][0] and t["best"] == 0 and t["ok"][0, 2] and t["opp"].tolist() == [-1, 0, 0]
    two = rk.query_stats(np.stack([X0, X1]), j, [4, 1])
    for key in ("kh", "wkh", "wsh"):
        assert s[key][:2].tolist() == two[key].tolist(), key                 # the copy changes nothing for the others


def test_span_zero_span_one_and_single_entry():
    R = 65
    out = rk.rell_kh(np.zeros((3, 4)), [0], {0: [0, 1, 2]}, [3], R, 1, [9, 1, 4])
    assert all(out[key].tolist() == [R, R, R] for key in ("kh", "wkh", "wsh"))
    assert out["best"].tolist() == [False, True, False]               # every L is 0.0: the smaller branch id
    # span 1: a replicate is the site itself, c = 0; every pair has q = 0 and is skipped
    out = rk.rell_kh([[-1.0], [-2.0], [-1.0], [-1.5]], [1], {0: [0, 1, 2, 3]}, [3], R, 1, [7, 1, 7, 2])
    assert out["kh"].tolist() == [R, 0, R, 0] and out["wkh"].tolist() == [R] * 4 and out["wsh"].tolist() == [R] * 4
    rows = np.random.RandomState(1).uniform(-5.0, -1.0, (1, 9))
    out = rk.rell_kh(rows, [9], {0: [0]}, [0], R, 1, [2])
    assert out["kh"].tolist() == [R] and out["wkh"].tolist() == [R] and out["wsh"].tolist() == [R]


def stat_restatement(entries=3):
    s = rr.stat_input()
    Q = len(s["reads"])
    keep = np.flatnonzero(np.arange(3 * Q) % 3 < entries)
    args = (s["rows"][keep], [rr.STAT_SPAN] * Q, rk.group_by_query(s["seq"][keep]), list(range(Q)), rr.STAT_R, 1, s["branch"][keep])
    return Q, rk.rell_kh(*args), rt.rell_tests(*args)


def test_invariants_on_the_statistical_input():
    R = rr.STAT_R
    Q, kh, sh = stat_restatement()
    # subtraction is monotone: c_b <= max c, so whatever KH counts SH counts too
    assert np.all(kh["kh"] <= sh["sh"])
    assert np.all(kh["kh"][kh["best"]] == R) and kh["best"].reshape(Q, 3).sum(axis=1).tolist() == [1] * Q
    # multiplication by w > 0 is monotone: t_k >= (c_k* - c_k) w >= (L_k* - L_k) w = T_k whenever weighted KH counts
    assert np.all(kh["wkh"] <= kh["wsh"])
    # the input is not vacuous: every column has values strictly inside (0, R) in at least a third of the reads
    for key in ("kh", "wkh", "wsh"):
        inside = int(np.sum(np.any((kh[key].reshape(Q, 3) > 0) & (kh[key].reshape(Q, 3) < R), axis=1)))
        assert 3 * inside >= Q, (key, inside)
    # two rows: KH is SH
    Q, kh2, sh2 = stat_restatement(entries=2)
    assert np.array_equal(kh2["kh"], sh2["sh"]) and np.any((kh2["kh"] > 0) & (kh2["kh"] < R))
    # w is symmetric, bit for bit, and so is the set of skipped pairs
    s = rr.stat_input()
    for q in range(Q):
        w, ok = rk.pair_scale(s["rows"][3 * q:3 * q + 3])
        assert np.array_equal(w, w.T) and np.array_equal(ok, ok.T) and ok.sum() == 6


def test_best_row_has_all_three_equal_to_one():
    """p_kh by its own rule (c_b - c_b = 0 >= 0); p_wkh and p_wsh because the best row has no opponent.  The formulas
    alone, with the row nearest below as the opponent, would give 0.655 .. 0.970 and 0.781 .. 0.996 here."""
    Q, kh, _ = stat_restatement()
    b = kh["best"]
    assert b.sum() == Q and np.all(kh["kh"][b] == rr.STAT_R)
    assert np.all(kh["wkh"][b] == rr.STAT_R) and np.all(kh["wsh"][b] == rr.STAT_R)


def test_restatement_against_multinomial_resampling():
    s = rr.stat_input()
    cpu = rk.stat_kh()
    Q, kh, _ = stat_restatement()
    worst = {}
    for key in ("kh", "wkh", "wsh"):
        p = kh[key] / float(rr.STAT_R)
        worst[key] = float(np.max(np.abs(p - cpu["p_" + key]) / rk.six_sigma(p, cpu["p_" + key], rr.STAT_R)))
    print("\n%d values of %d reads: max |restatement - default_rng| / bound: p_kh %.3g, p_wkh %.3g, p_wsh %.3g"
          % (len(s["seq"]), Q, worst["kh"], worst["wkh"], worst["wsh"]))
    assert all(v <= 1.0 for v in worst.values())


# ---- the executable: refused before any device is touched, named by --help

def test_kh_needs_rescore_and_rell(tmp_path):
    for tag, extra, rescore in (("a", ["--kh"], True), ("b", ["--kh"], False), ("c", ["--kh", "--posterior"], True),
                                ("d", ["--rell", "100", "--kh"], False)):
        sub = tmp_path / tag
        sub.mkdir()
        r = refused(sub, extra, rescore)
        assert "--kh" in r.stderr and "place first" in r.stderr and "--rescore out.jplace --rell N --kh" in r.stderr, r.stderr


def test_help_names_the_flag_and_the_fields():
    text = subprocess.run([hostlib.cli_exe(), "--help"], capture_output=True, text=True, timeout=60).stdout
    for word in ("--kh", '"p_kh"', '"p_wkh"', '"p_wsh"'):
        assert word in text
