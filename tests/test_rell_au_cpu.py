"""The specification of epa_dev_rell_au (include/epa_dev.h) restated in numpy (tests/rell_au_ref.py): draw counts and
counters against tables written by hand, the fit against proportions it must recover exactly, its symmetry and its
fallbacks, its rounding error against the same fit at 50 digits, the multiscale replicates against plain multinomial
resampling with numpy's own generator on brute-force site rows, and what the executable refuses.  No device.

Measured here:
  exact recovery: largest error of p_au, d, c 7.99e-15
  fit error e, the largest |float64 restatement - 50-digit fit| on the 2396 count vectors of rell_au_ref.fit_error_set():
  p_au 1.67e-14, d 3.15e-14, c 1.54e-14, so e = 3.15e-14 (rell_au_ref.AU_E; AU_TOL of tests/test_gpu_rell_au.py is 100 e)
  restatement (Philox) against default_rng at the ten scales, 22 reads of 30 sites x 3 branches, R = 4096: largest
  |difference| / six_sigma bound 0.398 (660 proportions); 19 of the 22 reads have an entry on which the fit applies, so the
  input of rell_ref.stat_input() serves as it is
"""
import subprocess

import numpy as np
from scipy.special import ndtr

import rell_au_ref as ra
import rell_ref as rr
from epa_ng_amd import hostlib
from test_rell_tests_cpu import refused


def test_draw_counts():
    assert list(ra.DEFAULT_SCALES) == list(range(500, 1500, 100))
    assert ra.draw_counts(0) == [0] * 10
    assert ra.draw_counts(1) == [1] * 10
    assert ra.draw_counts(2) == [1, 1, 1, 2, 2, 2, 2, 2, 3, 3]
    assert ra.draw_counts(3) == [2, 2, 2, 2, 3, 3, 3, 4, 4, 4]
    assert ra.draw_counts(30) == [15, 18, 21, 24, 27, 30, 33, 36, 39, 42]
    # 1537 x 0.5 = 768.5 rounds up, x 0.7 = 1075.9, x 0.9 = 1383.3, x 1.1 = 1690.7, x 1.3 = 1998.1
    assert ra.draw_counts(1537) == [769, 922, 1076, 1230, 1383, 1537, 1691, 1844, 1998, 2152]
    assert ra.draw_counts(7, [100, 4000, 1000]) == [1, 28, 7] and ra.draw_counts(4, [100]) == [1]   # 0.4 rounds to 0: one draw


def test_counter():
    seed, t, n_q = 5, 9 + (3 << 32), 30
    # word 1 of scale 0, replicate 0 is 1 << 20; the draw is word d % 4 of block d / 4
    w = rr.philox4x32_10((0, 1 << 20, t & rr.MASK, t >> 32), (seed, 0))
    j = ra.ms_draws(n_q, 4, 1, 0, t, seed)
    assert j.tolist() == [[(int(x) * n_q) >> 32 for x in w]]
    w = rr.philox4x32_10((1, (3 << 20) | 7, t & rr.MASK, t >> 32), (seed, 0))
    assert ra.ms_draws(n_q, 7, 8, 2, t, seed)[7, 4:].tolist() == [(int(x) * n_q) >> 32 for x in w[:3]]
    # scale 1000 of the default ten (index 5) makes n_q draws, and they are not those of the plain RELL call
    assert ra.draw_counts(n_q)[5] == n_q
    ms, plain = ra.ms_draws(n_q, n_q, 64, 5, t, seed), rr.draws(n_q, 64, t, seed)
    assert ms.shape == plain.shape and not np.array_equal(ms, plain) and np.mean(ms == plain) < 0.2
    assert not np.array_equal(ra.ms_draws(n_q, n_q, 64, 4, t, seed), ms)          # another scale, another stream
    assert ms.min() >= 0 and ms.max() < n_q
    # more draws than sites still draw from the n_q sites
    many = ra.ms_draws(3, 12, 257, 9, 1, 1)
    assert many.shape == (257, 12) and sorted(set(many.ravel().tolist())) == [0, 1, 2]


def test_ms_counts_on_hand_made_rows():
    R, spans = 257, [13, 1, 0]
    rng = np.random.RandomState(5)
    rows = rng.uniform(-9.0, -1.0, (8, 13))
    groups = {0: [0, 2, 4, 6, 7], 1: [1, 3], 2: [5]}
    branch = [3, 1, 4, 1, 5, 9, 2, 6]
    got = ra.ms_counts(rows, spans, groups, [7, 8, 9], R, 3, branch)
    assert got.shape == (10, 8) and got.dtype == np.int64
    for members in groups.values():
        assert np.all(got[:, members].sum(axis=1) == R)                          # every scale's counts add up to R
    assert np.all(got[:, 5] == R)                                                # a single entry, span 0
    # span 1: every scale draws the one site once, the larger value wins every replicate of every scale
    assert got[:, [1, 3]].tolist() == [[R, 0] if rows[1, 0] > rows[3, 0] else [0, R]] * 10
    assert len({tuple(x) for x in got[:, groups[0]].tolist()}) > 1               # the scales differ
    # a query alone gives the same counts; a custom list of scales selects the streams by index, not by value
    alone = ra.ms_counts(rows, spans, {0: groups[0]}, [7, 8, 9], R, 3, branch)
    assert np.array_equal(alone[:, groups[0]], got[:, groups[0]])
    sub = ra.ms_counts(rows, spans, {0: groups[0]}, [7, 8, 9], R, 3, branch, scale_pm=[500, 600])
    assert np.array_equal(sub[:, groups[0]], got[:2][:, groups[0]])
    moved = ra.ms_counts(rows, spans, {0: groups[0]}, [7, 8, 9], R, 3, branch, scale_pm=[600])
    assert not np.array_equal(moved[0, groups[0]], got[1, groups[0]])


def test_exact_recovery():
    """the model is linear in (d, c): exact proportions 1 - Phi(d sqrt(r) + c / sqrt(r)) give (d, c) back up to rounding
    times the conditioning of the 2 x 2 system"""
    worst = 0.0
    for d, c in ((1.2, 0.3), (-0.5, -0.8), (0.0, 0.4), (2.0, -0.5)):
        for n_q in (3, 30, 1537):
            n_draws = ra.draw_counts(n_q)
            p = ra.model_proportions(d, c, n_draws, n_q)
            p_au, d_fit, c_fit = ra.au_fit(p, n_draws, n_q)
            worst = max(worst, abs(p_au - ndtr(c - d)), abs(d_fit - d), abs(c_fit - c))
            assert abs(p_au - ndtr(c - d)) <= 1e-9 and abs(d_fit - d) <= 1e-9 and abs(c_fit - c) <= 1e-9, (d, c, n_q)
    print("\nexact recovery: largest error of p_au, d, c %.3g" % worst)


def test_two_entries_are_complementary():
    """z, d and c flip their signs, the weights stay: p_au[0] + p_au[1] = 1"""
    rng = np.random.default_rng(3)
    for R, n_q in ((257, 30), (1000, 3), (4096, 400)):
        n_draws = ra.draw_counts(n_q)
        first = rng.binomial(R, ra.model_proportions(0.4, 0.2, n_draws, n_q))
        assert ra.usable_scales(first / R, n_draws) is not None
        a, b = ra.au_fit(first, n_draws, n_q, R), ra.au_fit(R - first, n_draws, n_q, R)
        assert abs(a[0] + b[0] - 1.0) <= 1e-12 and abs(a[1] + b[1]) <= 1e-12 and abs(a[2] + b[2]) <= 1e-12
        assert 0.0 < a[0] < 1.0


def test_fallbacks():
    R = 100
    n30, n1 = ra.draw_counts(30), ra.draw_counts(1)
    isnan = lambda out: np.isnan(out[1]) and np.isnan(out[2])   # noqa: E731
    out = ra.au_fit([R] * 10, n30, 30, R)
    assert out[0] == 1.0 and isnan(out)
    out = ra.au_fit([0] * 10, n30, 30, R)
    assert out[0] == 0.0 and isnan(out)
    out = ra.au_fit([0, 0, 0, 0, 0, 7, 12, R, R, R], n30, 30, R)            # two usable scales only
    assert out[0] == 0.07 and isnan(out)
    out = ra.au_fit([40, 50, 60, 0, 0, 0, 0, 0, 0, 0], n1, 1, R)            # three usable scales, one distinct n' (span 1)
    assert out[0] == 0.0 and isnan(out)
    out = ra.au_fit([3, 5, 8, 0, 0, 9, 0, 0, 0, 0], n1, 1, R)
    assert out[0] == 0.09 and isnan(out)
    assert not isnan(ra.au_fit([40, 50, 60, 0, 0, 0, 0, 0, 0, 0], n30, 30, R))   # the same counts at span 30 are fitted
    # the scale nearest 1000, ties to the smaller index
    assert ra.fallback_scale(ra.DEFAULT_SCALES) == 5 and ra.fallback_scale([900, 1100]) == 0
    assert ra.fallback_scale([700, 1300, 1200]) == 2 and ra.fallback_scale([4000]) == 0
    assert ra.au_fit([3, 9], [27, 33], 30, 10, scale_pm=[900, 1100])[0] == 0.3
    # the 50-digit version takes the same path
    out = ra.au_fit_mp([0, 0, 0, 0, 0, 7, 12, R, R, R], n30, 30, R)
    assert float(out[0]) == 0.07 and isnan((0, float(out[1]), float(out[2])))


def test_fit_error():
    """e: the float64 restatement against the same fit at 50 digits.  AU_TOL of the device test is max(100 e, 1e-12)"""
    vectors = ra.fit_error_set()
    assert len(vectors) >= 2000
    e = {"p_au": 0.0, "d": 0.0, "c": 0.0}
    for counts, n_draws, n_q, R in vectors:
        got, want = ra.au_fit(counts, n_draws, n_q, R), ra.au_fit_mp(counts, n_draws, n_q, R)
        for key, g, w in zip(("p_au", "d", "c"), got, want):
            e[key] = max(e[key], abs(float(g - w)))
    print("\nfit error on %d count vectors: p_au %.3g, d %.3g, c %.3g" % (len(vectors), e["p_au"], e["d"], e["c"]))
    assert max(e.values()) <= ra.AU_E                    # the figure the device test's tolerance is built on still holds


def test_restatement_against_multinomial_resampling():
    s = rr.stat_input()
    cpu = ra.stat_ms()
    Q = len(s["reads"])
    counts = ra.ms_counts(s["rows"], [rr.STAT_SPAN] * Q, rr.group_by_query(s["seq"]), list(range(Q)), rr.STAT_R, 1, s["branch"])
    assert np.all(counts.reshape(10, Q, 3).sum(axis=2) == rr.STAT_R)
    p = counts / float(rr.STAT_R)
    ratio = np.abs(p - cpu) / rr.six_sigma(p, cpu, rr.STAT_R)
    # the input is not vacuous: at least a third of the reads have an entry on which the fit applies
    n_draws = ra.draw_counts(rr.STAT_SPAN)
    fitted = [any(ra.usable_scales(p[:, i], n_draws) is not None for i in range(3 * q, 3 * q + 3)) for q in range(Q)]
    p_au, _ = ra.au_all(counts, [rr.STAT_SPAN] * Q, s["seq"], rr.STAT_R)
    print("\n%d proportions of %d reads at ten scales: max |restatement - default_rng| / bound %.3g; %d reads with a fitted entry"
          % (p.size, Q, ratio.max(), sum(fitted)))
    assert 3 * sum(fitted) >= Q
    assert np.all(ratio <= 1.0)
    assert np.all((p_au >= 0.0) & (p_au <= 1.0))


# ---- the executable: refused before any device is touched, named by --help

def test_au_needs_rescore_and_rell(tmp_path):
    for tag, extra, rescore in (("a", ["--au"], False), ("b", ["--au"], True), ("c", ["--au", "--rell", "100"], False),
                                ("d", ["--au", "--posterior"], True)):
        sub = tmp_path / tag
        sub.mkdir()
        r = refused(sub, extra, rescore)
        assert "--au" in r.stderr and "--rescore out.jplace --rell N" in r.stderr, r.stderr


def test_help_names_the_flag_and_the_field():
    text = subprocess.run([hostlib.cli_exe(), "--help"], capture_output=True, text=True, timeout=60).stdout
    for word in ("--au", '"p_au"', "10000", "CONSEL"):
        assert word in text
