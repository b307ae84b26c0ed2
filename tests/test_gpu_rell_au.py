"""epa_dev_rell_au (Evaluator.rell_au): the p-value of the approximately unbiased test of competing placements from
multiscale RELL replicates.

  1. exact and near-exact: the counts equal, as integers and entry for entry at every scale, the numpy restatement of the
     specification (tests/rell_au_ref.py) fed with the device's own site_lnl rows, and add up to R per query and scale;
     p_au and fit = (d, c) agree with the restatement's fit on those counts to AU_TOL; where the fit does not apply p_au
     has the bits of count / R at the scale nearest 1000 and fit is NaN; a single entry gets exactly 1.  Shapes: the
     spans 1, 3, 30, 64, 65, 63, 150, ... of D5 (more draws than sites, draw counts that are no multiple of 4, equal draw
     counts at several scales) with 1, 2, 3, 4, 5, 8, 9 and all B entries per query (tile remainders, several tiles) at
     R = 1, 65, 257 and 1000; 20 states (A4); windows of 90, 1536, 1537 and 1700 sites (L: either side of the LDS tile's
     limit, 1.4 x the draws); the 40-tip tree with 77 entries x 300 and 150 sites (770 counters: in LDS); 1100 entries
     on one 3-site query (11 000 counters: global atomics).
  2. scales: one scale takes the fallback everywhere; three and sixteen are accepted; seventeen, none, 99 and 4001 refused.
  3. outputs asked for singly; one call twice gives equal bits; other seeds and stream ids differ; the "rell_au" timer;
     an empty window; rell_tests gives the same bits before and after a large rell_au call on the same context.
  4. against CPU proportions: on the 22 x 3 x 30-site input of the statistical tests at R = 4096 the proportions of all
     ten scales are within rell_ref.six_sigma of default_rng multinomial resampling of the BRUTE-FORCE rows at n'_s draws.

Measured on MI355X: test 1, largest |p_au - restatement| 5.5e-15 and |fit - restatement| 4.75e-14 (D5 at R = 1000; 2.6e-15
and 1.15e-14 on A4, 6.3e-16 and 3.2e-15 on L, 3.7e-15 and 1.35e-14 on the 1100 entries), 6 to 7 of D5's and A4's queries
with a fitted p_au strictly inside (0, 1), all of L's, the wide case's and the 1100-entry case's; test 2, 7.3e-15 and 1.1e-14
at sixteen scales; test 4, largest |device - default_rng| / bound 0.398 (660 proportions), 19 of 22 reads with a fitted entry.
"""
import numpy as np
import pytest

import brute_cases as bc
import epa_ng_amd as epa
import rell_au_ref as ra
import rell_ref as rr
from test_gpu_rell import FRACTIONS, PENDANTS, entry_lists, wide_case
from test_gpu_rell_tests import PER_QUERY
from test_gpu_score_at import evaluator, make_pairs, queries, reference

pytestmark = pytest.mark.gpu

# 100 x e, e = 3.2e-14 the float64 restatement's own error against the fit at 50 digits (rell_au_ref.AU_E, measured
# 3.15e-14 by tests/test_rell_au_cpu.py::test_fit_error); the factor covers normcdfinv / normcdf of the device differing
# from scipy's by a few ulp each through the same conditioning
AU_TOL = max(100.0 * ra.AU_E, 1e-12)


def check(ev, codes, wb, ws, pb, ps, pen, dis, R, seed=1, stream_id=None, scales=None, min_fitted=2):
    """the three outputs against the restatement on the device's own rows, and the properties every answer has ->
    (outputs, the restatement's counts)"""
    pairs = make_pairs(pb, ps)
    scale_pm = ra.DEFAULT_SCALES if scales is None else tuple(int(x) for x in scales)
    S, n = len(scale_pm), len(pb)
    rows = ev.site_lnl(pairs, pen, dis, codes, wb, ws)
    got = ev.rell_au(pairs, pen, dis, codes, wb, ws, R, seed=seed, stream_id=stream_id, scales=scales)
    assert sorted(got) == ["counts", "fit", "p_au"]
    assert got["counts"].shape == (S, n) and got["counts"].dtype == np.uint32
    assert got["p_au"].shape == (n,) and got["fit"].shape == (n, 2) and got["p_au"].dtype == got["fit"].dtype == np.float64
    sid = np.arange(len(ws)) if stream_id is None else stream_id
    groups = rr.group_by_query(ps)
    want = ra.ms_counts(rows, ws, groups, sid, R, seed, pb, scale_pm)
    counts = got["counts"].astype(np.int64)
    assert np.array_equal(counts, want), np.argwhere(counts != want)[:10]
    want_p, want_fit = ra.au_all(counts, ws, ps, R, scale_pm)
    fitted = ~np.isnan(want_fit[:, 0])
    assert np.array_equal(np.isnan(got["fit"]), np.isnan(want_fit))            # the same entries take the fallback, d and c together
    assert np.array_equal(got["p_au"][~fitted], want_p[~fitted])                # count / R, nothing else
    star = ra.fallback_scale(scale_pm)
    assert np.array_equal(got["p_au"][~fitted], counts[star][~fitted] / float(R))
    err_p = float(np.max(np.abs(got["p_au"] - want_p)))
    err_fit = float(np.max(np.abs(got["fit"][fitted] - want_fit[fitted]))) if fitted.any() else 0.0
    inside = 0
    for members in groups.values():
        assert np.all(counts[:, members].sum(axis=1) == R)
        if len(members) == 1:
            assert got["p_au"][members[0]] == 1.0 and np.all(np.isnan(got["fit"][members[0]]))
        m = np.array(members)
        inside += bool(np.any(fitted[m] & (got["p_au"][m] > 0.0) & (got["p_au"][m] < 1.0)))
    print("\n%d entries of %d queries, R %d, %d scales: %d fitted; max |p_au - restatement| %.3g, |fit - restatement| %.3g; "
          "%d queries with a fitted p_au in (0, 1)" % (n, len(groups), R, S, int(fitted.sum()), err_p, err_fit, inside))
    assert np.all((got["p_au"] >= 0.0) & (got["p_au"] <= 1.0))
    assert err_p <= AU_TOL and err_fit <= AU_TOL
    if R >= 64:
        assert inside >= min_fitted                            # the comparison is not one of fallback values only
    return got, want


@pytest.mark.parametrize("name,R", [("D5", 1), ("D5", 65), ("D5", 257), ("D5", 1000), ("A4", 65), ("L", 65)])
def test_exact_and_near_exact(name, R):
    bf = bc.brute(name)
    codes, wb, ws = queries(name)
    ws = np.array(ws).copy()
    if name == "D5":
        assert [int(x) for x in ws[:5]] == [1, 3, 30, 64, 65] and ws[7] == 128 and ws[9] == 160
        ws[7], ws[9] = 63, 150                                # windows cut short at their end
    if name == "L":
        assert sorted(int(x) for x in ws) == [90, 1536, 1537, 1700]
    Q = len(ws)
    per_query = [PER_QUERY[(q + 1) % 8] for q in range(Q)]
    if name == "D5":
        assert set(per_query) == set(PER_QUERY)
    pb, ps, pen, dis = entry_lists(bf.B, bf.lengths, per_query)
    ev = evaluator(name, "plain")
    if name == "L":
        # as test_gpu_rell: every read on all B branches at the optimiser's own lengths, and again with the pendant
        # length 1 % longer, so that the replicates of 1500 sites and more go both ways
        pb, ps = np.tile(np.repeat(np.arange(bf.B), Q), 2), np.tile(np.arange(Q), 2 * bf.B)
        res = ev.thorough(make_pairs(pb[:bf.B * Q], ps[:bf.B * Q]), codes, wb, ws)
        pen = np.concatenate([res["pendant_length"], 1.01 * res["pendant_length"]])
        dis = np.tile(np.minimum(res["distal_length"], bf.lengths[pb[:bf.B * Q]]), 2)
    check(ev, codes, wb, ws, pb, ps, pen, dis, R, seed=R + 7)


def test_tiled_query_larger_than_lds():
    c, ref, ev, lengths = wide_case()
    codes, wb, ws = epa.encode_queries(4, c["reads"], compact=True)
    assert ref.B == 77 and [int(x) for x in ws] == [300, 150]
    pb, ps, pen, dis = entry_lists(ref.B, lengths, ["all", "all"])
    got, _ = check(ev, codes, wb, ws, pb, ps, pen, dis, 300, seed=5)
    assert np.count_nonzero(got["counts"][5]) > 2


def test_more_counters_than_lds_holds():
    name = "D5"
    bf = bc.brute(name)
    codes, wb, ws = queries(name)
    n = 1100
    assert ws[1] == 3 and n * 10 > 1024
    # query 1 (3 sites): 1100 entries over all branches, every (branch, lengths) combination several times; queries 2 and 3
    # (30 and 64 sites): every branch
    pb = np.concatenate([np.arange(n) % bf.B, np.arange(bf.B), np.arange(bf.B)])
    ps = np.concatenate([np.full(n, 1), np.full(bf.B, 2), np.full(bf.B, 3)])
    i = np.arange(len(pb))
    pen, dis = np.array(PENDANTS)[(i // bf.B) % 4], np.array(FRACTIONS)[(i // (4 * bf.B)) % 4] * bf.lengths[pb]
    got, _ = check(evaluator(name, "plain"), codes, wb, ws, pb, ps, pen, dis, 64, seed=11)
    # duplicates (entries 0 and 4 * 4 * B are the same placement): the tie rule gives every win to the earlier one
    twin = 4 * 4 * bf.B
    assert np.all(got["counts"][:, twin] == 0) and got["p_au"][twin] == 0.0


def test_custom_scales():
    name = "D5"
    bf = bc.brute(name)
    ev = evaluator(name, "plain")
    codes, wb, ws = queries(name)
    Q = len(ws)
    pb, ps, pen, dis = entry_lists(bf.B, bf.lengths, [PER_QUERY[q % 8] for q in range(Q)])
    # one scale: the fallback everywhere, the counts still those of the restatement
    got, _ = check(ev, codes, wb, ws, pb, ps, pen, dis, 65, seed=2, scales=[1000], min_fitted=0)
    assert np.all(np.isnan(got["fit"])) and np.array_equal(got["p_au"], got["counts"][0] / 65.0)
    check(ev, codes, wb, ws, pb, ps, pen, dis, 65, seed=2, scales=[700, 1000, 1300])
    # sixteen scales, out of order, the ends of the range, one value twice: streams go by index
    sixteen = [4000, 100, 500, 650, 800, 950, 1000, 1000, 1150, 1300, 1450, 1600, 2000, 2500, 3000, 333]
    got, _ = check(ev, codes, wb, ws, pb, ps, pen, dis, 65, seed=2, scales=sixteen)
    assert not np.array_equal(got["counts"][6], got["counts"][7])
    pairs = make_pairs(pb, ps)
    for bad in (list(range(500, 2200, 100)), [500, 99, 1000], [1000, 4001]):
        with pytest.raises(epa.EpaError) as e:
            ev.rell_au(pairs, pen, dis, codes, wb, ws, 10, scales=bad)
        assert e.value.code == -1 and "rell_au" in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        ev.rell_au(pairs, pen, dis, codes, wb, ws, 10, scales=[])


def test_outputs_singly_and_reproducibility():
    name = "D5"
    bf = bc.brute(name)
    ev = evaluator(name, "plain")
    codes, wb, ws = queries(name)
    Q = len(ws)
    pb, ps, pen, dis = entry_lists(bf.B, bf.lengths, [PER_QUERY[q % 8] for q in range(Q)])
    pairs = make_pairs(pb, ps)

    def same(a, b):
        return all(np.array_equal(a[key], b[key], equal_nan=True) for key in ("p_au", "counts", "fit"))

    both = ev.rell_au(pairs, pen, dis, codes, wb, ws, 257, seed=3)
    assert same(ev.rell_au(pairs, pen, dis, codes, wb, ws, 257, seed=3), both)               # one call twice: equal bits
    for want in (("p_au",), ("counts",), ("fit",), ("fit", "p_au")):
        got = ev.rell_au(pairs, pen, dis, codes, wb, ws, 257, seed=3, want=want)
        assert sorted(got) == sorted(want)
        for key in want:
            assert np.array_equal(got[key], both[key], equal_nan=True), key
    assert same(ev.rell_au(pairs, pen, dis, codes, wb, ws, 257, seed=3, stream_id=np.arange(Q)), both)   # the default stream ids
    for other in (dict(seed=3, stream_id=np.arange(Q) + (1 << 33)), dict(seed=4), dict(seed=3 + (1 << 32))):
        assert not np.array_equal(ev.rell_au(pairs, pen, dis, codes, wb, ws, 257, **other)["counts"], both["counts"])
    # the scale of 1000 per mille is a stream of its own, not the replicates of rell_support
    assert not np.array_equal(both["counts"][5] / 257.0, ev.rell_support(pairs, pen, dis, codes, wb, ws, 257, seed=3))
    # shuffled entries: the same counts and p-values per entry
    order = np.random.RandomState(3).permutation(len(pb))
    got = ev.rell_au(np.ascontiguousarray(pairs[order]), pen[order], dis[order], codes, wb, ws, 257, seed=3)
    assert np.array_equal(got["counts"], both["counts"][:, order])
    assert np.array_equal(got["p_au"], both["p_au"][order]) and np.array_equal(got["fit"], both["fit"][order], equal_nan=True)


def test_argument_checks_timer_and_call_history():
    name = "D5"
    bf = bc.brute(name)
    ev = reference(name).evaluator()
    codes, wb, ws = queries(name)
    Q = len(ws)
    pb, ps, pen, dis = entry_lists(bf.B, bf.lengths, [2] * Q)
    pairs = make_pairs(pb, ps)
    probe = ev.rell_tests(pairs, pen, dis, codes, wb, ws, 65, seed=4)
    assert ev.kernel_ms("rell_au") < 0
    got = ev.rell_au(pairs, pen, dis, codes, wb, ws, 10)
    assert ev.kernel_ms("rell_au") > 0 and ev.kernel_ms("rell") < 0
    assert np.all((got["p_au"] >= 0) & (got["p_au"] <= 1))
    # an empty window: every score is 0.0 at every scale, the tie rule gives every replicate to the smaller branch id
    ws0 = np.array(ws).copy()
    ws0[4] = 0
    got = ev.rell_au(pairs, pen, dis, codes, wb, ws0, 10)
    m = np.flatnonzero(ps == 4)
    first = m[np.argmin(pb[m])]
    assert np.all(got["counts"][:, first] == 10) and got["counts"][:, m].sum() == 100
    assert got["p_au"][first] == 1.0 and sorted(got["p_au"][m]) == [0.0, 1.0] and np.all(np.isnan(got["fit"][m]))
    # a single entry gets 1
    got = ev.rell_au(pairs[:1], pen[:1], dis[:1], codes, wb, ws, 10)
    assert got["p_au"].tolist() == [1.0] and got["counts"].tolist() == [[10]] * 10 and np.all(np.isnan(got["fit"]))
    with pytest.raises(epa.EpaError) as e:
        ev.rell_au(pairs, pen, dis, codes, wb, ws, 10, want=())
    assert e.value.code == -1 and "rell_au" in str(e.value)
    with pytest.raises(ValueError):
        ev.rell_au(pairs, pen, dis, codes, wb, ws, 10, want=("p_au", "p_sh"))
    for R in (0, (1 << 20) + 1):
        with pytest.raises(epa.EpaError) as e:
            ev.rell_au(pairs, pen, dis, codes, wb, ws, R)
        assert e.value.code == -1 and "rell_au" in str(e.value) and "replicates" in str(e.value)
    for bad in (dict(pb=bf.B), dict(ps=Q), dict(pen=np.nan), dict(dis=-1e-9)):
        a = dict(pb=pb.copy(), ps=ps.copy(), pen=pen.copy(), dis=dis.copy())
        for k, v in bad.items():
            a[k][3] = v
        with pytest.raises(epa.EpaError) as e:
            ev.rell_au(make_pairs(a["pb"], a["ps"]), a["pen"], a["dis"], codes, wb, ws, 10)
        assert e.value.code == -1 and "rell_au: entry 3" in str(e.value), (bad, str(e.value))
    got = ev.rell_au(make_pairs([], []), np.zeros(0), np.zeros(0), codes, wb, ws, 10)
    assert got["p_au"].shape == (0,) and got["counts"].shape == (10, 0) and got["fit"].shape == (0, 2)
    # a large call, then the probe again: rell_tests answers with the bits it gave on the fresh context
    big = entry_lists(bf.B, bf.lengths, ["all"] * Q)
    ev.rell_au(make_pairs(big[0], big[1]), big[2], big[3], codes, wb, ws, 300, seed=9)
    n = 1100
    ev.rell_au(make_pairs(np.arange(n) % bf.B, np.full(n, 1)), np.full(n, 0.05), np.zeros(n), codes, wb, ws, 64, seed=2)
    again = ev.rell_tests(pairs, pen, dis, codes, wb, ws, 65, seed=4)
    for key in ("support", "elw", "p_sh"):
        assert np.array_equal(again[key], probe[key]), key
    assert np.any((probe["elw"] > 0.01) & (probe["elw"] < 0.99))


def test_against_cpu_proportions():
    s = rr.stat_input()
    cpu = ra.stat_ms()
    ev = evaluator("D5", "plain")
    codes, wb, ws = epa.encode_queries(4, s["reads"], compact=True)
    assert np.all(np.asarray(ws) == rr.STAT_SPAN)
    got = ev.rell_au(make_pairs(s["branch"], s["seq"]), s["pendant"], s["distal"], codes, wb, ws, rr.STAT_R, want=("counts", "fit"))
    p = got["counts"] / float(rr.STAT_R)
    ratio = np.abs(p - cpu) / rr.six_sigma(p, cpu, rr.STAT_R)
    fitted = int(np.sum(np.any(~np.isnan(got["fit"][:, 0]).reshape(-1, 3), axis=1)))
    print("\n%d proportions: max |device - default_rng on brute-force rows| / bound %.3g; %d of %d reads with a fitted entry"
          % (p.size, ratio.max(), fitted, len(s["reads"])))
    assert 3 * fitted >= len(s["reads"])
    assert np.all(ratio <= 1.0)
