"""epa_dev_rell_tests (Evaluator.rell_tests): RELL support, expected likelihood weight and SH p-value of competing
placements from one set of replicates.

  1. exact and near-exact: support x R and p_sh x R equal, as integers and entry for entry, the numpy restatement of
     the specification (tests/rell_tests_ref.py) fed with the device's own site_lnl rows; elw agrees to 1e-12 (the bound
     of include/epa_dev.h: bit-exact scores, a few ulp from exp and the sums).  Shapes: the spans of test_gpu_rell
     (1, 3, 30, 63, 64, 65, 96, 150, ... on D5) with 1, 2, 3, 4, 5, 8, 9 and all B entries per query -- 4 | 5 and 8 | 9
     are tile boundaries, 8 the last count whose scores stay in registers -- at R = 1, 64, 65, 256, 257 (the
     replicate round's boundary) and 1000; 20 states (A4); windows of 1536, 1537 and 1700 sites (L); the 40-tip tree
     with 77 entries x 300 sites; 1100 entries on one query (more than the kernel accumulates in LDS).
  2. ties to the existing entry points: support has the bits of Evaluator.rell_support on every shape above; outputs
     asked for singly equal the same outputs asked for together.
  3. order and reproducibility: query-major, branch-major and shuffled order give equal p_sh and support bit for bit
     and elw within 1e-12; one seed twice gives equal bits; other seeds and stream ids differ; a duplicated entry gets
     its twin's elw and p_sh; elw adds up to 1 per query; the entry with the largest L has p_sh == 1.0.
  4. call history: a large call, a small one, rell_support, the small one again on one context: the small call's
     answers equal a fresh context's bit for bit.
  5. argument checks (those of rell_support, and all outputs left out) and the "rell_tests" timer.
  6. against CPU proportions: on the 22 x 3 x 30-site input of the statistical tests at R = 4096, elw and p_sh are within
     rell_ref.six_sigma of default_rng multinomial resampling of the BRUTE-FORCE rows, centred at those rows' own sums.

Measured on MI355X: test 1, largest |elw - restatement| 1.25e-14 (D5 at R = 1000; 4.8e-15 at R = 256, 1.1e-15 on A4,
2.2e-16 on the 1100 entries), 9 to 11 of D5's and A4's queries with a p_sh strictly inside (0, 1), all of L's and the
wide case's; test 6, largest |device - default_rng| / bound: elw 0.138, p_sh 0.23 (66 values each).
"""
import numpy as np
import pytest

import brute_cases as bc
import epa_ng_amd as epa
import rell_ref as rr
import rell_tests_ref as rt
from test_gpu_rell import FRACTIONS, PENDANTS, entry_lists, wide_case
from test_gpu_score_at import evaluator, make_pairs, queries, reference

pytestmark = pytest.mark.gpu

ELW_TOL = 1e-12
PER_QUERY = (1, 2, 3, "all", 4, 5, 8, 9)


def check(ev, codes, wb, ws, pb, ps, pen, dis, R, seed=1, stream_id=None):
    """the three outputs against the restatement on the device's own rows, and the properties every answer has ->
    (outputs, restatement)"""
    pairs = make_pairs(pb, ps)
    rows = ev.site_lnl(pairs, pen, dis, codes, wb, ws)
    got = ev.rell_tests(pairs, pen, dis, codes, wb, ws, R, seed=seed, stream_id=stream_id)
    assert sorted(got) == ["elw", "p_sh", "support"] and all(v.shape == (len(pb),) and v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got["support"], ev.rell_support(pairs, pen, dis, codes, wb, ws, R, seed=seed, stream_id=stream_id))
    sid = np.arange(len(ws)) if stream_id is None else stream_id
    groups = rt.group_by_query(ps)
    want = rt.rell_tests(rows, ws, groups, sid, R, seed, pb)
    wins, sh = np.rint(got["support"] * R).astype(np.int64), np.rint(got["p_sh"] * R).astype(np.int64)
    assert np.array_equal(got["support"], wins / float(R)) and np.array_equal(got["p_sh"], sh / float(R))   # count / R, nothing else
    assert np.array_equal(wins, want["wins"]), np.flatnonzero(wins != want["wins"])[:10]
    assert np.array_equal(sh, want["sh"]), np.flatnonzero(sh != want["sh"])[:10]
    err = float(np.max(np.abs(got["elw"] - want["elw"])))
    inside = 0
    for members in groups.values():
        assert wins[members].sum() == R
        assert abs(got["elw"][members].sum() - 1.0) <= ELW_TOL
        assert got["p_sh"][members[int(np.argmax(want["L"][members]))]] == 1.0
        inside += bool(np.any((got["p_sh"][members] > 0.0) & (got["p_sh"][members] < 1.0)))
    print("\n%d entries of %d queries, R %d: max |elw - restatement| %.3g; %d queries with a p_sh in (0, 1)"
          % (len(pb), len(groups), R, err, inside))
    assert err <= ELW_TOL
    if R >= 64:
        assert inside >= 2                                    # the comparison is not one of trivial values only
    return got, want


@pytest.mark.parametrize("name,R", [("D5", 1), ("D5", 64), ("D5", 65), ("D5", 256), ("D5", 257), ("D5", 1000), ("A4", 65), ("L", 65)])
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
    assert np.count_nonzero(got["elw"] > 1e-6) > 2


def test_more_entries_than_lds_accumulators():
    name = "D5"
    bf = bc.brute(name)
    codes, wb, ws = queries(name)
    n = 1100
    # query 1 (3 sites): 1100 entries over all branches, every (branch, lengths) combination several times; query 2: three
    pb = np.concatenate([np.arange(n) % bf.B, [0, 5, 9]])
    ps = np.concatenate([np.full(n, 1), [2, 2, 2]])
    i = np.arange(len(pb))
    pen, dis = np.array(PENDANTS)[(i // bf.B) % 4], np.array(FRACTIONS)[(i // (4 * bf.B)) % 4] * bf.lengths[pb]
    got, _ = check(evaluator(name, "plain"), codes, wb, ws, pb, ps, pen, dis, 64, seed=11)
    # duplicates (entries 0 and 4 * 4 * B are the same placement) share the weight and the p-value
    twin = 4 * 4 * bf.B
    assert got["p_sh"][twin] == got["p_sh"][0] and abs(got["elw"][twin] - got["elw"][0]) <= ELW_TOL and got["elw"][0] > 0


def test_outputs_asked_for_singly():
    name = "D5"
    bf = bc.brute(name)
    ev = evaluator(name, "plain")
    codes, wb, ws = queries(name)
    pb, ps, pen, dis = entry_lists(bf.B, bf.lengths, [PER_QUERY[q % 8] for q in range(len(ws))])
    pairs = make_pairs(pb, ps)
    both = ev.rell_tests(pairs, pen, dis, codes, wb, ws, 257, seed=3)
    for want in (("support",), ("elw",), ("p_sh",), ("p_sh", "support")):
        got = ev.rell_tests(pairs, pen, dis, codes, wb, ws, 257, seed=3, want=want)
        assert sorted(got) == sorted(want)
        for key in want:
            assert np.array_equal(got[key], both[key]), key


def test_order_and_reproducibility():
    name = "D5"
    bf = bc.brute(name)
    ev = evaluator(name, "plain")
    codes, wb, ws = queries(name)
    Q, R = len(ws), 200
    pb, ps, pen, dis = entry_lists(bf.B, bf.lengths, [3, "all"] * (Q // 2))

    def run(order=None, **kw):
        o = np.arange(len(pb)) if order is None else order
        got = ev.rell_tests(np.ascontiguousarray(make_pairs(pb, ps)[o]), pen[o], dis[o], codes, wb, ws, R, **kw)
        out = {}
        for key, v in got.items():
            out[key] = np.empty(len(pb))
            out[key][o] = v
        return out

    def same(a, b):
        return all(np.array_equal(a[key], b[key]) for key in ("support", "elw", "p_sh"))

    base = run()
    assert same(run(), base)                                                      # one seed twice: equal bits
    for order in (np.lexsort((ps, pb)), np.random.RandomState(3).permutation(len(pb))):
        assert not np.array_equal(order, np.arange(len(pb)))
        got = run(order)
        assert np.array_equal(got["p_sh"], base["p_sh"]) and np.array_equal(got["support"], base["support"])
        assert np.max(np.abs(got["elw"] - base["elw"])) <= ELW_TOL
    assert same(run(stream_id=np.arange(Q)), base)                                # the default stream ids
    for other in (run(stream_id=np.arange(Q) + (1 << 33)), run(seed=2), run(seed=1 + (1 << 32))):
        assert not np.array_equal(other["elw"], base["elw"]) and not np.array_equal(other["p_sh"], base["p_sh"])
    # a duplicated entry: the same elw and p_sh as its twin (support goes to the earlier index, as in rell_support)
    top = int(np.argmax(np.where(ps == 1, base["elw"], -1.0)))
    dup = np.concatenate([np.arange(len(pb)), [top]])
    got = ev.rell_tests(np.ascontiguousarray(make_pairs(pb, ps)[dup]), pen[dup], dis[dup], codes, wb, ws, R)
    assert got["p_sh"][-1] == got["p_sh"][top] and abs(got["elw"][-1] - got["elw"][top]) <= ELW_TOL
    assert got["support"][-1] == 0.0 and got["elw"][top] < base["elw"][top]
    for members in rr.group_by_query(ps[dup]).values():
        assert abs(got["elw"][members].sum() - 1.0) <= ELW_TOL


def test_call_history():
    name = "D5"
    bf = bc.brute(name)
    codes, wb, ws = queries(name)
    Q = len(ws)
    big = entry_lists(bf.B, bf.lengths, ["all"] * Q)
    n = 1100
    huge_b, huge_s = np.arange(n) % bf.B, np.full(n, 1)
    small = entry_lists(bf.B, bf.lengths, [0, 0, 2, 0, 3] + [0] * (Q - 5))

    def small_call(ev):
        pb, ps, pen, dis = small
        return ev.rell_tests(make_pairs(pb, ps), pen, dis, codes, wb, ws, 65, seed=4)

    fresh = small_call(reference(name).evaluator())
    ev = reference(name).evaluator()
    ev.rell_tests(make_pairs(big[0], big[1]), big[2], big[3], codes, wb, ws, 300, seed=9)
    ev.rell_tests(make_pairs(huge_b, huge_s), np.full(n, 0.05), np.zeros(n), codes, wb, ws, 64, seed=2)
    first = small_call(ev)
    ev.rell_support(make_pairs(big[0], big[1]), big[2], big[3], codes, wb, ws, 100)
    second = small_call(ev)
    for key in ("support", "elw", "p_sh"):
        assert np.array_equal(first[key], fresh[key]) and np.array_equal(second[key], fresh[key]), key
    assert np.any((fresh["p_sh"] > 0) & (fresh["p_sh"] < 1)) or np.any((fresh["elw"] > 0.01) & (fresh["elw"] < 0.99))


def test_argument_checks_and_timer():
    name = "D5"
    bf = bc.brute(name)
    ev = reference(name).evaluator()
    codes, wb, ws = queries(name)
    Q = len(ws)
    pb, ps, pen, dis = entry_lists(bf.B, bf.lengths, [2] * Q)
    pairs = make_pairs(pb, ps)
    assert ev.kernel_ms("rell_tests") < 0
    got = ev.rell_tests(pairs, pen, dis, codes, wb, ws, 10)
    assert ev.kernel_ms("rell_tests") > 0 and ev.kernel_ms("rell") < 0
    assert all(np.all((v >= 0) & (v <= 1)) for v in got.values())
    # an empty window: every score and every L is 0.0
    ws0 = np.array(ws).copy()
    ws0[4] = 0
    got = ev.rell_tests(pairs, pen, dis, codes, wb, ws0, 10)
    m = np.flatnonzero(ps == 4)
    assert sorted(got["support"][m]) == [0.0, 1.0] and got["support"][m[np.argmin(pb[m])]] == 1.0
    assert np.all(np.abs(got["elw"][m] - 0.5) <= ELW_TOL) and np.all(got["p_sh"][m] == 1.0)
    # a single entry gets 1, 1, 1
    got = ev.rell_tests(pairs[:1], pen[:1], dis[:1], codes, wb, ws, 10)
    assert [got[k].tolist() for k in ("support", "elw", "p_sh")] == [[1.0], [1.0], [1.0]]
    with pytest.raises(epa.EpaError) as e:
        ev.rell_tests(pairs, pen, dis, codes, wb, ws, 10, want=())
    assert e.value.code == -1 and "rell_tests" in str(e.value)
    with pytest.raises(ValueError):
        ev.rell_tests(pairs, pen, dis, codes, wb, ws, 10, want=("elw", "lwr"))
    for R in (0, (1 << 20) + 1):
        with pytest.raises(epa.EpaError) as e:
            ev.rell_tests(pairs, pen, dis, codes, wb, ws, R)
        assert e.value.code == -1 and "replicates" in str(e.value)
    got = ev.rell_tests(pairs[:2], pen[:2], dis[:2], codes, wb, ws, 1 << 20)
    assert all(np.all(np.isfinite(v)) for v in got.values()) and abs(got["elw"].sum() - 1.0) <= ELW_TOL
    for bad in (dict(pb=bf.B), dict(ps=Q), dict(pen=np.nan), dict(dis=-1e-9)):
        a = dict(pb=pb.copy(), ps=ps.copy(), pen=pen.copy(), dis=dis.copy())
        for k, v in bad.items():
            a[k][3] = v
        with pytest.raises(epa.EpaError) as e:
            ev.rell_tests(make_pairs(a["pb"], a["ps"]), a["pen"], a["dis"], codes, wb, ws, 10)
        assert e.value.code == -1 and "rell_tests: entry 3" in str(e.value), (bad, str(e.value))
    got = ev.rell_tests(make_pairs([], []), np.zeros(0), np.zeros(0), codes, wb, ws, 10)
    assert all(got[k].shape == (0,) for k in ("support", "elw", "p_sh"))


def test_against_cpu_proportions():
    s = rr.stat_input()
    cpu = rt.stat_tests()
    ev = evaluator("D5", "plain")
    codes, wb, ws = epa.encode_queries(4, s["reads"], compact=True)
    assert np.all(np.asarray(ws) == rr.STAT_SPAN)
    got = ev.rell_tests(make_pairs(s["branch"], s["seq"]), s["pendant"], s["distal"], codes, wb, ws, rr.STAT_R)
    r_elw = np.abs(got["elw"] - cpu["elw"]) / rt.six_sigma(got["elw"], cpu["elw"], rr.STAT_R)
    r_sh = np.abs(got["p_sh"] - cpu["p_sh"]) / rt.six_sigma(got["p_sh"], cpu["p_sh"], rr.STAT_R)
    print("\n%d values: max |device - default_rng on brute-force rows| / bound: elw %.3g, p_sh %.3g"
          % (len(r_elw), r_elw.max(), r_sh.max()))
    assert np.all(r_elw <= 1.0) and np.all(r_sh <= 1.0)
