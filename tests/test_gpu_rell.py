"""epa_dev_rell_support (Evaluator.rell_support): RELL bootstrap support of competing placements.

  1. exact counts: support x R equals, as integers and entry for entry, the numpy restatement of the specification
     (tests/rell_ref.py: Philox4x32-10, the counter layout, sequential fp64 adds, the tie rule) fed with the device's
     own site_lnl rows.  Shapes: spans 1, 3, 30, 63, 64, 65, 96, 150, ... 200 with 1, 2, 3 and all B entries per query
     (D5) at R = 1, 64, 65 and 1000; 20 states (A4); windows of 1536, 1537 and 1700 sites on either side of the LDS
     tile's limit (L); a 40-tip tree whose 300-site read competes on all 77 branches (184 800 bytes of site rows: more
     than the LDS of a compute unit, so the entries are worked off in tiles); a query with 1100 entries (more than
     the kernel counts in LDS).
  2. order and reproducibility: query-major and branch-major order of the same entries give the same support per
     entry; a duplicated entry follows the tie rule; stream_id = arange(Q) is the default, other ids give other
     draws; two seeds differ, one seed twice gives equal bits; the counts of a query add up to R exactly.
  3. argument checks and the "rell" timer.
  4. against CPU proportions: on the input of the CPU statistical test (22 reads of 30 sites on D5, three branches
     each) the device's support at R = 4096 is within six standard deviations of the difference of two binomial
     proportions (+ 1 / R) of plain default_rng multinomial resampling of the BRUTE-FORCE rows: this check shares
     neither the generator nor the site values with the device.

Measured on MI355X: test 4, largest |device - default_rng| / bound 0.44 (66 proportions).
"""
import functools

import numpy as np
import pytest

import brute_cases as bc
import epa_ng_amd as epa
import rell_ref as rr
from epa_ng_amd import hostlib
from gen_golden import DEFAULT_BL
from test_gpu_score_at import evaluator, make_pairs, queries, reference

pytestmark = pytest.mark.gpu

PENDANTS = (1e-4, DEFAULT_BL, 0.3, 2.5)
FRACTIONS = (0.0, 0.3, 0.5, 1.0)


def entry_lists(B, lengths, per_query):
    """per_query: entries of query q (an int: that many branches spread over the tree, "all": every branch) ->
    query-major (branch ids, read ids, pendant, distal)"""
    pb, ps = [], []
    for q, k in enumerate(per_query):
        br = np.arange(B) if k == "all" else (np.arange(k) * (B // 3) + q) % B
        pb += list(br)
        ps += [q] * len(br)
    pb, ps = np.array(pb, np.int64), np.array(ps, np.int64)
    i = np.arange(len(pb))
    return pb, ps, np.array(PENDANTS)[i % 4], np.array(FRACTIONS)[(i // 2) % 4] * lengths[pb]


def check_exact(ev, codes, wb, ws, pb, ps, pen, dis, R, seed=1, stream_id=None):
    """device support against the restatement on the device's own rows -> (support, counts)"""
    pairs = make_pairs(pb, ps)
    rows = ev.site_lnl(pairs, pen, dis, codes, wb, ws)
    sup = ev.rell_support(pairs, pen, dis, codes, wb, ws, R, seed=seed, stream_id=stream_id)
    sid = np.arange(len(ws)) if stream_id is None else stream_id
    want = rr.rell_counts(rows, ws, rr.group_by_query(ps), sid, R, seed, pb)
    got = np.rint(sup * R).astype(np.int64)
    assert np.array_equal(sup, got / float(R))                 # support is count / R, nothing else
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    for members in rr.group_by_query(ps).values():
        assert got[members].sum() == R
    return sup, got


@pytest.mark.parametrize("name,R", [("D5", 1), ("D5", 64), ("D5", 65), ("D5", 1000), ("A4", 65), ("A4", 1000), ("L", 65)])
def test_exact_counts(name, R):
    bf = bc.brute(name)
    codes, wb, ws = queries(name)
    ws = np.array(ws).copy()
    if name == "D5":
        assert [int(x) for x in ws[:5]] == [1, 3, 30, 64, 65] and ws[3] == 64 and ws[9] == 160
        ws[7], ws[9] = 63, 150                                # 128 -> 63, 160 -> 150: windows cut short at their end
    if name == "L":
        assert sorted(int(x) for x in ws) == [90, 1536, 1537, 1700]
    Q = len(ws)
    per_query = [(1, 2, 3, "all")[(q + 1) % 4] for q in range(Q)]
    pb, ps, pen, dis = entry_lists(bf.B, bf.lengths, per_query)
    ev = evaluator(name, "plain")
    if name == "L":
        # 1500 sites and more decide between branches at arbitrary lengths in every replicate.  Every read on all B
        # branches at the optimiser's own lengths, and again with the pendant length 1 % longer: at an optimum the
        # lnL is stationary in the pendant length, so the two entries of the best branch differ at first order site by
        # site and at second order in the sum, and the replicates go both ways
        pb, ps = np.tile(np.repeat(np.arange(bf.B), Q), 2), np.tile(np.arange(Q), 2 * bf.B)
        res = ev.thorough(make_pairs(pb[:bf.B * Q], ps[:bf.B * Q]), codes, wb, ws)
        pen = np.concatenate([res["pendant_length"], 1.01 * res["pendant_length"]])
        dis = np.tile(np.minimum(res["distal_length"], bf.lengths[pb[:bf.B * Q]]), 2)
    _, got = check_exact(ev, codes, wb, ws, pb, ps, pen, dis, R, seed=R + 7)
    if R >= 64:
        undecided = sum(1 for m in rr.group_by_query(ps).values() if len(m) > 1 and got[m].max() < R)
        print("\n%s R %d: %d entries, %d of %d queries with more than one winner" % (name, R, len(pb), undecided, Q))
        assert undecided >= 2                                 # the comparison is not one of trivial winners only


@functools.lru_cache(maxsize=None)
def wide_case():
    """40 tips (B = 77), 320 sites, reads of 300 and 150 sites"""
    c = bc._simulated(4, 40, 320, (300, 150), 8000)
    c["rates"], c["weights"] = bc.free_rates(4, 8004)
    ref = hostlib.Reference(c["newick"], c["labels"], c["seqs"], states=4, subst=c["subst"], freqs=c["freqs"],
                            rates=c["rates"], weights=c["weights"], pinv=0.0)
    lengths = np.array([ref.branch(b)["length"] for b in range(ref.B)])
    return c, ref, ref.evaluator(), lengths


def test_tiled_query_larger_than_lds():
    c, ref, ev, lengths = wide_case()
    assert ref.B == 77
    codes, wb, ws = epa.encode_queries(4, c["reads"], compact=True)
    assert [int(x) for x in ws] == [300, 150] and ref.B * 300 * 8 > 160 * 1024
    pb, ps, pen, dis = entry_lists(ref.B, lengths, ["all", "all"])
    _, got = check_exact(ev, codes, wb, ws, pb, ps, pen, dis, 300, seed=5)
    assert np.count_nonzero(got) > 2


def test_more_entries_than_lds_counters():
    name = "D5"
    bf = bc.brute(name)
    codes, wb, ws = queries(name)
    n = 1100
    # query 1 (3 sites): 1100 entries over all branches, every (branch, lengths) combination several times; query 2: three
    pb = np.concatenate([np.arange(n) % bf.B, [0, 5, 9]])
    ps = np.concatenate([np.full(n, 1), [2, 2, 2]])
    i = np.arange(len(pb))
    pen, dis = np.array(PENDANTS)[(i // bf.B) % 4], np.array(FRACTIONS)[(i // (4 * bf.B)) % 4] * bf.lengths[pb]
    _, got = check_exact(evaluator(name, "plain"), codes, wb, ws, pb, ps, pen, dis, 64, seed=11)
    # duplicates (entries 0 and 4 * 4 * B are the same placement) never win: the tie rule prefers the smaller index
    assert got[4 * 4 * bf.B:n].sum() == 0


def test_order_and_reproducibility():
    name = "D5"
    bf = bc.brute(name)
    ev = evaluator(name, "plain")
    codes, wb, ws = queries(name)
    Q, R = len(ws), 200
    pb, ps, pen, dis = entry_lists(bf.B, bf.lengths, [3, "all"] * (Q // 2))

    def run(order=None, **kw):
        o = np.arange(len(pb)) if order is None else order
        out = np.empty(len(pb))
        out[o] = ev.rell_support(np.ascontiguousarray(make_pairs(pb, ps)[o]), pen[o], dis[o], codes, wb, ws, R, **kw)
        return out

    base = run()
    branch_major = np.lexsort((ps, pb))
    assert not np.array_equal(branch_major, np.arange(len(pb)))
    assert np.array_equal(run(branch_major), base)
    shuffled = np.random.RandomState(3).permutation(len(pb))
    # any order: equal placements keep their support as a set; without duplicates every entry keeps its own
    assert np.array_equal(run(shuffled), base)
    assert np.array_equal(run(), base)                                            # one seed twice: equal bits
    assert np.array_equal(run(stream_id=np.arange(Q)), base)                      # the default stream ids
    other = run(stream_id=np.arange(Q) + (1 << 33))
    assert not np.array_equal(other, base)
    assert not np.array_equal(run(seed=2), base) and not np.array_equal(run(seed=1 + (1 << 32)), base)
    counts = np.rint(base * R).astype(np.int64)
    for members in rr.group_by_query(ps).values():
        assert counts[members].sum() == R
    # a duplicated entry: the earlier index takes what the placement wins, the later one nothing
    top = int(np.argmax(np.where(ps == 1, base, -1.0)))
    assert base[top] > 0
    dup = np.concatenate([np.arange(len(pb)), [top]])
    got = ev.rell_support(np.ascontiguousarray(make_pairs(pb, ps)[dup]), pen[dup], dis[dup], codes, wb, ws, R)
    assert np.array_equal(got[:-1], base) and got[-1] == 0.0
    dup = np.concatenate([[top], np.arange(len(pb))])
    got = ev.rell_support(np.ascontiguousarray(make_pairs(pb, ps)[dup]), pen[dup], dis[dup], codes, wb, ws, R)
    assert got[0] == base[top] and got[1 + top] == 0.0


def test_argument_checks_and_timer():
    name = "D5"
    bf = bc.brute(name)
    ev = reference(name).evaluator()
    codes, wb, ws = queries(name)
    Q = len(ws)
    pb, ps, pen, dis = entry_lists(bf.B, bf.lengths, [2] * Q)
    pairs = make_pairs(pb, ps)
    assert ev.kernel_ms("rell") < 0
    sup = ev.rell_support(pairs, pen, dis, codes, wb, ws, 10)
    assert ev.kernel_ms("rell") > 0
    assert np.all((sup >= 0) & (sup <= 1))
    # an empty window: every score is 0.0, the smaller branch id takes everything
    ws0 = np.array(ws).copy()
    ws0[4] = 0
    sup = ev.rell_support(pairs, pen, dis, codes, wb, ws0, 10)
    m = np.flatnonzero(ps == 4)
    assert sorted(sup[m]) == [0.0, 1.0] and sup[m[np.argmin(pb[m])]] == 1.0
    for R in (0, (1 << 20) + 1):
        with pytest.raises(epa.EpaError) as e:
            ev.rell_support(pairs, pen, dis, codes, wb, ws, R)
        assert e.value.code == -1 and "replicates" in str(e.value)
    assert np.all(np.isfinite(ev.rell_support(pairs[:2], pen[:2], dis[:2], codes, wb, ws, 1 << 20)))
    for bad in (dict(pb=bf.B), dict(ps=Q), dict(pen=np.nan), dict(dis=-1e-9)):
        a = dict(pb=pb.copy(), ps=ps.copy(), pen=pen.copy(), dis=dis.copy())
        for k, v in bad.items():
            a[k][3] = v
        with pytest.raises(epa.EpaError) as e:
            ev.rell_support(make_pairs(a["pb"], a["ps"]), a["pen"], a["dis"], codes, wb, ws, 10)
        assert e.value.code == -1 and "entry 3" in str(e.value), (bad, str(e.value))
    assert ev.rell_support(make_pairs([], []), np.zeros(0), np.zeros(0), codes, wb, ws, 10).shape == (0,)


def test_against_cpu_proportions():
    s = rr.stat_input()
    ev = evaluator("D5", "plain")
    codes, wb, ws = epa.encode_queries(4, s["reads"], compact=True)
    assert np.all(np.asarray(ws) == rr.STAT_SPAN)
    sup = ev.rell_support(make_pairs(s["branch"], s["seq"]), s["pendant"], s["distal"], codes, wb, ws, rr.STAT_R)
    ratio = np.abs(sup - s["cpu"]) / rr.six_sigma(sup, s["cpu"], rr.STAT_R)
    print("\n%d proportions: max |device - default_rng on brute-force rows| / bound %.3g" % (len(sup), ratio.max()))
    assert np.all(ratio <= 1.0)
