"""epa_dev_score_at (Evaluator.score_at): the lnL of a placement at branch lengths the caller names, no optimiser.

The checkers are the independent log-space evaluator of tests/brute_force.py (BruteForce.score_pairs) and, where a free
proximal length is needed, the oracle (Oracle.score_at) -- on the configurations of tests/brute_cases.py, at lengths
the device's own optimiser never ends at: pendant 1e-4 .. 12, distal exactly 0 and exactly the branch's length, and
distal + proximal different from the branch's length.  Every bound is LNL_TOL = 1e-6, the suite's device bound.

  1. against the brute force on a grid away from optima: branches {0, B // 2, B - 1} x every read x pendant
     {1e-4, -ln 0.9, 2.5, 12} x distal {0, 0.3, 1} x branch length, for D1 D3 D5 (device precompute, host CLVs,
     blocked lookup layout, verbatim eigenvalues) D6 D16 A1 A4 (plain, aa_valu) A8 A9 S4 S20 (per-site and per-rate
     scalers) L Xlong Xshort; D5 resident and blocked are the same bits (the kernel reads only buffers the two
     layouts share).  A pendant of 1e-6 is not in the grid: through the eigenbasis exp(lambda r t) cancels like
     1 / pendant, and there the CPU restatement of the same arithmetic is itself 5e-7 .. 8e-7 from the brute force.
  2. explicit proximal lengths (distal + proximal on both sides of the branch's length) against the oracle, D5 and A4;
     proximal=None is bitwise proximal = length - distal.
  3. ties to the existing entry points, D5 and A4: score_at(-ln 0.9, length / 2) is the preplacement table, score_at at
     the lengths `thorough` returns is the lnL it returns (pairs that took the revert exit included).
  4. 4-bit packed, compact and full-width query rows give the same bits.
  5. entries are independent: D16's and A9's lists tiled and shuffled so that every wave runs several entries in a row
     with different tables; each result is bitwise the one of the entry submitted alone and in the unshuffled list.
  6. argument checks, n = 0, an empty window, the "score_at" timer.

Largest |device - checker| measured on MI355X (the tests print them):

    test 1, group                      |score_at - brute force|
    D  (4 states, 1 .. 16 categories)  1.7e-10
    A  (20 states, 1 .. 9 categories)  7.5e-09
    S  (ladders, both scaler modes)    1.2e-09
    L  (1700-site window)              8.7e-10
    X  (branch lengths 1e-6 .. 12)     Xlong 2.1e-10, Xshort 9.7e-08
    test 2, |score_at - oracle| with a free proximal length   2.7e-12
    test 3, |score_at - preplacement table|                   1.4e-12
    test 3, |score_at(returned lengths) - thorough's lnL|     4.5e-13  (54 / 21 reverted pairs among them)

Nearly every maximum sits at pendant 1e-4 with distal exactly 0.  That point is what the kernel's noise cut is for:
libpll and both checkers take P(0) as the exact identity, so the states a tip excludes are exactly 0 in the inner CLV;
the device holds the tip in the eigenbasis and U (U^-1 tip) leaves ~1e-16 there, which a pendant length of 1e-4 divides
by at every site where the query shows such a state.  Before the kernel took entries below the rounding-error bound of
their own sum as 0, the same table read D 1.4e-08, A 5.0e-07, S 2.4e-09, L 1.0e-08, Xlong 3.9e-10 and Xshort 2.2e-06,
above the bound.
"""
import functools

import numpy as np
import pytest

import brute_cases as bc
import epa_ng_amd as epa
from epa_ng_amd import hostlib
from gen_golden import DEFAULT_BL
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

LNL_TOL = 1e-6
PENDANTS = (1e-4, DEFAULT_BL, 2.5, 12.0)
DISTAL_FRACTIONS = (0.0, 0.3, 1.0)

PLAIN = dict(device_precompute=True, rate_scalers=False)
VARIANTS = {
    "plain": PLAIN,
    "host": dict(device_precompute=False, rate_scalers=False),
    "blocks": dict(PLAIN, blocks=True),
    "keep_eigenvalues": dict(PLAIN, keep_eigenvalues=True),
    "aa_valu": dict(PLAIN, options=(("aa_valu", 1),)),
    "rate_scalers": dict(device_precompute=True, rate_scalers=True),
}
GRID_CASES = [("D1", "plain"), ("D3", "plain"), ("D5", "plain"), ("D5", "host"), ("D5", "blocks"),
              ("D5", "keep_eigenvalues"), ("D6", "plain"), ("D16", "plain"), ("A1", "plain"), ("A4", "plain"),
              ("A4", "aa_valu"), ("A8", "plain"), ("A9", "plain"), ("S4", "plain"), ("S4", "rate_scalers"),
              ("S20", "plain"), ("S20", "rate_scalers"), ("L", "plain"), ("Xlong", "plain"), ("Xshort", "plain")]


@functools.lru_cache(maxsize=None)
def reference(name):
    c = bc.case(name)
    ref = hostlib.Reference(c["newick"], c["labels"], c["seqs"], states=c["states"], subst=c["subst"], freqs=c["freqs"],
                            rates=c["rates"], weights=c["weights"], pinv=c["pinv"])
    bf = bc.brute(name)
    assert ref.B == bf.B and ref.W == bf.W
    assert all(ref.branch(b)["length"] == bf.lengths[b] for b in range(bf.B))          # same edge numbering
    return ref


@functools.lru_cache(maxsize=None)
def evaluator(name, variant="plain"):
    v = VARIANTS[variant]
    ev = reference(name).evaluator(device_precompute=v["device_precompute"], rate_scalers=v["rate_scalers"],
                                   keep_eigenvalues=v.get("keep_eigenvalues", False),
                                   flags=epa.FLAG_LOOKUP_BLOCKS if v.get("blocks") else 0)
    assert ev.lookup_mode()[0] == (epa.LOOKUP_BLOCKS if v.get("blocks") else epa.LOOKUP_RESIDENT)
    for key, value in v.get("options", ()):
        ev.set_option(key, value)
    return ev


@functools.lru_cache(maxsize=None)
def queries(name, compact=True):
    c = bc.case(name)
    return epa.encode_queries(c["states"], c["reads"], compact=compact)


def make_pairs(pb, ps):
    pairs = np.zeros(len(pb), epa.PAIR_DTYPE)
    pairs["branch_id"], pairs["seq_id"] = pb, ps
    return pairs


@functools.lru_cache(maxsize=None)
def grid(name):
    """-> (branch ids, read ids, pendant, distal) of test 1's entries and the brute force's lnL at them"""
    c, bf = bc.case(name), bc.brute(name)
    Q = len(c["reads"])
    rows = [(b, q, p, f) for b in (0, bf.B // 2, bf.B - 1) for q in range(Q) for p in PENDANTS for f in DISTAL_FRACTIONS]
    assert len(rows) <= 504
    pb = np.array([r[0] for r in rows], np.int64)
    ps = np.array([r[1] for r in rows], np.int64)
    pen = np.array([r[2] for r in rows])
    dis = np.array([r[3] for r in rows]) * bf.lengths[pb]
    want = bf.score_pairs(pb, ps, c["reads"], pen, dis)
    for a in (pb, ps, pen, dis, want):
        a.setflags(write=False)
    return pb, ps, pen, dis, want


def score(name, variant, pb, ps, pen, dis, proximal=None):
    codes, wb, ws = queries(name)
    return evaluator(name, variant).score_at(make_pairs(pb, ps), pen, dis, codes, wb, ws, proximal=proximal)


# ---- 1. against the brute force, away from optima

@pytest.mark.parametrize("name,variant", GRID_CASES, ids=["%s-%s" % nv for nv in GRID_CASES])
def test_grid_against_brute_force(name, variant):
    pb, ps, pen, dis, want = grid(name)
    got = score(name, variant, pb, ps, pen, dis)
    assert np.all(np.isfinite(got))
    d = np.abs(got - want)
    worst = int(np.argmax(d))
    print("\n%s %s: %d entries, max |score_at - brute force| %.3g (branch %d read %d pendant %.3g distal %.3g)"
          % (name, variant, len(pb), d[worst], pb[worst], ps[worst], pen[worst], dis[worst]))
    assert d[worst] < LNL_TOL
    if name == "L":
        assert max(int(s) for s in queries(name)[2]) >= 1700
    if variant == "blocks":
        # refT and scSum are built the same way in both layouts and are all the kernel reads
        assert np.array_equal(got, score(name, "plain", pb, ps, pen, dis))


# ---- 2. explicit proximal length

@pytest.mark.parametrize("name", ["D5", "A4"])
def test_explicit_proximal_length_against_the_oracle(name):
    c, bf = bc.case(name), bc.brute(name)
    o = Oracle(c["newick"], c["labels"], c["seqs"], c["states"], c["subst"], c["freqs"], c["rates"], weights=c["weights"],
               pinv=c["pinv"])
    assert o.B == bf.B and all(o.branch_info(b)[0] == bf.lengths[b] for b in range(bf.B))
    reads = [0, 4, len(c["reads"]) - 1]
    pb = np.repeat(np.arange(bf.B), len(reads))
    ps = np.tile(np.array(reads), bf.B)
    length = bf.lengths[pb]
    worst = 0.0
    for pendant, fd, fx in ((0.3, 0.2, 0.5), (0.05, 1.1, 0.4)):
        pen, dis, prox = np.full(len(pb), pendant), fd * length, fx * length
        got = score(name, "plain", pb, ps, pen, dis, proximal=prox)
        want = o.score_at(pb, ps, c["reads"], pen, dis, proximal=prox)
        d = float(np.max(np.abs(got - want)))
        print("\n%s pendant %g distal %g x proximal %g x length: max |score_at - oracle| %.3g" % (name, pendant, fd, fx, d))
        worst = max(worst, d)
        assert d < LNL_TOL
    # proximal = None is the sliding rule's length - distal, the same bits
    pen, dis = np.full(len(pb), 0.3), 0.2 * length
    assert np.array_equal(score(name, "plain", pb, ps, pen, dis), score(name, "plain", pb, ps, pen, dis, proximal=length - dis))


# ---- 3. ties to the existing entry points

@pytest.mark.parametrize("name", ["D5", "A4"])
def test_ties_to_preplace_and_thorough(name):
    c, bf = bc.case(name), bc.brute(name)
    ev = evaluator(name, "plain")
    codes, wb, ws = queries(name)
    Q = len(c["reads"])
    pb, ps = np.repeat(np.arange(bf.B), Q), np.tile(np.arange(Q), bf.B)
    table = ev.preplace(codes, wb, ws)
    at_start = score(name, "plain", pb, ps, np.full(len(pb), DEFAULT_BL), bf.lengths[pb] / 2.0)
    d_pre = float(np.max(np.abs(at_start - table[ps, pb])))
    pb, ps = bc.pair_lists(c, bf.B)
    res = ev.thorough(make_pairs(pb, ps), codes, wb, ws)
    at_end = score(name, "plain", pb, ps, res["pendant_length"], res["distal_length"])
    d_th = float(np.max(np.abs(at_end - res["lnl"])))
    print("\n%s: max |score_at(start) - preplacement table| %.3g, |score_at(returned) - thorough lnL| %.3g (%d reverts)"
          % (name, d_pre, d_th, ev.last_stats["reverts"]))
    assert d_pre < LNL_TOL
    assert d_th < LNL_TOL


# ---- 4. query staging

def test_query_layouts_give_the_same_bits():
    name = "D5"
    pb, ps, pen, dis, _ = grid(name)
    ev, pairs = evaluator(name, "plain"), make_pairs(pb, ps)
    compact, wb, ws = queries(name, True)
    full, wb2, ws2 = queries(name, False)
    assert np.array_equal(wb, wb2) and np.array_equal(ws, ws2) and full.shape[1] == ev.W != compact.shape[1]
    a = ev.score_at(pairs, pen, dis, compact, wb, ws)
    b = ev.score_at(pairs, pen, dis, full, wb, ws)
    p = ev.score_at(pairs, pen, dis, epa.pack_codes_4bit(compact), wb, ws)
    assert np.array_equal(a, b) and np.array_equal(a, p)


# ---- 5. entries are independent

@pytest.mark.parametrize("name,total", [("D16", 5000), ("A9", 600)])
def test_entries_are_independent(name, total):
    pb, ps, pen, dis, _ = grid(name)
    n = len(pb)
    ev = evaluator(name, "plain")
    codes, wb, ws = queries(name)
    pairs = make_pairs(pb, ps)
    in_order = ev.score_at(pairs, pen, dis, codes, wb, ws)
    alone = np.array([ev.score_at(pairs[i:i + 1], pen[i:i + 1], dis[i:i + 1], codes, wb, ws)[0] for i in range(n)])
    assert np.array_equal(alone, in_order)
    idx = np.tile(np.arange(n), (total + n - 1) // n)[:total]
    np.random.RandomState(5).shuffle(idx)
    if name == "D16":
        assert total > 8 * 256          # more entries than the persistent grid has waves: every wave runs several
    shuffled = ev.score_at(np.ascontiguousarray(pairs[idx]), pen[idx], dis[idx], codes, wb, ws)
    assert np.array_equal(shuffled, alone[idx])


# ---- 6. argument checks

def test_argument_checks():
    name = "D5"
    c, bf = bc.case(name), bc.brute(name)
    ev = evaluator(name, "plain")
    codes, wb, ws = queries(name)
    Q = len(c["reads"])
    n, at = 5, 3
    b = bf.B // 2
    good = dict(pb=np.full(n, b), ps=np.arange(n), pen=np.full(n, 0.1), dis=np.full(n, 0.5 * bf.lengths[b]), prox=None)

    def call(**kw):
        a = dict(good, **{k: v.copy() if v is not None else None for k, v in good.items()})
        for k, v in kw.items():
            if a[k] is None:
                a[k] = np.full(n, 0.5 * bf.lengths[b])
            a[k][at] = v
        return ev.score_at(make_pairs(a["pb"], a["ps"]), a["pen"], a["dis"], codes, wb, ws, proximal=a["prox"])

    assert np.all(np.isfinite(call()))
    for bad in (dict(pb=bf.B), dict(ps=Q), dict(pen=np.nan), dict(dis=np.inf), dict(prox=np.nan), dict(pen=-0.1),
                dict(dis=-1e-9), dict(prox=-0.5), dict(dis=1.000001 * bf.lengths[b])):
        with pytest.raises(epa.EpaError) as e:
            call(**bad)
        assert e.value.code == -1, bad
        assert "entry %d" % at in str(e.value), (bad, str(e.value))
    # with an explicit proximal length a distal length beyond the branch's is the caller's business
    assert np.all(np.isfinite(call(dis=1.5 * bf.lengths[b], prox=0.1)))
    # lengths of exactly 0 are valid (P = I)
    assert np.all(np.isfinite(call(pen=0.0, dis=0.0)))
    # n = 0
    out = ev.score_at(make_pairs([], []), np.zeros(0), np.zeros(0), codes, wb, ws)
    assert out.shape == (0,)
    # an empty window is the empty sum
    ws0 = ws.copy()
    ws0[2] = 0
    got = ev.score_at(make_pairs(good["pb"], good["ps"]), good["pen"], good["dis"], codes, wb, ws0)
    assert got[2] == 0.0 and np.all(got[[0, 1, 3, 4]] < 0.0)


def test_score_at_timer():
    ev = reference("D1").evaluator()
    codes, wb, ws = queries("D1")
    pairs, pen, dis = make_pairs([0, 1], [0, 1]), np.full(2, 0.1), np.zeros(2)
    assert ev.kernel_ms("score_at") < 0
    ev.set_option("timers", 0)
    ev.score_at(pairs, pen, dis, codes, wb, ws)
    assert ev.kernel_ms("score_at") < 0
    ev.set_option("timers", 1)
    ev.score_at(pairs, pen, dis, codes, wb, ws)
    assert ev.kernel_ms("score_at") >= 0
