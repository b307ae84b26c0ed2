"""epa_dev_marginal_like (Evaluator.marginal_like): the marginal likelihood of "read q sits somewhere on edge b" over a
(distal x pendant) tensor rule, and the grid of lnLs it is made of.

The checker is tests/marginal_ref.py: brute_grid (BruteForce._star at every node) and combine (the M rule of
include/epa_dev.h in numpy, in the specified order).  Contexts, queries and pairs are those of
tests/test_gpu_score_at.py (imported).  Entries: branches {0, B // 2, B - 1} x every read of the case.  Rule of the
tests: Gauss-Legendre x Gauss-Laguerre with Kx = 3, Kp = 5 and a prior mean of 0.05 (smallest pendant node 0.013),
unless a test says otherwise.  Every bound against the brute force is LNL_TOL = 1e-6, the suite's device bound.

  1. the grid (grid=True) against brute_grid per grid point: D1, D5 (plain, host CLVs, blocks), D16 (+I, 16
     categories), A4, A9 (c * S = 180), S4 and S20 with per-site and per-rate scalers (every expected value carries
     scaler counts, asserted), L (1700-site window, 27 chunks, Kx = 2, Kp = 3); D5 resident and blocked: the same bits.
  2. M against combine(the device's own grid): 16 x 2^-52 x max(1, |M|) -- m is an exact maximum, the sum of at most
     4096 non-negative terms <= 1 carries a few unit roundoffs relatively, hence absolutely after the log, and the final
     add rounds once at the scale of |M|.
  3. M against combine(brute_grid): LNL_TOL (log-sum-exp is 1-Lipschitz in the sup norm; asserted because it is the
     number users get).
  4. ties to score_at: Kx = Kp = 1 with zero log weights is score_at at that point; the full grid of D5 and A4 is
     score_at called at every node, x_frac exactly 0 and exactly 1 and pendant 1e-4 among the nodes (the point of the
     noise cut).
  5. tile edges, one entry each of D5 and A4: every Kp from 1 to 64 with Kx = 2, Kx in {1, 2, 64} with Kp = 3; the nodes
     are prefixes of one 64-node list, so g_ij of a node is the same bits whatever K is; M against combine.
  6. 4-bit packed, compact and full-width query rows give the same bits.
  7. entries are independent: D16's and A9's lists tiled and shuffled to 3000 / 400 entries give, row for row, the bits
     of the entry submitted alone and in order; a query with win_span == 0 among them has M = log sum w and an all-zero
     grid, its neighbours unchanged.
  8. argument checks, n = 0, grid_lnl = NULL, a device buffer for M, the "marginal" timer.

Largest differences measured on MI355X (the tests print them):

    test 1, group                      |grid - brute_grid| per grid point
    D  (4 states, 1 .. 16 categories)  5.5e-12
    A  (20 states, 4 and 9 categories) 6.0e-11
    S  (ladders, both scaler modes)    1.5e-11
    L  (1700-site window)              9.1e-12
    test 2, |M - combine(device grid)| / max(1, |M|)   0  (bound 3.6e-15)
    test 3, |M - combine(brute_grid)|                  1.3e-11
    test 4, |M(1 x 1 rule) - score_at|                 4.5e-13  (not the same bits)
    test 4, |grid - score_at| at every node            D5 2.3e-13, A4 2.6e-11 (at pendant 1e-4)
"""
import functools

import numpy as np
import pytest

import brute_cases as bc
import epa_ng_amd as epa
import marginal_ref as mr
from test_gpu_score_at import LNL_TOL, evaluator, make_pairs, queries, reference

pytestmark = pytest.mark.gpu

PRIOR_MEAN = 0.05
M_EPS = 16 * 2.0 ** -52
GRID_CASES = [("D1", "plain"), ("D5", "plain"), ("D5", "host"), ("D5", "blocks"), ("D16", "plain"), ("A4", "plain"),
              ("A9", "plain"), ("S4", "plain"), ("S4", "rate_scalers"), ("S20", "plain"), ("S20", "rate_scalers"),
              ("L", "plain")]


@functools.lru_cache(maxsize=None)
def rule(name):
    """(x_frac, x_logw, p_len, p_logw) of the case: 3 x 5 nodes, L 2 x 3 (to bound the CPU side)"""
    r = epa.posterior_rule(PRIOR_MEAN, Kx=2, Kp=3) if name == "L" else epa.posterior_rule(PRIOR_MEAN, Kx=3, Kp=5)
    assert r[2].min() > 1e-3
    for a in r:
        a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def entry_list(name):
    pb, ps = mr.entries(bc.brute(name), len(bc.case(name)["reads"]))
    pb.setflags(write=False)
    ps.setflags(write=False)
    return pb, ps


@functools.lru_cache(maxsize=None)
def brute(name):
    """-> [n][Kx][Kp] brute_grid of every entry of the case at rule(name), computed once"""
    c, bf = bc.case(name), bc.brute(name)
    pb, ps = entry_list(name)
    x, _, p, _ = rule(name)
    out = np.stack([mr.brute_grid(bf, c["reads"][int(q)], int(b), x, p) for b, q in zip(pb, ps)])
    out.setflags(write=False)
    return out


def marginal(name, variant, pb, ps, r, grid=True, codes=None, ws=None, **kw):
    c, wb, ws_ = queries(name)
    return evaluator(name, variant).marginal_like(make_pairs(pb, ps), c if codes is None else codes, wb,
                                                  ws_ if ws is None else ws, r[0], r[1], r[2], r[3], grid=grid, **kw)


@functools.lru_cache(maxsize=None)
def device(name, variant):
    pb, ps = entry_list(name)
    M, g = marginal(name, variant, pb, ps, rule(name))
    M.setflags(write=False)
    g.setflags(write=False)
    return M, g


def combine_all(g, r):
    return np.array([mr.combine(g[e], r[1], r[3]) for e in range(len(g))])


# ---- 1. the grid against the brute force

@pytest.mark.parametrize("name,variant", GRID_CASES, ids=["%s-%s" % nv for nv in GRID_CASES])
def test_grid_against_brute_force(name, variant):
    pb, ps = entry_list(name)
    want = brute(name)
    M, got = device(name, variant)
    assert got.shape == want.shape and np.all(np.isfinite(got)) and np.all(np.isfinite(M))
    d = np.abs(got - want)
    e, i, j = np.unravel_index(int(np.argmax(d)), d.shape)
    print("\n%s %s: %d entries x %d x %d nodes, max |grid - brute_grid| %.3g (branch %d read %d x_frac %.3g pendant %.3g)"
          % (name, variant, len(pb), want.shape[1], want.shape[2], d[e, i, j], pb[e], ps[e], rule(name)[0][i], rule(name)[2][j]))
    assert d[e, i, j] < LNL_TOL
    spans = np.asarray(queries(name)[2])[ps].astype(np.float64)
    if name == "L":
        assert spans.max() >= 1700 and want.shape[1:] == (2, 3)
    else:
        assert want.shape[1:] == (3, 5)
    if name in ("S4", "S20"):
        assert np.all(want < -256 * np.log(2.0) * spans[:, None, None])       # every site carries a scaler count
    if variant == "blocks":
        # refT and scSum are built the same way in both layouts and are all the kernel reads
        Mp, gp = device(name, "plain")
        assert np.array_equal(got, gp) and np.array_equal(M, Mp)


# ---- 2. M against the device's own grid

@pytest.mark.parametrize("name,variant", GRID_CASES, ids=["%s-%s" % nv for nv in GRID_CASES])
def test_marginal_against_the_devices_own_grid(name, variant):
    M, g = device(name, variant)
    want = combine_all(g, rule(name))
    d = np.abs(M - want) / np.maximum(1.0, np.abs(M))
    print("\n%s %s: max |M - combine(device grid)| / max(1, |M|) %.3g" % (name, variant, d.max()))
    assert np.all(d <= M_EPS)


# ---- 3. M against the brute force

@pytest.mark.parametrize("name,variant", GRID_CASES, ids=["%s-%s" % nv for nv in GRID_CASES])
def test_marginal_against_brute_force(name, variant):
    M, _ = device(name, variant)
    want = combine_all(brute(name), rule(name))
    d = np.abs(M - want)
    print("\n%s %s: max |M - combine(brute_grid)| %.3g" % (name, variant, d.max()))
    assert np.all(d < LNL_TOL)


# ---- 4. ties to score_at

@pytest.mark.parametrize("name", ["D5", "A4"])
def test_one_node_rule_is_score_at(name):
    pb, ps = entry_list(name)
    bf = bc.brute(name)
    codes, wb, ws = queries(name)
    worst = 0.0
    for frac, pendant in ((0.3, 0.1), (0.0, 1e-4), (1.0, 1e-4)):
        r = (np.array([frac]), np.zeros(1), np.array([pendant]), np.zeros(1))
        M, g = marginal(name, "plain", pb, ps, r)
        lnl = evaluator(name, "plain").score_at(make_pairs(pb, ps), np.full(len(pb), pendant), frac * bf.lengths[pb],
                                                codes, wb, ws)
        d = float(np.max(np.abs(M - lnl)))
        print("\n%s x_frac %g pendant %g: max |M(1 x 1) - score_at| %.3g, same bits: %s"
              % (name, frac, pendant, d, np.array_equal(M, lnl)))
        worst = max(worst, d)
        assert d < LNL_TOL
        assert np.array_equal(g[:, 0, 0], M)      # m + log(exp(0)) = m


@pytest.mark.parametrize("name", ["D5", "A4"])
def test_grid_is_score_at_at_every_node(name):
    pb, ps = entry_list(name)
    bf = bc.brute(name)
    codes, wb, ws = queries(name)
    x = np.concatenate([[0.0], epa.quadrature_legendre01(3)[0], [1.0]])
    p = np.concatenate([[1e-4], PRIOR_MEAN * epa.quadrature_laguerre(5)[0]])
    r = (x, np.zeros(len(x)), p, np.zeros(len(p)))
    _, g = marginal(name, "plain", pb, ps, r)
    ev, pairs = evaluator(name, "plain"), make_pairs(pb, ps)
    worst, at = 0.0, None
    for i in range(len(x)):
        for j in range(len(p)):
            lnl = ev.score_at(pairs, np.full(len(pb), p[j]), x[i] * bf.lengths[pb], codes, wb, ws)
            d = float(np.max(np.abs(g[:, i, j] - lnl)))
            if d >= worst:
                worst, at = d, (x[i], p[j])
            assert d < LNL_TOL, (x[i], p[j], d)
    print("\n%s: %d x %d nodes, max |grid - score_at| %.3g (x_frac %g pendant %g)" % (name, len(x), len(p), worst, at[0], at[1]))


# ---- 5. tile edges

@pytest.mark.parametrize("name", ["D5", "A4"])
def test_tile_edges(name):
    bf = bc.brute(name)
    codes, wb, ws = queries(name)
    q = next(i for i, n in enumerate(ws) if n > 64 and n % 64)
    assert ws[q] > 64 and ws[q] % 64 != 0
    pb, ps = np.array([bf.B // 2]), np.array([q])
    X, XW = epa.quadrature_legendre01(64)
    T, PW = epa.quadrature_laguerre(64)
    P = PRIOR_MEAN * T
    assert P.min() > 1e-3

    def run(kx, kp):
        r = (X[:kx], XW[:kx], P[:kp], PW[:kp])
        M, g = marginal(name, "plain", pb, ps, r)
        want = mr.combine(g[0], r[1], r[3])
        assert abs(M[0] - want) <= M_EPS * max(1.0, abs(M[0])), (kx, kp, M[0], want)
        return g[0]

    full = run(2, 64)
    assert np.all(np.isfinite(full))
    for kp in range(1, 64):
        assert np.array_equal(run(2, kp), full[:, :kp]), kp
    tall = run(64, 3)
    assert np.array_equal(tall[:2], full[:, :3])
    for kx in (1, 2):
        assert np.array_equal(run(kx, 3), tall[:kx]), kx
    # the pendant tile's remainder on the last distal node of a long list
    assert np.array_equal(run(64, 17)[:, :3], tall)


# ---- 6. query staging

def test_query_layouts_give_the_same_bits():
    name = "D5"
    pb, ps = entry_list(name)
    ev = evaluator(name, "plain")
    compact, wb, ws = queries(name, True)
    full, wb2, ws2 = queries(name, False)
    assert np.array_equal(wb, wb2) and np.array_equal(ws, ws2) and full.shape[1] == ev.W != compact.shape[1]
    r = rule(name)
    a = marginal(name, "plain", pb, ps, r, codes=compact)
    b = marginal(name, "plain", pb, ps, r, codes=full)
    p = marginal(name, "plain", pb, ps, r, codes=epa.pack_codes_4bit(compact))
    for k in (0, 1):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], p[k])
    assert np.array_equal(a[0], device(name, "plain")[0])


# ---- 7. entries are independent

@pytest.mark.parametrize("name,total", [("D16", 3000), ("A9", 400)])
def test_entries_are_independent(name, total):
    pb, ps = entry_list(name)
    n = len(pb)
    r = rule(name)
    in_order = device(name, "plain")
    alone = [marginal(name, "plain", pb[i:i + 1], ps[i:i + 1], r) for i in range(n)]
    assert np.array_equal(np.array([a[0][0] for a in alone]), in_order[0])
    assert np.array_equal(np.stack([a[1][0] for a in alone]), in_order[1])
    idx = np.tile(np.arange(n), (total + n - 1) // n)[:total]
    np.random.RandomState(5).shuffle(idx)
    if name == "D16":
        assert total > 8 * 256          # more entries than the persistent grid has waves: every wave runs several
    M, g = marginal(name, "plain", pb[idx], ps[idx], r)
    assert np.array_equal(M, in_order[0][idx]) and np.array_equal(g, in_order[1][idx])
    # a query with an empty window among them: the empty sum at every node, the neighbours unchanged
    ws0 = np.array(queries(name)[2]).copy()
    ws0[2] = 0
    M0, g0 = marginal(name, "plain", pb[idx], ps[idx], r, ws=ws0)
    empty = ps[idx] == 2
    assert 0 < empty.sum() < total and empty[1:-1].any()
    assert np.all(g0[empty] == 0.0)
    log_total = mr.combine(np.zeros((len(r[0]), len(r[2]))), r[1], r[3])
    assert abs(log_total) < 1e-12                                      # the rule's weights sum to 1
    assert np.all(np.abs(M0[empty] - log_total) <= M_EPS)
    assert np.array_equal(M0[~empty], M[~empty]) and np.array_equal(g0[~empty], g[~empty])


# ---- 8. argument checks and timer

def test_argument_checks():
    name = "D5"
    c, bf = bc.case(name), bc.brute(name)
    ev = evaluator(name, "plain")
    codes, wb, ws = queries(name)
    Q = len(c["reads"])
    n, at = 5, 3
    b = bf.B // 2
    good = dict(pb=np.full(n, b), ps=np.arange(n), x=rule(name)[0], xw=rule(name)[1], p=rule(name)[2], pw=rule(name)[3])

    def call(grid=False, out=None, **kw):
        a = {k: np.array(v).copy() for k, v in good.items()}
        for k, (i, v) in kw.items():
            a[k][i] = v
        return ev.marginal_like(make_pairs(a["pb"], a["ps"]), codes, wb, ws, a["x"], a["xw"], a["p"], a["pw"], grid=grid, out=out)

    M = call()
    assert M.shape == (n,) and np.all(np.isfinite(M))
    for bad, named in ((dict(pb=(at, bf.B)), "entry %d" % at), (dict(ps=(at, Q)), "entry %d" % at),
                       (dict(x=(1, 1.5)), "distal node 1"), (dict(x=(1, -1e-9)), "distal node 1"),
                       (dict(x=(1, np.nan)), "distal node 1"), (dict(xw=(2, np.inf)), "distal node 2"),
                       (dict(xw=(0, np.nan)), "distal node 0"), (dict(p=(4, -0.1)), "pendant node 4"),
                       (dict(p=(2, np.inf)), "pendant node 2"), (dict(p=(2, np.nan)), "pendant node 2"),
                       (dict(pw=(3, -np.inf)), "pendant node 3")):
        with pytest.raises(epa.EpaError) as e:
            call(**bad)
        assert e.value.code == -1, bad
        assert named in str(e.value), (bad, str(e.value))
    # node counts outside 1 .. 64
    pairs = make_pairs(good["pb"], good["ps"])
    x65, p65 = np.linspace(0.0, 1.0, 65), np.linspace(0.01, 1.0, 65)
    for args, named in (((x65, np.zeros(65), good["p"], good["pw"]), "Kx"), ((good["x"], good["xw"], p65, np.zeros(65)), "Kp")):
        with pytest.raises(epa.EpaError) as e:
            ev.marginal_like(pairs, codes, wb, ws, *args)
        assert e.value.code == -1 and named in str(e.value) and "65" in str(e.value)
    for args in ((np.zeros(0), np.zeros(0), good["p"], good["pw"]), (good["x"], good["xw"], np.zeros(0), np.zeros(0))):
        with pytest.raises(epa.EpaError) as e:
            ev.marginal_like(pairs, codes, wb, ws, *args)
        assert e.value.code == -1
    # x_frac exactly 0 and 1 and a pendant node of exactly 0 are valid
    assert np.all(np.isfinite(call(x=(0, 0.0)))) and np.all(np.isfinite(call(x=(2, 1.0)))) and np.all(np.isfinite(call(p=(0, 0.0))))
    # n = 0
    out = ev.marginal_like(make_pairs([], []), codes, wb, ws, good["x"], good["xw"], good["p"], good["pw"])
    assert out.shape == (0,)
    out, g = ev.marginal_like(make_pairs([], []), codes, wb, ws, good["x"], good["xw"], good["p"], good["pw"], grid=True)
    assert out.shape == (0,) and g.shape == (0, 3, 5)
    # grid_lnl = NULL and a grid give the same M
    Mg, g = call(grid=True)
    assert np.array_equal(M, Mg) and g.shape == (n, 3, 5)
    # M into a device buffer
    import torch
    buf = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    call(out=buf)
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), M)


def test_marginal_timer():
    ev = reference("D1").evaluator()
    codes, wb, ws = queries("D1")
    pairs = make_pairs([0, 1], [3, 4])
    r = rule("D1")
    assert ev.kernel_ms("marginal") < 0
    M = ev.marginal_like(pairs, codes, wb, ws, *r)
    assert np.all(np.isfinite(M))
    assert ev.kernel_ms("marginal") > 0
    assert ev.kernel_ms("score_at") < 0
