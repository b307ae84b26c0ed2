"""epa_dev_site_lnl (Evaluator.site_lnl): the per-site log-likelihoods that epa_dev_score_at sums.

The checker is BruteForce._star of tests/brute_force.py, which returns per-site lnLs, on the grid of
tests/test_gpu_score_at.py (its helpers are imported, so both files use the same contexts and entries): branches
{0, B // 2, B - 1} x every read x pendant {1e-4, -ln 0.9, 2.5, 12} x distal {0, 0.3, 1} x branch length.
Every bound is LNL_TOL = 1e-6, the suite's device bound, per SITE.

  1. every site of every row against _star: D1, D5 (device precompute, host CLVs, blocked lookup layout), D16, A4, A9,
     S4 and S20 with per-site and per-rate scalers (every site below ln 2^-256, asserted), L (the 1700-site window,
     27 chunks), Xshort; D5 resident and blocked are the same bits.
  2. a row's sum is score_at of the same entry (1e-6); the columns beyond the span and the rows of an empty window
     are exactly 0.0, also in a buffer that held other values before and with a pitch beyond the longest window.
  3. 4-bit packed, compact and full-width query rows give the same bits.
  4. entries are independent: a tiled and shuffled list gives, row for row, the bits of the entry submitted alone.
  5. argument checks (a too-small pitch among them), n = 0, the "site_lnl" timer.

Largest differences measured on MI355X (the tests print them):

    test 1, group                      |site_lnl - _star| per site
    D  (4 states, 1 .. 16 categories)  3.2e-11
    A  (20 states, 4 and 9 categories) 6.7e-09
    S  (ladders, both scaler modes)    1.2e-09
    L  (1700-site window)              1.3e-11
    X  (Xshort)                        9.7e-08
    test 2, |row sum - score_at|       3.6e-12
"""
import numpy as np
import pytest

import brute_cases as bc
import epa_ng_amd as epa
import rell_ref as rr
from test_gpu_score_at import LNL_TOL, evaluator, grid, make_pairs, queries, reference

pytestmark = pytest.mark.gpu

GRID_CASES = [("D1", "plain"), ("D5", "plain"), ("D5", "host"), ("D5", "blocks"), ("D16", "plain"), ("A4", "plain"),
              ("A9", "plain"), ("S4", "plain"), ("S4", "rate_scalers"), ("S20", "plain"), ("S20", "rate_scalers"),
              ("L", "plain"), ("Xshort", "plain")]

_WANT = {}


def brute_rows(name):
    """-> (rows [n][pitch] of _star padded with 0.0, span per entry) on grid(name), computed once"""
    if name not in _WANT:
        c, bf = bc.case(name), bc.brute(name)
        pb, ps, pen, dis, _ = grid(name)
        rows, spans = rr.site_rows(bf, c["reads"], pb, ps, pen, dis)
        out = np.zeros((len(rows), int(spans.max())))
        for i, r in enumerate(rows):
            out[i, :len(r)] = r
        out.setflags(write=False)
        spans.setflags(write=False)
        _WANT[name] = (out, spans)
    return _WANT[name]


def site_lnl(name, variant, pb, ps, pen, dis, **kw):
    codes, wb, ws = queries(name)
    return evaluator(name, variant).site_lnl(make_pairs(pb, ps), pen, dis, codes, wb, ws, **kw)


@pytest.mark.parametrize("name,variant", GRID_CASES, ids=["%s-%s" % nv for nv in GRID_CASES])
def test_rows_against_brute_force(name, variant):
    pb, ps, pen, dis, _ = grid(name)
    want, spans = brute_rows(name)
    _, _, ws = queries(name)
    assert np.array_equal(spans, np.asarray(ws)[ps])
    got = site_lnl(name, variant, pb, ps, pen, dis)
    assert got.shape == want.shape
    inside = np.arange(want.shape[1])[None, :] < spans[:, None]
    assert np.all(np.isfinite(got)) and np.all(got[~inside] == 0.0)
    d = np.abs(got - want)
    i, j = np.unravel_index(int(np.argmax(d)), d.shape)
    print("\n%s %s: %d rows, %d sites, max |site_lnl - _star| %.3g (branch %d read %d site %d pendant %.3g distal %.3g)"
          % (name, variant, len(pb), int(inside.sum()), d[i, j], pb[i], ps[i], j, pen[i], dis[i]))
    assert d[i, j] < LNL_TOL
    if name == "L":
        assert int(spans.max()) >= 1700
    if name in ("S4", "S20"):
        assert np.all(want[inside] < -256 * np.log(2.0))       # every site carries a scaler count
    if variant == "blocks":
        assert np.array_equal(got, site_lnl(name, "plain", pb, ps, pen, dis))


@pytest.mark.parametrize("name", ["D5", "A4", "S4"])
def test_row_sums_and_padding(name):
    pb, ps, pen, dis, _ = grid(name)
    codes, wb, ws = queries(name)
    ev, pairs = evaluator(name, "plain"), make_pairs(pb, ps)
    rows = ev.site_lnl(pairs, pen, dis, codes, wb, ws)
    lnl = ev.score_at(pairs, pen, dis, codes, wb, ws)
    d = float(np.max(np.abs(rows.sum(1) - lnl)))
    print("\n%s: max |row sum - score_at| %.3g" % (name, d))
    assert d < LNL_TOL
    # a wider pitch into a buffer that held something else: the same values, the padding exactly 0.0
    pitch = rows.shape[1] + 37
    out = np.full((len(pairs), pitch), np.nan)
    wide = ev.site_lnl(pairs, pen, dis, codes, wb, ws, pitch=pitch, out=out)
    assert np.array_equal(wide[:, :rows.shape[1]], rows) and np.all(wide[:, rows.shape[1]:] == 0.0)
    # an empty window: an all-zero row, the other rows unchanged
    ws0 = np.array(ws).copy()
    ws0[2] = 0
    out = np.full(rows.shape, np.nan)
    got = ev.site_lnl(pairs, pen, dis, codes, wb, ws0, pitch=rows.shape[1], out=out)
    assert np.all(got[ps == 2] == 0.0) and np.array_equal(got[ps != 2], rows[ps != 2])


def test_query_layouts_give_the_same_bits():
    name = "D5"
    pb, ps, pen, dis, _ = grid(name)
    ev, pairs = evaluator(name, "plain"), make_pairs(pb, ps)
    compact, wb, ws = queries(name, True)
    full, _, _ = queries(name, False)
    a = ev.site_lnl(pairs, pen, dis, compact, wb, ws)
    b = ev.site_lnl(pairs, pen, dis, full, wb, ws)
    p = ev.site_lnl(pairs, pen, dis, epa.pack_codes_4bit(compact), wb, ws)
    assert np.array_equal(a, b) and np.array_equal(a, p)


@pytest.mark.parametrize("name,total", [("D16", 5000), ("A9", 600)])
def test_entries_are_independent(name, total):
    pb, ps, pen, dis, _ = grid(name)
    n = len(pb)
    ev = evaluator(name, "plain")
    codes, wb, ws = queries(name)
    pairs = make_pairs(pb, ps)
    in_order = ev.site_lnl(pairs, pen, dis, codes, wb, ws)
    alone = np.stack([ev.site_lnl(pairs[i:i + 1], pen[i:i + 1], dis[i:i + 1], codes, wb, ws, pitch=in_order.shape[1])[0]
                      for i in range(0, n, 7)])
    assert np.array_equal(alone, in_order[::7])
    idx = np.tile(np.arange(n), (total + n - 1) // n)[:total]
    np.random.RandomState(5).shuffle(idx)
    shuffled = ev.site_lnl(np.ascontiguousarray(pairs[idx]), pen[idx], dis[idx], codes, wb, ws)
    assert np.array_equal(shuffled, in_order[idx])


def test_argument_checks_and_timer():
    name = "D5"
    c, bf = bc.case(name), bc.brute(name)
    ev = reference(name).evaluator()
    codes, wb, ws = queries(name)
    Q = len(c["reads"])
    n, b = 5, bf.B // 2
    pb, ps, pen, dis = np.full(n, b), np.arange(n), np.full(n, 0.1), np.full(n, 0.5 * bf.lengths[b])
    assert ev.kernel_ms("site_lnl") < 0
    need = int(max(ws[q] for q in ps))
    assert need < int(max(ws))
    # the pitch has to hold the longest window among the ENTRIES' queries
    rows = ev.site_lnl(make_pairs(pb, ps), pen, dis, codes, wb, ws, pitch=need)
    assert rows.shape == (n, need) and np.all(np.isfinite(rows))
    assert ev.kernel_ms("site_lnl") > 0
    with pytest.raises(epa.EpaError) as e:
        ev.site_lnl(make_pairs(pb, ps), pen, dis, codes, wb, ws, pitch=need - 1)
    assert e.value.code == -1 and "pitch" in str(e.value)
    for bad in (dict(pb=bf.B), dict(ps=Q), dict(pen=np.nan), dict(dis=-1e-9), dict(dis=1.000001 * bf.lengths[b])):
        a = dict(pb=pb.copy(), ps=ps.copy(), pen=pen.copy(), dis=dis.copy())
        for k, v in bad.items():
            a[k][3] = v
        with pytest.raises(epa.EpaError) as e:
            ev.site_lnl(make_pairs(a["pb"], a["ps"]), a["pen"], a["dis"], codes, wb, ws, pitch=int(max(ws)))
        assert e.value.code == -1 and "entry 3" in str(e.value), (bad, str(e.value))
    assert ev.site_lnl(make_pairs([], []), np.zeros(0), np.zeros(0), codes, wb, ws).shape == (0, int(max(ws)))
