"""epa_dev_rell_kh (Evaluator.rell_kh): the p-values of the KH, the weighted KH and the weighted SH test of competing
placements from the replicates of rell_support.

  1. counts against the restatement: p x R is an integer, recovered exactly, and equals, entry for entry, the numpy
     restatement of the specification (tests/rell_kh_ref.py) fed with the device's own site_lnl rows.  D5 (4 states) and
     A4 (20 states) with 1, 2, 3, 4, 5, 8, 9 and 17 entries per query -- 4 | 5 and 8 | 9 are tile boundaries, 8 the last
     count whose centred scores stay in registers -- over spans 0, 1, 3, 30, 64, ... at R = 257 and 4096, with the
     default and with explicit stream ids, the entries of the queries interleaved (branch-major order); L's windows of
     1536, 1537 and 1700 sites (the last two do not fit the LDS tile) with 3 entries (registers) and all 2 B (spilled);
     257 entries on one query: one more than the kernel counts in LDS.
  2. ties to epa_dev_rell_tests with the same seed and ids: p_kh <= p_sh everywhere, and the same bits on queries of two
     entries.
  3. against CPU proportions: on the 22 x 3 x 30-site input of the statistical tests at R = 4096 the three columns are
     within rell_ref.six_sigma of default_rng multinomial resampling of the BRUTE-FORCE rows.
  4. call behaviour: outputs asked for singly equal those asked for together; one call twice gives equal bits; the
     "rell_kh" timer; the resident and the blocked lookup layout give equal bits.
  5. errors name rell_kh: replicates, no output, a sequence id out of range among device pairs, 1025 entries on a query
     (1024 are accepted).
  6. memory and history: all-device inputs and outputs, and p_kh alone on the device, give the all-host bits, also after
     another member of the family ran on the context.

Measured on MI355X: test 1, queries with a value strictly inside (0, 1) in p_kh / p_wkh / p_wsh: D5 4 / 4 / 6 of 14 at
R = 257 and 7 / 7 / 7 at 4096, A4 8 / 8 / 8 of 12, L 4 / 4 / 4 of 4; test 3, largest |device - default_rng| / bound: p_kh
0.356, p_wkh 0.41, p_wsh 0.418 (66 values each).
"""
import numpy as np
import pytest
import torch

import brute_cases as bc
import epa_ng_amd as epa
import rell_kh_ref as rk
import rell_ref as rr
from epa_ng_amd.api import _ptr
from test_gpu_entry_outputs import R as MEM_R, SEED as MEM_SEED, device_input, host_input
from test_gpu_rell import entry_lists
from test_gpu_score_at import evaluator, make_pairs, queries, reference

pytestmark = pytest.mark.gpu

KEYS = ("p_kh", "p_wkh", "p_wsh")
PER_QUERY = (2, 3, 17, 4, 5, 8, 9, 1)


def counts(got, R):
    """p x R as integers; p is count / R and nothing else"""
    out = {}
    for key in KEYS:
        out[key] = np.rint(got[key] * R).astype(np.int64)
        assert np.array_equal(got[key], out[key] / float(R)), key
    return out


def check(ev, codes, wb, ws, pb, ps, pen, dis, R, seed=1, stream_id=None):
    """the three outputs against the restatement on the device's own rows -> (outputs, restatement)"""
    pairs = make_pairs(pb, ps)
    rows = ev.site_lnl(pairs, pen, dis, codes, wb, ws)
    got = ev.rell_kh(pairs, pen, dis, codes, wb, ws, R, seed=seed, stream_id=stream_id)
    assert sorted(got) == sorted(KEYS) and all(v.shape == (len(pb),) and v.dtype == np.float64 for v in got.values())
    sid = np.arange(len(ws)) if stream_id is None else stream_id
    groups = rk.group_by_query(ps)
    want = rk.rell_kh(rows, ws, groups, sid, R, seed, pb)
    c = counts(got, R)
    inside = {key: 0 for key in KEYS}
    for key in KEYS:
        bad = np.flatnonzero(c[key] != want[key[2:]])
        assert len(bad) == 0, (key, bad[:10], c[key][bad[:10]], want[key[2:]][bad[:10]])
        for members in groups.values():
            inside[key] += bool(np.any((c[key][members] > 0) & (c[key][members] < R)))
    assert all(np.all(got[key][want["best"]] == 1.0) for key in KEYS) and np.all(c["p_wkh"] <= c["p_wsh"])
    print("\n%d entries of %d queries, R %d: queries with a value in (0, 1): %s" % (len(pb), len(groups), R, inside))
    return got, want, inside


@pytest.mark.parametrize("name,R,explicit", [("D5", 257, False), ("D5", 4096, True), ("A4", 257, True), ("A4", 4096, False)])
def test_counts_equal_the_restatement(name, R, explicit):
    bf = bc.brute(name)
    codes, wb, ws = queries(name)
    ws = np.array(ws).copy()
    Q = len(ws)
    per_query = [PER_QUERY[q % 8] for q in range(Q)]
    if name == "D5":
        assert [int(x) for x in ws[:5]] == [1, 3, 30, 64, 65] and Q >= 10 and set(per_query) == set(PER_QUERY)
        ws[9] = 0                                              # span 0 with three entries; span 1 has two, span 30 has 17
    pb, ps, pen, dis = entry_lists(bf.B, bf.lengths, per_query)
    order = np.lexsort((ps, pb))                               # branch-major: the entries of the queries interleaved
    assert not np.array_equal(ps[order], np.sort(ps))
    pb, ps, pen, dis = pb[order], ps[order], pen[order], dis[order]
    sid = (np.arange(Q, dtype=np.uint64) * 3 + (1 << 33)) if explicit else None
    got, _, inside = check(evaluator(name, "plain"), codes, wb, ws, pb, ps, pen, dis, R, seed=R + 7, stream_id=sid)
    if name == "D5":
        assert np.all(got["p_wkh"][ps == 0] == 1.0) and np.all(got["p_wsh"][ps == 0] == 1.0)      # span 1
        assert sorted(got["p_kh"][ps == 0]) in ([0.0, 1.0], [1.0, 1.0])
        assert all(np.all(got[key][ps == 9] == 1.0) for key in KEYS)                                # span 0
    assert all(got[key][ps == 7][0] == 1.0 for key in KEYS)                                         # a single entry
    assert max(inside.values()) >= 2                           # the comparison is not one of trivial values only


def test_long_windows():
    name = "L"
    bf = bc.brute(name)
    codes, wb, ws = queries(name)
    Q = len(ws)
    spans = [int(x) for x in ws]
    assert sorted(spans) == [90, 1536, 1537, 1700]
    ev = evaluator(name, "plain")
    # as test_gpu_rell: every read on all B branches at the optimiser's own lengths, and again with the pendant length
    # 1 % longer, so that the replicates of 1500 sites and more go both ways; the read of 1700 sites keeps its best
    # branch, twice, and the next one: three entries, the centred scores stay in registers
    pb, ps = np.tile(np.repeat(np.arange(bf.B), Q), 2), np.tile(np.arange(Q), 2 * bf.B)
    res = ev.thorough(make_pairs(pb[:bf.B * Q], ps[:bf.B * Q]), codes, wb, ws)
    pen = np.concatenate([res["pendant_length"], 1.01 * res["pendant_length"]])
    dis = np.tile(np.minimum(res["distal_length"], bf.lengths[pb[:bf.B * Q]]), 2)
    q_long = spans.index(1700)
    first, second = [int(i) for i in np.argsort(-np.where(ps[:bf.B * Q] == q_long, res["lnl"], -np.inf))[:2]]
    i = np.arange(len(pb))
    keep = (ps != q_long) | (i % (bf.B * Q) == first) | (i == second)
    pb, ps, pen, dis = pb[keep], ps[keep], pen[keep], dis[keep]
    assert np.sum(ps == q_long) == 3 and 2 * bf.B > 8
    _, _, inside = check(ev, codes, wb, ws, pb, ps, pen, dis, 257, seed=5)
    assert max(inside.values()) >= 2


def test_more_entries_than_lds_counters():
    name = "D5"
    bf = bc.brute(name)
    codes, wb, ws = queries(name)
    n = 257
    # query 1 (3 sites): 257 entries over all branches and lengths, some of them several times; query 2: three
    pb = np.concatenate([np.arange(n) % bf.B, [0, 5, 9 % bf.B]])
    ps = np.concatenate([np.full(n, 1), [2, 2, 2]])
    i = np.arange(len(pb))
    pen = np.array([0.05, 0.3])[(i // bf.B) % 2]
    dis = np.array([0.3, 1.0])[(i // (2 * bf.B)) % 2] * bf.lengths[pb]
    got, want, _ = check(evaluator(name, "plain"), codes, wb, ws, pb, ps, pen, dis, 257, seed=11)
    twin = 4 * bf.B                                            # entries 0 and 4 B are the same placement: a skipped pair
    assert twin < n and all(got[key][twin] == got[key][0] for key in KEYS)


def test_ties_to_rell_tests():
    name = "D5"
    bf = bc.brute(name)
    ev = evaluator(name, "plain")
    codes, wb, ws = queries(name)
    Q, R = len(ws), 1000
    per_query = [(2, 3, 9, 2)[q % 4] for q in range(Q)]
    pb, ps, pen, dis = entry_lists(bf.B, bf.lengths, per_query)
    sid = np.arange(Q, dtype=np.uint64) + 77
    pairs = make_pairs(pb, ps)
    kh = ev.rell_kh(pairs, pen, dis, codes, wb, ws, R, seed=3, stream_id=sid)
    sh = ev.rell_tests(pairs, pen, dis, codes, wb, ws, R, seed=3, stream_id=sid, want=("p_sh",))["p_sh"]
    assert np.all(kh["p_kh"] <= sh)
    two = np.isin(ps, [q for q in range(Q) if per_query[q] == 2])
    assert np.array_equal(kh["p_kh"][two], sh[two]) and np.any((sh[two] > 0) & (sh[two] < 1))
    assert np.any(kh["p_kh"][~two] < sh[~two])


def test_against_cpu_proportions():
    s = rr.stat_input()
    cpu = rk.stat_kh()
    ev = evaluator("D5", "plain")
    codes, wb, ws = epa.encode_queries(4, s["reads"], compact=True)
    assert np.all(np.asarray(ws) == rr.STAT_SPAN)
    got = ev.rell_kh(make_pairs(s["branch"], s["seq"]), s["pendant"], s["distal"], codes, wb, ws, rr.STAT_R)
    worst = {key: float(np.max(np.abs(got[key] - cpu[key]) / rk.six_sigma(got[key], cpu[key], rr.STAT_R))) for key in KEYS}
    print("\n%d values: max |device - default_rng on brute-force rows| / bound: %s" % (len(s["seq"]), worst))
    assert all(v <= 1.0 for v in worst.values())


def test_call_behaviour():
    name = "D5"
    bf = bc.brute(name)
    ev = reference(name).evaluator()
    codes, wb, ws = queries(name)
    pb, ps, pen, dis = entry_lists(bf.B, bf.lengths, [PER_QUERY[q % 8] for q in range(len(ws))])
    pairs = make_pairs(pb, ps)
    assert ev.kernel_ms("rell_kh") < 0
    all3 = ev.rell_kh(pairs, pen, dis, codes, wb, ws, 257, seed=3)
    assert ev.kernel_ms("rell_kh") > 0 and ev.kernel_ms("rell_tests") < 0
    again = ev.rell_kh(pairs, pen, dis, codes, wb, ws, 257, seed=3)
    assert all(np.array_equal(again[key], all3[key]) for key in KEYS)
    for want in (("p_kh",), ("p_wkh",), ("p_wsh",), ("p_wsh", "p_kh")):
        got = ev.rell_kh(pairs, pen, dis, codes, wb, ws, 257, seed=3, want=want)
        assert sorted(got) == sorted(want)
        for key in want:
            assert np.array_equal(got[key], all3[key]), key
    blocked = evaluator(name, "blocks").rell_kh(pairs, pen, dis, codes, wb, ws, 257, seed=3)
    assert all(np.array_equal(blocked[key], all3[key]) for key in KEYS)
    assert not np.array_equal(ev.rell_kh(pairs, pen, dis, codes, wb, ws, 257, seed=4)["p_wsh"], all3["p_wsh"])
    got = ev.rell_kh(make_pairs([], []), np.zeros(0), np.zeros(0), codes, wb, ws, 10)
    assert all(got[key].shape == (0,) for key in KEYS)


def test_errors_name_rell_kh():
    name = "D5"
    bf = bc.brute(name)
    ev = reference(name).evaluator()
    codes, wb, ws = queries(name)
    Q = len(ws)
    pb, ps, pen, dis = entry_lists(bf.B, bf.lengths, [2] * Q)
    pairs = make_pairs(pb, ps)
    for R in (0, (1 << 20) + 1):
        with pytest.raises(epa.EpaError) as e:
            ev.rell_kh(pairs, pen, dis, codes, wb, ws, R)
        assert e.value.code == -1 and "rell_kh" in str(e.value) and "replicates" in str(e.value)
    with pytest.raises(epa.EpaError) as e:
        ev.rell_kh(pairs, pen, dis, codes, wb, ws, 10, want=())
    assert e.value.code == -1 and "rell_kh" in str(e.value)
    with pytest.raises(ValueError):
        ev.rell_kh(pairs, pen, dis, codes, wb, ws, 10, want=("p_kh", "p_sh"))
    # device pairs are not read by the host: the grouping finds the id
    bad = pairs.copy()
    bad["seq_id"][3] = Q
    d_pairs = torch.from_numpy(bad.view(np.int32).reshape(-1, 2).copy()).cuda()
    with pytest.raises(epa.EpaError) as e:
        ev.rell_kh(d_pairs, pen, dis, codes, wb, ws, 10)
    assert e.value.code == -1 and "rell_kh" in str(e.value) and "sequence id" in str(e.value)
    # 1024 entries on the query of one site are accepted, 1025 are not
    assert int(ws[0]) == 1
    n = 1025
    pb = np.arange(n) % bf.B
    pen = 0.01 * (1 + np.arange(n) // bf.B)
    dis = np.zeros(n)
    with pytest.raises(epa.EpaError) as e:
        ev.rell_kh(make_pairs(pb, np.zeros(n, np.int64)), pen, dis, codes, wb, ws, 64)
    assert e.value.code == -1 and "rell_kh: query 0 has 1025 entries" in str(e.value), str(e.value)
    n = 1024
    pairs = make_pairs(pb[:n], np.zeros(n, np.int64))
    got = ev.rell_kh(pairs, pen[:n], dis[:n], codes, wb, ws, 64)
    site = ev.site_lnl(pairs, pen[:n], dis[:n], codes, wb, ws)[:, 0]
    assert len(np.unique(site)) > 100
    # span 1: every pair is skipped; a replicate is the site itself, so KH rejects every row below the best
    assert np.all(got["p_wkh"] == 1.0) and np.all(got["p_wsh"] == 1.0)
    assert np.array_equal(got["p_kh"], (site == site.max()).astype(np.float64))


def kh_call(ev, a, out):
    """epa_dev_rell_kh through the C ABI on inputs a into the buffers out (name -> numpy array or device tensor)"""
    ev._layout(a["codes"])
    ev._check(ev.L.epa_dev_rell_kh(ev.h, _ptr(a["pairs"]), _ptr(a["pen"]), _ptr(a["dis"]), None, len(a["pairs"]),
                                   _ptr(a["codes"]), _ptr(a["wb"]), _ptr(a["ws"]), len(a["wb"]), _ptr(a["sid"]), MEM_R, MEM_SEED,
                                   _ptr(out.get("p_kh")), _ptr(out.get("p_wkh")), _ptr(out.get("p_wsh"))))
    torch.cuda.synchronize()
    return {key: np.array(v if isinstance(v, np.ndarray) else v.cpu().numpy()) for key, v in out.items()}


@pytest.mark.parametrize("name", ["D5", "A4"])
def test_memory_placement_and_history(name):
    ev = evaluator(name, "plain")
    a = host_input(name)
    n = len(a["pairs"])
    host = lambda: np.full(n, np.nan)                                                    # noqa: E731
    dev = lambda: torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")     # noqa: E731
    want = kh_call(ev, a, {key: host() for key in KEYS})
    assert all(np.all(np.isfinite(want[key])) for key in KEYS) and np.any((want["p_wsh"] > 0) & (want["p_wsh"] < 1))
    got = kh_call(ev, device_input(name), {key: dev() for key in KEYS})
    assert all(np.array_equal(got[key], want[key]) for key in KEYS)
    out = dict(p_kh=dev(), p_wkh=host(), p_wsh=host())
    got = kh_call(ev, a, out)
    assert all(np.array_equal(got[key], want[key]) for key in KEYS)
    # another member of the family on the same context: the buffers keep their values, the call made again repeats them
    entries = (a["pairs"], a["pen"], a["dis"], a["codes"], a["wb"], a["ws"])
    ev.rell_tests(*entries, MEM_R, seed=MEM_SEED, stream_id=a["sid"])
    ev.marginal_like(a["pairs"], a["codes"], a["wb"], a["ws"], *epa.posterior_rule(0.05, Kx=3, Kp=5))
    assert np.array_equal(out["p_kh"].cpu().numpy(), want["p_kh"]) and np.array_equal(out["p_wkh"], want["p_wkh"])
    got = kh_call(ev, a, {key: host() for key in KEYS})
    assert all(np.array_equal(got[key], want[key]) for key in KEYS)
