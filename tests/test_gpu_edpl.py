"""epa_dev_set_topology / epa_dev_edpl (Evaluator.set_topology, Evaluator.edpl): path distances between placement points
and the expected distance between placement locations.

The references are restate() and brute() of tests/edpl_ref.py; the trees and objects are edpl_ref.case(): 3 tips, 4 tips
(both with a 1025-row object), a ladder of 600 tips (every level of the sparse table in use), synth.random_tree(40, 71)
and synth.random_tree(512, 1) with a tenth of its lengths set to 0 before the context is built; objects of 1, 2, 7, 64 and
65 rows, two rows on one edge in both orders, rows at distal 0 and at the full length, an edge and its ancestor, edges on
both sides of the root, the root's own edges, both orientations of child(b), a zero weight, weights that add up to 0.7 and
a query with no entry in the middle.  The contexts hold four sites of random CLVs under JC69: EDPL reads no CLV.

  1. row_dist and edpl equal restate() BIT FOR BIT and brute() within tol = 16 (h + k + 2) 2^-53 Dmax, per tree.
  2. entries shuffled across the queries give, per query, the bits of that query's entries in their order of appearance.
  3. host pointers and device pointers (torch tensors), inputs and outputs, give the same bits.
  4. refusals leave the context usable: no topology, a disconnected graph, B != n_nodes - 1, a node id out of range, a
     branch on one node, a negative weight, a distal length beyond the branch, ids out of range (host and device pairs);
     the valid call that follows returns what a fresh context returns.
  5. a second topology -- the same tree, two branches with their ends swapped -- replaces the first.
  6. a fixed score_at probe returns the same bits before and after set_topology + edpl; n == 0 writes Q zeros; the "edpl"
     timer runs.
"""
import functools

import numpy as np
import pytest

import edpl_ref as er
import epa_ng_amd as epa
from test_gpu_score_at import make_pairs

pytestmark = pytest.mark.gpu

H = 0.5 * np.array([[1.0, 1, 1, 1], [1, 1, -1, -1], [1, -1, 1, -1], [1, -1, -1, 1]])   # symmetric, H H = I


def make_ctx(blen, seed=3):
    """JC69, one rate category, four sites of random CLVs on branches of the given lengths"""
    clv = np.random.RandomState(seed).uniform(0.1, 1.0, (2, len(blen), 4, 1, 4))
    return epa.Evaluator(4, [1.0], [1.0], [0.0, -4.0 / 3, -4.0 / 3, -4.0 / 3], H, H, [0.25] * 4, blen, list(clv[0]), list(clv[1]))


@functools.lru_cache(maxsize=None)
def context(name):
    c = er.case(name)
    ev = make_ctx(c["blen"])
    ev.set_topology(c["prox"], c["dist"])
    return ev


def run(ev, c, order=None):
    """-> (edpl [Q], row_dist [n]) of the case's entries, in the given entry order"""
    o = np.arange(len(c["branch"])) if order is None else order
    return ev.edpl(make_pairs(c["branch"][o], c["seq"][o]), c["distal"][o], c["weight"][o], c["Q"], row_dist=True)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("name", er.TREES)
def test_bits_of_the_restatement_and_brute_within_tol(name):
    c, ev = er.case(name), context(name)
    edpl, rows = run(ev, c)
    wrong = np.flatnonzero(bits(rows) != bits(c["want_rows"]))
    print(name, "rows differing in bits: %d of %d; max |device - brute| / tol: row_dist %.3g edpl %.3g" %
          (len(wrong), len(rows), np.max(np.abs(rows - c["brute_rows"]) / c["tol_rows"]),
           np.max(np.abs(edpl - c["brute_edpl"]) / c["tol_q"])))
    assert len(wrong) == 0, (wrong[:5], rows[wrong[:5]], c["want_rows"][wrong[:5]])
    assert np.array_equal(bits(edpl), bits(c["want_edpl"]))
    assert np.all(np.abs(rows - c["brute_rows"]) <= c["tol_rows"]) and np.all(np.abs(edpl - c["brute_edpl"]) <= c["tol_q"])
    assert edpl[c["empty"]] == 0.0 and ev.kernel_ms("edpl") >= 0.0
    # row_dist left out: the same edpl
    assert np.array_equal(bits(ev.edpl(make_pairs(c["branch"], c["seq"]), c["distal"], c["weight"], c["Q"])), bits(edpl))


@pytest.mark.parametrize("name", ["tips4", "random40"])
def test_shuffled_entries_keep_their_order_of_appearance(name):
    c, ev = er.case(name), context(name)
    order = np.random.RandomState(17).permutation(len(c["branch"]))
    want_rows, want_edpl = er.restate(c["prox"], c["dist"], c["blen"], c["branch"][order], c["seq"][order], c["distal"][order],
                                      c["weight"][order], c["Q"])
    edpl, rows = run(ev, c, order)
    assert np.array_equal(bits(rows), bits(want_rows)) and np.array_equal(bits(edpl), bits(want_edpl))
    # another order of the sum: the values of the unshuffled call within tol, and not all of its bits
    assert np.all(np.abs(edpl - c["want_edpl"]) <= c["tol_q"])
    assert np.any(bits(rows) != bits(c["want_rows"][order]))


def test_device_pointers_give_the_same_bits():
    import torch
    c, ev = er.case("random40"), context("random40")
    edpl, rows = run(ev, c)
    pairs = make_pairs(c["branch"], c["seq"])
    d_pairs = torch.from_numpy(pairs.view(np.uint32).reshape(-1, 2).copy()).cuda()
    d_distal, d_weight = torch.from_numpy(c["distal"].copy()).cuda(), torch.from_numpy(c["weight"].copy()).cuda()
    d_rows = torch.full((len(pairs),), -1.0, dtype=torch.float64, device="cuda")
    d_edpl = torch.full((c["Q"],), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ev.edpl(d_pairs, d_distal, d_weight, c["Q"], row_dist=True, out=d_edpl, row_out=d_rows)
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_rows.cpu().numpy()), bits(rows)) and np.array_equal(bits(d_edpl.cpu().numpy()), bits(edpl))
    # mixed: device entries, host outputs
    e2, r2 = ev.edpl(d_pairs, d_distal, d_weight, c["Q"], row_dist=True)
    assert np.array_equal(bits(r2), bits(rows)) and np.array_equal(bits(e2), bits(edpl))
    # device pairs with an id out of range: found by the kernels, refused, and the context goes on
    bad = pairs.copy()
    bad["seq_id"][3] = c["Q"]
    with pytest.raises(epa.EpaError, match="sequence id"):
        ev.edpl(torch.from_numpy(bad.view(np.uint32).reshape(-1, 2).copy()).cuda(), d_distal, d_weight, c["Q"])
    bad = pairs.copy()
    bad["branch_id"][5] = len(c["blen"])
    with pytest.raises(epa.EpaError, match="branch id"):
        ev.edpl(torch.from_numpy(bad.view(np.uint32).reshape(-1, 2).copy()).cuda(), d_distal, d_weight, c["Q"])
    e3, r3 = run(ev, c)
    assert np.array_equal(bits(r3), bits(rows)) and np.array_equal(bits(e3), bits(edpl))


def test_refusals_leave_the_context_usable():
    c = er.case("random40")
    B = len(c["blen"])
    fresh_edpl, fresh_rows = run(context("random40"), c)
    ev = make_ctx(c["blen"])
    pairs = make_pairs(c["branch"], c["seq"])

    def refused(call, text):
        with pytest.raises(epa.EpaError, match=text) as info:
            call()
        assert info.value.code == -1, info.value

    refused(lambda: run(ev, c), "no topology")
    # a disconnected graph with B = n_nodes - 1 branches: the last branch tied to the ends of the one before it
    # (a double edge), which leaves one of its own ends unreachable
    prox, dist = c["prox"].copy(), c["dist"].copy()
    prox[B - 1], dist[B - 1] = prox[B - 2], dist[B - 2]
    refused(lambda: ev.set_topology(prox, dist), "not connected")
    # the same with a whole subtree cut off: the branch above the deepest inner node tied elsewhere
    t = er.rooted(c["prox"], c["dist"], c["blen"])
    inner = max((v for v in range(B + 1) if v in t["parent"]), key=lambda v: t["level"][v])
    cut = t["pedge"][inner]
    prox, dist = c["prox"].copy(), c["dist"].copy()
    prox[cut], dist[cut] = prox[0], dist[0]
    refused(lambda: ev.set_topology(prox, dist), "not connected: branch \\d+ cannot be reached")
    refused(lambda: ev.set_topology(c["prox"], c["dist"], n_nodes=B + 2), "nodes")
    refused(lambda: ev.set_topology(c["prox"], c["dist"], n_nodes=B), "nodes")
    prox = c["prox"].copy()
    prox[4] = B + 1
    refused(lambda: ev.set_topology(prox, c["dist"]), "branch 4: node id %d is out of range" % (B + 1))
    prox = c["prox"].copy()
    prox[6] = c["dist"][6]
    refused(lambda: ev.set_topology(prox, c["dist"]), "branch 6: both ends")
    refused(lambda: run(ev, c), "no topology")          # none of the refused calls left one behind
    ev.set_topology(c["prox"], c["dist"])
    w = c["weight"].copy()
    w[7] = -0.25
    refused(lambda: ev.edpl(pairs, c["distal"], w, c["Q"]), "entry 7: weight is negative or not finite")
    w[7] = np.nan
    refused(lambda: ev.edpl(pairs, c["distal"], w, c["Q"]), "entry 7: weight")
    d = c["distal"].copy()
    d[9] = c["blen"][c["branch"][9]] * 1.5 + 1e-3
    refused(lambda: ev.edpl(pairs, d, c["weight"], c["Q"]), "entry 9: distal length beyond the branch's length")
    d[9] = -1e-9
    refused(lambda: ev.edpl(pairs, d, c["weight"], c["Q"]), "entry 9: distal length is negative or not finite")
    bad = pairs.copy()
    bad["branch_id"][2] = B
    refused(lambda: ev.edpl(bad, c["distal"], c["weight"], c["Q"]), "entry 2: branch id out of range")
    bad = pairs.copy()
    bad["seq_id"][2] = c["Q"]
    refused(lambda: ev.edpl(bad, c["distal"], c["weight"], c["Q"]), "entry 2: sequence id out of range")
    # a refused set_topology keeps the topology that was set
    refused(lambda: ev.set_topology(prox, c["dist"]), "branch 6: both ends")
    edpl, rows = run(ev, c)
    assert np.array_equal(bits(rows), bits(fresh_rows)) and np.array_equal(bits(edpl), bits(fresh_edpl))


def test_a_second_topology_replaces_the_first():
    c = er.case("random40")
    ev = make_ctx(c["blen"])
    ev.set_topology(c["prox"], c["dist"])
    first_edpl, first_rows = run(ev, c)
    prox, dist = c["prox"].copy(), c["dist"].copy()
    swap = [int(c["branch"][0]), int(c["branch"][6])]      # two occupied branches, neither of them branch 0 (the root's)
    assert 0 not in swap and swap[0] != swap[1]
    prox[swap], dist[swap] = c["dist"][swap], c["prox"][swap]
    ev.set_topology(prox, dist)
    edpl, rows = run(ev, c)
    want_rows, want_edpl = er.restate(prox, dist, c["blen"], c["branch"], c["seq"], c["distal"], c["weight"], c["Q"])
    assert np.array_equal(bits(rows), bits(want_rows)) and np.array_equal(bits(edpl), bits(want_edpl))
    assert np.any(np.abs(edpl - first_edpl) > c["tol_q"])        # distal lengths now count from the other end
    ev.set_topology(c["prox"], c["dist"])
    edpl, rows = run(ev, c)
    assert np.array_equal(bits(rows), bits(first_rows)) and np.array_equal(bits(edpl), bits(first_edpl))


def test_other_entry_points_do_not_see_the_topology_and_empty_calls():
    c = er.case("tips4")
    B = len(c["blen"])
    ev = make_ctx(c["blen"])
    codes, wb, ws = epa.encode_queries(4, ["ACGT", "A-GT", "TTAC"])
    pb = np.arange(3 * B) % B
    ps = np.arange(3 * B) // B
    pen = np.linspace(0.01, 0.5, 3 * B)
    dis = np.linspace(0.0, 1.0, 3 * B) * c["blen"][pb]
    before = ev.score_at(make_pairs(pb, ps), pen, dis, codes, wb, ws)
    ev.set_topology(c["prox"], c["dist"])
    edpl, rows = run(ev, c)
    assert np.array_equal(bits(rows), bits(c["want_rows"]))
    after = ev.score_at(make_pairs(pb, ps), pen, dis, codes, wb, ws)
    assert np.array_equal(bits(before), bits(after)) and np.all(np.isfinite(before))
    # n == 0: Q zeros
    out = np.full(5, -1.0)
    ev.edpl(make_pairs([], []), np.zeros(0), np.zeros(0), 5, out=out)
    assert np.all(out == 0.0)
    edpl2, rows2 = run(ev, c)
    assert np.array_equal(bits(rows2), bits(rows)) and np.array_equal(bits(edpl2), bits(edpl))
