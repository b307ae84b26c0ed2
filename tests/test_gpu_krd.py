"""epa_dev_krd (Evaluator.krd): Kantorovich-Rubinstein distances between placement samples, edge and clade masses.

The references are restate() and brute() of tests/krd_ref.py on the trees of tests/edpl_ref.py; the samples are
krd_ref.case(): an empty sample, two single unit points (the deepest branch and branch 0), 300 points on one branch,
points at distal 0 and at the full length of two branches, four points at one x, random samples of 2, 7, 64, 65 and 257
rows, a copy of the 65-row sample, a sample of total 0.7, a sample of zero weights -- and on the 600-tip ladder a sample
with a point on every branch, which crosses the boundary of the pair kernel's 1024-rank tile.  All pairs where B <= 77,
the special pairs and 24 random ones on the two large trees.  The contexts are test_gpu_edpl.make_ctx's.

  1. krd within tol(a, b) = 8 (B + n_a + n_b + 4) 2^-53 (W_a + W_b) sum(blen) of restate() and of brute(); edge_mass and
     clade_mass within 8 (B + n_s) 2^-53 W_s of restate().
  2. the exact properties of the header: (a) a zero diagonal, (b) a bit-symmetric matrix, (c) a pair's bits in a call of
     its own with S = 2 and with the sample numbering reversed, (d) a copy at 0.0 with bit-equal rows, (e) the same bits
     from a second call.
  3. single-point samples against epa_dev_edpl's row_dist of the two-row object with weights (0, 1).
  4. S = 1, n == 0, device pointers for every array.
  5. refusals that leave the context usable; a second topology with another root is followed, and edpl on the same
     context is not disturbed.
"""
import functools

import numpy as np
import pytest

import edpl_ref as er
import epa_ng_amd as epa
import krd_ref as kr
from test_gpu_edpl import make_ctx
from test_gpu_score_at import make_pairs

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def context(name):
    prox, dist, blen = er.tree(name)
    ev = make_ctx(blen)
    ev.set_topology(prox, dist)
    return ev


def run(ev, c, masses=False, order=None):
    o = np.arange(len(c["branch"])) if order is None else order
    return ev.krd(make_pairs(c["branch"][o], c["seq"][o]), c["distal"][o], c["weight"][o], c["S"], masses=masses)


@functools.lru_cache(maxsize=None)
def full(name):
    out = run(context(name), kr.case(name), masses=True)
    for a in out:
        a.setflags(write=False)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def subset(c, samples):
    """the entries of the given samples, renumbered 0, 1, ... in the given order, in their order of appearance"""
    remap = {s: k for k, s in enumerate(samples)}
    keep = np.flatnonzero(np.isin(c["seq"], samples))
    seq = np.array([remap[int(s)] for s in c["seq"][keep]], np.uint32)
    return make_pairs(c["branch"][keep], seq), c["distal"][keep], c["weight"][keep]


@pytest.mark.parametrize("name", er.TREES)
def test_krd_and_masses_within_tol_of_both_references(name):
    c = kr.case(name)
    krd, edge, clade = full(name)
    worst = [0.0, 0.0]
    for a, b in c["pairs"]:
        for k, ref in enumerate((c["want"], c["brute"])):
            d, t = abs(krd[a, b] - ref[a, b]), c["tol"][a, b]
            worst[k] = max(worst[k], d / t if t > 0 else (0.0 if d == 0.0 else np.inf))
            assert d <= t, (name, a, b, krd[a, b], ref[a, b], t)
    mt = kr.mass_tol(c)
    print(name, "max |device - restate| / tol %.3g, |device - brute| / tol %.3g; masses / tol: edge %.3g clade %.3g" %
          (worst[0], worst[1], np.max(np.abs(edge - c["want_edge"]) / np.maximum(mt, 1e-300)),
           np.max(np.abs(clade - c["want_clade"]) / np.maximum(mt, 1e-300))))
    assert np.all(np.abs(edge - c["want_edge"]) <= mt) and np.all(np.abs(clade - c["want_clade"]) <= mt)
    # distances mean something: far from 0 where the samples differ
    ix = c["index"]
    assert krd[ix["unit_deep"], ix["unit_b0"]] > 1e6 * c["tol"][ix["unit_deep"], ix["unit_b0"]]
    assert context(name).kernel_ms("krd") >= 0.0
    # masses left out: the same matrix
    assert np.array_equal(bits(run(context(name), c)), bits(krd))


@pytest.mark.parametrize("name", ["tips4", "ladder600", "random40"])
def test_exact_properties(name):
    c, ev = kr.case(name), context(name)
    krd, edge, clade = full(name)
    S, ix = c["S"], c["index"]
    assert np.all(bits(np.diag(krd)) == 0)                                            # (a): +0.0
    assert np.array_equal(bits(krd), bits(krd.T))                                     # (b)
    again = run(ev, c, masses=True)                                                   # (e)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(again, (krd, edge, clade)))
    r65, cp = ix["r65"], ix["copy65"]                                                 # (d)
    assert bits(krd[r65:r65 + 1, cp])[0] == 0
    assert np.array_equal(bits(krd[r65]), bits(krd[cp]))
    assert np.array_equal(bits(edge[r65]), bits(edge[cp])) and np.array_equal(bits(clade[r65]), bits(clade[cp]))
    # (c): three pairs, each in a call of its own with S = 2, in both numberings
    chosen = [(ix["r257"], ix["w07"]), (ix["pile300"], ix["four_at_x"]), (ix["r64"], ix.get("every", ix["ends"]))]
    for a, b in chosen:
        for u, v in ((a, b), (b, a)):
            two = ev.krd(*subset(c, [u, v]), 2)
            assert bits(two)[0, 1] == bits(krd)[a, b] and bits(two)[1, 0] == bits(krd)[a, b], (name, a, b, u, v)
    # reversed sample numbering: the transposed entry, bit for bit
    rev = ev.krd(make_pairs(c["branch"], (S - 1 - c["seq"].astype(np.int64)).astype(np.uint32)), c["distal"], c["weight"], S)
    assert np.array_equal(bits(rev), bits(krd[::-1, ::-1]))


def test_sixty_five_samples_in_another_interleaving():
    """(c) once more: the 40-tip case's samples among 65, the others' entries interleaved otherwise"""
    c, ev = kr.case("random40"), context("random40")
    krd = full("random40")[0]
    S0, B = c["S"], len(c["blen"])
    rng = np.random.RandomState(5)
    n_more = 65 - S0
    mb = rng.randint(B, size=40 * n_more)
    more = dict(branch=mb, seq=S0 + rng.randint(n_more, size=len(mb)), distal=rng.uniform(size=len(mb)) * c["blen"][mb],
                weight=rng.uniform(size=len(mb)))
    # a merge that keeps the order of the case's own entries
    slot = np.sort(rng.choice(len(mb) + len(c["branch"]), len(c["branch"]), replace=False))
    n = len(mb) + len(c["branch"])
    mine = np.zeros(n, bool)
    mine[slot] = True
    cols = {}
    for k in ("branch", "seq", "distal", "weight"):
        col = np.zeros(n, np.float64 if k in ("distal", "weight") else np.uint32)
        col[mine], col[~mine] = c[k], more[k]
        cols[k] = col
    big = ev.krd(make_pairs(cols["branch"], cols["seq"]), cols["distal"], cols["weight"], 65)
    assert np.array_equal(bits(big[:S0, :S0]), bits(krd))
    assert np.array_equal(bits(big), bits(big.T)) and np.all(big[S0:, :S0] > 0.0)


@pytest.mark.parametrize("name", ["random40", "ladder600"])
def test_single_points_against_edpl_row_dist(name):
    c, ev = kr.case(name), context(name)
    ix = c["index"]
    a, b = ix["unit_deep"], ix["unit_b0"]
    rows = [int(np.flatnonzero(c["seq"] == s)[0]) for s in (a, b)]
    _, row_dist = ev.edpl(make_pairs(c["branch"][rows], [0, 0]), c["distal"][rows], [0.0, 1.0], 1, row_dist=True)
    assert abs(full(name)[0][a, b] - row_dist[0]) <= er.tol(c["prox"], c["dist"], c["blen"], 2) + c["tol"][a, b]
    assert row_dist[0] > 0.0


def test_one_sample_no_entries_and_device_pointers():
    import torch
    c, ev = kr.case("random40"), context("random40")
    krd, edge, clade = full("random40")
    S, B = c["S"], len(c["blen"])
    one = ev.krd(*subset(c, [c["index"]["r64"]]), 1)
    assert one.shape == (1, 1) and bits(one)[0, 0] == 0
    out = np.full((3, 3), -1.0)
    k0, e0, c0 = ev.krd(make_pairs([], []), np.zeros(0), np.zeros(0), 3, masses=True, out=out)
    assert k0 is out and np.all(bits(out) == 0) and np.all(bits(e0) == 0) and np.all(bits(c0) == 0) and e0.shape == (3, B)
    pairs = make_pairs(c["branch"], c["seq"])
    d_pairs = torch.from_numpy(pairs.view(np.uint32).reshape(-1, 2).copy()).cuda()
    d_distal, d_weight = torch.from_numpy(c["distal"].copy()).cuda(), torch.from_numpy(c["weight"].copy()).cuda()
    d_krd = torch.full((S, S), -1.0, dtype=torch.float64, device="cuda")
    d_edge = torch.full((S, B), -1.0, dtype=torch.float64, device="cuda")
    d_clade = torch.full((S, B), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ev.krd(d_pairs, d_distal, d_weight, S, masses=True, out=d_krd, edge_out=d_edge, clade_out=d_clade)
    torch.cuda.synchronize()
    for dev, host in ((d_krd, krd), (d_edge, edge), (d_clade, clade)):
        assert np.array_equal(bits(dev.cpu().numpy()), bits(host))
    assert np.array_equal(bits(ev.krd(d_pairs, d_distal, d_weight, S)), bits(krd))     # device entries, host output


def test_refusals_leave_the_context_usable():
    import torch
    c = kr.case("random40")
    B, S = len(c["blen"]), c["S"]
    fresh = full("random40")
    ev = make_ctx(c["blen"])
    pairs = make_pairs(c["branch"], c["seq"])

    def refused(call, text):
        with pytest.raises(epa.EpaError, match=text) as info:
            call()
        assert info.value.code == -1, info.value

    refused(lambda: run(ev, c), "krd: no topology")
    ev.set_topology(c["prox"], c["dist"])
    refused(lambda: ev.krd(pairs, c["distal"], c["weight"], 0), "krd: 0 samples")
    refused(lambda: ev.krd(pairs, c["distal"], c["weight"], 4097), "krd: 4097 samples")
    bad = pairs.copy()
    bad["seq_id"][3] = S
    refused(lambda: ev.krd(bad, c["distal"], c["weight"], S), "entry 3: sample id out of range")
    d_distal, d_weight = torch.from_numpy(c["distal"].copy()).cuda(), torch.from_numpy(c["weight"].copy()).cuda()
    refused(lambda: ev.krd(torch.from_numpy(bad.view(np.uint32).reshape(-1, 2).copy()).cuda(), d_distal, d_weight, S),
            "krd: a sample id is out of range")
    bad = pairs.copy()
    bad["branch_id"][2] = B
    refused(lambda: ev.krd(bad, c["distal"], c["weight"], S), "entry 2: branch id out of range")
    refused(lambda: ev.krd(torch.from_numpy(bad.view(np.uint32).reshape(-1, 2).copy()).cuda(), d_distal, d_weight, S),
            "krd: a branch id is out of range")
    d = c["distal"].copy()
    d[9] = c["blen"][c["branch"][9]] * 1.5 + 1e-3
    refused(lambda: ev.krd(pairs, d, c["weight"], S), "entry 9: distal length beyond the branch's length")
    w = c["weight"].copy()
    w[7] = -0.25
    refused(lambda: ev.krd(pairs, c["distal"], w, S), "entry 7: weight is negative or not finite")
    w[7] = np.nan
    refused(lambda: ev.krd(pairs, c["distal"], w, S), "entry 7: weight is negative or not finite")
    got = run(ev, c, masses=True)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(got, fresh))


def test_another_root_is_followed_and_edpl_is_not_disturbed():
    c = kr.case("random40")
    e = er.case("random40")
    ev = make_ctx(c["blen"])
    ev.set_topology(c["prox"], c["dist"])
    edpl_before = ev.edpl(make_pairs(e["branch"], e["seq"]), e["distal"], e["weight"], e["Q"], row_dist=True)
    first = run(ev, c)
    assert np.array_equal(bits(first), bits(full("random40")[0]))
    edpl_after = ev.edpl(make_pairs(e["branch"], e["seq"]), e["distal"], e["weight"], e["Q"], row_dist=True)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(edpl_before, edpl_after))
    # the same tree with a branch in another part of it listed first: node_prox[0], the root, moves
    t = er.rooted(c["prox"], c["dist"], c["blen"])
    far = max(range(len(c["blen"])), key=lambda b: t["level"][t["child"][b]])
    perm = np.arange(len(c["blen"]))
    perm[0], perm[far] = far, 0
    ev2 = make_ctx(c["blen"][perm])
    ev2.set_topology(c["prox"], c["dist"])                  # any topology of the right size first
    prox, dist, blen = c["prox"][perm], c["dist"][perm], c["blen"][perm]
    ev2.set_topology(prox, dist)
    inv = np.argsort(perm)
    branch = inv[c["branch"]].astype(np.uint32)
    want, _, _ = kr.restate(prox, dist, blen, branch, c["seq"], c["distal"], c["weight"], c["S"])
    assert int(prox[0]) != int(c["prox"][0])
    got = ev2.krd(make_pairs(branch, c["seq"]), c["distal"], c["weight"], c["S"])
    assert np.all(np.abs(got - want) <= c["tol"])
    w07, r7 = c["index"]["w07"], c["index"]["r7"]
    assert abs(got[w07, r7] - first[w07, r7]) > c["tol"][w07, r7]          # unequal totals: the rooted definition
    eq = [(a, b) for a, b in c["pairs"] if abs(c["W"][a] - c["W"][b]) < 1e-12]
    assert len(eq) > 20 and all(abs(got[a, b] - first[a, b]) <= c["tol"][a, b] for a, b in eq)
