"""epa_dev_epca (Evaluator.epca): edge principal components of placement samples.

The cases, the references and the bounds are tests/epca_ref.py's (each bound is derived in its docstring; test_epca_cpu
shows every compared component, its sign and its null status to be decided).  The contexts are test_gpu_krd's.

  1. per case: imbalance within tol_x of restate(), excluded columns exactly 0.0; gram bit-symmetric and within tol_g of the
     Gram matrix (math.fsum) of the device's own X, centred as the header specifies.  The exact case (weights k / 1024, 32
     samples: X, mean, Xc and every partial sum of G are exact in fp64): X equals restate()'s and gram equals Xc @ Xc.T
     bit for bit, every off-diagonal tile included -- the check that pins the lane maps of the matrix instruction.
  2. per case with components: eigenvalue (S - 1) within tol_jac of eigh(gram) of the device's own matrix, and within
     tol_eig + 2 ||Xc||_F ||dXc||_F of restate()'s; edge_vec follows the sign rule, is zero on excluded edges, is within
     the Davis-Kahan bound of restate()'s and orthonormal within 8 tol_eig / sqrt(l_i l_j); proj within 8 tol_eig /
     sqrt(l_k) of Xc_dev @ edge_vec[k]; total_var is the sequential sum of gram's diagonal / (S - 1), bit for bit;
     sweeps < 30 (1 where G is zero); null components are exactly zero on tips3 and tips4, and random40 with S = 2 has none.
  3. the same bits from a second call, from device buffers in and out, and after a shuffle of the entries that keeps each
     sample's relative order.
  4. refusals, each by its text, after which the same context returns the earlier krd, squash and edpl bits; the timers.
"""
import functools
import math

import numpy as np
import pytest

import edpl_ref as er
import epa_ng_amd as epa
import epca_ref as pr
import krd_ref as kr
from test_gpu_edpl import make_ctx
from test_gpu_krd import bits, context
from test_gpu_score_at import make_pairs

pytestmark = pytest.mark.gpu


def call(ev, c, order=None, K=None):
    o = np.arange(len(c["branch"])) if order is None else order
    return ev.epca(make_pairs(c["branch"][o], c["seq"][o]), c["distal"][o], c["weight"][o], c["S"], K or c["K"] or 1,
                   with_imbalance=True, with_gram=True)


@functools.lru_cache(maxsize=None)
def result(name):
    c = pr.case(name)
    out = call(context(c["tree"]), c)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def own(name):
    """the device's X centred as specified, and the exact Gram matrix of that"""
    X, G = result(name)[5:7]
    mean, Xc = pr.centre(X)
    return Xc, pr.gram_fsum(Xc)


def same_bits(x, y):
    return len(x) == len(y) and all(np.array_equal(np.ascontiguousarray(p).view(np.uint8), np.ascontiguousarray(q).view(np.uint8))
                                    for p, q in zip(x, y))


@pytest.mark.parametrize("name", sorted(pr.CASES))
def test_imbalance_and_gram(name):
    c = pr.case(name)
    X, G = result(name)[5:7]
    S, B = c["S"], len(c["blen"])
    assert X.shape == (S, B) and G.shape == (S, S)
    err = np.abs(X - c["X"])
    tol = np.broadcast_to(pr.tol_x(c), X.shape)
    print(name, "max |X - restate| / tol_x %.3g" % np.max(err / np.where(tol > 0, tol, 1.0)))
    assert np.all(err <= tol)
    assert not bits(X[:, c["excluded"]]).any()
    assert np.array_equal(bits(G), bits(G.T))
    Xc, G_own = own(name)
    tg = pr.tol_g(Xc)
    print(name, "max |gram - fsum| / tol_g %.3g" % np.max(np.abs(G - G_own) / np.where(tg > 0, tg, 1.0)))
    assert np.all(np.abs(G - G_own) <= tg)
    if name == "specials":
        assert not X[0].any() and abs(c["W"][1] - 0.7) < 1e-12
    if name == "exact":
        assert np.array_equal(bits(X + 0.0), bits(c["X"] + 0.0))
        want = Xc @ Xc.T
        assert np.array_equal(bits(G + 0.0), bits(want + 0.0)), np.argwhere(G != want)[:8]
        assert np.array_equal(bits(G + 0.0), bits(c["G"] + 0.0))


@pytest.mark.parametrize("name", pr.COMPONENT_CASES)
def test_components(name):
    c = pr.case(name)
    ev, vec, proj, total, sweeps, X, G = result(name)
    S, K, B = c["S"], c["K"], len(c["blen"])
    Xc, _ = own(name)
    sweeps = int(sweeps[0])
    assert 1 <= sweeps < pr.MAX_SWEEPS and ev.shape == (K,) and vec.shape == (K, B) and proj.shape == (S, K)
    # against the device's own matrix
    lam_d, _ = pr.sorted_eigh(G)
    tj = pr.tol_jac(G, sweeps)
    print(name, "sweeps", sweeps, "max |lambda - eigh(gram)| / tol_jac %.3g" % (np.max(np.abs(ev * (S - 1) - np.maximum(lam_d[:K], 0.0))) / tj
                                                                               if tj else 0.0))
    assert np.all(np.abs(ev * (S - 1) - np.maximum(lam_d[:K], 0.0)) <= tj)
    acc = 0.0
    for i in range(S):
        acc = acc + G[i, i]
    assert bits(total)[0] == bits(np.array([acc / (S - 1)]))[0]
    # against the restatement
    lam, gap = c["lam"], pr.gaps(c["lam"])
    te = pr.tol_eig(c["G"], sweeps, B)
    cross = te + 2.0 * np.linalg.norm(c["Xc"]) * np.linalg.norm(Xc - c["Xc"])
    assert np.all(np.abs(ev * (S - 1) - np.maximum(lam[:K], 0.0)) <= cross)
    assert abs(total[0] - c["total_var"]) <= cross * S / (S - 1)
    assert not bits(vec[:, c["excluded"]]).any()
    live = [k for k in range(K) if not c["null"][k]]
    for k in range(K):
        if c["null"][k]:
            assert not bits(vec[k]).any() and not bits(proj[:, k]).any(), (name, k)
            continue
        a = np.abs(vec[k])
        assert vec[k][int(np.flatnonzero(a == a.max())[0])] > 0.0, (name, k)
        dk = pr.davis_kahan(cross, gap[k])
        d = np.linalg.norm(vec[k] - c["edge_vec"][k])
        print(name, k, "|edge_vec - restate| %.3g, Davis-Kahan bound %.3g" % (d, dk))
        assert d <= dk, (name, k, d, dk)
        assert np.all(np.abs(proj[:, k] - Xc @ vec[k]) <= 8 * te / math.sqrt(lam[k])), (name, k)
        assert np.all(np.abs(proj[:, k] - c["proj"][:, k]) <= math.sqrt(lam[0]) * dk + cross / math.sqrt(lam[k])), (name, k)
    for i in live:
        for j in live:
            assert abs(vec[i] @ vec[j] - (i == j)) <= 8 * te / math.sqrt(lam[i] * lam[j]), (name, i, j)
    assert live == {"tips3": [], "tips4": [0]}.get(name, list(range(K)))
    if name == "tips3":
        assert sweeps == 1 and not bits(G).any() and not bits(ev).any() and bits(total)[0] == 0


def shuffled(c, seed):
    """the sample labels shuffled, every sample's entries dealt to its labels in their original order"""
    labels = np.random.RandomState(seed).permutation(c["seq"])
    by_sample = np.argsort(c["seq"], kind="stable")
    order = np.empty(len(labels), np.int64)
    order[np.argsort(labels, kind="stable")] = by_sample
    assert np.array_equal(c["seq"][order], labels) and not np.array_equal(order, np.arange(len(order)))
    for s in (0, c["S"] // 2, c["S"] - 1):
        assert np.all(np.diff(order[labels == s]) > 0)
    return order


@pytest.mark.parametrize("name", ["random40_s17", "random512z"])
def test_same_bits_again_permuted_and_from_device_buffers(name):
    import torch
    c = pr.case(name)
    ev, first = context(c["tree"]), result(name)
    S, K, B = c["S"], c["K"], len(c["blen"])
    assert same_bits(call(ev, c), first)
    assert same_bits(call(ev, c, order=shuffled(c, 11)), first)
    pairs = make_pairs(c["branch"], c["seq"])
    d_in = [torch.from_numpy(pairs.view(np.uint32).reshape(-1, 2).copy()).cuda(), torch.from_numpy(c["distal"].copy()).cuda(),
            torch.from_numpy(c["weight"].copy()).cuda()]
    f64 = dict(dtype=torch.float64, device="cuda")
    d_out = [torch.full((K,), -1.0, **f64), torch.full((K, B), -1.0, **f64), torch.full((S, K), -1.0, **f64), torch.full((1,), -1.0, **f64),
             torch.full((1,), 77, dtype=torch.int32, device="cuda"), torch.full((S, B), -1.0, **f64), torch.full((S, S), -1.0, **f64)]
    torch.cuda.synchronize()
    ev.epca(*d_in, S, K, with_imbalance=True, with_gram=True, out=d_out)
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in d_out]
    got[4] = got[4].view(np.uint32)
    assert same_bits(got, first)
    assert same_bits(ev.epca(*d_in, S, K), first[:5])                 # device entries, host outputs, no optional output
    fewer = call(ev, c, K=1)                                          # fewer components: the same leading ones
    assert same_bits([fewer[0], fewer[1], fewer[2][:, 0]], [first[0][:1], first[1][:1], first[2][:, 0]])


def test_refusals_leave_the_context_usable():
    import torch
    c, k, e = pr.case("random40_s17"), kr.case("random40"), er.case("random40")
    B, S = len(c["blen"]), c["S"]
    pairs = make_pairs(c["branch"], c["seq"])
    kpairs, epairs = make_pairs(k["branch"], k["seq"]), make_pairs(e["branch"], e["seq"])
    ev = make_ctx(c["blen"])

    def refused(fn, text):
        with pytest.raises(epa.EpaError, match=text) as info:
            fn()
        assert info.value.code == -1, info.value

    refused(lambda: call(ev, c), "epca: no topology")
    ev.set_topology(c["prox"], c["dist"])
    before = (ev.krd(kpairs, k["distal"], k["weight"], k["S"], masses=True) + ev.squash(kpairs, k["distal"], k["weight"], k["S"]) +
              ev.edpl(epairs, e["distal"], e["weight"], e["Q"], row_dist=True))
    args = (pairs, c["distal"], c["weight"])
    refused(lambda: ev.epca(*args, 1, 1), "epca: 1 samples: one call takes 2 .. 1024")
    refused(lambda: ev.epca(*args, 1025, 5), "epca: 1025 samples: one call takes 2 .. 1024")
    refused(lambda: ev.epca(*args, S, 0), "epca: 0 components: 17 samples have 1 .. 16")
    refused(lambda: ev.epca(*args, S, S), "epca: 17 components: 17 samples have 1 .. 16")
    d_distal, d_weight = torch.from_numpy(c["distal"].copy()).cuda(), torch.from_numpy(c["weight"].copy()).cuda()
    bad = pairs.copy()
    bad["branch_id"][2] = B
    refused(lambda: ev.epca(bad, c["distal"], c["weight"], S, 5), "epca: entry 2: branch id out of range")
    refused(lambda: ev.epca(torch.from_numpy(bad.view(np.uint32).reshape(-1, 2).copy()).cuda(), d_distal, d_weight, S, 5),
            "epca: a branch id is out of range")
    w = c["weight"].copy()
    w[7] = -0.25
    refused(lambda: ev.epca(pairs, c["distal"], w, S, 5), "epca: entry 7: weight is negative or not finite")
    assert same_bits(call(ev, c), result("random40_s17"))
    for which in ("epca", "epca_tables", "epca_gram", "epca_eig", "epca_project", "epca_loop_wall"):
        assert ev.kernel_ms(which) >= 0.0, which
    assert ev.kernel_ms("epca") >= ev.kernel_ms("epca_eig")
    after = (ev.krd(kpairs, k["distal"], k["weight"], k["S"], masses=True) + ev.squash(kpairs, k["distal"], k["weight"], k["S"]) +
             ev.edpl(epairs, e["distal"], e["weight"], e["Q"], row_dist=True))
    assert same_bits(before, after)
