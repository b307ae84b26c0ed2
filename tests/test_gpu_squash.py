"""epa_dev_squash (Evaluator.squash): squash clustering of placement samples.

The cases are squash_ref.CASES: krd_ref.case on the five trees of tests/edpl_ref.py (3 .. 1197 branches, 14 or 15 samples;
the 600-tip ladder carries a sample with a point on every branch, so ranks cross the row kernel's 1024-rank tile) and
case65 (65 samples on the 40-tip tree: many merges, slot reuse, a row pass over more than 64 active clusters).  The
contexts are test_gpu_krd's.

  1. replay against epa_dev_krd, BIT FOR BIT: at every step the active clusters are materialised (squash_ref.materialise)
     and given to Evaluator.krd; (merge_a, merge_b) must be the tie rule's argmin of that matrix and merge_dist must have
     its bits.  No tolerance: the comparison object is an entry point that is pinned against a brute force of its own.
  2. with the matrix asked for it has the bits of Evaluator.krd on the same input.
  3. against squash_ref.restate: the same (a, b) on every step (test_squash_cpu shows every step to be decided) and
     |merge_dist - d| <= tol of that pair.
  4. the same bits from a second call, from the entries permuted so that every sample keeps its relative order, and with
     device buffers for every input and output.
  5. edge shapes: S = 2, S = 1, and n = 0 with S = 5, which merges (0, 1), (2, 3), (4, 5), (6, 7) at 0.0.
  6. refusals -- no topology, S = 0, S = 4097, a branch id and a sample id out of range from host arrays (entry named) and
     from device arrays -- after which the same context returns the earlier krd and edpl bits; the timers.
"""
import functools

import numpy as np
import pytest

import edpl_ref as er
import epa_ng_amd as epa
import krd_ref as kr
import squash_ref as sr
from test_gpu_edpl import make_ctx
from test_gpu_krd import bits, context, subset
from test_gpu_score_at import make_pairs

pytestmark = pytest.mark.gpu


def call(ev, c, order=None, with_krd=False):
    o = np.arange(len(c["branch"])) if order is None else order
    return ev.squash(make_pairs(c["branch"][o], c["seq"][o]), c["distal"][o], c["weight"][o], c["S"], with_krd=with_krd)


@functools.lru_cache(maxsize=None)
def squashed(name):
    out = call(context(sr.tree_of(name)), sr.case(name), with_krd=True)
    for a in out:
        a.setflags(write=False)
    return out


def same_bits(x, y):
    return all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(x, y)) and len(x) == len(y)


@pytest.mark.parametrize("name", sr.CASES)
def test_replay_against_krd_bit_for_bit(name):
    c, ev = sr.case(name), context(sr.tree_of(name))
    ma, mb, md, ms, _ = squashed(name)
    S = c["S"]
    assert len(ma) == S - 1
    members = {s: [s] for s in range(S)}
    ids = list(range(S))
    for t in range(S - 1):
        m = sr.materialise(c, [members[i] for i in ids])           # ids ascending: position order is id order
        krd = ev.krd(make_pairs(m["branch"], m["seq"]), m["distal"], m["weight"], m["S"])
        iu = np.triu_indices(len(ids), 1)                           # row-major: (a, b) in lexicographic order
        k = int(np.argmin(krd[iu]))                                 # the first of the smallest
        a, b = ids[iu[0][k]], ids[iu[1][k]]
        assert (int(ma[t]), int(mb[t])) == (a, b), (name, t, ma[t], mb[t], a, b)
        assert bits(md[t:t + 1])[0] == bits(krd[iu][k:k + 1])[0], (name, t, md[t], krd[iu][k])
        assert int(ms[t]) == len(members[a]) + len(members[b])
        members[S + t] = sorted(members[a] + members[b])
        ids = [i for i in ids if i not in (a, b)] + [S + t]
    assert ev.kernel_ms("squash") >= 0.0


@pytest.mark.parametrize("name", ["tips4", "ladder600", "case65"])
def test_the_matrix_has_krds_bits(name):
    c, ev = sr.case(name), context(sr.tree_of(name))
    want = ev.krd(make_pairs(c["branch"], c["seq"]), c["distal"], c["weight"], c["S"])
    assert np.array_equal(bits(squashed(name)[4]), bits(want))
    assert same_bits(call(ev, c), squashed(name)[:4])               # without the matrix: the same merges


@pytest.mark.parametrize("name", sr.CASES)
def test_against_the_restatement(name):
    steps, _ = sr.run(name)
    ma, mb, md, ms, _ = squashed(name)
    worst = 0.0
    for t, s in enumerate(steps):
        assert (int(ma[t]), int(mb[t]), int(ms[t])) == (s["a"], s["b"], s["size"]), (name, t, ma[t], mb[t], s)
        d = abs(md[t] - s["d"])
        worst = max(worst, d / s["tol"] if s["tol"] > 0 else (0.0 if d == 0.0 else np.inf))
        assert d <= s["tol"], (name, t, md[t], s)
    print(name, "max |device - restate| / tol %.3g over %d steps" % (worst, len(steps)))


@pytest.mark.parametrize("name", ["ladder600", "case65"])
def test_same_bits_again_permuted_and_from_device_buffers(name):
    import torch
    c, ev = sr.case(name), context(sr.tree_of(name))
    first = squashed(name)
    assert same_bits(call(ev, c, with_krd=True), first)
    # the sample labels shuffled, every sample's entries dealt to its labels in their original order
    rng = np.random.RandomState(11)
    labels = rng.permutation(c["seq"])
    by_sample = np.argsort(c["seq"], kind="stable")
    order = np.empty(len(labels), np.int64)
    order[np.argsort(labels, kind="stable")] = by_sample
    assert np.array_equal(c["seq"][order], labels) and not np.array_equal(order, np.arange(len(order)))
    for s in (0, c["S"] // 2, c["S"] - 1):
        assert np.all(np.diff(order[labels == s]) > 0)
    assert same_bits(call(ev, c, order=order, with_krd=True), first)
    S = c["S"]
    pairs = make_pairs(c["branch"], c["seq"])
    d_in = [torch.from_numpy(pairs.view(np.uint32).reshape(-1, 2).copy()).cuda(), torch.from_numpy(c["distal"].copy()).cuda(),
            torch.from_numpy(c["weight"].copy()).cuda()]
    d_out = [torch.full((S - 1,), 7, dtype=torch.int32, device="cuda"), torch.full((S - 1,), 7, dtype=torch.int32, device="cuda"),
             torch.full((S - 1,), -1.0, dtype=torch.float64, device="cuda"), torch.full((S - 1,), 7, dtype=torch.int32, device="cuda")]
    d_krd = torch.full((S, S), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ev.squash(*d_in, S, with_krd=True, out=d_out, krd_out=d_krd)
    torch.cuda.synchronize()
    got = [d_out[0].cpu().numpy().view(np.uint32), d_out[1].cpu().numpy().view(np.uint32), d_out[2].cpu().numpy(),
           d_out[3].cpu().numpy().view(np.uint32), d_krd.cpu().numpy()]
    assert same_bits(got, first)
    assert same_bits(ev.squash(*d_in, S), first[:4])                # device entries, host outputs


def test_edge_shapes():
    c, ev = kr.case("random40"), context("random40")
    ix = c["index"]
    two = [ix["r257"], ix["w07"]]
    ma, mb, md, ms, krd = ev.squash(*subset(c, two), 2, with_krd=True)
    want = ev.krd(*subset(c, two), 2)
    assert (list(ma), list(mb), list(ms)) == ([0], [1], [2]) and bits(md)[0] == bits(want)[0, 1] and md[0] > 0.0
    assert np.array_equal(bits(krd), bits(want))
    one = ev.squash(*subset(c, [ix["r64"]]), 1, with_krd=True)
    assert all(len(x) == 0 for x in one[:4]) and one[4].shape == (1, 1) and bits(one[4])[0, 0] == 0
    ma, mb, md, ms = ev.squash(make_pairs([], []), np.zeros(0), np.zeros(0), 5)
    assert (list(ma), list(mb), list(ms)) == ([0, 2, 4, 6], [1, 3, 5, 7], [2, 2, 3, 5]) and np.all(bits(md) == 0)


def test_refusals_leave_the_context_usable():
    import torch
    c, e = kr.case("random40"), er.case("random40")
    B, S = len(c["blen"]), c["S"]
    pairs = make_pairs(c["branch"], c["seq"])
    ev = make_ctx(c["blen"])

    def refused(fn, text):
        with pytest.raises(epa.EpaError, match=text) as info:
            fn()
        assert info.value.code == -1, info.value

    refused(lambda: call(ev, c), "squash: no topology")
    ev.set_topology(c["prox"], c["dist"])
    krd_before = ev.krd(pairs, c["distal"], c["weight"], S, masses=True)
    edpl_before = ev.edpl(make_pairs(e["branch"], e["seq"]), e["distal"], e["weight"], e["Q"], row_dist=True)
    refused(lambda: ev.squash(pairs, c["distal"], c["weight"], 0), "squash: 0 samples")
    refused(lambda: ev.squash(pairs, c["distal"], c["weight"], 4097), "squash: 4097 samples")
    d_distal, d_weight = torch.from_numpy(c["distal"].copy()).cuda(), torch.from_numpy(c["weight"].copy()).cuda()
    bad = pairs.copy()
    bad["seq_id"][3] = S
    refused(lambda: ev.squash(bad, c["distal"], c["weight"], S), "squash: entry 3: sample id out of range")
    refused(lambda: ev.squash(torch.from_numpy(bad.view(np.uint32).reshape(-1, 2).copy()).cuda(), d_distal, d_weight, S),
            "squash: a sample id is out of range")
    bad = pairs.copy()
    bad["branch_id"][2] = B
    refused(lambda: ev.squash(bad, c["distal"], c["weight"], S), "squash: entry 2: branch id out of range")
    refused(lambda: ev.squash(torch.from_numpy(bad.view(np.uint32).reshape(-1, 2).copy()).cuda(), d_distal, d_weight, S),
            "squash: a branch id is out of range")
    w = c["weight"].copy()
    w[7] = np.nan
    refused(lambda: ev.squash(pairs, c["distal"], w, S), "squash: entry 7: weight is negative or not finite")
    got = call(ev, c, with_krd=True)
    assert same_bits(got, squashed("random40"))
    for which in ("squash", "squash_init", "squash_argmin", "squash_merge", "squash_row"):
        assert ev.kernel_ms(which) >= 0.0, which
    assert ev.kernel_ms("squash") >= ev.kernel_ms("squash_init")
    krd_after = ev.krd(pairs, c["distal"], c["weight"], S, masses=True)
    edpl_after = ev.edpl(make_pairs(e["branch"], e["seq"]), e["distal"], e["weight"], e["Q"], row_dist=True)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(krd_before + edpl_before, krd_after + edpl_after))
