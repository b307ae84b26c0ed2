"""Pairs whose branch ends in a tip run on the TIPD instantiations of the single-wave nucleotide Newton kernels
(option tip_distal, default 1): the distal side of such a branch is, per site, one of 16 four-vectors, so the kernels
read the tip's 4-bit state set instead of 16 rows of refT.  The arithmetic is the same operations on the same operands
in the same order, so every result and every counter must be bit-identical to the row form (tip_distal 0): for every
window class (each NCH with and without the half-chunk tail), both Newton forms, pair lists that are all tip, all inner
and interleaved, reference tips with gaps and 2-, 3- and 4-state ambiguity characters, through epa_dev_thorough and
through the fused chunk body (host-launched and queued), and against the oracle under the parity tests' tolerances."""
import numpy as np
import pytest

import epa_ng_amd as epa
from epa_ng_amd import hostlib, synth
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

LNL_TOL = 1e-6                                  # tests/test_gpu_parity.py
WINDOWS = (40, 64, 100, 128, 150, 190, 80)      # span classes 0, 0, 1, 1, 11, 2 -- and 10, the two-chunk half-chunk tail
N_TIPS, W = 10, 200
FIELDS = ("lnl", "pendant_length", "distal_length")
COUNTERS = ("rounds", "newton_evals", "reverts")


def _span_class(s):
    return 10 if 64 < s <= 96 else 11 if 128 < s <= 160 else min((s + 63) // 64, 4) - 1


def _window_read(seq, start, n):
    return "-" * start + seq[start:start + n] + "-" * (len(seq) - start - n)


def _build_case():
    root = synth.random_tree(N_TIPS, 311)
    rates = synth.gamma_rates(0.7)
    labels, clean = synth.simulate_msa(root, W, synth.CFG2_SUBST, synth.CFG2_FREQS, rates, 312)
    rng = np.random.RandomState(313)
    # reference tips: a third of the characters replaced by gaps and ambiguity codes (every state set occurs)
    amb = synth.NT_COLS
    seqs = []
    for s in clean:
        a = np.array(list(s))
        hit = rng.random_sample(W) < 0.35
        a[hit] = np.array(list(amb))[rng.randint(0, len(amb), int(hit.sum()))]
        seqs.append("".join(a))
    # reads: windows of the clean sequences (their first and last column are never a gap), 4 % substitutions
    reads = []
    for k, n in enumerate(WINDOWS):
        for j in range(3):
            src = clean[(3 * k + j) % N_TIPS]
            st = int(rng.randint(0, W - n + 1))
            r = np.array(list(src[st:st + n]))
            mut = rng.random_sample(n) < 0.04
            r[mut] = np.array(list("ACGT"))[rng.randint(0, 4, int(mut.sum()))]
            reads.append("-" * st + "".join(r) + "-" * (W - st - n))
    nw = synth.newick(root)
    ref = hostlib.Reference(nw, labels, seqs, states=4, subst=synth.CFG2_SUBST, freqs=synth.CFG2_FREQS, rates=rates)
    codes, wb, ws = epa.encode_queries(4, reads, compact=True)
    assert sorted(set(int(s) for s in ws)) == sorted(set(WINDOWS))
    assert {_span_class(int(s)) for s in ws} == {0, 1, 2, 10, 11}
    tipmap = ref.tipmap()
    tips, masks = [], set()
    for b in range(ref.B):
        t = ref.branch(b)["dist_tip"]
        if t is not None:
            tips.append(b)
            for q in range(len(reads)):
                masks |= set(int(m) for m in tipmap[t[wb[q]:wb[q] + ws[q]]])
    assert len(tips) == N_TIPS and masks == set(range(1, 16))   # every state set inside the windows
    inner = [b for b in range(ref.B) if b not in tips]
    o = Oracle(nw, labels, seqs, 4, synth.CFG2_SUBST, synth.CFG2_FREQS, rates)
    return dict(ref=ref, reads=reads, enc=(codes, wb, ws), tips=tips, inner=inner, oracle=o, clean=clean,
                labels=labels, seqs=seqs, nw=nw, rates=rates, shared={})


@pytest.fixture(scope="module")
def case():
    return _build_case()


def _pairs(branches, Q):
    p = np.zeros(len(branches) * Q, epa.PAIR_DTYPE)
    p["branch_id"] = np.repeat(np.asarray(branches, np.uint32), Q)
    p["seq_id"] = np.tile(np.arange(Q, dtype=np.uint32), len(branches))
    return p


def _pair_list(case, mix):
    Q = len(case["reads"])
    if mix == "tip":
        return _pairs(case["tips"], Q)
    if mix == "inner":
        return _pairs(case["inner"], Q)
    return _pairs(list(range(case["ref"].B)), Q)   # branch-major: tip and inner branches interleave


def _thorough(ev, pairs, enc, tip_distal):
    ev.set_option("tip_distal", tip_distal)
    res = ev.thorough(pairs, *enc)
    return res.copy(), dict(ev.last_stats)


@pytest.mark.parametrize("newton_lds", [0, 1])
@pytest.mark.parametrize("mix", ["tip", "inner", "interleaved"])
def test_tip_distal_equals_row_form_bitwise(case, mix, newton_lds):
    ev = case["ref"].evaluator()
    ev.set_option("newton_lds", newton_lds)
    pairs = _pair_list(case, mix)
    on, st_on = _thorough(ev, pairs, case["enc"], 1)
    off, st_off = _thorough(ev, pairs, case["enc"], 0)
    again, _ = _thorough(ev, pairs, case["enc"], 1)
    for f in FIELDS:
        assert np.all(np.isfinite(on[f])), f
        assert np.array_equal(on[f], off[f]), f
        assert np.array_equal(on[f], again[f]), f
    for k in COUNTERS:
        assert st_on[k] == st_off[k], k
    assert st_on["newton_evals"] > 0
    case["shared"][(mix, newton_lds)] = on
    ev.close()


@pytest.mark.parametrize("mix", ["tip", "inner", "interleaved"])
def test_tip_distal_oracle_parity(case, mix):
    pairs = _pair_list(case, mix)
    res = case["shared"].get((mix, 0))
    ev = case["ref"].evaluator()
    st = None
    if res is None:
        res, st = _thorough(ev, pairs, case["enc"], 1)
    o = case["oracle"]
    tl, tp, td = o.thorough(pairs["branch_id"], pairs["seq_id"], case["reads"])
    assert np.max(np.abs(res["lnl"] - tl)) < LNL_TOL
    assert np.max(np.abs(res["pendant_length"] - tp) / np.maximum(1.0, tp)) < 1e-6
    assert np.max(np.abs(res["distal_length"] - td)) < 1e-6
    if st is None:
        _, st = _thorough(ev, pairs, case["enc"], 1)
    assert st["rounds"] == o.last_stats["rounds"]
    assert st["reverts"] == o.last_stats["reverts"]
    ev.close()


def _one_length_reads(case, n_tip_like, n_random, seed):
    """150-site reads: windows of the clean tip sequences (they land on or next to their tip's branch) and random
    sequences (they land anywhere)"""
    rng = np.random.RandomState(seed)
    out = []
    for j in range(n_tip_like):
        src = case["clean"][j % N_TIPS]
        out.append(_window_read(src, int(rng.randint(0, W - 150 + 1)), 150))
    for j in range(n_random):
        s = "".join(np.array(list("ACGT"))[rng.randint(0, 4, W)])
        out.append(_window_read(s, int(rng.randint(0, W - 150 + 1)), 150))
    return out


def _chunk(ev, enc, tip_distal, queued, **kw):
    ev.set_option("tip_distal", tip_distal)
    ev.set_option("queued_thorough", queued)
    p, r = ev.place_chunk(*enc, **kw)
    return p.copy(), r.copy(), dict(ev.last_stats)


def _same_chunk(a, b):
    assert np.array_equal(a[0], b[0])
    for f in FIELDS:
        assert np.array_equal(a[1][f], b[1][f]), f
    for k in COUNTERS:
        assert a[2][k] == b[2][k], k


def test_fused_chunk_body_with_the_option_on_and_off(case):
    ev = case["ref"].evaluator()
    tips = set(case["tips"])
    one_len = _one_length_reads(case, 20, 40, 317)
    # one read length (the selection itself counts the tip-distal pairs apart) and mixed lengths (launch_thorough does)
    for reads, kw in ((one_len, dict(max_span=150)), (case["reads"], {})):
        enc = epa.encode_queries(4, reads, compact=True)
        base = _chunk(ev, enc, 0, 0, **kw)
        kinds = {int(b) in tips for b in base[0]["branch_id"]}
        assert kinds == {True, False} and len(base[0]) > len(reads)
        for tip_distal, queued in ((1, 0), (1, 1), (0, 1)):
            _same_chunk(_chunk(ev, enc, tip_distal, queued, **kw), base)
    # chunks whose candidates are all of one kind: one of the two launches is empty.  threshold 0.01 keeps the best
    # branch of a read only
    enc = epa.encode_queries(4, one_len, compact=True)
    best = _chunk(ev, enc, 0, 0, threshold=0.01, max_span=150)[0]
    assert len(best) == len(one_len)
    is_tip = np.zeros(len(one_len), bool)
    is_tip[best["seq_id"]] = np.isin(best["branch_id"], case["tips"])
    assert is_tip.any() and not is_tip.all()
    for kind in (True, False):
        sub = [r for r, t in zip(one_len, is_tip) if t == kind]
        enc = epa.encode_queries(4, sub, compact=True)
        base = _chunk(ev, enc, 0, 0, threshold=0.01, max_span=150)
        assert len(base[0]) == len(sub) and set(np.isin(base[0]["branch_id"], case["tips"])) == {kind}
        for tip_distal, queued in ((1, 0), (1, 1)):
            _same_chunk(_chunk(ev, enc, tip_distal, queued, threshold=0.01, max_span=150), base)
    ev.close()


def test_tip_distal_is_a_known_option(case):
    ev = case["ref"].evaluator()
    ev.set_option("tip_distal", 0)
    ev.set_option("tip_distal", 1)
    ev.close()
