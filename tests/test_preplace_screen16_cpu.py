"""The 16-bit four-branch screen of the pair preplacement ("16-bit screen") in numpy integer arithmetic, in
the kernel's own formulation, on the oracle's lookup tables: no GPU.

Formulation (preplace.hip): a read gathers n site-pair entries per branch -- (site 4k, 4k + 1) and (4k + 2, 4k + 3) of its
full groups of four, then up to three tail singles (symbol, none); base = the maximum over the real branches of an entry;
q = max(rint((entry - base) / h), -32768) as int16; s1 = a (+) b, sum = sum (+) s1 with saturating adds; a segment's value
= the maximum over its 64 branches (phantom branches of the last quad: the floor); C_q = the sum of base over the read's
entries; delta = n h / 2 + (n + 2) n M 2^-53, h = the largest power of two with delta <= 1 at the longest window (made
smaller by `shift` powers of two); a segment is included when seg >= r - ceil((band_t + 2 delta) / h).

Checked for every read, at the rule's h and at shifts of 2 and 6: the included set holds every segment whose exact maximum
lies within band_t of the exact row maximum; C_q + h seg + delta >= the exact segment maximum, for EVERY cell; |C_q + h sum
- exact sum| <= delta on every unsaturated (read, branch) cell.  At the rule's own h at most 1 % of the reads may be
unscreenable (row maximum at the floor).

Reference: a 67-tip tree (131 branches: three segments, the last quad incomplete), W = 97 and 163; reads are windows of
reference rows with 5 % substitutions and a few N, spans 1 .. 8 and up to the longest that fits 160.
"""
import functools
import math

import numpy as np
import pytest

from epa_ng_amd import synth
from oracle_lib import Oracle

FLOOR = -32768
THR = 0.99999
SYM_COL = (1, 2, 4, 8, 15)          # lookup column (state-set code) of A, C, G, T, N


@functools.lru_cache(maxsize=None)
def tables(W):
    """-> (T [B][W][16] lookup tables of the oracle, the alignment rows)"""
    root = synth.random_tree(67, 900 + W)
    rates = synth.gamma_rates(synth.CFG2_ALPHA)
    labels, seqs = synth.simulate_msa(root, W, synth.CFG2_SUBST, synth.CFG2_FREQS, rates, 901 + W)
    o = Oracle(synth.newick(root), labels, seqs, 4, synth.CFG2_SUBST, synth.CFG2_FREQS, rates)
    return np.stack([o.branch_lookup(b) for b in range(o.B)]), seqs


def reads_of(W, seqs, n, seed):
    """-> [(begin, symbols 0 .. 4)]: windows of reference rows, 5 % substitutions, 1 % N"""
    rng = np.random.default_rng(seed)
    cap = min(W, 160)
    out = []
    for i in range(n):
        span = int(rng.integers(1, 9)) if i % 5 == 0 else int(rng.integers(cap // 2, cap + 1))
        if i % 11 == 0:
            span = cap - i % 4
        begin = int(rng.integers(0, W - span + 1))
        row = seqs[int(rng.integers(len(seqs)))][begin:begin + span]
        sym = np.array(["ACGT".index(c) if c in "ACGT" else 4 for c in row])
        sub = rng.random(span)
        sym = np.where(sub < 0.05, rng.integers(0, 4, span), sym)
        sym = np.where(sub > 0.99, 4, sym)
        out.append((begin, sym))
    return out


def entries(T, begin, sym):
    """the read's gathered pair entries, per branch -> [B][n] in gather order (pairs of the full quads, tail singles)"""
    span = len(sym)
    cols = np.array(SYM_COL)[sym]
    site = T[:, begin + np.arange(span), cols]                 # [B][span]
    full = span & ~3
    pairs = site[:, 0:full:2] + site[:, 1:full:2]              # a0 + a1, a2 + a3, ...: the pair table's entries
    return np.concatenate([pairs, site[:, full:]], axis=1)


def rule(max_span, M, shift=0):
    n = 2 * (max_span >> 2) + 3
    cq_err = (n + 2) * n * M * 2.0 ** -53
    h = 0.5
    while 0.5 * n * h + cq_err > 1.0:
        h *= 0.5
    h *= 2.0 ** -shift
    return h, 0.5 * n * h + cq_err


def sat_add(a, b):
    return np.clip(a.astype(np.int32) + b.astype(np.int32), FLOOR, 32767).astype(np.int16)


def screen16(E, base, h):
    """E [B][n] -> the kernel's int16 sums [B]: quantise, then (a (+) b) pairs added to the running sum, saturating"""
    q = np.maximum(np.rint((E - base[None, :]) / h), FLOOR).astype(np.int16)
    assert (q <= 0).all()
    B, n = q.shape
    total = np.zeros(B, np.int16)
    i = 0
    while i + 1 < n:
        total = sat_add(total, sat_add(q[:, i], q[:, i + 1]))
        i += 2
    if i < n:
        total = sat_add(total, q[:, i])
    return total


@pytest.mark.parametrize("W", (97, 163))
@pytest.mark.parametrize("shift", (0, 2, 6))
def test_superset_one_sided_bound_and_error(W, shift):
    T, seqs = tables(W)
    B = T.shape[0]
    nseg = (B + 63) // 64
    band_t = max(1.0 - math.log((1.0 - THR) / B), math.log(B) + 38.0)
    M = float(np.abs(T[:, :, SYM_COL]).max()) * 2.0           # pair entries: two sites
    max_span = min(W, 160)
    h, delta = rule(max_span, M, shift)
    assert 0.0 < delta <= 1.0
    band_i = math.ceil((band_t + 2.0 * delta) / h)
    reads = reads_of(W, seqs, 300, 7 * W + shift)
    unscreenable = saturated = 0
    worst = 0.0
    for begin, sym in reads:
        E = entries(T, begin, sym)
        base = E.max(axis=0)
        cq = base.sum()
        exact = E.sum(axis=1)
        s16 = screen16(E, base, h)
        live = s16 > FLOOR
        err = np.abs(cq + h * s16.astype(np.float64) - exact)
        if live.any():
            worst = max(worst, float(err[live].max()))
        assert (err[live] <= delta).all(), "an unsaturated cell is off by more than delta"
        assert (cq + h * s16.astype(np.float64) + delta >= exact).all(), "a cell's upper bound is below its exact sum"
        saturated += int((~live).sum())
        pad = np.full(nseg * 64, FLOOR, np.int32)
        pad[:B] = s16
        seg = pad.reshape(nseg, 64).max(axis=1)
        padx = np.full(nseg * 64, -np.inf)
        padx[:B] = exact
        segx = padx.reshape(nseg, 64).max(axis=1)
        assert (cq + h * seg + delta >= segx).all()
        r = int(seg.max())
        included = seg >= r - band_i
        inband = segx >= segx.max() - band_t
        assert not (inband & ~included).any(), "an in-band segment was excluded"
        if r == FLOOR:
            unscreenable += 1
            assert included.all()
    print("W %d shift %d: h 2^%d, delta %.4g, largest error on unsaturated cells %.4g, %d saturated cells, "
          "%d of %d reads unscreenable" % (W, shift, round(math.log2(h)), delta, worst, saturated, unscreenable, len(reads)))
    if shift == 0:
        assert unscreenable <= len(reads) // 100, "more than 1 % of the reads cannot be screened at the rule's own h"
        assert h == (2.0 ** -6 if W == 163 else 2.0 ** -5)     # n = 83 / 51 gathered entries
    if shift == 6:
        assert saturated > 0, "the shift of 6 was meant to exercise saturation"
