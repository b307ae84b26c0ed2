"""The chunk body's two-pass preplacement (fp32 two-branch screen -> band test -> exact pass over the included
(query, segment) cells) against the one-pass preplacement, through the chunk entry points.

`preplace_screen=2` (the screen without its lower size condition: by default only chunks of 8e7 reads x branches and more
take it, which no quick test reaches -- test_small_chunks_stay_on_one_pass_by_default) and `=0` must give array_equal pairs and results and equal statistics from place_chunk and from
the staged chunk_stage / chunk_launch / chunk_finish path (the per-query counts and the span-class histogram are
functions of the pair list and the spans, so equal pairs carry them -- the histogram k_select_seg itself sums has no
accessor and is NOT observed here; it sizes the Newton launches per span class, whose results are compared); every
comparison also asserts, through
preplace_screen_runs, that the first run took the two-pass route and the second did not.

References: one 67-tip tree per alignment width, the evaluator fed with the oracle's sides of the FIRST B branches, so
that B = 5, 9 (odd: padded partner), 63, 64, 65, 67, 125, 128, 129, 131 (last pair alone in a new segment) all exist.
Widths 97 and 131 (odd), and 163 for the spans 157 .. 160.  Spans 1, 2, 3, 4, 5, 7, 8 and the longest four that fit,
at both start parities and both alignment ends; Q = 1, 2, 1023, 1025 (wide slices) and 5000 reads in two far clusters
(narrow slices at W = 97 and 163: empty groups, groups cut at 1024 and at the 96-site grid); a flat reference whose
every segment is included; reads with a rare ambiguity code or an inner gap among the others.

Superset property, from the probe of the screen and the table of the one-pass path (preplace_bounded): every segment
whose exact maximum is within band_t of the exact row maximum is in the included mask, and |seg32 - exact segment
maximum| <= delta, for every (query, segment).
"""
import functools

import numpy as np
import pytest

import epa_ng_amd as epa
from epa_ng_amd import synth
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

THR = 0.99999
ALL_B = (5, 9, 63, 64, 65, 67, 125, 128, 129, 131)
CASES = [(97, b) for b in ALL_B] + [(w, b) for w in (131, 163) for b in (9, 67, 131)]


@functools.lru_cache(maxsize=None)
def base(W, flat=False):
    """-> (oracle-side inputs of a 67-tip reference of width W, its alignment rows)"""
    root = synth.random_tree(67, 900 + W, mean_bl=2e-4, lo=1e-5, hi=1e-3) if flat else synth.random_tree(67, 900 + W)
    rates = synth.gamma_rates(synth.CFG2_ALPHA)
    labels, seqs = synth.simulate_msa(root, W, synth.CFG2_SUBST, synth.CFG2_FREQS, rates, 901 + W)
    o = Oracle(synth.newick(root), labels, seqs, 4, synth.CFG2_SUBST, synth.CFG2_FREQS, rates)
    sides = [o.branch_sides(b) for b in range(o.B)]
    bl = [o.branch_info(b)[0] for b in range(o.B)]
    return {"eigen": o.eigen(), "rates": rates, "sides": sides, "bl": bl, "seqs": seqs, "B": o.B}


_EVS = {}


def evaluator(W, B, flat=False, poison=False):
    key = (W, B, flat, poison)
    if key not in _EVS:
        g = base(W, flat)
        assert B <= g["B"]
        ev, u, ui = g["eigen"]
        pc = [np.array(s[0], copy=True) for s in g["sides"][:B]]
        if poison:                      # site 0 of branch 0 has likelihood 0: log -> -inf in the lookup tables
            pc[0][0] = 0.0
        _EVS[key] = epa.Evaluator(4, g["rates"], np.full(len(g["rates"]), 1.0 / len(g["rates"])), ev, u, ui,
                                  synth.CFG2_FREQS, g["bl"][:B], pc, [s[2] for s in g["sides"][:B]],
                                  [s[1] for s in g["sides"][:B]], [s[3] for s in g["sides"][:B]])
    return _EVS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for e in _EVS.values():
        e.close()
    _EVS.clear()


def reads_at(W, windows, seed, seqs, sub=0.05):
    """one read per (begin, span): the window of a reference row with a few substitutions, gaps outside"""
    rng = np.random.default_rng(seed)
    out = []
    for begin, span in windows:
        row = list(seqs[int(rng.integers(len(seqs)))][begin:begin + span])
        for i in range(span):
            if rng.random() < sub:
                row[i] = "ACGT"[int(rng.integers(4))]
        out.append("-" * begin + "".join(row) + "-" * (W - begin - span))
    return out


def spans_of(W):
    cap = min(W, 160)
    return [1, 2, 3, 4, 5, 7, 8] + list(range(cap - 3, cap + 1))


def edge_windows(W):
    """every span of spans_of at both start parities and at both ends of the alignment"""
    out = []
    for span in spans_of(W):
        for begin in (0, 1, W - span - 1, W - span):
            if 0 <= begin and begin + span <= W:
                out.append((begin, span))
    return out


def cluster_windows(W, n, seed):
    """n windows with starts in two far clusters (the 96-site buckets between them stay empty at W = 163)"""
    rng = np.random.default_rng(seed)
    cap = min(W, 160)
    out = []
    for i in range(n):
        span = int(rng.integers(max(1, cap // 2), cap + 1)) if i % 7 else int(rng.integers(1, 9))
        lo = int(rng.integers(0, 4)) if i % 2 else max(0, W - span - int(rng.integers(0, 4)))
        out.append((min(lo, W - span), span))
    return out


def both_ways(ev, enc, max_span, staged):
    """the chunk body with the screen on and off -> the common (pairs, results); asserts the routes taken (short
    windows have flat rows: the pair capacity is every branch of every read)"""
    got = []
    Q = len(enc[1])
    for on in (2, 0):
        ev.set_option("preplace_screen", on)
        n0 = ev.preplace_screen_runs()
        if staged:
            ev.chunk_stage(0, *enc)
            ev.chunk_launch(0, threshold=THR, max_span=max_span, max_pairs=Q * ev.B)
            pairs, res = ev.chunk_finish(0)
        else:
            pairs, res = ev.place_chunk(*enc, threshold=THR, max_span=max_span, max_pairs=Q * ev.B)
        assert ev.preplace_screen_runs() - n0 == (1 if on else 0), "screen %d: the preplacement took the other route" % on
        got.append((pairs, res, dict(ev.last_stats)))
    ev.set_option("preplace_screen", 1)
    (p1, r1, s1), (p0, r0, s0) = got
    assert len(p0) > 0
    assert np.array_equal(p1, p0)
    assert np.array_equal(r1.view(np.uint64), r0.view(np.uint64))
    assert s1 == s0
    return p1, r1


@pytest.mark.parametrize("W,B", CASES)
@pytest.mark.parametrize("staged", (False, True))
def test_window_shapes_at_segment_and_pair_edges(W, B, staged):
    ev = evaluator(W, B)
    g = base(W)
    enc = epa.encode_queries(4, reads_at(W, edge_windows(W) * 3, 11 * W + B, g["seqs"]))
    both_ways(ev, enc, min(W, 160), staged)


@pytest.mark.parametrize("W,B", [(97, 131), (163, 131), (97, 65)])
@pytest.mark.parametrize("Q", (1, 2, 1023, 1025, 5000))
def test_query_counts_and_grouping(W, B, Q):
    ev = evaluator(W, B)
    g = base(W)
    enc = epa.encode_queries(4, reads_at(W, cluster_windows(W, Q, 5 * Q + W), 3 * Q + B, g["seqs"]))
    both_ways(ev, enc, min(W, 160), staged=Q == 1025)


def test_flat_reference_includes_every_segment():
    W, B = 97, 131
    ev = evaluator(W, B, flat=True)
    g = base(W, True)
    enc = epa.encode_queries(4, reads_at(W, cluster_windows(W, 1500, 77), 78, g["seqs"], sub=0.0))
    probe = ev.preplace_screen_probe(*enc, max_span=W, threshold=THR)
    assert probe["ran"]
    assert (probe["mask"] == np.uint64((1 << ((B + 63) // 64)) - 1)).all(), "the reference is not flat within the band"
    both_ways(ev, enc, W, staged=False)


def test_rare_codes_and_inner_gaps_among_the_reads():
    W, B = 97, 129
    ev = evaluator(W, B)
    g = base(W)
    reads = reads_at(W, cluster_windows(W, 1600, 31), 32, g["seqs"])
    for i in range(0, len(reads), 9):            # a rare ambiguity code: the generic kernel's queries
        r = reads[i]
        k = len(r) - len(r.lstrip("-"))
        reads[i] = r[:k] + "R" + r[k + 1:]
    n_gap = 0
    for i in range(4, len(reads), 9):            # an inner gap: stays on the pair path
        r = reads[i]
        k, e = len(r) - len(r.lstrip("-")), len(r.rstrip("-"))
        if e - k >= 3:
            reads[i] = r[:k + 1] + "-" + r[k + 2:]
            n_gap += 1
    assert n_gap > 50
    enc = epa.encode_queries(4, reads)
    both_ways(ev, enc, W, staged=False)
    both_ways(ev, enc, W, staged=True)


def exact_segments(ev, enc, max_span):
    lnl = ev.preplace_bounded(*enc, max_span=max_span)
    Q, B = lnl.shape
    nseg = (B + 63) // 64
    pad = np.full((Q, nseg * 64), -np.inf)
    pad[:, :B] = lnl
    return pad.reshape(Q, nseg, 64).max(axis=2)


@pytest.mark.parametrize("W,B", [(97, 131), (163, 131), (97, 65), (97, 9)])
def test_included_mask_is_a_superset_and_seg32_within_delta(W, B):
    ev = evaluator(W, B)
    g = base(W)
    wins = edge_windows(W) + cluster_windows(W, 1500, 41)
    enc = epa.encode_queries(4, reads_at(W, wins, 42, g["seqs"]))
    ms = min(W, 160)
    segmax = exact_segments(ev, enc, ms)
    probe = ev.preplace_screen_probe(*enc, max_span=ms, threshold=THR)
    assert probe["ran"] and 0.0 < probe["delta"] <= 1.0
    nseg = segmax.shape[1]
    assert not np.isnan(probe["seg32"]).any()
    err = np.abs(probe["seg32"].astype(np.float64) - segmax)
    print("W %d B %d: max |seg32 - exact| %.3g, delta %.3g, M %.4g" % (W, B, err.max(), probe["delta"], probe["M"]))
    assert (err <= probe["delta"]).all()
    inband = segmax >= (segmax.max(axis=1) - probe["band_t"])[:, None]
    mask = ((probe["mask"][:, None] >> np.arange(nseg, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    assert not (inband & ~mask).any()
    assert probe["included"] == int(mask.sum())


def test_a_64_times_wider_delta_changes_nothing():
    W, B = 97, 131
    ev = evaluator(W, B)
    g = base(W)
    rng = np.random.default_rng(5)
    wins = [(int(rng.integers(0, W - 8)), int(rng.integers(1, 9))) for _ in range(1500)]
    enc = epa.encode_queries(4, reads_at(W, wins, 6, g["seqs"]))
    d1 = ev.preplace_screen_probe(*enc, max_span=8, threshold=THR, arrays=False)
    ev.set_option("preplace_screen_scale", 64)
    try:
        d64 = ev.preplace_screen_probe(*enc, max_span=8, threshold=THR, arrays=False)
        assert d1["ran"] and d64["ran"] and d64["delta"] == 64 * d1["delta"]
        assert d64["included"] >= d1["included"]
        both_ways(ev, enc, 8, staged=False)
    finally:
        ev.set_option("preplace_screen_scale", 1)


def refused(ev, enc, max_span):
    """the context reports the screen off and the chunk body runs (and equals) the one-pass preplacement"""
    assert not ev.preplace_screen_probe(*enc, max_span=max_span, threshold=THR, arrays=False)["ran"]
    got = []
    for on in (2, 0):
        ev.set_option("preplace_screen", on)
        n0 = ev.preplace_screen_runs()
        got.append(ev.place_chunk(*enc, threshold=THR, max_span=max_span, max_pairs=len(enc[1]) * ev.B))
        assert ev.preplace_screen_runs() == n0
    ev.set_option("preplace_screen", 1)
    assert len(got[0][0]) > 0 and np.array_equal(got[0][0], got[1][0])
    assert np.array_equal(got[0][1].view(np.uint64), got[1][1].view(np.uint64))


def test_refusal_when_delta_exceeds_one():
    W, B = 97, 131
    ev = evaluator(W, B)
    g = base(W)
    enc = epa.encode_queries(4, reads_at(W, cluster_windows(W, 300, 51), 52, g["seqs"]))
    ev.set_option("preplace_screen_scale", 1 << 24)
    try:
        refused(ev, enc, W)
    finally:
        ev.set_option("preplace_screen_scale", 1)
    assert ev.preplace_screen_probe(*enc, max_span=W, threshold=THR, arrays=False)["ran"]


def test_refusal_when_the_table_holds_a_non_finite_entry():
    W, B = 97, 67
    ev = evaluator(W, B, poison=True)
    g = base(W)
    wins = [(b, s) for b, s in cluster_windows(W, 300, 61)]
    wins = [(max(b, 2), min(s, W - max(b, 2))) for b, s in wins]     # the reads stay off the poisoned site
    enc = epa.encode_queries(4, reads_at(W, wins, 62, g["seqs"]))
    info = ev.preplace_screen_probe(*enc, max_span=W, threshold=THR, arrays=False)
    assert info["nonfinite"] > 0
    refused(ev, enc, W)


def test_small_chunks_stay_on_one_pass_by_default():
    W, B = 97, 131
    ev = evaluator(W, B)
    g = base(W)
    enc = epa.encode_queries(4, reads_at(W, cluster_windows(W, 1500, 71), 72, g["seqs"]))
    ev.set_option("preplace_screen", 1)
    n0 = ev.preplace_screen_runs()
    ev.place_chunk(*enc, threshold=THR, max_span=W, max_pairs=len(enc[1]) * B)
    assert ev.preplace_screen_runs() == n0      # 1500 x 131 cells: far below the size at which two passes pay
