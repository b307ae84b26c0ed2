"""The 16-bit four-branch screen of the chunk body's preplacement ("16-bit screen") against the fp32 screen and
the one-pass preplacement, through the chunk entry points, and its own probe against the exact table.

Pairs, results (as uint64) and last_stats must be array_equal from place_chunk and from the staged path across the options
preplace_screen_i16 = 1 (default) and 0 (the fp32 screen), preplace_screen = 0 (one pass), and preplace_screen_i16_shift = 2
and 6 (a smaller quantum: sums saturate, reads become unscreenable and have every segment included).  preplace_screen_runs
asserts the route taken, the probe that the 16-bit screen's conditions hold for the shape.

Shapes: the references, windows and read sets of test_gpu_preplace_screen.py (67-tip trees, the evaluator fed with the
first B branches) with B at the quad and segment edges -- 3, 4, 5, 63, 64, 65, 67, 129, 131 -- at W = 97 and 163; every span
edge at both start parities and both alignment ends; Q = 1, 2, 1023, 1025, 5000; a flat reference whose every segment is
included; reads with a rare ambiguity code or an inner gap.

Probe (preplace_screen16_probe) against preplace_bounded's table, at shifts 0, 2 and 6: every segment whose exact maximum
is within band_t of the exact row maximum is in the mask; cq + h seg16 + delta >= the exact segment maximum for every
segment, and |cq + h seg16 - exact| <= delta where seg16 is above the floor (the cell that attains
it never saturated); the included count is the masks' popcount; the unscreenable count is the number of rows at the
floor, whose masks are full.  The bounds are the ones derived in DESIGN 4.3: h / 2 per gathered entry plus the fp64
rounding of C_q.
"""
import numpy as np
import pytest

import epa_ng_amd as epa
import test_gpu_preplace_screen as scr
from test_gpu_preplace_screen import THR, base, cluster_windows, edge_windows, evaluator, exact_segments, reads_at

pytestmark = pytest.mark.gpu

FLOOR = -32768
ALL_B = (3, 4, 5, 63, 64, 65, 67, 129, 131)
WIDTHS = (97, 163)
# (preplace_screen, preplace_screen_i16, preplace_screen_i16_shift) -> does the chunk body take the two-pass route
SETTINGS = (((2, 1, 0), 1), ((2, 0, 0), 1), ((0, 1, 0), 0), ((2, 1, 2), 1), ((2, 1, 6), 1))


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for e in scr._EVS.values():
        e.close()
    scr._EVS.clear()


def set_options(ev, screen, i16, shift):
    ev.set_option("preplace_screen", screen)
    ev.set_option("preplace_screen_i16", i16)
    ev.set_option("preplace_screen_i16_shift", shift)


def all_ways(ev, enc, max_span, staged):
    """the chunk body under every setting -> the common (pairs, results)"""
    Q = len(enc[1])
    got = []
    try:
        assert ev.preplace_screen16_probe(*enc, max_span=max_span, threshold=THR)["ran"], "the 16-bit screen's conditions do not hold"
        for (screen, i16, shift), two_pass in SETTINGS:
            set_options(ev, screen, i16, shift)
            n0 = ev.preplace_screen_runs()
            if staged:
                ev.chunk_stage(0, *enc)
                ev.chunk_launch(0, threshold=THR, max_span=max_span, max_pairs=Q * ev.B)
                pairs, res = ev.chunk_finish(0)
            else:
                pairs, res = ev.place_chunk(*enc, threshold=THR, max_span=max_span, max_pairs=Q * ev.B)
            assert ev.preplace_screen_runs() - n0 == two_pass, "settings %r: the preplacement took the other route" % ((screen, i16, shift),)
            got.append((pairs, res, dict(ev.last_stats)))
    finally:
        set_options(ev, 1, 1, 0)
    p0, r0, s0 = got[0]
    assert len(p0) > 0
    for (p, r, s), (setting, _) in zip(got[1:], SETTINGS[1:]):
        assert np.array_equal(p, p0), setting
        assert np.array_equal(r.view(np.uint64), r0.view(np.uint64)), setting
        assert s == s0, setting
    return p0, r0


@pytest.mark.parametrize("B", ALL_B)
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("staged", (False, True))
def test_window_shapes_at_quad_and_segment_edges(W, B, staged):
    ev = evaluator(W, B)
    enc = epa.encode_queries(4, reads_at(W, edge_windows(W) * 3, 13 * W + B, base(W)["seqs"]))
    all_ways(ev, enc, min(W, 160), staged)


@pytest.mark.parametrize("W,B", [(97, 131), (163, 131), (97, 65)])
@pytest.mark.parametrize("Q", (1, 2, 1023, 1025, 5000))
def test_query_counts_and_grouping(W, B, Q):
    ev = evaluator(W, B)
    enc = epa.encode_queries(4, reads_at(W, cluster_windows(W, Q, 5 * Q + W), 3 * Q + B, base(W)["seqs"]))
    all_ways(ev, enc, min(W, 160), staged=Q == 1025)


def test_flat_reference_includes_every_segment():
    W, B = 97, 131
    ev = evaluator(W, B, flat=True)
    enc = epa.encode_queries(4, reads_at(W, cluster_windows(W, 1500, 77), 78, base(W, True)["seqs"], sub=0.0))
    probe = ev.preplace_screen16_probe(*enc, max_span=W, threshold=THR)
    assert probe["ran"] and probe["unscreenable"] == 0
    assert (probe["mask"] == np.uint64((1 << ((B + 63) // 64)) - 1)).all(), "the reference is not flat within the band"
    all_ways(ev, enc, W, staged=False)


def test_rare_codes_and_inner_gaps_among_the_reads():
    W, B = 97, 129
    ev = evaluator(W, B)
    reads = reads_at(W, cluster_windows(W, 1600, 31), 32, base(W)["seqs"])
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
    all_ways(ev, enc, W, staged=False)
    all_ways(ev, enc, W, staged=True)


@pytest.mark.parametrize("W,B", [(97, 131), (163, 131), (97, 65), (163, 5)])
def test_probe_superset_bounds_and_counts(W, B):
    ev = evaluator(W, B)
    wins = edge_windows(W) + cluster_windows(W, 1500, 41)
    enc = epa.encode_queries(4, reads_at(W, wins, 42, base(W)["seqs"]))
    ms = min(W, 160)
    segmax = exact_segments(ev, enc, ms)
    nseg = segmax.shape[1]
    full = np.uint64((1 << nseg) - 1)
    h0 = 2.0 ** -6 if W == 163 else 2.0 ** -5          # n = 83 / 51 gathered entries: the largest h with n h / 2 <= 1
    try:
        for shift in (0, 2, 6):
            ev.set_option("preplace_screen_i16_shift", shift)
            probe = ev.preplace_screen16_probe(*enc, max_span=ms, threshold=THR)
            assert probe["ran"] and 0.0 < probe["delta"] <= 1.0
            h, delta, seg16 = probe["h"], probe["delta"], probe["seg16"]
            assert h == h0 * 2.0 ** -shift
            assert (seg16 >= FLOOR).all() and (seg16 <= 0).all()
            upper = probe["cq"][:, None] + h * seg16 + delta
            live = seg16 > FLOOR
            err = np.abs(probe["cq"][:, None] + h * seg16 - segmax)
            floor_rows = ~live.any(axis=1)
            print("W %d B %d shift %d: h %g, delta %.3g, max error above the floor %.3g, %d segments at the floor, %d unscreenable "
                  "reads, %d cells included" % (W, B, shift, h, delta, err[live].max() if live.any() else 0.0, int((~live).sum()),
                                                probe["unscreenable"], probe["included"]))
            assert (upper >= segmax).all()
            assert (err[live] <= delta).all()
            inband = segmax >= (segmax.max(axis=1) - probe["band_t"])[:, None]
            mask = ((probe["mask"][:, None] >> np.arange(nseg, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
            assert not (inband & ~mask).any()
            assert probe["included"] == int(mask.sum())
            assert probe["unscreenable"] == int(floor_rows.sum())
            assert (probe["mask"][floor_rows] == full).all()
            if shift == 0:
                assert probe["unscreenable"] <= len(wins) // 100
            if shift == 6 and B > 64:
                assert (~live).any() and probe["unscreenable"] >= 1, "the shift of 6 was meant to saturate"
    finally:
        ev.set_option("preplace_screen_i16_shift", 0)
