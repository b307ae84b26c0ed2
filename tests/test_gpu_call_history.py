"""A context's answers must not depend on the calls it served before.

The CLI's chunk loop, the slot pipeline and --rescore keep ONE epa_ctx alive for millions of reads, and that context
carries state from call to call: scratch banks that only grow and keep their old contents, the "already cleared" marks of
the statistics block and the work counters, the staging width of the sorted selection, table pitch / segment maxima /
window-status pointers, query layout and packing, heuristic and options, the block buffers of the blocked lookup layout,
the slots' and groups' bookkeeping.  Every other test builds a context, makes a call or two and drops it.

Here a PROBE (history_util.probe: preplace, place_chunk, thorough on an explicit list, select, place_all, score_at on
fixed reads that cover every span class in one call) runs on a new context after some HISTORY of other calls, and every
output -- table, pair lists, lnL, both lengths, counts, LWR, the Newton counters -- must equal BIT FOR BIT what a context
that has done nothing else returns.  include/epa_dev.h promises that options, XCD shares and group launches do not change
results, so no tolerance applies anywhere.

H8 pins a defect found by reading the code: the span-class histogram that the candidate selection hands to the Newton
launch of its chunk body used to live in the context, keyed by nothing but the pair count, and a chunk body that ended in
a window error left it behind; a later epa_dev_thorough with as many pairs was then partitioned by that other call's
histogram (windows of 100 .. 160 sites on the 64-site instantiation: EPA_OK and a likelihood over part of the window).
The histogram now travels in SelectPending and cannot outlive its chunk body."""
import numpy as np
import pytest

import epa_ng_amd as epa
import history_util as hu

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_QUERY_WIDTH, ERR_QUERY_ALL_GAP, ERR_PAIR_OVERFLOW = -1, -4, -5, -9


def check_probe(ev, name, what, form="full", options=()):
    """the probe on `ev` equals the probe of a context without history"""
    got = hu.probe(ev, *hu.inputs(name)["probe"][form])
    hu.assert_same(got, hu.fresh_probe(name, "full", options), "%s %s (%s rows)" % (name, what, form))
    return got


def everyday_calls(ev, name, which="mixed", form="full", **kw):
    """place_chunk, preplace and thorough on input `which`"""
    codes, wb, ws = hu.inputs(name)[which][form]
    ev.place_chunk(codes, wb, ws, max_pairs=len(wb) * ev.B, **kw)
    ev.preplace(codes, wb, ws)
    ev.thorough(hu.grid_pairs(ev.B, len(wb)), codes, wb, ws)


def raises(code, fn, *a, **kw):
    with pytest.raises(epa.EpaError) as ei:
        fn(*a, **kw)
    assert ei.value.code == code, ei.value


@pytest.mark.parametrize("name", ["R4", "R4B", "R20"])
def test_h1_grow_then_shrink(name):
    """a 600-read chunk grows every scratch buffer and leaves it full of other reads' rows, keys and counters; a 3-read
    call follows; then the probe: a kernel that reads one row, lane or counter past what its own call wrote would see
    the big chunk's data instead of zeros"""
    ev = hu.new_context(name)
    everyday_calls(ev, name, "big")
    everyday_calls(ev, name, "small")
    check_probe(ev, name, "after a 600-read and a 3-read call")


def test_h2_shrink_then_grow():
    """the 3-read call first: every buffer of the probe is reallocated"""
    ev = hu.new_context("R4")
    everyday_calls(ev, "R4", "small")
    check_probe(ev, "R4", "after a 3-read call")


def test_h3_query_layouts():
    """aligned rows, compact rows and 4-bit packed rows in turn through preplace / thorough / place_chunk (the context
    keeps the layout and the packing of the last call), then the probe in each form: all equal, and equal to a fresh one's"""
    name = "R4"
    ev = hu.new_context(name)
    mixed, small = hu.inputs(name)["mixed"], hu.inputs(name)["small"]
    B = ev.B
    ev.preplace(*mixed["full"])
    ev.thorough(hu.grid_pairs(B, 40), *mixed["compact"])
    ev.place_chunk(*mixed["packed"], max_pairs=40 * B)
    ev.preplace(*small["packed"])
    ev.thorough(hu.grid_pairs(B, 3), *small["full"])
    ev.place_chunk(*small["compact"], max_pairs=3 * B)
    ev.thorough(hu.grid_pairs(B, 40), *mixed["packed"])
    got = {form: check_probe(ev, name, "after calls in all three query forms", form)
           for form in ("packed", "full", "compact", "packed")}
    hu.assert_same(got["full"], got["compact"], "full against compact rows")
    hu.assert_same(got["full"], got["packed"], "full against packed rows")
    for form in ("compact", "packed"):      # the expected answers do not depend on the form either
        hu.assert_same(hu.fresh_probe(name, form), hu.fresh_probe(name, "full"), "fresh contexts, %s rows" % form)


def test_h4_heuristics():
    """fixed and baseball rule (no segment maxima, select_cap raised to the rule's limit), back to the dynamic rule"""
    name = "R4"
    ev = hu.new_context(name)
    codes, wb, ws = hu.inputs(name)["mixed"]["full"]
    ev.set_heuristic("fixed", 0.9)
    p, _ = ev.place_chunk(codes, wb, ws, max_pairs=len(wb) * ev.B)
    assert len(p) == len(wb) * int(np.ceil(0.9 * ev.B))
    ev.set_heuristic("baseball")
    ev.place_chunk(codes, wb, ws, max_pairs=len(wb) * ev.B)
    ev.set_heuristic("dynamic")
    check_probe(ev, name, "after the fixed and the baseball rule")


SAME_BITS = ("select_sort", "select_full_rows", "queued_thorough")      # the probe while set equals the default's
OPTIONS = [("R4", o) for o in ("thorough_generic", "preplace_generic", "select_full_rows", "select_sort",
                               "queued_thorough", "newton_lds", "timers")] + \
          [("R20", o) for o in ("thorough_generic", "preplace_generic", "select_full_rows", "select_sort",
                                "queued_thorough", "newton_lds", "timers", "aa_valu")]


@pytest.mark.parametrize("name,option", OPTIONS, ids=["%s-%s" % o for o in OPTIONS])
def test_h5_option_on_and_off_again(name, option):
    """an option set, used (a mixed chunk; a chunk of one span class with its bound given, which is what lets the queued
    Newton launch run; thorough) and restored leaves nothing behind; the options that only reroute the selection or the
    launch order return the default's bits while set"""
    ev = hu.new_context(name)
    on, off = (0, 1) if option == "timers" else (1, 0)
    ev.set_option(option, on)
    everyday_calls(ev, name, "mixed")
    everyday_calls(ev, name, "short", max_span=64)
    if option in SAME_BITS:
        check_probe(ev, name, "while %s is set" % option)
    ev.set_option(option, off)
    check_probe(ev, name, "after %s was set and restored" % option)


def test_h6_widened_selection_staging():
    """sorted selection: reads of 1 .. 3 sites at threshold 0.9999999 select more than the 64 staging slots of a query
    (a site's likelihood differs by far less than 1e7 between branches, so nearly all 77 branches are needed to reach the
    threshold), the selection widens select_cap and runs again; the width never narrows.  The probe under select_sort
    then equals a fresh context's under select_sort and the default one, and the default path is untouched"""
    name = "R4"
    ev = hu.new_context(name)
    ev.set_option("select_sort", 1)
    codes, wb, ws = hu.inputs(name)["tiny"]["full"]
    pairs, _ = ev.place_chunk(codes, wb, ws, threshold=0.9999999, max_pairs=len(wb) * ev.B)
    assert np.bincount(pairs["seq_id"]).max() > 64, "precondition: no query overflowed the 64 staging slots"
    check_probe(ev, name, "under select_sort after a widened selection", options=(("select_sort", 1),))
    hu.assert_same(hu.fresh_probe(name, "full", (("select_sort", 1),)), hu.fresh_probe(name), "fresh: select_sort against default")
    ev.set_option("select_sort", 0)
    check_probe(ev, name, "after select_sort with a widened selection")


@pytest.mark.parametrize("name", ["R4", "R4B", "R20"])
def test_h7_recoverable_errors(name):
    """refused inputs (no GPU fault is involved) must leave the context as it was: the probe after each, and after all"""
    ev = hu.new_context(name)
    codes, wb, ws = hu.inputs(name)["mixed"]["full"]
    Q, B = len(wb), ev.B
    ws_gap = ws.copy()
    ws_gap[7] = 0
    raises(ERR_PAIR_OVERFLOW, ev.place_chunk, codes, wb, ws, max_pairs=1)
    ev.place_chunk(codes, wb, ws, max_pairs=Q * B)                           # the same call with room
    check_probe(ev, name, "after a candidate overflow")
    raises(ERR_QUERY_ALL_GAP, ev.place_chunk, codes, wb, ws_gap, max_pairs=Q * B)
    check_probe(ev, name, "after an all-gap window in place_chunk")
    raises(ERR_QUERY_ALL_GAP, ev.preplace, codes, wb, ws_gap)
    check_probe(ev, name, "after an all-gap window in preplace")
    bad = hu.grid_pairs(B, Q)
    bad["branch_id"][5] = B
    raises(ERR_INVALID_ARG, ev.thorough, bad, codes, wb, ws)
    check_probe(ev, name, "after a branch id out of range")
    # a window longer than the caller's max_span: the single-call preplacement refuses it on the host (INVALID_ARG), the
    # fused chunk body finds it on the device with the other window checks and reports it as they are reported
    # (EPA_ERR_QUERY_WIDTH, as test_wrong_max_span_is_rejected pins)
    assert int(ws.max()) > 100
    raises(ERR_INVALID_ARG, ev.preplace_bounded, codes, wb, ws, 100)
    raises(ERR_QUERY_WIDTH, ev.place_chunk, codes, wb, ws, max_span=100, max_pairs=Q * B)
    check_probe(ev, name, "after a window longer than max_span")
    raises(ERR_PAIR_OVERFLOW, ev.place_chunk, codes, wb, ws, max_pairs=1)
    raises(ERR_QUERY_ALL_GAP, ev.place_chunk, codes, wb, ws_gap, max_pairs=Q * B)
    raises(ERR_QUERY_WIDTH, ev.place_chunk, codes, wb, ws, max_span=100, max_pairs=Q * B)
    raises(ERR_INVALID_ARG, ev.thorough, bad, codes, wb, ws)
    check_probe(ev, name, "after all the errors in a row")


@pytest.mark.parametrize("through_slot", [False, True], ids=["place_chunk", "slot"])
@pytest.mark.parametrize("n_pairs", [80, 72])
def test_h8_histogram_of_a_failed_chunk_is_not_reused(n_pairs, through_slot):
    """fixed rule, k = ceil(0.1 * 77) = 8 candidates per read: a chunk of 10 reads of at most 64 sites, one with an empty
    window, selects 10 k or 9 k pairs (whether the empty row selects is not specified) -- all of span class 0 -- and fails
    with EPA_ERR_QUERY_ALL_GAP after the selection ran.  A thorough call with exactly that many pairs over OTHER reads,
    of 100 .. 160 sites (classes 1 and 11), must then return what a fresh context returns"""
    name = "R4"
    ev = hu.new_context(name)
    assert int(np.ceil(0.1 * ev.B)) == 8
    ev.set_heuristic("fixed", 0.1)
    codes, wb, ws = hu.inputs(name)["ten"]["full"]
    ws_gap = ws.copy()
    ws_gap[4] = 0
    if through_slot:
        ev.chunk_stage(0, codes, wb, ws_gap)
        raises(ERR_QUERY_ALL_GAP, ev.chunk_launch, 0, max_pairs=10 * ev.B)
    else:
        raises(ERR_QUERY_ALL_GAP, ev.place_chunk, codes, wb, ws_gap, max_pairs=10 * ev.B)
    mid = hu.inputs(name)["mid"]["full"]
    assert 100 <= int(mid[2].min()) and int(mid[2].max()) <= 160
    pairs = hu.grid_pairs(ev.B, len(mid[1]), step=1, seed=11)[:n_pairs]
    got = hu.thorough_rows(ev, pairs, *mid)
    hu.assert_same(got, hu.fresh_thorough(name, "mid", pairs, tag="h8-%d" % n_pairs),
                   "thorough on %d pairs after a chunk that failed on a window error" % n_pairs)
    if through_slot:        # the slot stayed staged: with the window mended it launches, and gives the direct call's rows
        ev.chunk_stage(0, codes, wb, ws)
        ev.chunk_launch(0, max_pairs=10 * ev.B)
        p, r = ev.chunk_finish(0)
        ref = hu.new_context(name)
        ref.set_heuristic("fixed", 0.1)
        ep, er = ref.place_chunk(codes, wb, ws, max_pairs=10 * ev.B)
        hu.assert_same(hu.chunk_rows(p, r), hu.chunk_rows(ep, er), "the slot's relaunch")


@pytest.mark.parametrize("swapped", [False, True], ids=["probe-on-0", "probe-on-1"])
def test_h9_slots_interleaved_with_direct_calls(swapped):
    """two slots begun (their own streams and scratch banks), direct preplace and thorough on bank 0 in between, then
    both ended and finished: the probe chunk's slot returns the rows of a fresh place_chunk, the direct calls what a fresh
    context returns.  Second case: roles swapped, the other chunk ten times larger instead of ten times smaller"""
    name = "R4"
    ev = hu.new_context(name)
    inp = hu.inputs(name)
    mine, other = (1, 0) if swapped else (0, 1)
    other_in = hu.head(inp["big"]["compact"], 480) if swapped else hu.head(inp["ten"]["compact"], 5)
    B = ev.B
    ev.chunk_stage(mine, *inp["probe"]["compact"])
    ev.chunk_stage(other, *other_in)
    ev.chunk_launch_begin(mine, max_pairs=48 * B)
    ev.chunk_launch_begin(other, max_pairs=len(other_in[1]) * B)
    codes, wb, ws = inp["mixed"]["full"]
    direct = {"preplace": ev.preplace(codes, wb, ws)}
    direct.update(hu.thorough_rows(ev, hu.grid_pairs(B, len(wb)), codes, wb, ws))
    ev.chunk_launch_end(mine)
    ev.chunk_launch_end(other)
    got_other = ev.chunk_finish(other)
    p, r = ev.chunk_finish(mine)
    got = hu.chunk_rows(p, r, ev)
    hu.assert_same(got, hu.fresh_chunk(name, "probe"), "slot %d" % mine)
    expect = dict(hu.fresh_preplace(name, "mixed"))
    expect.update(hu.fresh_thorough(name, "mixed", hu.grid_pairs(B, len(wb))))
    hu.assert_same(direct, expect, "direct calls between launch_begin and launch_end")
    fresh = hu.new_context(name)
    ep, er = fresh.place_chunk(*other_in, max_pairs=len(other_in[1]) * B)
    hu.assert_same(hu.chunk_rows(*got_other), hu.chunk_rows(ep, er), "slot %d" % other)
    check_probe(ev, name, "after two slots and direct calls in between")


def test_h10_group_launch_then_single_launches():
    """a group launch over slots {2, 3, 4} (leader 2), all finished; then ordinary launches of the probe chunk on slot 3
    (a former member) and slot 2 (the former leader, whose own_* / merged-chunk pointers were restored)"""
    name = "R4"
    ev = hu.new_context(name)
    inp = hu.inputs(name)
    B = ev.B
    members = {2: "small", 3: "probe", 4: "mixed"}
    for slot, which in members.items():
        ev.chunk_stage(slot, *inp[which]["full"])
    ev.chunk_launch_many([2, 3, 4], max_pairs=(3 + 48 + 40) * B)
    for slot in (4, 2, 3):
        p, r = ev.chunk_finish(slot)
        expect = {k: v for k, v in hu.fresh_chunk(name, members[slot]).items() if not k.endswith("counters")}
        hu.assert_same(hu.chunk_rows(p, r), expect, "member slot %d of the group" % slot)
    for slot in (3, 2):
        ev.chunk_stage(slot, *inp["probe"]["full"])
        ev.chunk_launch(slot, max_pairs=48 * B)
        p, r = ev.chunk_finish(slot)
        hu.assert_same(hu.chunk_rows(p, r, ev), hu.fresh_chunk(name, "probe"), "single launch on slot %d after the group" % slot)
    check_probe(ev, name, "after a group launch and single launches")


def test_h11_other_entry_points_in_between():
    """score_at, site_lnl and rell_support (scratch slots 3 and 13 .. 17 of bank 0, their own staging of pairs and
    queries) over a 300-entry list between two probes"""
    name = "R4"
    ev = hu.new_context(name)
    first = check_probe(ev, name, "first probe")
    codes, wb, ws = hu.inputs(name)["probe"]["full"]
    pairs = hu.grid_pairs(ev.B, len(wb))[:300]
    pend, dist = first["thorough.pendant_length"][:300], first["thorough.distal_length"][:300]
    lnl = ev.score_at(pairs, pend, dist, codes, wb, ws)
    rows = ev.site_lnl(pairs, pend, dist, codes, wb, ws)
    sup = ev.rell_support(pairs, pend, dist, codes, wb, ws, replicates=200)
    assert np.all(np.isfinite(lnl)) and rows.shape == (300, 256) and np.all((sup >= 0) & (sup <= 1))
    second = check_probe(ev, name, "after score_at, site_lnl and rell_support")
    hu.assert_same(second, first, "second probe against the first")


def test_h12_repetition():
    """the probe five times on one context; launches this small teach the XCD balance nothing"""
    name = "R4"
    ev = hu.new_context(name)
    got = [check_probe(ev, name, "repetition %d" % i) for i in range(5)]
    for i in range(1, 5):
        hu.assert_same(got[i], got[0], "repetition %d against the first" % i)
    if ev.kernel_ms("thorough") < 0.7:
        assert np.array_equal(ev.xcd_shares(), np.full(8, 0.125))
