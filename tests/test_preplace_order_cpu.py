"""The restated summation order of tests/preplace_ref.py and the read sets of tests/test_gpu_preplace_edges.py, proven on
the CPU with the oracle in the device's place -- before anything runs on a GPU.

1. The lookup table extracted by single-site reads (Oracle.preplace(extraction_reads)), summed by expected_rows in the
   promised order ((t0 + t1) + (t2 + t3) per four sites from the window start, then the singles), is Oracle.preplace
   of every read set on every reference, bit for bit (np.array_equal).
2. The inputs can tell orders apart: the same terms summed left to right, or with the groups of four shifted by one
   site, differ from the oracle in at least one bit on at least 90 % of the rows of span >= 8 of `short` and `long`, on
   every reference.
3. encode_queries finds the intended window of every read, and every (set, bound) reaches the kernel instantiation it
   is listed under (preplace_ref.instantiation restates launch_preplace's conditions).

`short` has 4 reads per span and so 382 reads on W = 97, not the 600 the plan of this file estimated: the narrow pair
kernel (Q x 96 >= 1400 x W: 1415 reads) needs it four times over, not three (preplace_ref.narrow_factor)."""
import functools

import numpy as np
import pytest

import epa_ng_amd as epa
import preplace_ref as pr
from oracle_lib import Oracle

RIDS = list(pr.REFS)


@functools.lru_cache(maxsize=None)
def oracle(rid):
    c = pr.reference_case(rid)
    o = Oracle(c["newick"], c["labels"], c["seqs"], c["states"], c["subst"], c["freqs"], c["rates"])
    assert o.B == c["B"] and o.W == c["W"]
    return o


@functools.lru_cache(maxsize=None)
def table(rid):
    c = pr.reference_case(rid)
    ex = pr.extraction_set(rid)
    codes, wb, ws = epa.encode_queries(c["states"], ex.reads)
    assert [(int(a), int(b)) for a, b in zip(wb, ws)] == ex.windows
    chars = pr.extraction_chars(c["states"])
    return pr.table_from_rows(oracle(rid).preplace(ex.reads), codes, c["W"], chars, pr.any_char(c["states"]))


def cpu_sets(rid):
    """(name, ReadSet) of every read set; `tiled` as its 40 distinct reads"""
    return [(n, pr.read_set(rid, n)[0]) for n in pr.set_names(rid) if not n.startswith("short x")]


def test_ordered_sum_is_the_stated_order():
    t = np.array([[1e16], [1.0], [-1e16], [1.0], [3.0], [1e-3], [7.0]])
    want = 0.0 + ((t[0] + t[1]) + (t[2] + t[3]))
    want = ((want + t[4]) + t[5]) + t[6]
    assert np.array_equal(pr.ordered_sum(t), want)
    assert pr.ordered_sum(t)[0] != pr.left_to_right_sum(t)[0]
    assert np.array_equal(pr.ordered_sum(t[:0]), [0.0]) and np.array_equal(pr.ordered_sum(t[:3]), (t[0] + t[1]) + t[2])
    assert np.array_equal(pr.shifted_sum(t[:6]), ((0.0 + t[0]) + ((t[1] + t[2]) + (t[3] + t[4]))) + t[5])


@pytest.mark.parametrize("rid", RIDS)
def test_table_is_complete_and_a_gap_takes_the_any_column(rid):
    c = pr.reference_case(rid)
    t = table(rid)
    chars = pr.extraction_chars(c["states"])
    assert t.shape[0] == c["W"] and t.shape[2] == c["B"] == 2 * pr.REFS[rid][1] - 3
    assert np.sum(~np.isnan(t[:, :, 0]).any(axis=0)) == len(chars) + 1          # every character + the gap
    # a gap between two plain sites: the oracle's row is the three-term sum with the any-character column
    mid = c["W"] // 2
    read = "-" * (mid - 1) + c["seqs"][0][mid - 1] + "-" + c["seqs"][0][mid + 1] + "-" * (c["W"] - mid - 2)
    codes, wb, ws = epa.encode_queries(c["states"], [read])
    assert (int(wb[0]), int(ws[0])) == (mid - 1, 3)
    assert np.array_equal(pr.expected_rows(t, codes, wb, ws), oracle(rid).preplace([read]))


@pytest.mark.parametrize("rid", RIDS)
def test_expected_rows_are_the_oracle_bit_for_bit(rid):
    c = pr.reference_case(rid)
    o, t = oracle(rid), table(rid)
    for name, rs in cpu_sets(rid):
        codes, wb, ws = epa.encode_queries(c["states"], rs.reads)
        assert [(int(a), int(b)) for a, b in zip(wb, ws)] == rs.windows, name       # the intended windows
        want = o.preplace(rs.reads)
        got = pr.expected_rows(t, codes, wb, ws)
        assert np.array_equal(got, want), (name, int(np.sum(np.any(got != want, axis=1))), len(rs))
        # the compact layout carries the same codes: the GPU file feeds both
        cc, cb, cs = epa.encode_queries(c["states"], rs.reads, compact=True)
        assert np.array_equal(cb, wb) and np.array_equal(cs, ws)
        for i in range(0, len(rs), max(1, len(rs) // 50)):
            assert np.array_equal(cc[i, :ws[i]], codes[i, wb[i]:wb[i] + ws[i]]), (name, i)


@pytest.mark.parametrize("rid", RIDS)
def test_inputs_tell_summation_orders_apart(rid):
    c = pr.reference_case(rid)
    o, t = oracle(rid), table(rid)
    for name, rs in (("short", pr.short_set(rid)), ("long", pr.long_set(rid))):
        codes, wb, ws = epa.encode_queries(c["states"], rs.reads)
        want = o.preplace(rs.reads)
        rows = ws >= 8
        assert rows.sum() >= 10
        for what, order in (("left to right", pr.left_to_right_sum), ("shifted by one site", pr.shifted_sum)):
            differ = np.any(pr.expected_rows(t, codes, wb, ws, order=order) != want, axis=1)
            share = differ[rows].sum() / rows.sum()
            print("%s %s, %s: %d of %d rows of span >= 8 differ from the oracle (%.1f %%)"
                  % (rid, name, what, differ[rows].sum(), rows.sum(), 100 * share))
            assert share >= 0.9, (name, what, share)


def test_read_sets_have_the_shapes_they_are_meant_to_have():
    for rid in RIDS:
        states, tips, W = pr.REFS[rid]
        cap = pr.cap_of(states)
        s = pr.short_set(rid)
        spans = {}
        for b, n in s.windows:
            spans.setdefault(n, []).append(b)
        assert sorted(spans) == list(range(1, min(cap, W) + 1))
        for n, begins in spans.items():
            assert 0 in begins and W - n in begins
            if W - n >= 4:
                assert {b % 2 for b in begins if 0 < b < W - n} == {0, 1}, (rid, n)
        assert {n % 4 for n in spans} == {0, 1, 2, 3} and set(range(1, 8)) <= set(spans)
        assert any(b + n == W and n > 1 for b, n in s.windows)                   # a window ends on the last column
        assert W % 2 == 1 and (2 * tips - 3) % 2 == 1
        lg = pr.long_set(rid)
        assert sorted({n for _, n in lg.windows}) == pr.LONG_SPANS[rid] and max(pr.LONG_SPANS[rid]) == W
        for n in pr.LONG_SPANS[rid]:
            begins = [b for b, m in lg.windows if m == n]
            assert 0 in begins and W - n in begins and (W - n == 0 or {b % 2 for b in begins} == {0, 1})
        sp = pr.sparse_set(rid)
        assert len(sp) == 40 and all(5 <= n <= 20 and (b < 8 or W - 28 <= b < W - 20) for b, n in sp.windows)
        td = pr.tiled_distinct(rid)
        assert len(td) == 40 and not td.rare.any()
        tl = pr.tiled_set(rid)
        assert len(tl) == 41000 and tl.reads[40] == tl.reads[0] and tl.windows[:40] == td.windows
        ex = pr.extraction_set(rid)
        assert len(ex) == W * len(pr.extraction_chars(states)) and ex.max_span == 1
        # characters: every third read has the any-character and a gap inside, DNA: every seventh a rare code
        anyc = pr.any_char(states)
        for i in range(0, len(s), 3):
            b, n = s.windows[i]
            inner = s.reads[i][b + 1:b + n - 1]
            if n >= 13:                                                        # two or more of the inner sites
                assert anyc in inner and "-" in inner, (rid, i)
            assert s.reads[i][b] != "-" and s.reads[i][b + n - 1] != "-"
        has_rare = np.array([states == 4 and any(ch in pr.DNA_RARE for ch in r) for r in s.reads])
        assert np.array_equal(has_rare, s.rare)
        assert s.rare.any() == (states == 4) and (states == 20 or np.array_equal(np.nonzero(s.rare)[0] % 7, np.full(s.rare.sum(), 3)))


def test_every_set_and_bound_reaches_its_instantiation():
    reached = set()
    for rid in RIDS:
        states, _, W = pr.REFS[rid]
        for name, Q, bound, want in pr.variant_cases(rid):
            assert pr.instantiation(states, Q, W, bound) == want, (rid, name, Q, bound)
            reached.add(want)
            reached.add(pr.instantiation(states, Q, W, 0, generic=True))           # the generic setting: bound open
            if states == 4:
                reached.add(pr.generic_instantiation(states, bound))               # the rare-code reads of the call
        if states == 4:
            assert pr.short_set(rid).rare.any() and pr.extraction_set(rid).rare.any()
            assert pr.narrow_factor(rid) * len(pr.short_set(rid)) * 96 >= 1400 * W > len(pr.short_set(rid)) * 96
    assert {n for n, _, b, _ in pr.variant_cases("N125") if b} == {"short", "sparse", "tiled", "extraction", "short x 9",
                                                              "few1", "few15", "few16", "few17"}
    assert "long" in {n for n, _, b, _ in pr.variant_cases("N67") if b}
    assert reached == {pr.NARROW, pr.WIDE, pr.PAIRS_ACC, pr.SITES, pr.SITES_ACC, "k_preplace<16, true>",
                       "k_preplace<16, false>", "k_preplace<24, true>"}
    # the thresholds themselves
    assert pr.instantiation(4, 1415, 97, 160) == pr.NARROW and pr.instantiation(4, 1414, 97, 160) == pr.WIDE
    assert pr.instantiation(4, 10 ** 6, 97, 161) == pr.PAIRS_ACC and pr.instantiation(4, 1, 97, 1) == pr.WIDE
    assert pr.instantiation(20, 5, 131, 128) == pr.SITES and pr.instantiation(20, 5, 131, 129) == pr.SITES_ACC
