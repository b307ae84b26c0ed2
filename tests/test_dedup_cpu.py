"""The yardstick of the dedup tests, tests/dedup_ref.py, on hand-written cases (no GPU, no library): every item of the
definition in include/epa_dev.h ("Duplicate queries"), the order of the classes, and the same chunk in every layout."""
import numpy as np
import pytest

import dedup_ref as dr

W = 11


def w(*codes):
    return np.array(codes, np.uint8)


def run(windows, **kw):
    """(rep, first) lists from every layout of the same chunk, which must agree"""
    got = {name: dr.dedup(*enc, W) for name, enc in dr.layouts(windows, W, 8, True, **kw).items()}
    assert set(got) == {"full", "compact", "packed", "packed_full"}
    rep, first = got["full"]
    for name, (r, f) in got.items():
        assert np.array_equal(r, rep) and np.array_equal(f, first), name
        assert r.dtype == np.uint32 and f.dtype == np.uint32
    dr.check_invariants(rep, first)
    return rep.tolist(), first.tolist()


def test_one_query_and_none():
    assert run([(3, w(1, 2, 4))]) == ([0], [0])
    rep, first = dr.dedup(np.zeros((0, W), np.uint8), np.zeros(0, np.uint32), np.zeros(0, np.uint32), W)
    assert len(rep) == 0 and len(first) == 0


def test_equal_begin_span_and_codes_is_one_class():
    assert run([(3, w(1, 2, 4)), (3, w(1, 2, 4))]) == ([0, 0], [0])


@pytest.mark.parametrize("other", [w(1, 2, 8), w(8, 2, 4), w(1, 8, 4)], ids=["last", "first", "middle"])
def test_one_differing_code_splits(other):
    assert run([(3, w(1, 2, 4)), (3, other)]) == ([0, 1], [0, 1])


def test_begin_alone_splits():
    assert run([(3, w(1, 2, 4)), (4, w(1, 2, 4))]) == ([0, 1], [0, 1])
    assert run([(2, w(1, 2, 4)), (4, w(1, 2, 4))]) == ([0, 1], [0, 1])    # begins of one parity


def test_span_alone_splits_a_prefix_from_its_row():
    assert run([(3, w(1, 2, 4)), (3, w(1, 2))]) == ([0, 1], [0, 1])
    assert run([(3, w(1, 2, 0)), (3, w(1, 2))], fill=0) == ([0, 1], [0, 1])   # the longer row ends in the fill value


def test_empty_windows_are_identical_when_their_begin_is():
    assert run([(5, w()), (5, w()), (6, w()), (5, w())]) == ([0, 0, 1, 0], [0, 2])
    assert run([(5, w()), (5, w(1))]) == ([0, 1], [0, 1])


def test_nothing_outside_the_window_is_compared():
    rows = [(2, w(1, 2, 4, 8, 1)), (2, w(1, 2, 4, 8, 1)), (2, w(1, 2, 4, 8, 1))]
    for fill in ([0, 0xff, "random"], ["random", 0, 0xff]):
        # span..stride padding (compact), pad nibble (odd rows of 11 codes, packed_full) and outside columns (full) differ
        enc = dr.layouts(rows, W, 8, True, fill=fill, seed=3)
        assert not np.array_equal(enc["full"][0][0], enc["full"][0][1])
        assert not np.array_equal(enc["compact"][0][0], enc["compact"][0][1])
        assert enc["packed_full"][0].data[0, -1] & 15 != enc["packed_full"][0].data[1, -1] & 15
        assert run(rows, fill=fill, seed=3) == ([0, 0, 0], [0])
    enc = dr.layouts([(0, w(1, 2, 4)), (0, w(1, 2, 4))], W, 3, True, fill=[0, 0xff])   # odd compact rows: their pad nibble
    assert enc["packed"][0].data[0, -1] & 15 == 0 and enc["packed"][0].data[1, -1] & 15 == 15
    assert dr.dedup(*enc["packed"], W)[0].tolist() == [0, 0]


def test_classes_are_numbered_by_first_appearance():
    a, b, c = (1, w(1, 1)), (1, w(2, 2)), (1, w(4, 4))
    assert run([b, a, b, c, a, c, c]) == ([0, 1, 0, 2, 1, 2, 2], [0, 1, 3])
    assert run([c, c, c, b]) == ([0, 0, 0, 1], [0, 3])


def test_either_nibble_starts_a_full_width_window():
    for b in (0, 1, 2, 3):
        enc = dr.layouts([(b, w(1, 2, 4, 8, 3, 5, 9))], W, 8, True, fill=0xff)
        for name, e in enc.items():
            assert dr.window_codes(*e, W)[0].tolist() == [1, 2, 4, 8, 3, 5, 9], (b, name)


def test_one_byte_codes_above_fifteen():
    rows = [(0, w(23, 0, 200)), (0, w(23, 0, 200)), (0, w(23, 0, 201))]
    got = {n: dr.dedup(*e, W) for n, e in dr.layouts(rows, W, 8, False, fill="random").items()}
    assert set(got) == {"full", "compact"}
    for r, f in got.values():
        assert r.tolist() == [0, 0, 1] and f.tolist() == [0, 2]


@pytest.mark.parametrize("name", dr.STRUCTURES)
def test_structures(name):
    ids = dr.structure(name, 65, seed=1)
    pool = dr.distinct_windows(int(ids.max()) + 1, 33, (8, 9, 15, 16, 17), 16, 5)
    got = {n: dr.dedup(*e, 33) for n, e in dr.layouts([pool[i] for i in ids], 33, 32, True, fill="random", seed=2).items()}
    order = {}
    want = np.array([order.setdefault(int(i), len(order)) for i in ids])
    for n, (rep, first) in got.items():
        assert np.array_equal(rep, want), n
        dr.check_invariants(rep, first)
    sizes = np.bincount(want)
    assert {"identical": sizes.tolist() == [65], "distinct": len(sizes) == 65, "blocks": sizes[:16].tolist() == [4] * 16,
            "interleaved": len(sizes) == 8, "skewed": sizes.max() == 58 and len(sizes) == 8}[name]
