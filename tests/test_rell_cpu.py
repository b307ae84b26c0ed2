"""The RELL resampling specification (include/epa_dev.h, epa_dev_rell_support) restated in numpy (tests/rell_ref.py):
the generator's known answers, the restatement on matrices made by hand, and the restatement against plain multinomial
resampling with numpy's own generator on brute-force site rows.  No device.

Measured here: the statistical check compares 66 proportions (22 reads x 3 branches); the largest
|restatement - default_rng| / bound is 0.44, and 11 of the 22 reads have their top support inside (0.05, 0.95).
"""
import numpy as np

import rell_ref as rr

KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
)


def test_philox_known_answers():
    for counter, key, want in KNOWN_ANSWERS:
        got = " ".join("%08x" % int(x) for x in rr.philox4x32_10(counter, key))
        assert got == want
    # an array of counters gives, element for element, the words of the single counters
    counter, key, want = KNOWN_ANSWERS[2]
    words = rr.philox4x32_10([np.array([c, c + 1], np.uint64) for c in counter], key)
    assert " ".join("%08x" % int(x[0]) for x in words) == want
    shifted = rr.philox4x32_10([c + 1 for c in counter], key)
    assert [int(x[1]) for x in words] == [int(x) for x in shifted]


def test_draws_follow_the_counter_layout():
    n_q, R, t, seed = 11, 5, (7 << 32) | 9, (3 << 32) | 2
    j = rr.draws(n_q, R, t, seed)
    assert j.shape == (R, n_q) and j.min() >= 0 and j.max() < n_q
    for r in (0, 4):
        for d in (0, 3, 4, 10):
            word = int(rr.philox4x32_10((d // 4, r, 9, 7), (2, 3))[d % 4])
            assert j[r, d] == (word * n_q) >> 32
    assert rr.draws(0, 3, 0, 1).shape == (3, 0)


def test_restatement_on_hand_made_matrices():
    R, n_q = 257, 13
    rng = np.random.RandomState(3)
    low = rng.uniform(-9.0, -1.0, n_q)
    # one entry larger at every site wins every replicate, whatever the branch ids
    rows = np.stack([low, low + 0.5])
    counts = rr.rell_counts(rows, [n_q], {0: [0, 1]}, [0], R, 1, [0, 1])
    assert counts.tolist() == [0, R]
    # identical rows: everything to the smaller branch id, then to the smaller entry index
    rows = np.stack([low, low, low])
    assert rr.rell_counts(rows, [n_q], {0: [0, 1, 2]}, [0], R, 1, [5, 2, 2]).tolist() == [0, R, 0]
    assert rr.rell_counts(rows, [n_q], {0: [0, 1, 2]}, [0], R, 1, [4, 4, 4]).tolist() == [R, 0, 0]
    # an empty window: every score is 0.0, the tie rule gives the whole support to one entry
    assert rr.rell_counts(np.zeros((2, 4)), [0], {0: [0, 1]}, [3], R, 1, [9, 1]).tolist() == [0, R]
    # counts of a query sum to R; two queries are independent of each other and of their order in the dict
    rows = rng.uniform(-9.0, -1.0, (5, n_q))
    groups = {0: [0, 3], 1: [1, 2, 4]}
    counts = rr.rell_counts(rows, [n_q, 7], groups, [0, 1], R, 9, [3, 1, 4, 1, 5])
    assert counts[[0, 3]].sum() == R and counts[[1, 2, 4]].sum() == R and counts.min() >= 0
    alone = rr.rell_counts(rows, [n_q, 7], {1: [1, 2, 4]}, [0, 1], R, 9, [3, 1, 4, 1, 5])
    assert np.array_equal(alone[[1, 2, 4]], counts[[1, 2, 4]]) and alone[[0, 3]].sum() == 0
    # the stream id and the seed select the draws
    other = rr.rell_counts(rows, [n_q, 7], groups, [5, 1], R, 9, [3, 1, 4, 1, 5])
    assert np.array_equal(other[[1, 2, 4]], counts[[1, 2, 4]]) and not np.array_equal(other[[0, 3]], counts[[0, 3]])
    assert not np.array_equal(rr.rell_counts(rows, [n_q, 7], groups, [0, 1], R, 10, [3, 1, 4, 1, 5]), counts)


def test_restatement_against_multinomial_resampling():
    s = rr.stat_input()
    Q = len(s["reads"])
    counts = rr.rell_counts(s["rows"], [rr.STAT_SPAN] * Q, rr.group_by_query(s["seq"]), list(range(Q)), rr.STAT_R, 1,
                            s["branch"])
    p = counts / float(rr.STAT_R)
    assert np.all(counts.reshape(Q, 3).sum(1) == rr.STAT_R)
    # the input is not vacuous: at least a third of the queries are undecided
    top = p.reshape(Q, 3).max(1)
    undecided = int(np.sum((top > 0.05) & (top < 0.95)))
    ratio = np.abs(p - s["cpu"]) / rr.six_sigma(p, s["cpu"], rr.STAT_R)
    print("\n%d proportions of %d reads: max |restatement - default_rng| / bound %.3g; %d reads with top support in "
          "(0.05, 0.95)" % (len(p), Q, ratio.max(), undecided))
    assert 3 * undecided >= Q
    assert np.all(ratio <= 1.0)
