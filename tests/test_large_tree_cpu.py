"""CPU tests of the large-tree work: the chunk loop's memory clamp (hostlib.device_chunk_reads, the function
place.cpp's loop calls with its kSlots = 4 pipeline slots) and the vectorised generator the GPU tests use."""
import numpy as np
import pytest

from epa_ng_amd import hostlib

import large_tree_gen as gen

BRANCHES = (1021, 65537, 200001)
BUDGETS = [1 << 20, 64 << 20, 1 << 30, 20 << 30, 192 << 30, 288 * 10 ** 9]


def _pitch(B):
    return (B * 8 + 63) // 64 * 64


def _bytes(reads, B, slots):
    """what the loop allocates for `reads` reads per chunk: `slots` tables + a quarter for the other buffers"""
    return reads * _pitch(B) * slots * 5 // 4


@pytest.mark.parametrize("B", BRANCHES)
def test_four_slots_fit_half_of_free_memory(B):
    for free in BUDGETS:
        for wanted in (1, 500, 5000, 50000, 1000000):
            n = hostlib.device_chunk_reads(free, B, 4, wanted)
            assert 1 <= n <= wanted, (free, B, wanted, n)
            if n > 1:
                assert _bytes(n, B, 4) <= free // 2, (free, B, wanted, n)
            if n < wanted:      # clamped: one more read per chunk would not fit (or nothing fits: 1)
                assert _bytes(n + 1, B, 4) > free // 2, (free, B, wanted, n)


def test_never_zero():
    for B in BRANCHES:
        assert hostlib.device_chunk_reads(0, B, 4, 5000) == 1
        assert hostlib.device_chunk_reads(1 << 10, B, 4, 5000) == 1
        assert hostlib.device_chunk_reads(1 << 40, B, 4, 0) == 1


@pytest.mark.parametrize("B", BRANCHES)
def test_explicit_chunk_size_is_only_lowered(B):
    for free in BUDGETS:
        for user in (1, 100, 5000, 100000):
            for wanted in (user, 10 * user):     # (--device-min-chunk may ask for more than --chunk-size)
                n = hostlib.device_chunk_reads(free, B, 4, wanted, user)
                assert 1 <= n <= user, (free, B, user, wanted, n)
                assert n == min(user, hostlib.device_chunk_reads(free, B, 4, wanted))


@pytest.mark.parametrize("B", BRANCHES)
def test_two_slots_reproduce_the_two_slot_figure(B):
    """the clamp the loop had budgeted two slots: room = (free / 2) / (pitch * 2 * 5 / 4), applied when the
    wanted chunk exceeds it.  (It never went below the default chunk size, whatever the room: that floor is
    gone -- it is what let four tables of a large tree outgrow the device -- so the figures are compared where
    the room is at least that size.)"""
    default_chunk = 5000
    for free in BUDGETS:
        room = (free // 2) // (_pitch(B) * 2 * 5 // 4)
        for wanted in (5000, 50000, 1000000):
            old = wanted if room >= wanted else max(min(default_chunk, wanted), max(room, 1))
            if room >= default_chunk:
                assert hostlib.device_chunk_reads(free, B, 2, wanted) == old, (free, B, wanted)
    # and four slots hold half of what two do
    assert hostlib.device_chunk_reads(20 << 30, 65537, 4, 10 ** 9) == hostlib.device_chunk_reads(20 << 30, 65537, 2, 10 ** 9) // 2


def test_generator_builds_an_unrooted_binary_tree():
    n = 1000
    w = gen.dna_workload(n, 48, 8, 24, (201, 202, 203))
    assert len(w["seqs"]) == n and all(len(s) == 48 and set(s) <= set("ACGT") for s in w["seqs"])
    assert w["newick"].count(",") == n - 1 and w["newick"].count("(") == n - 2
    r = hostlib.Reference(w["newick"], w["labels"], w["seqs"], states=4, subst=w["subst"], freqs=w["freqs"],
                          rates=w["rates"])
    assert r.B == 2 * n - 3
    assert np.isfinite(r.tree_lnl(0))
    # the sequences carry the tree's signal: sister tips differ less than random pairs
    a = np.array([list(s) for s in w["seqs"]])
    _, _, levels, _ = gen.random_join_levels(n, 201)
    p, ka, kb = levels[0]
    sis = np.mean(a[ka] != a[kb])
    rnd = np.mean(a[ka] != a[kb[::-1]])
    assert sis < rnd
