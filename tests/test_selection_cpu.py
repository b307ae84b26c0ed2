"""CPU tests of the host's candidate selection (apply_heuristic) and LWR filter against the plain
restatement of the reference in selection_ref.py, on crafted tables: exact ties between branches,
LWRs that underflow to 0 or are subnormal, thresholds crossed exactly and thresholds at the ends of
their range.  One tie rule throughout: lnL descending, then branch id ascending."""
import subprocess

import numpy as np
import pytest

from epa_ng_amd import hostlib
import selection_ref as ref


def test_restatement_literal_cases():
    # four equal values: each LWR is exactly 0.25, so 0.5 and 0.75 are crossed exactly by 2 and 3
    row = [-5.0, -5.0, -5.0, -5.0]
    assert ref.lwr(row) == [0.25] * 4
    assert [len(ref.select_row(row, "dynamic", t)) for t in (0.0, 1e-300, 0.5, 0.75, 1.0)] == [0, 1, 2, 3, 4]
    # equal LWRs of different lnL (both 0 after underflow): ordered by lnL, not by branch id
    row = [-3000.0, -2000.0, 0.0, -2500.0, -2000.0]
    assert ref.lwr(row) == [0.0, 0.0, 1.0, 0.0, 0.0]
    assert ref.select_row(row, "fixed", 0.6) == [2, 1, 4]
    assert ref.select_row(row, "fixed", 1.0) == [2, 1, 4, 3, 0]
    # until_accumulated_reached tops up to min - 1, not min (src/set_manipulators.cpp:104-107)
    assert ref.until_accumulated_reached([1.0, 0.0, 0.0, 0.0], 0.5, mn=3, mx=4) == 2
    assert ref.until_accumulated_reached([1.0, 0.0, 0.0, 0.0], 0.0, mn=1, mx=4) == 0
    # discard_by_support_threshold: the max clamp looks at the count before the min top-up
    assert ref.discard_by_support_threshold([0.5, 0.3, 0.2], 0.6, 3, 2) == 3
    assert ref.discard_by_support_threshold([0.5, 0.3, 0.2], 0.1, 1, 2) == 2
    # baseball: 40 hits -> none more; 41 -> 6 more (size_t wrap); clamped at B
    assert ref.baseball_count([0.0] * 40 + [-10.0] * 20) == 40
    assert ref.baseball_count([0.0] * 41 + [-10.0] * 20) == 47
    assert ref.baseball_count([0.0] * 43 + [-10.0] * 2) == 45
    assert ref.baseball_count([0.0, -3.0, -3.0000000000000004] + [-10.0] * 20) == 2 + 6
    # -G: ceil(x * B) in doubles; x just above 1/3 gives 3 * x == 1.0 exactly
    assert ref.until_top_percent(3, ref.fixed_fractions(3)[-1]) == 1


def _host_pairs(table, mode, thr):
    hb, hs = hostlib.heuristic(table, mode, thr)
    return list(zip(hb.tolist(), hs.tolist()))


def _ref_pairs(table, mode, thr):
    b, q = ref.heuristic(table, mode, thr)
    return list(zip(b, q))


@pytest.mark.parametrize("B", [3, 63, 129, 257, 513])
def test_host_heuristic_matches_restatement_on_crafted_rows(B):
    rows = ref.crafted_rows(B)
    for thr in ref.DYN_THRESHOLDS:
        table = np.array([r for _, r, exact in rows if ref.robust(r, thr, exact)])
        assert len(table)
        assert _host_pairs(table, "dynamic", thr) == _ref_pairs(table, "dynamic", thr), thr
    table = np.array([r for _, r, _ in rows])
    for x in ref.fixed_fractions(B):
        assert _host_pairs(table, "fixed", x) == _ref_pairs(table, "fixed", x), x
    assert _host_pairs(table, "baseball", 0.0) == _ref_pairs(table, "baseball", 0.0)


def test_host_dynamic_threshold_zero_keeps_no_candidates():
    """-g 0 is inside the reference's range (src/main.cpp:205-212); until_accumulated_reached(pq, 0, 1,
    max) keeps none of the placements"""
    table = np.array([[-1.0, -2.0, -3.0], [-5.0, -5.0, -5.0]])
    assert _host_pairs(table, "dynamic", 0.0) == []
    assert _host_pairs(table, "dynamic", 1e-300) == [(0, 0), (0, 1)]


def test_host_fixed_rule_orders_underflowed_lwrs_by_lnl():
    """-G on a row whose LWRs underflow: the kept ones are the best by lnL, whatever the branch ids"""
    row = np.full(63, -2000.0) - np.arange(63)[::-1] * 800.0   # lnL rises with the branch id: LWRs 0 but one
    table = row[None, :]
    hb, _ = hostlib.heuristic(table, "fixed", 0.1)               # ceil(6.3) = 7
    assert sorted(hb.tolist()) == list(range(56, 63))
    assert _host_pairs(table, "fixed", 0.1) == _ref_pairs(table, "fixed", 0.1)


def _pqueries():
    """-> (lnl, branch ids, exact): ties, zero LWRs of different lnL, subnormal LWRs, equal values.
    exact: LWRs 1/2^k or 0, or 1 and subnormals (every accumulated decision is exact)"""
    rng = np.random.RandomState(7)
    out = []
    # ties at the top and a tail of underflowed placements with distinct lnL (the top-ups go there)
    out.append(([-10.0, -10.0, -11.0, -3000.0, -2500.0, -2000.0, -2500.0, -2100.0], [4, 9, 0, 1, 2, 3, 5, 6], False))
    # four equal values: LWRs 0.25; the rest underflow, some tied
    out.append(([-7.0] * 4 + [-900.0, -1800.0, -900.0, -1200.0, -2000.0], [8, 3, 6, 1, 0, 2, 4, 5, 7], True))
    # the maximum at the last position, subnormal LWRs before it
    out.append((list(-1000.0 - rng.uniform(708.0, 744.0, 10)) + [-1000.0], list(range(11)), True))
    # a spread of 2000 lnL units over 64 placements, a few equal values among them
    ll = list(-rng.uniform(0.0, 2000.0, 64))
    ll[10] = ll[20] = ll[30]
    ll[40] = ll[41] = max(ll)
    out.append((ll, [int(i) for i in rng.permutation(64)], False))
    # all equal (odd count)
    out.append(([-3.5] * 7, [6, 5, 4, 3, 2, 1, 0], False))
    return out


@pytest.mark.parametrize("acc", [False, True])
def test_host_filter_matches_restatement(acc):
    """filter() after compute_and_set_lwr, as the chunk loop runs them, against
    discard_by_support_threshold / discard_by_accumulated_threshold: same placements in the same order,
    LWRs within 1e-12"""
    threshs = (0.0, 0.01, 0.25, 0.5, 0.75, 0.9999, 1.0)
    limits = [(1, 7), (1, 64), (3, 3), (5, 8), (10, 64), (64, 64), (1, 1)]
    if not acc:
        limits += [(4, 2), (2, 0)]      # the support filter takes min > max (min wins) and max 0 (no max)
    checked = 0
    for lnl, ids, exact in _pqueries():
        for t in threshs:
            if acc and not (exact or ref.margin(lnl, t, ids) > 1e-10):
                continue
            for mn, mx in limits:
                exp = ref.filter_pquery(lnl, ids, t, acc, mn, mx)
                got_ids, got_lwr = hostlib.filter_pquery(lnl, ids, t, acc, mn, mx)
                assert got_ids.tolist() == [b for b, _ in exp], (lnl, t, mn, mx)
                assert np.allclose(got_lwr, [w for _, w in exp], rtol=0, atol=1e-12)
                checked += 1
    assert checked > 100


def test_host_filter_rejects_what_the_reference_rejects():
    with pytest.raises(RuntimeError):
        hostlib.filter_pquery([0.0, -1.0], [0, 1], 1.5)
    with pytest.raises(RuntimeError):
        hostlib.filter_pquery([0.0, -1.0], [0, 1], 0.5, acc=True, mn=0)
    with pytest.raises(RuntimeError):
        hostlib.filter_pquery([0.0, -1.0], [0, 1], 0.5, acc=True, mn=3, mx=2)


def test_lwr_only_filter_entry_keeps_its_meaning():
    """epa_host_filter takes LWRs only: ordered by LWR, equal LWRs by position"""
    assert hostlib.filter_lwr([0.1, 0.4, 0.1, 0.4, 0.0, 0.0], 0.0, mn=1, mx=6).tolist() == [1, 3, 0, 2]
    assert hostlib.filter_lwr([0.1, 0.4, 0.1, 0.4, 0.0, 0.0], 0.5, mn=6, mx=6).tolist() == [1, 3, 0, 2, 4, 5]


@pytest.mark.parametrize("flags", [["-g", "1.5"], ["-G", "-0.1"], ["-g", "nan"], ["--filter-min-lwr", "2"],
                                   ["--filter-min", "8", "--filter-max", "7"]])
def test_cli_rejects_thresholds_outside_the_reference_range(flags, tmp_path):
    """-g / -G / --filter-*-lwr in [0, 1] and filter-min <= filter-max (src/main.cpp:165-218, 368-370):
    refused before any file is read"""
    exe = hostlib.cli_exe()
    r = subprocess.run([exe, "-t", str(tmp_path / "t"), "-s", str(tmp_path / "s"), "-q", str(tmp_path / "q"),
                        "-m", "GTR+G", "-w", str(tmp_path)] + flags, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "file_check" not in r.stderr and ("[0, 1]" in r.stderr or "filter-min" in r.stderr), r.stderr


def test_place_file_rejects_a_threshold_above_one(tmp_path):
    """epa_host_place_file: a threshold above 1 is refused before the run (0 no longer means "default")"""
    from golden_util import load_case
    g = load_case("dna8_gtr_fu_g4")
    labels = [a for a, _ in g["msa"]]
    seqs = [b for _, b in g["msa"]]
    r = hostlib.Reference(g["newick"], labels, seqs, states=4, subst=g["subst"], freqs=g["freqs"],
                          rates=g["gamma_rates"])
    with pytest.raises(RuntimeError, match=r"\[0,1\]"):
        r.place_file(str(tmp_path / "none.fasta"), str(tmp_path), threshold=1.5)
