"""Independent restatement of the reference's candidate selection and LWR filter, in plain Python
(no libepa_host, no device).  Every function names the reference file:line it restates.

One order everywhere: lnL descending, then branch id ascending.  The reference sorts by LWR with an
unstable std::sort (src/set_manipulators.cpp:71-80), so any order of equal LWRs conforms to it;
LWR is a monotone function of lnL, so "lnL descending, ties by the lowest branch id" is one of
those orders, and the one the device kernels use.

LWRs are exp(lnL - max) over a correctly rounded denominator (math.fsum), as float64 -- what the
reference stores; values that underflow in the reference (lnL more than ~745 below the row maximum)
come out as exactly 0.0.  Decisions on accumulated LWR sums are made on the float64 values summed in
selection order, as the reference does; `margin()` reports how far the exactly rounded prefix sums
stay from a threshold, so that a test can keep to rows where float64 rounding (another summation
order, another exp) cannot flip a decision, or to rows built to be exact."""
import math

import numpy as np


def order(lnl, ids=None):
    """positions of `lnl` in selection order: lnL descending, then branch id ascending"""
    ids = list(range(len(lnl))) if ids is None else list(ids)
    return sorted(range(len(lnl)), key=lambda i: (-float(lnl[i]), ids[i]))


def lwr(lnl):
    """compute_and_set_lwr (src/set_manipulators.cpp:43-69): exp(lnL - max) / sum, the sum exactly rounded"""
    x = [float(v) for v in lnl]
    mx = max(x)
    e = [math.exp(v - mx) for v in x]
    tot = math.fsum(e)
    return [v / tot for v in e]


def until_accumulated_reached(lw_sorted, thresh, mn=1, mx=None):
    """src/set_manipulators.cpp:90-110 -> number kept.  Sums LWRs (already in selection order) while
    fewer than `mx` are summed and the sum is below `thresh` -- the crossing element is included,
    a threshold <= 0 keeps none -- then tops up to `mn - 1` (not `mn`: distance(iter, begin + min - 1),
    :104-107).  The reference's loop does not stop at the end of the list; here it does (the
    counterpart of quirk D7)."""
    n, s = 0, 0.0
    size = len(lw_sorted)
    while (mx is None or n < mx) and s < thresh and n < size:
        s += lw_sorted[n]
        n += 1
    if (mn - 1) - n > 0:
        n = min(size, mn - 1)
    return n


def until_top_percent(B, x):
    """src/set_manipulators.cpp:82-88: ceil(x * B) in doubles, clamped at B"""
    return min(B, int(math.ceil(float(x) * float(B))))


def baseball_count(lnl_sorted):
    """baseball_heuristic (src/core/heuristics.hpp:74-117) -> number kept.  hits = placements not
    below best - 3.0 (strike box, float64 arithmetic); then std::min(max_pitches - hits, max_strikes)
    more in size_t arithmetic: max_pitches - hits wraps when hits > 40, so 6 more are added; clamped
    at B (quirk D7: std::advance past the end)"""
    strike_box, max_strikes, max_pitches = 3.0, 6, 40
    best = float(lnl_sorted[0])
    thresh = best - strike_box
    hits = 0
    while hits < len(lnl_sorted) and not (float(lnl_sorted[hits]) < thresh):
        hits += 1
    diff = (max_pitches - hits) % (1 << 64)
    to_add = min(diff, max_strikes)
    return min(len(lnl_sorted), hits + to_add)


def select_row(row, mode, thresh):
    """apply_heuristic (src/core/heuristics.hpp:119-127) on one preplacement row -> kept branch ids,
    in selection order.  mode: "dynamic" (until_accumulated_reached(pq, thresh, 1, inf)),
    "fixed" (until_top_percent) or "baseball" """
    o = order(row)
    if mode == "baseball":
        n = baseball_count([row[i] for i in o])
    elif mode == "fixed":
        n = until_top_percent(len(row), thresh)
    else:
        lw = lwr(row)
        n = until_accumulated_reached([lw[i] for i in o], thresh)
    return o[:n]


def work_order(keep):
    """Work (src/core/Work.hpp: map<branch, vector<seq>>): (branch, query) pairs, branch-major,
    queries ascending.  keep: list (per query) of kept branch ids"""
    return sorted((b, q) for q, ks in enumerate(keep) for b in ks)


def heuristic(lnl, mode="dynamic", thresh=0.99999):
    """the whole table [Q][B] -> (branch ids, query ids) in Work order"""
    pairs = work_order([select_row(list(r), mode, thresh) for r in lnl])
    return [b for b, _ in pairs], [q for _, q in pairs]


def discard_by_support_threshold(lw_sorted, thresh, mn, mx):
    """src/set_manipulators.cpp:131-163 -> number kept: those with LWR > thresh; at least `mn`
    (clamped at the list's end); at most `mx` unless 0 -- the max clamp uses the count before the
    min top-up, so with mn > mx a short list keeps mn"""
    if thresh < 0.0 or thresh > 1.0:
        raise ValueError("thresh is not a valid likelihood weight ratio (outside of [0,1])")
    if mn < 1:
        raise ValueError("Filter min cannot be smaller than 1!")
    num_kept = 0
    while num_kept < len(lw_sorted) and lw_sorted[num_kept] > thresh:
        num_kept += 1
    end = num_kept
    if num_kept < mn:
        end = min(len(lw_sorted), mn)
    if mx and num_kept > mx:
        end = mx
    return end


def discard_by_accumulated_threshold(lw_sorted, thresh, mn, mx):
    """src/set_manipulators.cpp:165-190 -> number kept (until_accumulated_reached(pq, thresh, min, max))"""
    if thresh < 0.0 or thresh > 1.0:
        raise ValueError("thresh is not a valid likelihood weight ratio (outside of [0,1])")
    if mn < 1:
        raise ValueError("Filter min cannot be smaller than 1!")
    if mn > mx:
        raise ValueError("Filter min cannot be smaller than max!")
    return until_accumulated_reached(lw_sorted, thresh, mn, mx)


def filter_pquery(lnl, ids, thresh, acc, mn, mx):
    """compute_and_set_lwr + filter (src/set_manipulators.cpp:192-205) on one pquery of placements
    (lnl[i] on branch ids[i]) -> [(branch id, lwr)] kept, in selection order"""
    lw = lwr(lnl)
    o = order(lnl, ids)
    s = [lw[i] for i in o]
    n = (discard_by_accumulated_threshold if acc else discard_by_support_threshold)(s, thresh, mn, mx)
    return [(ids[i], lw[i]) for i in o[:n]]


def margin(row, thresh, ids=None):
    """smallest |prefix LWR sum - thresh| over the prefix sums the dynamic rule compares (selection
    order, sums exactly rounded), 0 when one of them meets the threshold exactly"""
    lw = lwr(row)
    o = order(row, ids)
    t = float(thresh)
    s, c, m = 0.0, 0.0, math.inf    # compensated running sum; the empty prefix (0 < thresh) is exact
    for i in o:
        if not s + c < t:
            break
        x = lw[i]
        y = s + x
        c += (s - y) + x if abs(s) >= abs(x) else (x - y) + s
        s = y
        m = min(m, abs((s + c) - t))
    return m


def robust(row, thresh, exact=False):
    """the dynamic rule's decision on `row` at `thresh` cannot depend on float64 rounding: the prefix
    sums stay 1e-10 away from the threshold, or the row was built to be exact (LWRs 1/2^k and 0)"""
    return exact or margin(row, thresh) > 1e-10


# ---- crafted preplacement rows ---------------------------------------------------------------------
DYN_THRESHOLDS = (0.0, 1e-300, 0.3, 0.5, 0.75, 0.9, 0.99999, 1.0 - 1e-16, 1.0)


def fixed_fractions(B):
    """-G values for a reference of B branches: 0, 1, two plain ones, and one just above k / B whose
    product x * B rounds to the integer k in doubles (ceil keeps k; the exact product would keep k + 1)"""
    from fractions import Fraction
    xs = [0.0, 0.1, 0.5, 1.0]
    for k in range(1, B):
        x = math.nextafter(k / B, 2.0)
        if x * B == k and Fraction(x) * B > k:
            xs.append(x)
            break
    return xs


def crafted_rows(B, seed=0):
    """-> list of (name, row float64[B], exact).  exact: every LWR is 1/2^k or 0 in float64 and so
    is every prefix sum, whatever the summation order (the threshold crossings are exact)"""
    rng = np.random.RandomState(1000 + seed + B)
    base = -1000.0

    def below(lo, hi):
        return base - rng.uniform(lo, hi, B)
    rows = [("all_equal", np.full(B, base), B == 1)]
    # a tie group straddling the cutoff: the best, then g equal values scattered over the row
    r = below(30.0, 60.0)
    g = min(B - 1, 7)
    ids = rng.choice(B, g + 1, replace=False)
    r[ids[0]] = base
    r[ids[1:]] = base - 0.5
    rows.append(("tie_group", r, False))
    # equal maxima on both sides of a lane / wave / segment boundary, and across the row's ends
    for a, b in ((63, 64), (255, 256), (B - 1, 0)):
        if max(a, b) < B and a != b:
            r = below(0.2, 40.0)
            r[a] = r[b] = base
            rows.append(("tie_%d_%d" % (a, b), r, False))
    r = below(0.1, 20.0)
    r[B - 1] = base
    rows.append(("max_last", r, False))
    # spread of 2000 lnL units: most LWRs underflow to 0, with equal values among them
    r = below(0.0, 2000.0)
    r[rng.randint(B)] = base
    if B > 8:
        src = rng.choice(B, 4, replace=False)
        dst = rng.choice(B, 4, replace=False)
        r[dst] = r[src]
    rows.append(("spread_2000", r, False))
    # four equal at the top, everything else underflows (some of it tied): LWRs exactly 0.25 and 0
    if B >= 4:
        r = below(800.0, 2000.0)
        r[rng.choice(B, 4, replace=False)] = base
        if B > 12:
            r[rng.choice(B, 4, replace=False)] = base - 900.0
        top = np.flatnonzero(r == base)
        if len(top) == 4:
            rows.append(("four_top_underflow", r, True))
    # one maximum, the rest 708-744 below it: subnormal LWRs, the maximum's LWR is exactly 1
    r = below(708.0, 744.0)
    r[rng.randint(B)] = base
    rows.append(("subnormal", r, True))
    # the baseball strike box: values exactly 3.0 below the best count as hits
    for hits in (1, 40, 41, 60):
        if hits > B:
            continue
        r = below(3.5, 60.0)
        ids = rng.choice(B, hits, replace=False)
        r[ids] = base - np.where(rng.rand(hits) < 0.5, 3.0, rng.uniform(0.0, 3.0, hits))
        r[ids[0]] = base
        rows.append(("strike_box_%d" % hits, r, False))
    return rows
