"""The error bound of the preplacement's fp32 screen (epa_screen_delta, csrc/preplace.hip) on the CPU.

The screen sums a window's n pair-table entries, each rounded to fp32 once, in fp32 and in the exact pass's own
association: ((e0 + e1) + acc) per packed word, then the three tail singles.  With u = 2^-24 and |entry| <= M the
formula promises |s32 - s64| <= (n + 1) u n M (delta is twice that).  Numpy float32 restates the kernel's loop; on
random tables with entries in [-M, 0], M = 1, 60 and 1e4, at every window span of tests/test_gpu_preplace_screen.py,
10 000 windows per M, not one may exceed the bound before the factor 2: the bound is a theorem.
"""
import numpy as np
import pytest

U = 2.0 ** -24
SPANS = [1, 2, 3, 4, 5, 7, 8] + list(range(93, 98)) + list(range(128, 132)) + list(range(157, 161))
N_WINDOWS = 10000


def entries_of(span):
    """pair entries of the full quads (two per word), tail singles"""
    return 2 * (span >> 2), 3 if span & 3 else 0


def bound(span_bound, M):
    n = 2.0 * (span_bound >> 2) + 3.0            # as epa_screen_delta counts them
    return (n + 1.0) * U * n * M


def kernel_sum32(words, tails):
    """words float32 [N][nw][2], tails float32 [N][nt] -> the screen's fp32 sums [N]"""
    acc = np.zeros(words.shape[0], np.float32)
    for w in range(words.shape[1]):
        acc = (acc + (words[:, w, 0] + words[:, w, 1]).astype(np.float32)).astype(np.float32)
    for k in range(tails.shape[1]):
        acc = (acc + tails[:, k]).astype(np.float32)
    return acc


def kernel_sum64(words, tails):
    acc = np.zeros(words.shape[0], np.float64)
    for w in range(words.shape[1]):
        acc = acc + (words[:, w, 0] + words[:, w, 1])
    for k in range(tails.shape[1]):
        acc = acc + tails[:, k]
    return acc


@pytest.mark.parametrize("M", (1.0, 60.0, 1e4))
def test_fp32_loop_stays_within_the_formula(M):
    rng = np.random.default_rng(int(M) + 17)
    per = -(-N_WINDOWS // len(SPANS))
    worst = 0.0
    for span in SPANS:
        npair, ntail = entries_of(span)
        w64 = -M * rng.random((per, npair // 2, 2))
        t64 = -M * rng.random((per, ntail))
        if span == SPANS[-1]:                      # the extreme table: every entry at the magnitude bound
            w64[: per // 4] = -M
            t64[: per // 4] = -M
        s64 = kernel_sum64(w64, t64)
        s32 = kernel_sum32(w64.astype(np.float32), t64.astype(np.float32)).astype(np.float64)
        err = np.abs(s32 - s64)
        b = bound(span, M)
        worst = max(worst, float((err / b).max()))
        assert (err <= b).all(), "span %d, M %g: |s32 - s64| = %.6g exceeds (n + 1) u n M = %.6g" % (span, M, err.max(), b)
    print("M %g: largest |s32 - s64| / bound = %.3g" % (M, worst))
    assert per * len(SPANS) >= N_WINDOWS
