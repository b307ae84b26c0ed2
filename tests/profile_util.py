"""Helpers of the profile-query tests (tests/test_profile_cpu.py, tests/test_gpu_profile.py, tests/test_gpu_profile_cli.py):
numpy restatements of the column -> state-set map and of epa_profile_from_phred, random rows, and a BruteForce whose
queries are rows.  No likelihood code of the product.
"""
import numpy as np

from brute_force import BruteForce
from gen_golden import valid_range

NT_COLS = "-TGKCYSBAWRDMHVN"                       # lookup column -> character (the 4-bit codes of the .bfast format)
AA_COLS = "ACDEFGHIKLMNPQRSTVWY-XBZ"
AA_STATE_ORDER = "ARNDCQEGHILKMFPSTWYV"


def column_masks(states):
    """[ncols][states] 0/1: the state set of every lookup column"""
    if states == 4:
        out = np.zeros((16, 4))
        for col in range(16):
            bits = 15 if col == 0 else ((col >> 3) & 1) | ((col >> 2) & 1) << 1 | ((col >> 1) & 1) << 2 | (col & 1) << 3
            out[col] = [(bits >> i) & 1 for i in range(4)]
        return out
    out = np.zeros((24, 20))
    for col, ch in enumerate(AA_COLS):
        if ch in AA_STATE_ORDER:
            out[col, AA_STATE_ORDER.index(ch)] = 1.0
        elif ch == "B":
            out[col, [2, 3]] = 1.0
        elif ch == "Z":
            out[col, [5, 6]] = 1.0
        else:
            out[col] = 1.0
    return out


def zero_one_rows(states, codes, win_span, fill=0.0):
    """compact code rows [Q][stride] -> profile rows [Q][stride][states] holding every code's state set; the rows beyond a
    query's span are `fill`"""
    codes = np.asarray(codes)
    rows = column_masks(states)[codes]
    pad = np.arange(codes.shape[1])[None, :] >= np.asarray(win_span)[:, None]
    rows[pad] = fill
    return np.ascontiguousarray(rows)


def phred_rows(states, codes, phred, win_span, fill=0.0):
    """numpy restatement of epa_profile_from_phred"""
    masks = column_masks(states)
    codes, phred = np.asarray(codes), np.asarray(phred)
    rows = masks[codes]
    pure = rows.sum(2) == 1
    eps = np.minimum(np.power(10.0, -phred.astype(np.float64) / 10.0), (states - 1.0) / states)
    noisy = np.where(rows > 0, (1.0 - eps)[:, :, None], (eps / (states - 1.0))[:, :, None])
    rows = np.where(pure[:, :, None], noisy, rows)
    pad = np.arange(codes.shape[1])[None, :] >= np.asarray(win_span)[:, None]
    rows[pad] = fill
    return np.ascontiguousarray(rows)


def dense_rows(states, shape, seed):
    """[Q][stride][states] random rows, every entry in (0.05, 1]"""
    return np.random.RandomState(seed).uniform(0.05, 1.0, tuple(shape) + (states,))


class ProfileBrute(BruteForce):
    """BruteForce whose queries are rows: set_rows(read, rows [n][s]) makes tip_vectors(read) return the rows on the
    read's window (the read's own state sets elsewhere), so that score_at, _star and optimise run on them unchanged"""

    def __init__(self, *a, **kw):
        self._rows = {}
        super().__init__(*a, **kw)

    def set_rows(self, read, rows):
        lo, n = valid_range(read)
        full = BruteForce.tip_vectors(self, read).copy()
        full[lo:lo + n] = np.asarray(rows)[:n]
        self._rows[read] = full

    def tip_vectors(self, seq):
        got = self._rows.get(seq)
        return got if got is not None else BruteForce.tip_vectors(self, seq)


def brute_of(case):
    return ProfileBrute(case["newick"], case["labels"], case["seqs"], case["states"], case["subst"], case["freqs"], case["rates"],
                        weights=case["weights"], pinv=case["pinv"])
