"""Restatement of the marginal likelihood that epa_dev_marginal_like specifies (include/epa_dev.h), from the brute force
of tests/brute_force.py alone: no code of the product.

  g_ij = lnL(b, q; pendant p_len[j], distal x_frac[i] * length(b), proximal the rest of the branch)     brute_grid
  v_ij = (x_logw[i] + p_logw[j]) + g_ij
  M    = m + log(sum exp(v_ij - m)), m = max v_ij, the sum in the order i ascending, then j ascending   combine
"""
import math

import numpy as np

from brute_force import valid_range


def brute_grid(bf, read, b, x_frac, p_len):
    """-> [Kx][Kp]: BruteForce._star over the read's own window, summed, at every node of the tensor rule"""
    lo, n = valid_range(read)
    tipv = bf.tip_vectors(read)[lo:lo + n]
    out = np.empty((len(x_frac), len(p_len)))
    for i, x in enumerate(x_frac):
        for j, p in enumerate(p_len):
            out[i, j] = float(bf._star(int(b), tipv, float(p), float(x) * float(bf.lengths[b]), lo, n).sum())
    return out


def combine(grid, x_logw, p_logw):
    """the M rule: plain fp64 adds in the specified order"""
    v = (np.asarray(x_logw, np.float64)[:, None] + np.asarray(p_logw, np.float64)[None, :]) + np.asarray(grid, np.float64)
    m = float(v.max())
    total = 0.0
    for t in v.reshape(-1):            # row-major: i ascending, then j ascending
        total += math.exp(float(t) - m)
    return m + math.log(total)


def entries(bf, n_reads):
    """branches {0, B // 2, B - 1} x every read -> (branch ids, read ids)"""
    rows = [(b, q) for b in (0, bf.B // 2, bf.B - 1) for q in range(n_reads)]
    return np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], np.int64)
