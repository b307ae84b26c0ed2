"""Pure-numpy restatement of the three statistics that epa_dev_rell_kh specifies (include/epa_dev.h): the p-values of the
KH, the weighted KH and the weighted SH test, from the replicates of epa_dev_rell_support.  No code of the product:
generator and draws are rell_ref's restatement, the rest is written out from the header, every step one float64
operation, every sum sequential in the specified order, nothing fused.

  score     s_k^(r): 0.0, then one add per draw in draw order
  observed  L_k: 0.0, then one add per site j = 0 .. n_q - 1 in this order
  centred   c_k^(r) = s_k^(r) - L_k
  best      b: the largest L; ties to the smaller branch id, then to the smaller entry index
  scale     d_j = x_k'[j] - x_k[j]; a = 0.0 plus the d_j in site order; m = a / n_q; q = 0.0 plus (d_j - m) * (d_j - m)
            in site order; v = sqrt(q); w_kk' = 1.0 / v; the pair is skipped when q == 0 or w is not finite
  p_kh      #{r: c_b - c_k >= L_b - L_k} / R
  p_wkh     k* = argmax over the pairs not skipped of (L_k' - L_k) * w_kk' (ties: branch id, index);
            #{r: c_k* - c_k >= L_k* - L_k} / R; no opponent: 1
  p_wsh     T_k = max (L_k' - L_k) * w_kk'; t_k^(r) = max (c_k' - c_k) * w_kk', both over the pairs not skipped;
            #{r: t_k >= T_k} / R; no opponent: 1
  best entry b, and a copy of b (L_b - L_k == 0 and the pair with b skipped), has no opponent: all three are 1

and a second version on numpy's own generator (multinomial site counts, scores as count-weighted sums).
"""
import numpy as np

from rell_ref import draws, group_by_query, site_rows, six_sigma, stat_input  # noqa: F401  (re-exported for the tests)
import rell_ref as rr

BIG = np.iinfo(np.int64).max


def pair_scale(sub):
    """sub [E][n_q]: site values per entry -> (w [E][E], ok [E][E]): the scale of every ordered pair and whether the
    pair takes part (the diagonal never does); w is 0.0 where ok is False"""
    sub = np.asarray(sub, np.float64)
    E, n_q = sub.shape
    d = sub[None, :, :] - sub[:, None, :]          # d[k][k'][j] = x_k'[j] - x_k[j]
    a = np.zeros((E, E))
    for j in range(n_q):                           # one add per site, in site order
        a = a + d[:, :, j]
    with np.errstate(divide="ignore", invalid="ignore"):
        m = a / np.float64(n_q)
        q = np.zeros((E, E))
        for j in range(n_q):
            e = d[:, :, j] - m
            p = e * e                              # the product is rounded before it is added
            q = q + p
        v = np.sqrt(q)
        w = np.float64(1.0) / v
    ok = (q != 0.0) & np.isfinite(w)
    ok[np.arange(E), np.arange(E)] = False
    return np.where(ok, w, 0.0), ok


def first_by_branch(tied, branch):
    """tied [E] bool, at least one True -> the tied position with the smallest branch id, then the smallest index"""
    return int(np.argmin(np.where(tied, branch, BIG)))          # argmin: the first minimum


def query_stats(sub, j, branch):
    """one query.  sub [E][n_q]: site values per entry, j [R][n_q]: the drawn sites, branch [E] -> dict: L [E], c [R][E],
    best (position), w, ok [E][E], opp [E] (position of k*, -1: none), T [E], kh, wkh, wsh [E] (counts of replicates)"""
    sub = np.asarray(sub, np.float64)
    E, n_q = sub.shape
    R = j.shape[0]
    branch = np.asarray(branch, np.int64)
    score = np.zeros((R, E))
    for d in range(n_q):                           # one add per draw, in draw order
        score += sub[:, j[:, d]].T
    L = np.zeros(E)
    for site in range(n_q):                        # one add per site, in site order
        L += sub[:, site]
    c = score - L[None, :]
    best = first_by_branch(L == L.max(), branch)
    w, ok = pair_scale(sub)
    kh = np.sum((c[:, best][:, None] - c) >= (L[best] - L)[None, :], axis=0)
    opp = np.full(E, -1, np.int64)
    T = np.full(E, np.nan)
    wkh = np.full(E, R, np.int64)
    wsh = np.full(E, R, np.int64)
    for k in range(E):
        top = k == best or (L[best] - L[k] == 0.0 and not ok[best, k])      # the best entry or a copy of it
        if top or not ok[k].any():
            continue
        val = np.where(ok[k], (L - L[k]) * w[k], -np.inf)
        T[k] = val.max()
        opp[k] = first_by_branch((val == T[k]) & ok[k], branch)
        wkh[k] = np.sum((c[:, opp[k]] - c[:, k]) >= (L[opp[k]] - L[k]))
        t = np.max(np.where(ok[k][None, :], (c - c[:, k][:, None]) * w[k][None, :], -np.inf), axis=1)
        wsh[k] = np.sum(t >= T[k])
    return dict(L=L, c=c, best=best, w=w, ok=ok, opp=opp, T=T, kh=kh, wkh=wkh, wsh=wsh)


def rell_kh(rows_by_entry, spans, groups, stream_ids, R, seed, branch_ids):
    """the arguments of rell_ref.rell_counts -> dict: kh, wkh, wsh int64 [n] (replicates counted), L float64 [n], best
    bool [n] (the entry is its query's b)"""
    n = len(rows_by_entry)
    out = dict(kh=np.zeros(n, np.int64), wkh=np.zeros(n, np.int64), wsh=np.zeros(n, np.int64), L=np.zeros(n),
               best=np.zeros(n, bool))
    for q, members in groups.items():
        members = sorted(int(i) for i in members)
        n_q = int(spans[q])
        sub = np.stack([np.asarray(rows_by_entry[i], np.float64)[:n_q] for i in members])
        s = query_stats(sub, draws(n_q, R, stream_ids[q], seed), [int(branch_ids[i]) for i in members])
        for key in ("kh", "wkh", "wsh", "L"):
            out[key][members] = s[key]
        out["best"][members[s["best"]]] = True
    return out


def multinomial_kh(rows, R, rng):
    """plain resampling of one query's rows [E][n_q] with numpy's own generator: site counts drawn as a multinomial, a
    replicate's score the count-weighted sum, the scale of a pair the standard deviation of the resampled difference
    written as a formula -> dict: p_kh, p_wkh, p_wsh [E]"""
    rows = np.asarray(rows, np.float64)
    E, n_q = rows.shape
    counts = rng.multinomial(n_q, np.full(n_q, 1.0 / n_q), size=R)      # [R][n_q]
    s = counts @ rows.T
    L = rows.sum(axis=1)
    c = s - L[None, :]
    d = rows[None, :, :] - rows[:, None, :]
    sd = np.sqrt(n_q * d.var(axis=2))                                   # Var(sum of n_q draws of d) = n_q Var(d)
    ok = sd > 0.0
    w = np.where(ok, 1.0 / np.where(ok, sd, 1.0), 0.0)
    b = int(np.argmax(L))
    out = dict(p_kh=np.mean((c[:, b][:, None] - c) >= (L[b] - L)[None, :], axis=0), p_wkh=np.ones(E), p_wsh=np.ones(E))
    for k in range(E):
        if k == b or (L[k] == L[b] and not ok[b, k]) or not ok[k].any():
            continue
        val = np.where(ok[k], (L - L[k]) * w[k], -np.inf)
        o = int(np.argmax(val))
        out["p_wkh"][k] = np.mean((c[:, o] - c[:, k]) >= (L[o] - L[k]))
        t = np.max(np.where(ok[k][None, :], (c - c[:, k][:, None]) * w[k][None, :], -np.inf), axis=1)
        out["p_wsh"][k] = np.mean(t >= val[o])
    return out


_STAT = {}


def stat_kh():
    """rell_ref.stat_input() (22 reads of 30 sites, three entries each, brute-force rows) through multinomial_kh at
    STAT_R replicates -> dict of [n] arrays: p_kh, p_wkh, p_wsh.  Built once per process."""
    if not _STAT:
        s = stat_input()
        rng = np.random.default_rng(20261020)
        per_query = [multinomial_kh(s["rows"][3 * q:3 * q + 3], rr.STAT_R, rng) for q in range(len(s["reads"]))]
        for key in ("p_kh", "p_wkh", "p_wsh"):
            _STAT[key] = np.concatenate([p[key] for p in per_query])
            _STAT[key].setflags(write=False)
    return _STAT
