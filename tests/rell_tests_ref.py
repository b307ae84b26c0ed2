"""Pure-numpy restatement of the three statistics that epa_dev_rell_tests specifies (include/epa_dev.h): RELL support,
expected likelihood weight (ELW) and the SH test p-value, from the replicates of epa_dev_rell_support.  No code of the
product: generator and draws are rell_ref's restatement, the rest is written out from the header.

  score     s_k^(r): 0.0, then one fp64 add per draw in draw order
  observed  L_k: 0.0, then one fp64 add per site j = 0 .. n_q - 1 in this order
  support   the largest score wins; ties to the smaller branch id, then to the smaller entry index
  elw       m = max_k s_k^(r); w_k^(r) = exp(s_k^(r) - m) / sum_k' exp(s_k'^(r) - m); elw[k] = sum_r w_k^(r) / R
  p_sh      c = s - L; t_k^(r) = max_k' c_k'^(r) - c_k^(r); T_k = max L - L_k; p_sh[k] = #{r: t_k^(r) >= T_k} / R,
            one fp64 subtraction per step

and a second version on numpy's own generator (multinomial site counts, scores as count-weighted sums), centred at the
observed L of its own rows, which also records the classic SH recipe that centres at the mean of the replicates.
"""
import numpy as np

from rell_ref import draws, group_by_query, site_rows, six_sigma, stat_input  # noqa: F401  (re-exported for the tests)
import rell_ref as rr


def query_stats(sub, j, branch):
    """one query.  sub [E][n_q]: site values per entry, j [R][n_q]: the drawn sites, branch [E] -> dict: score [R][E],
    L [E], best [R] (the winner's position), w [R][E], t [R][E], T [E]"""
    sub = np.asarray(sub, np.float64)
    E, n_q = sub.shape
    R = j.shape[0]
    score = np.zeros((R, E))
    for d in range(n_q):                           # one add per draw, in draw order
        score += sub[:, j[:, d]].T
    L = np.zeros(E)
    for site in range(n_q):                        # one add per site, in site order
        L += sub[:, site]
    branch = np.asarray(branch, np.int64)
    tied = score == score.max(axis=1)[:, None]
    best = np.argmin(np.where(tied, branch[None, :], np.iinfo(np.int64).max), axis=1)   # argmin: the first minimum
    e = np.exp(score - score.max(axis=1)[:, None])
    w = e / e.sum(axis=1)[:, None]
    c = score - L[None, :]
    t = c.max(axis=1)[:, None] - c
    T = L.max() - L
    return dict(score=score, L=L, best=best, w=w, t=t, T=T)


def rell_tests(rows_by_entry, spans, groups, stream_ids, R, seed, branch_ids):
    """the arguments of rell_ref.rell_counts -> dict: wins int64 [n] (replicates won), elw float64 [n], sh int64 [n]
    (replicates with t >= T), L float64 [n]"""
    rows = np.asarray(rows_by_entry, np.float64)
    n = len(rows)
    out = dict(wins=np.zeros(n, np.int64), elw=np.zeros(n), sh=np.zeros(n, np.int64), L=np.zeros(n))
    for q, members in groups.items():
        members = sorted(int(i) for i in members)
        n_q = int(spans[q])
        s = query_stats(rows[members][:, :n_q], draws(n_q, R, stream_ids[q], seed), [int(branch_ids[i]) for i in members])
        out["wins"][members] = np.bincount(s["best"], minlength=len(members))
        out["elw"][members] = s["w"].sum(axis=0) / float(R)
        out["sh"][members] = np.sum(s["t"] >= s["T"][None, :], axis=0)
        out["L"][members] = s["L"]
    return out


def multinomial_tests(rows, R, rng):
    """plain resampling of one query's rows [E][n_q] with numpy's own generator: site counts drawn as a multinomial, a
    replicate's score the count-weighted sum -> dict: elw [E], p_sh [E] (centred at the rows' own sums), p_sh_classic
    [E] (centred at the mean of the replicates' scores, the classic SH recipe)"""
    rows = np.asarray(rows, np.float64)
    n_q = rows.shape[1]
    counts = rng.multinomial(n_q, np.full(n_q, 1.0 / n_q), size=R)      # [R][n_q]
    s = counts @ rows.T
    L = rows.sum(axis=1)
    e = np.exp(s - s.max(axis=1)[:, None])
    elw = (e / e.sum(axis=1)[:, None]).mean(axis=0)
    T = L.max() - L
    out = dict(elw=elw)
    for key, centre in (("p_sh", L), ("p_sh_classic", s.mean(axis=0))):
        c = s - centre[None, :]
        out[key] = np.mean(c.max(axis=1)[:, None] - c >= T[None, :], axis=0)
    return out


_STAT = {}


def stat_tests():
    """rell_ref.stat_input() (22 reads of 30 sites, three entries each, brute-force rows) through multinomial_tests at
    STAT_R replicates -> dict of [n] arrays: elw, p_sh, p_sh_classic.  Built once per process."""
    if not _STAT:
        s = stat_input()
        rng = np.random.default_rng(20250311)
        per_query = [multinomial_tests(s["rows"][3 * q:3 * q + 3], rr.STAT_R, rng) for q in range(len(s["reads"]))]
        for key in ("elw", "p_sh", "p_sh_classic"):
            _STAT[key] = np.concatenate([p[key] for p in per_query])
            _STAT[key].setflags(write=False)
    return _STAT
