"""Pure-numpy restatement of what epa_dev_rell_au specifies (include/epa_dev.h): the multiscale RELL replicates and
the fit that turns an entry's win counts into the p-value of the approximately unbiased test.  No code of the product:
the generator is rell_ref's restatement, the rest is written out from the header.

  scales      per mille of the span; the default 500, 600, ..., 1400
  draw count  n'_s = max(1, (n_q * scale_pm[s] + 500) // 1000), 0 for n_q = 0
  draws       replicate r of scale s: draw d = output word d % 4 of counter (d / 4, ((s + 1) << 20) | r, t low, t high);
              site j = (word * n_q) >> 32
  score       0.0, then one fp64 add per draw in draw order; winner as rell_ref
  fit         usable scales 0 < count < R; at least 3 of them with at least 2 distinct n': z = -ndtri(p), a = sqrt(n' /
              n_q), b = 1 / a, w = phi(z)^2 / (p (1 - p)); (d, c) from the 2 x 2 normal equations, the five sums in scale
              order; p_au = ndtr(c - d)
  fallback    count / R at the scale nearest 1000 (ties to the smaller index), fit (nan, nan)

au_fit does this in float64 with scipy's ndtri / ndtr, au_fit_mp in mpmath at 50 digits; and a second version of the
replicates on numpy's own generator (multinomial site counts at n'_s draws) for the statistical checks.
"""
import numpy as np

import rell_ref as rr
from rell_ref import MASK, philox4x32_10

DEFAULT_SCALES = (500, 600, 700, 800, 900, 1000, 1100, 1200, 1300, 1400)
# e: the largest |au_fit - au_fit_mp| over p_au, d and c on fit_error_set(), measured 3.15e-14 (p_au 1.67e-14, d 3.15e-14,
# c 1.54e-14; tests/test_rell_au_cpu.py::test_fit_error checks that it still holds)
AU_E = 3.2e-14


def draw_counts(n_q, scale_pm=DEFAULT_SCALES):
    """-> list of n'_s, python integers"""
    n_q = int(n_q)
    return [0 if n_q == 0 else max(1, (n_q * int(pm) + 500) // 1000) for pm in scale_pm]


def ms_draws(n_q, n_draw, R, s, stream_id, seed):
    """-> int64 [R][n_draw]: the site every draw of every replicate of scale index s takes"""
    if n_draw == 0:
        return np.zeros((R, 0), np.int64)
    t, seed = int(stream_id), int(seed)
    blocks = (n_draw + 3) // 4
    word1 = (np.uint64((s + 1) << 20) | np.arange(R, dtype=np.uint64))[:, None]
    ctr = (np.arange(blocks, dtype=np.uint64)[None, :], word1, t & MASK, (t >> 32) & MASK)
    words = np.stack(philox4x32_10(ctr, (seed & MASK, (seed >> 32) & MASK)), axis=2).reshape(R, 4 * blocks)[:, :n_draw]
    return ((words * np.uint64(n_q)) >> np.uint64(32)).astype(np.int64)


def ms_counts(rows_by_entry, spans, groups, stream_ids, R, seed, branch_ids, scale_pm=DEFAULT_SCALES):
    """the arguments of rell_ref.rell_counts and the scales -> int64 [S][n]: the replicates every entry wins at every scale"""
    rows = np.asarray(rows_by_entry, np.float64)
    counts = np.zeros((len(scale_pm), len(rows)), np.int64)
    for q, members in groups.items():
        members = sorted(int(i) for i in members)
        n_q = int(spans[q])
        sub = rows[members][:, :n_q]
        branch = np.array([int(branch_ids[i]) for i in members], np.int64)
        for s, n_draw in enumerate(draw_counts(n_q, scale_pm)):
            j = ms_draws(n_q, n_draw, R, s, stream_ids[q], seed)
            score = np.zeros((R, len(members)))
            for d in range(n_draw):                    # one add per draw, in draw order
                score += sub[:, j[:, d]].T
            tied = score == score.max(axis=1)[:, None]
            best = np.argmin(np.where(tied, branch[None, :], np.iinfo(np.int64).max), axis=1)   # argmin: the first minimum
            counts[s, members] += np.bincount(best, minlength=len(members))
    return counts


def usable_scales(p, n_draws):
    """p [S] proportions -> the indices of the usable scales if the fit applies (3 or more, 2 or more distinct n'), else None"""
    use = [s for s in range(len(p)) if 0.0 < p[s] < 1.0]
    if len(use) >= 3 and len({int(n_draws[s]) for s in use}) >= 2:
        return use
    return None


def fallback_scale(scale_pm):
    off = [abs(int(pm) - 1000) for pm in scale_pm]
    return off.index(min(off))


def au_fit(counts, n_draws, n_q, R=None, scale_pm=DEFAULT_SCALES):
    """counts [S] of R replicates (R None: `counts` are proportions already), n_draws [S], the span -> (p_au, d, c) in
    float64; the fallback gives (count / R at the scale nearest 1000, nan, nan)"""
    from scipy.special import ndtr, ndtri
    p = np.asarray(counts, np.float64) if R is None else np.asarray(counts, np.float64) / float(R)
    use = usable_scales(p, n_draws)
    if use is None:
        return float(p[fallback_scale(scale_pm)]), float("nan"), float("nan")
    Saa = Sab = Sbb = Saz = Sbz = 0.0
    for s in use:                                      # the five sums in scale order
        ps = float(p[s])
        r = float(n_draws[s]) / float(n_q)
        z = -float(ndtri(ps))
        a = np.sqrt(r)
        b = 1.0 / a
        phi = 0.3989422804014327 * np.exp(-0.5 * z * z)
        w = phi * phi / (ps * (1.0 - ps))
        Saa += w * a * a
        Sab += w * a * b
        Sbb += w * b * b
        Saz += w * a * z
        Sbz += w * b * z
    det = Saa * Sbb - Sab * Sab
    d = (Saz * Sbb - Sbz * Sab) / det
    c = (Sbz * Saa - Saz * Sab) / det
    return float(ndtr(c - d)), float(d), float(c)


def au_fit_mp(counts, n_draws, n_q, R=None, scale_pm=DEFAULT_SCALES, digits=50):
    """au_fit in mpmath at `digits` digits -> (p_au, d, c) as mpf (the fallback: nan for d and c)"""
    import mpmath as mp
    from scipy.special import ndtri
    with mp.workdps(digits):
        p = [mp.mpf(float(x)) if R is None else mp.mpf(int(x)) / int(R) for x in counts]
        use = usable_scales(p, n_draws)
        if use is None:
            return p[fallback_scale(scale_pm)], mp.nan, mp.nan
        Saa = Sab = Sbb = Saz = Sbz = mp.mpf(0)
        for s in use:
            r = mp.mpf(int(n_draws[s])) / int(n_q)
            # Phi^-1 by Newton steps on ncdf from the float64 value: 1e-16 -> 1e-32 -> 1e-64, whatever the start's last
            # bits are (sqrt(2) erfinv(2 p - 1) gives the same digits three times slower)
            x = mp.mpf(float(ndtri(float(p[s]))))
            for _ in range(2):
                x -= (mp.ncdf(x) - p[s]) / mp.npdf(x)
            z = -x
            a = mp.sqrt(r)
            b = 1 / a
            w = mp.npdf(z) ** 2 / (p[s] * (1 - p[s]))
            Saa += w * a * a
            Sab += w * a * b
            Sbb += w * b * b
            Saz += w * a * z
            Sbz += w * b * z
        det = Saa * Sbb - Sab * Sab
        d = (Saz * Sbb - Sbz * Sab) / det
        c = (Sbz * Saa - Saz * Sab) / det
        return mp.ncdf(c - d), d, c


def au_all(counts, spans, seq_ids, R, scale_pm=DEFAULT_SCALES):
    """counts [S][n], spans per query, seq_ids [n] -> (p_au [n], fit [n][2]) by au_fit"""
    counts = np.asarray(counts)
    n = counts.shape[1]
    p_au, fit = np.empty(n), np.empty((n, 2))
    for i in range(n):
        n_q = int(spans[int(seq_ids[i])])
        p_au[i], fit[i, 0], fit[i, 1] = au_fit(counts[:, i], draw_counts(n_q, scale_pm), n_q, R, scale_pm)
    return p_au, fit


def model_proportions(d, c, n_draws, n_q):
    """the bootstrap proportions the model of the fit gives a region of signed distance d and curvature c:
    1 - Phi(d sqrt(r) + c / sqrt(r)), r = n' / n_q"""
    from scipy.special import ndtr
    r = np.asarray(n_draws, np.float64) / float(n_q)
    return ndtr(-(d * np.sqrt(r) + c / np.sqrt(r)))


def fit_error_set(n_vectors=2400, seed=20260114):
    """the fixed set of count vectors the fit's rounding error is measured on: binomial counts around the model for
    spans 4 .. 2000, R in {256, 1000, 4096, 100000}, d in [-2, 2.5], c in [-1, 1], at the default scales; only those on
    which the fit applies -> list of (counts, n_draws, n_q, R)"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n_vectors):
        n_q = int(rng.integers(4, 2001))
        R = (256, 1000, 4096, 100000)[k % 4]
        d, c = rng.uniform(-2.0, 2.5), rng.uniform(-1.0, 1.0)
        n_draws = draw_counts(n_q)
        counts = rng.binomial(R, model_proportions(d, c, n_draws, n_q))
        if usable_scales(counts / float(R), n_draws) is not None:
            out.append((counts, n_draws, n_q, R))
    return out


# ---- the statistical checks (tests/test_rell_au_cpu.py, tests/test_gpu_rell_au.py): rell_ref.stat_input()

def multinomial_ms_proportions(rows, R, rng, scale_pm=DEFAULT_SCALES):
    """rell_ref.multinomial_proportions at every scale: n'_s draws from the n_q sites -> [S][E]"""
    rows = np.asarray(rows, np.float64)
    n_q = rows.shape[1]
    out = []
    for n_draw in draw_counts(n_q, scale_pm):
        w = rng.multinomial(n_draw, np.full(n_q, 1.0 / n_q), size=R)      # [R][n_q]
        out.append(np.bincount(np.argmax(w @ rows.T, axis=1), minlength=len(rows)) / float(R))
    return np.array(out)


_STAT = {}


def stat_ms():
    """rell_ref.stat_input() (22 reads of 30 sites, three entries each, brute-force rows) through
    multinomial_ms_proportions at STAT_R replicates -> float64 [10][n].  Built once per process."""
    if not _STAT:
        s = rr.stat_input()
        rng = np.random.default_rng(20260115)
        cpu = np.concatenate([multinomial_ms_proportions(s["rows"][3 * q:3 * q + 3], rr.STAT_R, rng)
                              for q in range(len(s["reads"]))], axis=1)
        cpu.setflags(write=False)
        _STAT["cpu"] = cpu
    return _STAT["cpu"]
