"""Independent log-space likelihood evaluator (pure numpy / scipy, CPU): a library, not a generator.

It shares no machinery with the kernels or with the C restatement of their design that the parity tests load:
  * P(t) = scipy.linalg.expm(Q r_k t / (1 - pinv)) on the rate matrix itself -- no eigenbasis;
  * partials are normalised per (site, category) and carry one float64 LOG factor per (site, category) -- no 2^256
    scaler counts, no per-site / per-rate modes, no alignment of categories to a site minimum;
  * categories are combined with logsumexp(log w_k + ...), any weights (+R) -- no padded categories;
  * a query is scored by physically forming the three-branch star at the insertion point -- no lookup columns.
From tests/gen_golden.py it takes the alphabet and the tree helpers only (char_vec, parse_newick, branches_postorder,
valid_range, DEFAULT_BL), the rate-matrix construction of its Model and, for optimise() alone, its 1-D solver newton.

Linear time: one downward partial per node and one upward partial per branch, each computed once in the constructor
(gen_golden.reroot_partials recomputes subtrees per branch and gen_golden.prune normalises per site ACROSS categories,
which flushes a category 1e-300 below another one: neither is usable on a 200-level ladder).

+I: log((1 - p) L + p pi_inv); the invariant sites come from the reference tips alone (the intersection of the tips'
state sets is a single state), as in gen_golden.make_case.
"""
import sys

import numpy as np
from scipy.linalg import expm
from scipy.special import logsumexp

from gen_golden import (DEF_OPT_BL, DEFAULT_BL, MAX_BL, Model, branches_postorder, char_vec, newton, parse_newick,
                        valid_range, walk)

_ALPHABET = {4: "ACGTURYSWKMBDHVNOX-?.", 20: "ARNDCQEGHILKMFPSTWYVBZX-?*"}


def _char_table(s):
    t = np.full((256, s), np.nan)
    for ch in _ALPHABET[s]:
        t[ord(ch)] = t[ord(ch.lower())] = char_vec(s, ch)
    return t


class BruteForce:
    def __init__(self, newick, labels, seqs, states, subst, freqs, rates, weights=None, pinv=0.0):
        sys.setrecursionlimit(max(10000, sys.getrecursionlimit()))    # ladder trees: the parser recurses per level
        self.s, self.pinv = states, float(pinv)
        self.m = Model(states, subst, freqs, None, rates=rates, pinv=pinv, weights=weights)
        self.logw = np.log(self.m.weights)
        self.c = len(self.m.rates)
        self.root = parse_newick(newick)
        self.brs = branches_postorder(self.root)
        self.B = len(self.brs)
        self.lengths = np.array([n.length for n in self.brs])
        self.W = len(seqs[0])
        self._chars = _char_table(states)
        self._P = {}
        by_label = dict(zip(labels, seqs))
        tips = {id(n): self.tip_vectors(by_label[n.label]) for n in walk(self.root) if not n.kids}
        # +I: sites on which the reference tips' state sets intersect in exactly one state
        inter = np.ones((self.W, states), bool)
        for v in tips.values():
            inter &= v > 0
        self.invariant_state = np.where(inter.sum(1) == 1, inter.argmax(1), -1)
        with np.errstate(divide="ignore"):
            self.log_cinv = np.where(self.invariant_state >= 0,
                                     np.log(self.pinv * self.m.freqs[np.maximum(self.invariant_state, 0)]), -np.inf)
        self._partials(tips)

    # ---------------------------------------------------------------- pieces
    def _expm(self, t):
        return np.stack([expm(self.m.Q * (r * t / (1.0 - self.pinv))) for r in self.m.rates])

    def P(self, t):
        """[c][i][j] transition matrices of a branch of the tree (kept: ladders repeat one length)"""
        t = float(t)
        if t not in self._P:
            self._P[t] = self._expm(t)
        return self._P[t]

    def tip_vectors(self, seq):
        """[W][s] 0/1 state sets of a sequence"""
        v = self._chars[np.frombuffer(seq.encode(), np.uint8)]
        if np.isnan(v).any():
            raise ValueError("character outside the alphabet")
        return v

    @staticmethod
    def _normalise(acc):
        """[W][c][s] -> (the same with maximum 1 per (site, category), log factor [W][c])"""
        mx = acc.max(axis=2)
        return acc / mx[:, :, None], np.log(mx)

    @staticmethod
    def _push(P, part):
        """partial at the far end of a branch -> partial at its near end"""
        return np.einsum("cij,wcj->wci", P, part)

    def _partials(self, tips):
        order = list(walk(self.root))               # post-order: children first
        zero = np.zeros((self.W, self.c))
        down, pushed = {}, {}                       # id(node) -> (partial [W][c][s], log factor [W][c])
        for n in order:
            if not n.kids:
                down[id(n)] = (np.repeat(tips[id(n)][:, None, :], self.c, 1), zero)
            else:
                acc, lf = 1.0, 0.0
                for k in n.kids:
                    acc, lf = acc * pushed[id(k)][0], lf + pushed[id(k)][1]
                acc, l2 = self._normalise(acc)
                down[id(n)] = (acc, lf + l2)
            if n is not self.root:
                pushed[id(n)] = (self._push(self.P(n.length), down[id(n)][0]), down[id(n)][1])
        up, up_pushed = {}, {}                      # the rest of the tree seen from the upper end of n's branch
        for n in reversed(order):                   # parents first
            if n is self.root:
                continue
            par = n.parent
            acc, lf = 1.0, 0.0
            for k in par.kids:
                if k is not n:
                    acc, lf = acc * pushed[id(k)][0], lf + pushed[id(k)][1]
            if par is not self.root:
                acc, lf = acc * up_pushed[id(par)][0], lf + up_pushed[id(par)][1]
            acc, l2 = self._normalise(acc)
            up[id(n)] = (acc, lf + l2)
            if n.kids:
                up_pushed[id(n)] = (self._push(self.P(n.length), acc), lf + l2)
        self.down = [down[id(n)] for n in self.brs]
        self.up = [up[id(n)] for n in self.brs]

    def _site_lnl(self, lik, logf, log_cinv):
        """lik [..][W][c] > 0 with log factors [W][c] -> per-site lnL [..][W] (category mix, then +I)"""
        with np.errstate(divide="ignore"):
            l = logsumexp(self.logw + np.log(lik) + logf, axis=-1)
        if self.pinv == 0.0:
            return l
        return np.logaddexp(np.log1p(-self.pinv) + l, log_cinv)

    # ---------------------------------------------------------------- the three quantities
    def tree_lnl(self, branch):
        """lnL of the reference tree evaluated across `branch`"""
        n = self.brs[branch]
        (d, ld), (u, lu) = self.down[branch], self.up[branch]
        lik = np.einsum("i,wci,wci->wc", self.m.freqs, d, self._push(self.P(n.length), u))
        return float(self._site_lnl(lik, ld + lu, self.log_cinv).sum())

    def _star(self, branch, tipv, pendant, distal, lo, n, proximal=None):
        """per-site lnL of query state sets tipv [..][n][s] hung on `branch` over the window [lo, lo + n); proximal
        None: branch length - distal"""
        sl = slice(lo, lo + n)
        (d, ld), (u, lu) = self.down[branch], self.up[branch]
        x = (self.m.freqs * self._push(self._expm(distal), d[sl])
             * self._push(self._expm(self.lengths[branch] - distal if proximal is None else proximal), u[sl]))
        lik = np.einsum("cij,...wj,wci->...wc", self._expm(pendant), tipv, x)
        return self._site_lnl(lik, (ld + lu)[sl], self.log_cinv[sl])

    def preplace(self, queries):
        """-> [Q][B]: every query at every branch midpoint with pendant -ln 0.9, summed over its own window"""
        tipv = np.stack([self.tip_vectors(q) for q in queries])
        mask = np.zeros((len(queries), self.W), bool)
        for i, q in enumerate(queries):
            lo, n = valid_range(q)
            mask[i, lo:lo + n] = True
        out = np.empty((len(queries), self.B))
        for b in range(self.B):
            half = self.lengths[b] / 2.0
            (d, ld), (u, lu) = self.down[b], self.up[b]
            x = self.m.freqs * self._push(self.P(half), d) * self._push(self.P(half), u)
            lik = np.einsum("cij,qwj,wci->qwc", self.P(DEFAULT_BL), tipv, x)
            out[:, b] = np.where(mask, self._site_lnl(lik, ld + lu, self.log_cinv), 0.0).sum(1)
        return out

    def score_at(self, branch, query, pendant, distal, proximal=None):
        """lnL over the query's window at given lengths; distal is measured from the node below the edge, the
        proximal length is original - distal unless given (the star at three free lengths)"""
        lo, n = valid_range(query)
        return float(self._star(branch, self.tip_vectors(query)[lo:lo + n], float(pendant), float(distal), lo, n,
                                None if proximal is None else float(proximal)).sum())

    def score_pairs(self, branches, seq_ids, queries, pendant, distal):
        """score_at over many (branch, query) pairs"""
        return np.array([self.score_at(int(b), queries[int(q)], pendant[i], distal[i])
                         for i, (b, q) in enumerate(zip(branches, seq_ids))])

    # ---------------------------------------------------------------- the optimiser
    def _deriv_logw(self):
        """log category weights as the derivatives see them (a hook for the teeth tests)"""
        return self.logw

    def _deriv_log_cinv(self, sl):
        """log(p pi_inv) per site as the derivatives see it (a hook for the teeth tests)"""
        return self.log_cinv[sl]

    def _derivatives(self, branch, tipv, lo, n, lens, which):
        """-> deriv(t) = (f, f') of -lnL over the window in the length `which` (0 pendant, 1 distal, 2 proximal) of
        the star on `branch`, the two other lengths fixed at lens.  P' = r / (1 - p) Q P and P'' likewise, on the
        rate matrix; per site the categories are combined after subtracting the site's largest log factor; +I
        adds p pi_inv to the site likelihood alone"""
        sl = slice(lo, lo + n)
        (d, ld), (u, lu) = self.down[branch], self.up[branch]
        sides = [np.repeat(tipv[:, None, :], self.c, 1), d[sl], u[sl]]
        other = self.m.freqs * np.prod([self._push(self._expm(lens[j]), sides[j]) for j in range(3) if j != which], 0)
        lf = self._deriv_logw() + (ld + lu)[sl]
        top = lf.max(1)
        e = np.exp(lf - top[:, None])
        with np.errstate(over="ignore"):
            cinv = np.exp(self._deriv_log_cinv(sl) - top) if self.pinv > 0.0 else 0.0
        rq = (self.m.rates / (1.0 - self.pinv))[:, None, None] * self.m.Q

        def deriv(t):
            P0 = self._expm(t)
            P1 = rq @ P0
            P2 = rq @ P1
            l0, l1, l2 = ((e * np.einsum("wci,wci->wc", other, self._push(P, sides[which]))).sum(1) for P in (P0, P1, P2))
            if self.pinv > 0.0:
                l0, l1, l2 = (1.0 - self.pinv) * l0 + cinv, (1.0 - self.pinv) * l1, (1.0 - self.pinv) * l2
            d1 = -l1 / l0
            return float(d1.sum()), float((d1 * d1 - l2 / l0).sum())
        return deriv

    def optimise(self, branch, query, mode="sliding", min_branch=1e-4):
        """Branch-length optimisation of one (branch, query) pair -> dict lnl, pendant, distal, rounds, reverted.

        Shared with the C oracle (oracle/epa_oracle.c) and the kernels: the RECOLLECTED control flow alone --
          sliding  opt_branch_lengths_pplacer (reference src/core/pll/optimize.cpp:60-248) as gen_golden.thorough
                   states it: pendant solve on [MIN, MAX], distal solve on [min(MIN / 2, orig / 2), orig - xtol] with
                   the proximal length orig - distal taken up afterwards, the revert test new - old > new 1e-14 and
                   the 0.1 stop, at most 32 rounds;
          raxml    pllmod_opt_optimize_branch_lengths_local(radius 1) as the project documents it: per round pendant,
                   distal, proximal, pendant on [MIN, MAX]; a length is replaced when the solver moved it by more than
                   1e-10; three independent lengths; the distal is rescaled by orig / (distal + proximal) at the end;
          and the 1-D solver gen_golden.newton (imported, not copied).
        NOT shared: all arithmetic.  f and f' come from Q^k expm(Q r t / (1 - p)) products on this class's normalised
        partials with their per-(site, category) log factors -- no eigenbasis, no sumtable, no scaler counts, no
        padded categories -- and the reported lnL is this class's own score_at at the returned lengths."""
        assert mode in ("sliding", "raxml")
        lo, n = valid_range(query)
        tipv = self.tip_vectors(query)[lo:lo + n]
        orig = float(self.lengths[branch])
        MIN = float(min_branch)
        lens = [DEFAULT_BL, orig / 2.0, orig / 2.0]
        smoothings, rounds, reverted = 32, 0, False
        if mode == "sliding":
            negll = -self.score_at(branch, query, lens[0], lens[1])
            while smoothings:
                old = list(lens)
                xmin, xmax = MIN, MAX_BL
                xguess = lens[0] if xmin <= lens[0] <= xmax else DEF_OPT_BL
                lens[0] = newton(xmin, xguess, xmax, xmin / 10.0, 30, self._derivatives(branch, tipv, lo, n, lens, 0))
                xmin = min(MIN / 2.0, orig / 2.0)
                xtol = xmin / 10.0
                xmax = orig - xtol
                xguess = lens[1] if xmin <= lens[1] <= xmax else orig / 2.0
                lens[1] = newton(xmin, xguess, xmax, xtol, 30, self._derivatives(branch, tipv, lo, n, lens, 1))
                lens[2] = orig - lens[1]                                  # the proximal P was still the old one
                new = -self.score_at(branch, query, lens[0], lens[1])
                rounds += 1
                if new - negll > new * 1e-14:
                    lens, reverted = old, True
                    break
                smoothings -= 1
                if abs(new - negll) < 0.1:
                    smoothings = 0
                negll = new
        else:
            negll = -self.score_at(branch, query, *lens)
            while smoothings:
                for which in (0, 1, 2, 0):
                    xguess = lens[which] if MIN <= lens[which] <= MAX_BL else DEF_OPT_BL
                    r = newton(MIN, xguess, MAX_BL, MIN / 10.0, 30, self._derivatives(branch, tipv, lo, n, lens, which))
                    if np.isfinite(r) and abs(lens[which] - r) > 1e-10:
                        lens[which] = r
                new = -self.score_at(branch, query, *lens)
                rounds += 1
                smoothings -= 1
                if abs(new - negll) < 0.1:
                    smoothings = 0
                negll = new
        return {"lnl": -negll, "pendant": lens[0], "distal": (orig / (lens[1] + lens[2])) * lens[1], "rounds": rounds,
                "reverted": reverted}
