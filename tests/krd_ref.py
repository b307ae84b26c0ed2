"""Two independent references for epa_dev_krd (include/epa_dev.h), the samples the KRD tests share and the bound they are
compared within.  No test lives here.

  restate()  the rooted definition in plain Python: branches in a pre-order of the tree rooted at node_prox[0] (the subtree
             of a branch is a range of ranks), per sample M (the weights of a branch's points, added in x order) and P (the
             running sum of M over the ranks), T = P[rank + size - 1] - P[rank], and per branch the two-pointer merge of the
             two samples' points.  The header leaves the order of the operations open, so the device is compared with it
             within tol(), not bit for bit.
  brute()    knows no root order and no prefix sums.  Every branch of positive length is cut at the two samples' points;
             for every piece the weights on the side away from the root are added up with math.fsum, and so are the
             pieces.  Which side a node is on is decided by comparing its path sums from the branch's two ends
             (edpl_ref.brute's way of walking the tree): crossing the branch adds its length.  The path arrays and the
             per-branch side masks are cached across pairs.

  tol(a, b)  8 (B + n_a + n_b + 4) 2^-53 (W_a + W_b) sum(blen).  Derived, not measured: every F is a difference of prefix
             values that carry at most B + n roundings relative to W; it is integrated over at most the whole tree's
             length; the factor 8 covers the handful of single roundings (x, the segment, the product, the sums).
  mass_tol(s)  8 (B + n_s) 2^-53 W_s for edge_mass and clade_mass.
"""
import functools
import math

import numpy as np

import edpl_ref as er


# ---- the rooted view

def preorder(node_prox, node_dist, blen, root=None):
    """-> dict: rank [B] (a pre-order of the branches), size [B] (branches in the subtree of child(b), b included),
    child [B], at_root (the root's branches), root"""
    t = er.rooted(node_prox, node_dist, blen, root)
    B = len(blen)
    kids = [[] for _ in range(B + 1)]
    for b in range(B):
        kids[t["parent"][t["child"][b]]].append(b)
    rank, size = [-1] * B, [0] * B
    count = 0
    stack = [(b, 0) for b in reversed(kids[t["root"]])]
    while stack:
        b, done = stack.pop()
        if done:
            size[b] = count - rank[b]
            continue
        rank[b] = count
        count += 1
        stack.append((b, 1))
        stack.extend((k, 0) for k in reversed(kids[t["child"][b]]))
    assert count == B
    return dict(rank=rank, size=size, child=t["child"], at_root=kids[t["root"]], root=t["root"], level=t["level"])


def child_x(node_dist, blen, child, branch, distal):
    """x_i: the distance from the child end, EDPL's expression"""
    return [float(distal[i]) if child[int(b)] == int(node_dist[int(b)]) else float(blen[int(b)]) - float(distal[i])
            for i, b in enumerate(branch)]


def restate(node_prox, node_dist, blen, branch, seq, distal, weight, S, pairs=None, root=None):
    """-> (krd [S][S] with NaN where the pair was not asked for, edge_mass [S][B], clade_mass [S][B]); pairs: a list of
    (a, b), None = all"""
    B = len(blen)
    p = preorder(node_prox, node_dist, blen, root)
    rank, size = p["rank"], p["size"]
    x = child_x(node_dist, blen, p["child"], branch, distal)
    pts = [[[] for _ in range(B)] for _ in range(S)]          # [sample][rank] -> (x, w) in entry order
    for i in range(len(branch)):
        pts[int(seq[i])][rank[int(branch[i])]].append((x[i], float(weight[i])))
    M, P = np.zeros((S, B)), np.zeros((S, B))
    for s in range(S):
        run = 0.0
        for r in range(B):
            pts[s][r].sort(key=lambda xw: xw[0])              # stable: equal x keep entry order
            m = 0.0
            for _, w in pts[s][r]:
                m = m + w
            M[s, r] = m
            run = run + m
            P[s, r] = run
    len_r = [0.0] * B
    for b in range(B):
        len_r[rank[b]] = float(blen[b])
    size_r = [0] * B
    for b in range(B):
        size_r[rank[b]] = size[b]
    T = np.array([[P[s, r + size_r[r] - 1] - P[s, r] for r in range(B)] for s in range(S)]).reshape(S, B)
    krd = np.full((S, S), np.nan)
    for s in range(S):
        krd[s, s] = 0.0
    for a, b in ([(a, b) for a in range(S) for b in range(a + 1, S)] if pairs is None else pairs):
        total = 0.0
        for r in range(B):
            f = T[a, r] - T[b, r]
            pa, pb = pts[a][r], pts[b][r]
            ia = ib = 0
            xprev = 0.0
            while ia < len(pa) or ib < len(pb):
                if ia < len(pa) and (ib >= len(pb) or pa[ia][0] <= pb[ib][0]):
                    xt, dw = pa[ia][0], pa[ia][1]
                    ia += 1
                else:
                    xt, dw = pb[ib][0], -pb[ib][1]
                    ib += 1
                total = total + abs(f) * (xt - xprev)
                f = f + dw
                xprev = xt
            total = total + abs(f) * (len_r[r] - xprev)
        krd[a, b] = krd[b, a] = total
    edge, clade = np.zeros((S, B)), np.zeros((S, B))
    for b in range(B):
        edge[:, b] = M[:, rank[b]]
        clade[:, b] = T[:, rank[b]] + M[:, rank[b]]
    return krd, edge, clade


# ---- brute(): cached per tree

class Brute:
    def __init__(self, node_prox, node_dist, blen, root=None):
        self.prox, self.dist = np.asarray(node_prox, np.int64), np.asarray(node_dist, np.int64)
        self.blen = np.asarray(blen, np.float64)
        self.B, self.N = len(blen), len(blen) + 1
        self.root = int(node_prox[0]) if root is None else int(root)
        self.adj = [[] for _ in range(self.N)]
        for b in range(self.B):
            u, v = int(self.prox[b]), int(self.dist[b])
            self.adj[u].append((v, float(self.blen[b])))
            self.adj[v].append((u, float(self.blen[b])))
        self._paths, self._side, self._T = {}, {}, {}

    def paths_from(self, u):
        if u not in self._paths:
            out = np.full(self.N, np.nan)
            out[u] = 0.0
            todo = [u]
            while todo:
                v = todo.pop()
                for w, ln in self.adj[v]:
                    if np.isnan(out[w]):
                        out[w] = out[v] + ln
                        todo.append(w)
            self._paths[u] = out
        return self._paths[u]

    def side(self, e):
        """-> (far, mask): the end of e away from the root, and per branch whether it lies beyond that end"""
        if e not in self._side:
            u, v = int(self.prox[e]), int(self.dist[e])
            pu, pv = self.paths_from(u), self.paths_from(v)
            far, near_paths, far_paths = (u, pv, pu) if pu[self.root] > pv[self.root] else (v, pu, pv)
            beyond = far_paths < near_paths                     # nodes: nearer to the far end
            mask = beyond[self.prox] & beyond[self.dist]
            mask[e] = False
            self._side[e] = (far, mask)
        return self._side[e]

    def sample(self, key, branch, distal, weight):
        """per branch of positive length: the sample's mass beyond it, and its own points as (from the far end, w)"""
        if key not in self._T:
            branch = np.asarray(branch, np.int64)
            distal, weight = np.asarray(distal, np.float64), np.asarray(weight, np.float64)
            beyond, own = {}, {}
            for e in range(self.B):
                if not self.blen[e] > 0.0:
                    continue
                far, mask = self.side(e)
                beyond[e] = math.fsum(weight[mask[branch]])
                on = np.flatnonzero(branch == e)
                own[e] = [((float(distal[i]) if far == int(self.dist[e]) else float(self.blen[e]) - float(distal[i])),
                           float(weight[i])) for i in on]
            self._T[key] = (beyond, own)
        return self._T[key]

    def pair(self, sa, sb):
        """sa, sb: what sample() returned"""
        terms = []
        for e in sa[0]:
            L = float(self.blen[e])
            cuts = sorted({0.0, L} | {min(max(x, 0.0), L) for x, _ in sa[1][e]} | {min(max(x, 0.0), L) for x, _ in sb[1][e]})
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                fa = math.fsum([sa[0][e]] + [w for x, w in sa[1][e] if x <= lo])
                fb = math.fsum([sb[0][e]] + [w for x, w in sb[1][e] if x <= lo])
                terms.append(abs(fa - fb) * (hi - lo))
        return math.fsum(terms)


# ---- the samples of the tests

SPECIAL = ("empty", "unit_deep", "unit_b0", "pile300", "ends", "four_at_x", "r2", "r7", "r64", "r65", "r257", "copy65", "w07",
           "zeros")


def make_samples(node_prox, node_dist, blen, seed, every_branch=False):
    """-> dict: branch, seq, distal, weight (one shuffled entry list), S, index (name -> sample id).  The copy of the
    65-row sample holds the same entries in the same relative order."""
    rng = np.random.RandomState(seed)
    B = len(blen)
    p = preorder(node_prox, node_dist, blen)
    deep = max(range(B), key=lambda b: p["level"][p["child"][b]])
    rows = {}

    def rand(k, total=1.0):
        bs = rng.randint(B, size=k)
        return [(int(b), float(rng.uniform() * blen[b]), float(w)) for b, w in zip(bs, total * rng.dirichlet(np.ones(k)))]
    rows["empty"] = []
    rows["unit_deep"] = [(deep, 0.3 * blen[deep], 1.0)]
    rows["unit_b0"] = [(0, 0.6 * blen[0], 1.0)]
    b300 = int(rng.randint(B))
    rows["pile300"] = [(b300, float(rng.uniform() * blen[b300]), float(w)) for w in rng.dirichlet(np.ones(300))]
    b1, b2 = int(rng.randint(B)), deep
    rows["ends"] = [(b1, 0.0, 0.25), (b1, blen[b1], 0.25), (b2, 0.0, 0.25), (b2, blen[b2], 0.25)]
    b4 = int(rng.randint(B))
    rows["four_at_x"] = [(b4, 0.5 * blen[b4], 0.1), (b4, 0.5 * blen[b4], 0.2), (b4, 0.5 * blen[b4], 0.3), (b4, 0.5 * blen[b4], 0.4)]
    for k in (2, 7, 64, 65, 257):
        rows["r%d" % k] = rand(k)
    rows["copy65"] = list(rows["r65"])
    rows["w07"] = rand(9, total=0.7)
    rows["zeros"] = [(b, x, 0.0) for b, x, _ in rand(5)]
    names = list(SPECIAL)
    if every_branch:
        rows["every"] = [(b, float(rng.uniform() * blen[b]), float(w)) for b, w in zip(range(B), rng.dirichlet(np.ones(B)))]
        names.append("every")
    index = {nm: s for s, nm in enumerate(names)}
    flat = [(index[nm], i) for nm in names for i in range(len(rows[nm]))]
    order = rng.permutation(len(flat))
    flat = [flat[i] for i in order]
    # the copy's slots take the original's entries in the original's order of appearance
    seen65 = [i for s, i in flat if s == index["r65"]]
    it = iter(seen65)
    flat = [(s, next(it)) if s == index["copy65"] else (s, i) for s, i in flat]
    branch = np.array([rows[names[s]][i][0] for s, i in flat], np.uint32)
    distal = np.array([min(float(rows[names[s]][i][1]), float(blen[rows[names[s]][i][0]])) for s, i in flat], np.float64)
    weight = np.array([rows[names[s]][i][2] for s, i in flat], np.float64)
    seq = np.array([s for s, _ in flat], np.uint32)
    return dict(branch=branch, seq=seq, distal=distal, weight=weight, S=len(names), index=index, names=names)


def tol(c, a, b):
    n = np.bincount(c["seq"], minlength=c["S"])
    return 8.0 * (len(c["blen"]) + n[a] + n[b] + 4) * 2.0 ** -53 * (c["W"][a] + c["W"][b]) * float(np.sum(c["blen"]))


def mass_tol(c):
    n = np.bincount(c["seq"], minlength=c["S"])
    return (8.0 * (len(c["blen"]) + n) * 2.0 ** -53 * c["W"])[:, None]


def pair_set(c):
    """all pairs where B <= 77; else every pair among the special samples that the issue names, and 24 random pairs"""
    S, ix = c["S"], c["index"]
    every = [(a, b) for a in range(S) for b in range(a + 1, S)]
    if len(c["blen"]) <= 77:
        return every
    want = {tuple(sorted((ix[u], ix[v]))) for u, v in (("empty", "r7"), ("unit_deep", "unit_b0"), ("pile300", "r64"),
                                                       ("ends", "four_at_x"), ("r65", "copy65"), ("w07", "r257"),
                                                       ("zeros", "empty"), ("zeros", "r2"))}
    if "every" in ix:
        want |= {tuple(sorted((ix["every"], ix[v]))) for v in ("r257", "unit_deep", "empty")}
    rest = [p for p in every if p not in want]
    pick = np.random.RandomState(S).choice(len(rest), 24, replace=False)
    return sorted(want | {rest[i] for i in pick})


@functools.lru_cache(maxsize=None)
def brute_of(name):
    return Brute(*er.tree(name))


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: the tree, the samples, the pairs the tests cover, restate's and brute's values for them"""
    prox, dist, blen = er.tree(name)
    c = make_samples(prox, dist, blen, seed=100 + len(blen), every_branch=name == "ladder600")
    c.update(prox=prox, dist=dist, blen=blen)
    c["W"] = np.array([math.fsum(c["weight"][c["seq"] == s]) for s in range(c["S"])])
    c["pairs"] = pair_set(c)
    c["want"], c["want_edge"], c["want_clade"] = restate(prox, dist, blen, c["branch"], c["seq"], c["distal"], c["weight"],
                                                         c["S"], c["pairs"])
    bt = brute_of(name)
    smp = [bt.sample((name, s), c["branch"][c["seq"] == s], c["distal"][c["seq"] == s], c["weight"][c["seq"] == s])
           for s in range(c["S"])]
    c["brute"] = np.full((c["S"], c["S"]), np.nan)
    for a, b in c["pairs"]:
        c["brute"][a, b] = c["brute"][b, a] = bt.pair(smp[a], smp[b])
    c["tol"] = np.array([[tol(c, a, b) for b in range(c["S"])] for a in range(c["S"])])
    for k in ("want", "want_edge", "want_clade", "brute", "tol", "branch", "seq", "distal", "weight"):
        c[k].setflags(write=False)
    return c
