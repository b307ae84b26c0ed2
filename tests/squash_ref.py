"""References for epa_dev_squash (include/epa_dev.h) and for the two texts of epa-ng-amd --squash.  No test lives here.

  materialise(c, clusters)  the clusters (lists of member sample ids of the case c) as an epa_dev_krd input: cluster k's
                            entries are its members' in ascending sample id, each member's in entry order, with
                            weight / |members| -- one division of the original weight.  The result also carries blen and W
                            (the clusters' total weights), which krd_ref.tol reads.
  restate(c)                the clustering loop in plain Python on krd_ref.restate distances of materialised clusters.  Per
                            step: a, b, d, size, the runner-up distance, tol (krd_ref.tol of the winning pair: n a
                            cluster's entry count, W its total weight) and tol_step = tol + the runner-up pair's tol.
  brute_step(name, ma, mb)  the distance of two clusters (member lists) once more through krd_ref.Brute.
  case65()                  krd_ref.case("random40")'s samples among 65: 51 more samples of 1 .. 40 rows each, all entries
                            interleaved -- many merges, slot reuse, a row pass over more than 64 active clusters.
  case(name), run(name)     the six cases by name (edpl_ref.TREES and "case65") and their restated clusterings, cached.
  newick(names, merges, precision), table(names, merges, precision)
                            the two output formats restated; merges = (merge_a, merge_b, merge_dist, merge_size).
"""
import functools
import math

import numpy as np

import edpl_ref as er
import krd_ref as kr

CASES = er.TREES + ("case65",)


def tree_of(name):
    return "random40" if name == "case65" else name


def materialise(c, clusters):
    order = np.argsort(c["seq"], kind="stable")                      # by sample, entry order within
    lo = np.searchsorted(c["seq"][order], np.arange(c["S"] + 1))
    idx, seq, scale = [], [], []
    for k, members in enumerate(clusters):
        for s in sorted(int(m) for m in members):
            e = order[lo[s]:lo[s + 1]]
            idx.append(e)
            seq.append(np.full(len(e), k, np.uint32))
            scale.append(np.full(len(e), float(len(members))))
    idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
    seq = np.concatenate(seq) if seq else np.zeros(0, np.uint32)
    weight = c["weight"][idx] / (np.concatenate(scale) if scale else np.zeros(0))
    W = np.array([math.fsum(weight[seq == k]) for k in range(len(clusters))])
    return dict(branch=c["branch"][idx], seq=seq, distal=c["distal"][idx], weight=weight, S=len(clusters), blen=c["blen"], W=W)


def _distances(c, clusters, pairs):
    """-> (krd_ref.restate's values for the pairs (positions in `clusters`), their tol)"""
    m = materialise(c, clusters)
    d = kr.restate(c["prox"], c["dist"], c["blen"], m["branch"], m["seq"], m["distal"], m["weight"], m["S"], pairs)[0]
    return {p: float(d[p]) for p in pairs}, {p: kr.tol(m, *p) for p in pairs}


def argmin(D):
    """D: {(id_a, id_b) with id_a < id_b: distance} -> the pair at the smallest distance under <, ties to the smallest a,
    then the smallest b"""
    best = None
    for p in sorted(D):
        if best is None or D[p] < D[best]:
            best = p
    return best


def restate(c):
    """-> (steps, members): steps[t] = dict(a, b, d, size, runner, tol, tol_step); members[id] = sorted sample ids"""
    S = c["S"]
    members = {s: [s] for s in range(S)}
    ids = list(range(S))
    every = [(a, b) for a in range(S) for b in range(a + 1, S)]
    D, T = _distances(c, [members[i] for i in ids], every)
    steps = []
    for t in range(S - 1):
        a, b = argmin(D)
        rest = [p for p in D if p != (a, b)]
        second = min(rest, key=lambda p: D[p]) if rest else None
        new = S + t
        members[new] = sorted(members[a] + members[b])
        steps.append(dict(a=a, b=b, d=D[(a, b)], size=len(members[new]), runner=D[second] if rest else math.inf,
                          tol=T[(a, b)], tol_step=T[(a, b)] + (T[second] if rest else 0.0)))
        ids = [i for i in ids if i not in (a, b)]
        D = {p: v for p, v in D.items() if a not in p and b not in p}
        T = {p: v for p, v in T.items() if p in D}
        if ids:
            d, tl = _distances(c, [members[new]] + [members[i] for i in ids], [(0, k + 1) for k in range(len(ids))])
            for k, i in enumerate(ids):
                D[(i, new)], T[(i, new)] = d[(0, k + 1)], tl[(0, k + 1)]
        ids.append(new)
    return steps, members


def brute_step(name, ma, mb):
    c = case(name)
    bt = kr.brute_of(tree_of(name))
    m = materialise(c, [ma, mb])
    smp = [bt.sample(("squash", name, tuple(mem)), m["branch"][m["seq"] == k], m["distal"][m["seq"] == k], m["weight"][m["seq"] == k])
           for k, mem in enumerate((ma, mb))]
    return bt.pair(*smp)


@functools.lru_cache(maxsize=None)
def case65(seed=5):
    c = kr.case("random40")
    S0, B = c["S"], len(c["blen"])
    rng = np.random.RandomState(seed)
    rows = rng.randint(1, 41, size=65 - S0)
    more = dict(branch=[], seq=[], distal=[], weight=[])
    for k, r in enumerate(rows):
        b = rng.randint(B, size=r)
        more["branch"] += list(b)
        more["seq"] += [S0 + k] * r
        more["distal"] += list(rng.uniform(size=r) * c["blen"][b])
        more["weight"] += list(rng.dirichlet(np.ones(r)))
    n_more, n0 = len(more["seq"]), len(c["seq"])
    shuffle = rng.permutation(n_more)
    # a merge that keeps the order of the 40-tip case's own entries
    mine = np.zeros(n0 + n_more, bool)
    mine[np.sort(rng.choice(n0 + n_more, n0, replace=False))] = True
    out = {}
    for k in ("branch", "seq", "distal", "weight"):
        col = np.zeros(n0 + n_more, np.float64 if k in ("distal", "weight") else np.uint32)
        col[mine], col[~mine] = c[k], np.asarray(more[k])[shuffle]
        col.setflags(write=False)
        out[k] = col
    out.update(S=65, prox=c["prox"], dist=c["dist"], blen=c["blen"], names=list(c["names"]) + ["x%d" % k for k in range(65 - S0)])
    out["W"] = np.array([math.fsum(out["weight"][out["seq"] == s]) for s in range(65)])
    return out


def case(name):
    return case65() if name == "case65" else kr.case(name)


@functools.lru_cache(maxsize=None)
def run(name):
    return restate(case(name))


# ---- the texts of --squash

def label(names, i):
    return names[i] if i < len(names) else "cluster%d" % (i - len(names))


def table(names, merges, precision):
    a, b, d, size = merges
    lines = ["step\ta\tb\tdistance\tsize"]
    for t in range(len(a)):
        lines.append("%d\t%s\t%s\t%.*f\t%d" % (t, label(names, int(a[t])), label(names, int(b[t])), precision, float(d[t]), int(size[t])))
    return "\n".join(lines) + "\n"


def newick(names, merges, precision):
    a, b, d, _ = merges
    S = len(names)

    def height(i):
        return 0.0 if i < S else float(d[i - S]) / 2

    text = {i: names[i] for i in range(S)}
    for t in range(len(a)):
        me = S + t
        text[me] = "(%s)%s" % (",".join("%s:%.*f" % (text.pop(int(k)), precision, height(me) - height(int(k))) for k in (a[t], b[t])),
                               label(names, me))
    return text[2 * S - 2] + ";\n"
