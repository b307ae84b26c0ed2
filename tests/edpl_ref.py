"""Two independent references for epa_dev_edpl (include/epa_dev.h), and the trees the EDPL tests share.  No test lives here.

  restate()  the specification line for line: rooted at node_prox[0], depth[child] = depth[parent] + length with one add
             per level, the LCA found by walking parent pointers, Python loops in entry order, every product rounded
             before it is added (CPython never fuses).  The device must reach its bits.
  brute()    knows no root.  It builds an adjacency list, splits the two occupied edges at the attachment points and sums
             the lengths along the unique path between the two new nodes.  The split is carried out on the path sums: a
             point at distance a from end u of an edge (u, v) of length L reaches any node x over u or over v, and on a
             tree the way that is not the path runs back across the whole edge, so the path has length
             min(a + path(u, x), (L - a) + path(v, x)); path(u, .) are the sums of the lengths along the unique paths from
             u, accumulated edge by edge on a breadth-first walk.  Two points on one edge are |a_i - a_j| apart.

  tol()      16 (h + k + 2) 2^-53 Dmax, h the height of the tree in edges below node_prox[0], k the rows of the object,
             Dmax the largest root depth.  Derived, not measured: h + 1 roundings go into each of D_i, D_j and twice m;
             a path sum of brute() has at most 2 h roundings; row_dist has k multiply-adds with weights that add up to at
             most 1.  The factor 16 covers the handful of further single roundings (x_i, the two differences and their
             sum, brute's min of two sums).
"""
import functools

import numpy as np


# ---- trees: (node_prox uint32 [B], node_dist uint32 [B], blen float64 [B])

def from_synth(root, flip=3):
    """the tree of synth.random_tree (a trifurcation at the top) with branches numbered in a depth-first walk from the
    top; every `flip`-th branch has its CHILD end as node_prox, the others as node_dist, so both orientations occur"""
    prox, dist, blen = [], [], []
    ids = {id(root): 0}
    stack = [root]
    while stack:
        nd = stack.pop()
        for kid in nd.kids:
            ids[id(kid)] = len(ids)
            b = len(blen)
            up, down = ids[id(nd)], ids[id(kid)]
            if b and b % flip == 0:
                up, down = down, up
            prox.append(up), dist.append(down), blen.append(kid.length)
            stack.append(kid)
    return np.array(prox, np.uint32), np.array(dist, np.uint32), np.array(blen, np.float64)


def caterpillar(n_tips, seed):
    """a ladder: spine nodes s_0 .. s_{n-3}, tips hanging off them (two at each end); branch 0 starts at s_0, so the tree
    is n - 2 levels high as the device roots it"""
    rng = np.random.RandomState(seed)
    n_spine = n_tips - 2
    prox, dist = [], []
    tip = n_spine

    def edge(a, b):
        if len(prox) % 2 and len(prox) > 1:
            a, b = b, a
        prox.append(a), dist.append(b)
    edge(0, tip)
    tip += 1
    edge(0, tip)
    tip += 1
    for s in range(1, n_spine):
        edge(s - 1, s)
        edge(s, tip)
        tip += 1
    edge(n_spine - 1, tip)
    blen = np.clip(rng.exponential(0.05, len(prox)), 1e-4, 1.0)
    assert tip + 1 == 2 * n_tips - 2 and len(prox) == 2 * n_tips - 3 and prox[0] == 0
    return np.array(prox, np.uint32), np.array(dist, np.uint32), blen


# ---- the rooted view restate() works on

def rooted(node_prox, node_dist, blen, root=None):
    """-> dict: parent, pedge (edge to the parent), depth, level (edges below the root) per node; child per branch"""
    B, N = len(blen), len(blen) + 1
    root = int(node_prox[0]) if root is None else int(root)
    adj = [[] for _ in range(N)]
    for b in range(B):
        adj[int(node_prox[b])].append(b)
        adj[int(node_dist[b])].append(b)
    parent, pedge = [-1] * N, [-1] * N
    depth, level = [None] * N, [0] * N
    depth[root] = 0.0
    child = [-1] * B
    todo = [root]
    while todo:
        v = todo.pop()
        for b in adj[v]:
            if b == pedge[v]:
                continue
            w = int(node_dist[b]) if int(node_prox[b]) == v else int(node_prox[b])
            assert depth[w] is None, "not a tree"
            parent[w], pedge[w] = v, b
            depth[w] = depth[v] + float(blen[b])          # one fp64 add per level
            level[w] = level[v] + 1
            child[b] = w
            todo.append(w)
    assert all(d is not None for d in depth), "not connected"
    return dict(parent=parent, pedge=pedge, depth=depth, level=level, child=child, root=root)


def groups(seq, Q):
    """entries of every query in order of appearance"""
    g = [[] for _ in range(Q)]
    for i, q in enumerate(seq):
        g[int(q)].append(i)
    return g


def restate(node_prox, node_dist, blen, branch, seq, distal, weight, Q, root=None):
    """-> (row_dist float64 [n], edpl float64 [Q]) by the header's specification, line for line"""
    t = rooted(node_prox, node_dist, blen, root)
    parent, depth, level, child = t["parent"], t["depth"], t["level"], t["child"]

    @functools.lru_cache(maxsize=None)
    def lca_depth(u, v):
        while level[u] > level[v]:
            u = parent[u]
        while level[v] > level[u]:
            v = parent[v]
        while u != v:
            u, v = parent[u], parent[v]
        return depth[u]

    n = len(branch)
    row_dist, edpl = np.zeros(n), np.zeros(Q)
    for q, idx in enumerate(groups(seq, Q)):
        c = [child[int(branch[i])] for i in idx]
        D = []
        for i, ci in zip(idx, c):
            e = int(branch[i])
            x = float(distal[i]) if ci == int(node_dist[e]) else float(blen[e]) - float(distal[i])
            D.append(depth[ci] - x)
        w = [float(weight[i]) for i in idx]
        total = 0.0
        for a, i in enumerate(idx):
            acc = 0.0
            for b in range(len(idx)):
                m = min(lca_depth(c[a], c[b]), D[a], D[b])
                d = (D[a] - m) + (D[b] - m)
                term = w[b] * d
                acc = acc + term
            row_dist[i] = acc
            term = w[a] * acc
            total = total + term
        edpl[q] = total
    return row_dist, edpl


def brute(node_prox, node_dist, blen, branch, seq, distal, weight, Q):
    """-> (row_dist, edpl) from path lengths on the unrooted tree"""
    node_prox, node_dist, blen = np.asarray(node_prox), np.asarray(node_dist), np.asarray(blen, np.float64)
    B, N = len(blen), len(blen) + 1
    adj = [[] for _ in range(N)]
    for b in range(B):
        u, v = int(node_prox[b]), int(node_dist[b])
        adj[u].append((v, float(blen[b])))
        adj[v].append((u, float(blen[b])))

    @functools.lru_cache(maxsize=None)
    def paths_from(u):
        out = np.full(N, np.nan)
        out[u] = 0.0
        todo = [u]
        while todo:
            v = todo.pop()
            for w, ln in adj[v]:
                if np.isnan(out[w]):
                    out[w] = out[v] + ln
                    todo.append(w)
        assert not np.isnan(out).any()
        return out

    n = len(branch)
    row_dist, edpl = np.zeros(n), np.zeros(Q)
    branch = np.asarray(branch, np.int64)
    distal = np.asarray(distal, np.float64)
    weight = np.asarray(weight, np.float64)
    for q, idx in enumerate(groups(seq, Q)):
        if not idx:
            continue
        idx = np.array(idx)
        e = branch[idx]
        nd, npx = node_dist[e].astype(np.int64), node_prox[e].astype(np.int64)
        a = distal[idx]                      # from the node_dist end
        rest = blen[e] - a                   # from the node_prox end
        w = weight[idx]
        rows = np.zeros(len(idx))
        for k in range(len(idx)):
            to_node = np.minimum(a[k] + paths_from(int(nd[k])), rest[k] + paths_from(int(npx[k])))
            d = np.minimum(to_node[nd] + a, to_node[npx] + rest)
            same = e == e[k]
            d[same] = np.abs(a[same] - a[k])
            rows[k] = float(np.sum(w * d))
        row_dist[idx] = rows
        edpl[q] = float(np.sum(w * rows))
    return row_dist, edpl


def tol(node_prox, node_dist, blen, k):
    t = rooted(node_prox, node_dist, blen)
    return 16.0 * (max(t["level"]) + k + 2) * 2.0 ** -53 * max(t["depth"])


# ---- the objects of the tests: (branch, seq, distal, weight, Q) on a tree, covering what the issue lists

def case_entries(node_prox, node_dist, blen, seed, sizes=(1, 2, 7, 64, 65), big=0):
    """queries in this order: the special objects, an EMPTY query, then one object per size in `sizes` (and of `big` rows
    when asked), rows on random branches at random distal lengths.  Special objects: two rows on one edge in both orders;
    rows at distal 0 and at the full length (points on nodes); an edge and its ancestor edge; edges on both sides of the
    root; all edges at the root; one edge whose child end is node_prox and one whose child end is node_dist; a zero
    weight; weights that add up to 0.7"""
    rng = np.random.RandomState(seed)
    B = len(blen)
    t = rooted(node_prox, node_dist, blen)
    child, pedge, parent, root = t["child"], t["pedge"], t["parent"], t["root"]
    at_root = [b for b in range(B) if root in (int(node_prox[b]), int(node_dist[b]))]
    deep = max(range(B), key=lambda b: t["level"][child[b]])
    above = pedge[parent[child[deep]]] if parent[child[deep]] != root else at_root[0]
    child_is_prox = [b for b in range(B) if child[b] == int(node_prox[b])]
    child_is_dist = [b for b in range(B) if child[b] == int(node_dist[b])]
    objs = []

    def obj(rows, weights=None):
        rows = [(int(b), float(x)) for b, x in rows]
        if weights is None:
            weights = rng.dirichlet(np.ones(len(rows)))
        objs.append((rows, [float(v) for v in weights]))
    b0 = int(rng.randint(B))
    obj([(b0, 0.25 * blen[b0]), (b0, 0.75 * blen[b0])], [0.625, 0.375])
    obj([(b0, 0.75 * blen[b0]), (b0, 0.25 * blen[b0])], [0.375, 0.625])
    obj([(b0, 0.0), (b0, blen[b0]), (deep, 0.0), (deep, blen[deep])])
    obj([(deep, 0.3 * blen[deep]), (above, 0.6 * blen[above])])
    obj([(at_root[0], 0.5 * blen[at_root[0]]), (at_root[-1], 0.5 * blen[at_root[-1]]), (deep, 0.1 * blen[deep])])
    obj([(b, 0.4 * blen[b]) for b in at_root])
    if child_is_prox:
        obj([(child_is_prox[0], 0.2 * blen[child_is_prox[0]]), (child_is_dist[-1], 0.2 * blen[child_is_dist[-1]])])
    obj([(b0, 0.5 * blen[b0]), (deep, 0.5 * blen[deep]), (at_root[0], 0.1 * blen[at_root[0]])], [0.5, 0.0, 0.5])
    obj([(b0, 0.5 * blen[b0]), (deep, 0.5 * blen[deep])], [0.3, 0.4])
    n_special = len(objs)
    objs.append(([], []))                                   # a query with no entry in the middle of the range
    for k in tuple(sizes) + ((big,) if big else ()):
        bs = rng.randint(B, size=k)
        obj([(b, rng.uniform() * blen[b]) for b in bs])
    branch, seq, distal, weight = [], [], [], []
    for q, (rows, ws) in enumerate(objs):
        for (b, x), w in zip(rows, ws):
            branch.append(b), seq.append(q), distal.append(min(x, float(blen[b]))), weight.append(w)
    return dict(branch=np.array(branch, np.uint32), seq=np.array(seq, np.uint32), distal=np.array(distal),
                weight=np.array(weight), Q=len(objs), empty=n_special,
                rows_of=[len(r) for r, _ in objs])


# ---- the trees and objects both test files use, with their references computed once

TREES = ("tips3", "tips4", "ladder600", "random40", "random512z")


@functools.lru_cache(maxsize=None)
def tree(name):
    from epa_ng_amd import synth
    if name == "tips3":
        return from_synth(synth.random_tree(3, 5))
    if name == "tips4":
        return from_synth(synth.random_tree(4, 6))
    if name == "ladder600":
        return caterpillar(600, 7)
    if name == "random40":
        return from_synth(synth.random_tree(40, 71))
    if name == "random512z":          # a tenth of the branches have length 0 before any context is built
        prox, dist, blen = from_synth(synth.random_tree(512, 1))
        blen[np.random.RandomState(9).choice(len(blen), len(blen) // 10, replace=False)] = 0.0
        return prox, dist, blen
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: the tree, its entries (case_entries; the two smallest trees also carry the 1025-row object, whose pairs
    fall on a handful of branches) and both references"""
    prox, dist, blen = tree(name)
    e = case_entries(prox, dist, blen, seed=len(blen), big=1025 if len(blen) <= 5 else 0)
    want_rows, want_edpl = restate(prox, dist, blen, e["branch"], e["seq"], e["distal"], e["weight"], e["Q"])
    brute_rows, brute_edpl = brute(prox, dist, blen, e["branch"], e["seq"], e["distal"], e["weight"], e["Q"])
    for a in (want_rows, want_edpl, brute_rows, brute_edpl):
        a.setflags(write=False)
    tols = np.array([tol(prox, dist, blen, k) for k in e["rows_of"]])
    return dict(e, prox=prox, dist=dist, blen=blen, want_rows=want_rows, want_edpl=want_edpl, brute_rows=brute_rows,
                brute_edpl=brute_edpl, tol_q=tols, tol_rows=tols[e["seq"]])
