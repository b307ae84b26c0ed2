"""References for epa_dev_epca (include/epa_dev.h), the samples its tests share and the bounds they are compared within.
No test lives here.

  samples()   S samples that differ along latent gradients, so that the leading eigenvalues are well separated: four
              "communities" of <= 12 random branches each, mixed per sample with weights 1.5 (1 - t), 1.5 t,
              0.6 |sin 3 t| and 0.25 [s % 3 == 0] (each + 0.02, normalised per sample) along t = linspace(0, 1, S); 40
              reads per sample with Dirichlet weights; the entries shuffled.  seed = 7 + B.
  restate()   X, mean and Xc as the header specifies them, from krd_ref.restate's masses (T = clade - edge, W by
              math.fsum); G by math.fsum of the products; numpy.linalg.eigh; components, sign rule and null rule.
  jacobi()    the header's sweep rule in numpy, rotation after rotation.

The bounds.  B branches, S samples, u = 2^-53.
  tol_x(c)        4 krd_ref.mass_tol: X = T - ((W - T) - M) is 2 T + M - W, and each of the four terms is within mass_tol
                  of its exact value (T and M as clade and edge mass are; W is the clade mass of everything).
  tol_g(Xc)       [a][b]: (B + S + 4) u sum_e |Xc_a[e]| |Xc_b[e]|: the dot product's gamma_n bound, which holds for any
                  order of the additions, with or without fused multiply-adds (n = B terms; S + 4 is slack for the
                  reference's own fsum rounding and the first-order form of gamma).
  tol_jac(G, sw)  16 S sw u trace(G).  In every step every element passes one row rotation and one column rotation of a
                  few roundings each (two products, one sum: <= 4 u relative to the 2 x 2 block's norm, twice), there are
                  S - 1 steps per sweep, and the elements are bounded by the trace; the off-diagonal mass left under the
                  threshold (S^2 elements below u max|a_ii|) is far below this.  It bounds |lambda_jacobi - lambda_exact|
                  (Weyl) for the matrix the sweeps started from.
  tol_eig(G, sw, B)  tol_jac + (B + 2) u trace(G), for comparisons that also cross the Gram sum: |G_ab - exact| <=
                  gamma_B sqrt(G_aa G_bb), whose spectral norm is within gamma_B trace(G).
  Eigenvectors    Davis-Kahan: ||u_dev - u_ref||_2 <= 2 sqrt(2) tol / gap_k after the sign fix, gap_k the distance from
                  lambda'_k to its nearest neighbour among all S Gram eigenvalues, tol the spectral-norm bound of the
                  difference of the two matrices.  edge_vec[k] is the eigenvector of C = Xc^T Xc, whose non-zero spectrum
                  is G's (G keeps at least one zero eigenvalue, from the centring, so the gap to C's null space is among
                  G's gaps): the same bound with the same gap applies to it.
  orthonormality  |v_i . v_j - delta_ij| <= 8 tol_eig / sqrt(lambda'_i lambda'_j): v_i . v_j = u_i^T G u_j /
                  sqrt(lambda'_i lambda'_j), and u_i^T G u_j is within a few tol_eig of lambda'_i delta_ij.
  projections     |proj[s][k] - (Xc v_k)[s]| <= 8 tol_eig / sqrt(lambda'_k): Xc v_k = G u_k / sqrt(lambda'_k), and
                  ||G u_k - lambda'_k u_k|| is within a few tol_eig.
"""
import functools
import math

import numpy as np

import edpl_ref as er
import krd_ref as kr

U = 2.0 ** -53
NULL_REL = 2.0 ** -40
MAX_SWEEPS = 30

# name -> (tree, S, K, kind); kind "plain": samples(); "exact": weights k / 1024; "specials": X and G only
CASES = {
    "tips3": ("tips3", 3, 2, "plain"),
    "tips4": ("tips4", 5, 4, "plain"),
    "random40_s2": ("random40", 2, 1, "plain"),
    "random40_s3": ("random40", 3, 2, "plain"),
    "random40_s17": ("random40", 17, 5, "plain"),
    "ladder600": ("ladder600", 33, 5, "plain"),
    "random512z": ("random512z", 65, 5, "plain"),
    "exact": ("random40", 32, 5, "exact"),
    "specials": ("random40", 17, 0, "specials"),
}
COMPONENT_CASES = [k for k, v in CASES.items() if v[3] != "specials"]


def samples(prox, dist, blen, S, seed, reads=40, exact=False):
    rng = np.random.RandomState(seed)
    B = len(blen)
    K = 4
    comm = [rng.choice(B, size=min(B, 12), replace=False) for _ in range(K)]
    t = np.linspace(0, 1, S)
    mix = np.stack([1.5 * (1 - t), 1.5 * t, 0.6 * np.abs(np.sin(3 * t)), 0.25 * (np.arange(S) % 3 == 0)], 1) + 0.02
    mix /= mix.sum(1, keepdims=True)
    br, sq, dl, wt = [], [], [], []
    for s in range(S):
        ks = rng.choice(K, size=reads, p=mix[s])
        w = rng.multinomial(1024, np.ones(reads) / reads) / 1024.0 if exact else rng.dirichlet(np.ones(reads))
        for k, wi in zip(ks, w):
            b = int(rng.choice(comm[k]))
            br.append(b)
            sq.append(s)
            dl.append(rng.uniform() * blen[b])
            wt.append(wi)
    o = rng.permutation(len(br))
    return (np.array(br, np.uint32)[o], np.array(sq, np.uint32)[o], np.array(dl)[o], np.array(wt)[o])


def excluded(prox, dist, blen):
    size = np.array(kr.preorder(prox, dist, blen)["size"])
    return (size == 1) | (size == len(blen))


def centre(X):
    """mean and Xc in the header's order: (0.0 + X[0] + ... + X[S-1]) / S, then X - mean"""
    acc = np.zeros(X.shape[1])
    for s in range(X.shape[0]):
        acc = acc + X[s]
    mean = acc / X.shape[0]
    return mean, X - mean


def gram_fsum(Xc):
    S = Xc.shape[0]
    G = np.zeros((S, S))
    for a in range(S):
        for b in range(a, S):
            G[a, b] = G[b, a] = math.fsum(Xc[a] * Xc[b])
    return G


def sorted_eigh(G):
    """-> lambda' descending, the matching columns"""
    lam, vec = np.linalg.eigh(G)
    return lam[::-1].copy(), vec[:, ::-1].copy()


def gaps(lam):
    """per eigenvalue the distance to its nearest neighbour"""
    d = np.abs(lam[:, None] - lam[None, :])
    np.fill_diagonal(d, np.inf)
    return d.min(1)


def is_null(lam, k):
    return bool(lam[0] <= 0.0 or lam[k] <= NULL_REL * lam[0])


def sign_of(v):
    """+-1 such that the entry with the largest |value| is positive; equal |value|: the lowest index decides"""
    a = np.abs(v)
    at = int(np.flatnonzero(a == a.max())[0])
    return -1.0 if v[at] < 0.0 else 1.0


def components(Xc, lam, vec, K):
    """-> eigenvalue [K], edge_vec [K][B], proj [S][K], null [K] from the sorted eigenpairs of G"""
    S, B = Xc.shape
    eigenvalue = np.maximum(lam[:K], 0.0) / (S - 1)
    edge_vec, proj, null = np.zeros((K, B)), np.zeros((S, K)), np.zeros(K, bool)
    for k in range(K):
        null[k] = is_null(lam, k)
        if null[k]:
            continue
        acc = np.zeros(B)
        for s in range(S):
            acc = acc + Xc[s] * vec[s, k]
        v = acc / math.sqrt(lam[k])
        sg = sign_of(v)
        edge_vec[k] = sg * v
        proj[:, k] = sg * math.sqrt(lam[k]) * vec[:, k]
    return eigenvalue, edge_vec, proj, null


def jacobi(G, cap=MAX_SWEEPS):
    """the header's rule -> (the diagonal, the accumulated rotations, sweeps run)"""
    n = G.shape[0]
    A, V = G.copy(), np.eye(n)
    m = n + (n & 1)
    for sw in range(cap):
        thr = U * np.max(np.abs(np.diag(A))) if n else 0.0
        rot = 0
        idx = list(range(m))
        for _ in range(m - 1):
            for i in range(m // 2):
                p, q = sorted((idx[i], idx[m - 1 - i]))
                if q >= n:
                    continue
                apq = A[p, q]
                if not abs(apq) > thr:
                    continue
                rot += 1
                th = (A[q, q] - A[p, p]) / (2 * apq)
                t_ = (1.0 if th >= 0 else -1.0) / (abs(th) + math.sqrt(th * th + 1))
                c = 1 / math.sqrt(t_ * t_ + 1)
                s_ = t_ * c
                Ap, Aq = A[:, p].copy(), A[:, q].copy()
                A[:, p], A[:, q] = c * Ap - s_ * Aq, s_ * Ap + c * Aq
                Ap, Aq = A[p, :].copy(), A[q, :].copy()
                A[p, :], A[q, :] = c * Ap - s_ * Aq, s_ * Ap + c * Aq
                Vp, Vq = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = c * Vp - s_ * Vq, s_ * Vp + c * Vq
            idx = [idx[0]] + [idx[-1]] + idx[1:-1]
        if rot == 0:
            return np.diag(A).copy(), V, sw + 1
    return np.diag(A).copy(), V, cap


def sorted_jacobi(G):
    """-> lambda' descending (equal values by ascending column), the matching columns, sweeps"""
    d, V, sw = jacobi(G)
    o = np.argsort(-d, kind="stable")
    return d[o], V[:, o], sw


# ---- the bounds

def tol_x(c):
    return 4.0 * kr.mass_tol(c)


def tol_g(Xc):
    S, B = Xc.shape
    a = np.abs(Xc)
    return (B + S + 4) * U * (a @ a.T)


def tol_jac(G, sweeps):
    return 16.0 * G.shape[0] * sweeps * U * float(np.trace(G))


def tol_eig(G, sweeps, B):
    return tol_jac(G, sweeps) + (B + 2) * U * float(np.trace(G))


def davis_kahan(tol, gap):
    return 2.0 * math.sqrt(2.0) * tol / gap if gap > 0 else np.inf


# ---- the three texts of epa-ng-amd --epca

def texts(names, eigenvalue, total_var, edge_vec, proj, precision):
    """-> (epca_eigenvalues.tsv, epca_projection.tsv, epca_edges.tsv)"""
    K, total = len(eigenvalue), float(np.ravel(total_var)[0])
    edge_vec, proj = np.asarray(edge_vec, np.float64).reshape(K, -1), np.asarray(proj, np.float64).reshape(len(names), K)
    pcs = "".join("\tpc%d" % (k + 1) for k in range(K))
    e = ["component\teigenvalue\tfraction"]
    for k in range(K):
        e.append("%d\t%.*f\t%.*f" % (k + 1, precision, float(eigenvalue[k]), precision,
                                    0.0 if total == 0.0 else float(eigenvalue[k]) / total))
    p = ["sample" + pcs] + [nm + "".join("\t%.*f" % (precision, float(v)) for v in proj[s]) for s, nm in enumerate(names)]
    g = ["edge_num" + pcs] + ["%d" % b + "".join("\t%.*f" % (precision, float(v)) for v in edge_vec[:, b])
                             for b in range(edge_vec.shape[1])]
    return tuple("\n".join(x) + "\n" for x in (e, p, g))


# ---- the cases

def restate(prox, dist, blen, branch, seq, distal, weight, S, K):
    """-> dict: X, mean, Xc, G, lam (all S, descending), vec, eigenvalue, edge_vec, proj, null, total_var, excluded"""
    _, edge, clade = kr.restate(prox, dist, blen, branch, seq, distal, weight, S, pairs=[])
    W = np.array([math.fsum(weight[seq == s]) for s in range(S)])
    T = clade - edge
    X = T - ((W[:, None] - T) - edge)
    ex = excluded(prox, dist, blen)
    X[:, ex] = 0.0
    mean, Xc = centre(X)
    G = gram_fsum(Xc)
    lam, vec = sorted_eigh(G)
    out = dict(X=X, mean=mean, Xc=Xc, G=G, lam=lam, vec=vec, excluded=ex, W=W)
    acc = 0.0
    for i in range(S):
        acc = acc + G[i, i]
    out["total_var"] = acc / (S - 1)
    if K:
        out["eigenvalue"], out["edge_vec"], out["proj"], out["null"] = components(Xc, lam, vec, K)
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    tree, S, K, kind = CASES[name]
    prox, dist, blen = er.tree(tree)
    B = len(blen)
    branch, seq, distal, weight = samples(prox, dist, blen, S, 7 + B, exact=kind == "exact")
    if kind == "specials":                 # sample 0 empty, sample 1 with a total of 0.7
        keep = seq != 0
        branch, seq, distal, weight = branch[keep], seq[keep], distal[keep], weight[keep].copy()
        weight[seq == 1] *= 0.7
    c = dict(name=name, tree=tree, prox=prox, dist=dist, blen=blen, branch=branch, seq=seq, distal=distal, weight=weight, S=S, K=K,
             kind=kind)
    c.update(restate(prox, dist, blen, branch, seq, distal, weight, S, K))
    for k, v in c.items():
        if isinstance(v, np.ndarray) and k not in ("prox", "dist", "blen"):      # the tree's arrays are edpl_ref's
            v.setflags(write=False)
    return c
