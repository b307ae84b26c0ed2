"""Vectorised generator of large synthetic references for the large-tree tests and measurements: what
synth.random_tree + synth.simulate_msa do (random-join tree, MSA simulated down it under GTR+G), in time
linear in the tips.  The stock pair costs 24 s at 32 770 tips (O(n^2) pool draws, one eigen-decomposition per
node and category); this one joins the pool level by level (a random perfect matching per level) and draws
the branch lengths from N_LEN values, so every P-matrix is computed once: about 1 s at 32 770 tips.
Pure numpy; data generation only, no likelihood code."""
import numpy as np

from epa_ng_amd import synth

N_LEN = 256


def _lengths(seed, mean_bl=0.05, lo=1e-4, hi=1.0):
    """the N_LEN branch lengths: Exp(mean) quantiles, clamped as synth.random_tree does"""
    p = (np.arange(N_LEN) + 0.5) / N_LEN
    return np.clip(-mean_bl * np.log1p(-p), lo, hi)


def random_join_levels(n_tips, seed):
    """-> (parent int64[n_nodes] (-1 for the three top nodes), len_idx int64[n_nodes], levels: list of
    (parents, kids_a, kids_b) arrays, bottom level first).  Nodes 0 .. n_tips-1 are the tips t0 .. ; every
    level pairs a random half of the pool, the last three nodes hang off the top trifurcation."""
    rng = np.random.RandomState(seed)
    n_nodes = 2 * n_tips - 3
    parent = np.full(n_nodes, -1, np.int64)
    len_idx = rng.randint(0, N_LEN, n_nodes)
    pool = np.arange(n_tips, dtype=np.int64)
    nxt = n_tips
    levels = []
    while len(pool) > 3:
        k = min(len(pool) // 2, len(pool) - 3)
        pool = pool[rng.permutation(len(pool))]
        a, b = pool[0:2 * k:2], pool[1:2 * k:2]
        p = np.arange(nxt, nxt + k, dtype=np.int64)
        nxt += k
        parent[a] = p
        parent[b] = p
        levels.append((p, a, b))
        pool = np.concatenate([pool[2 * k:], p])
    assert nxt == n_nodes
    return parent, len_idx, levels, pool


def newick(n_tips, lengths, len_idx, levels, top):
    txt = [None] * len(len_idx)
    ls = ["%r" % float(v) for v in lengths]
    for i in range(n_tips):
        txt[i] = "t%d:%s" % (i, ls[len_idx[i]])
    for p, a, b in levels:
        for pi, ai, bi in zip(p.tolist(), a.tolist(), b.tolist()):
            txt[pi] = "(%s,%s):%s" % (txt[ai], txt[bi], ls[len_idx[pi]])
            txt[ai] = txt[bi] = None
    return "(" + ",".join(txt[i] for i in top.tolist()) + ");"


def simulate(n_tips, W, lengths, len_idx, levels, top, subst, freqs, cat_rates, seed):
    """tip states uint8[n_tips][W] (0..3), simulated from the top trifurcation down, level by level"""
    rng = np.random.RandomState(seed)
    s = len(freqs)
    Q = synth.rate_matrix(subst, freqs)
    cats = rng.randint(0, len(cat_rates), W)
    # cdf[length value][category][parent state][child state]
    cdf = np.array([[np.cumsum(synth.pmatrix(Q, freqs, t * r), axis=1) for r in cat_rates] for t in lengths])
    states = np.zeros((len(len_idx), W), np.uint8)
    root = rng.choice(s, W, p=np.asarray(freqs) / np.sum(freqs)).astype(np.uint8)

    def draw(kids, parent_states):
        u = rng.random_sample((len(kids), W))
        c = cdf[len_idx[kids][:, None], cats[None, :], parent_states]        # [k][W][s]
        states[kids] = (u[:, :, None] > c).sum(2).clip(0, s - 1).astype(np.uint8)

    draw(top, np.broadcast_to(root, (len(top), W)))
    for p, a, b in reversed(levels):
        draw(a, states[p])
        draw(b, states[p])
    return states[:n_tips]


def _rows(states):
    alpha = np.frombuffer(synth.DNA.encode(), dtype=np.uint8)
    return [r.tobytes().decode() for r in alpha[states]]


def dna_workload(n_tips, W, n_reads, read_len, seeds):
    """the large-tree counterpart of synth.dna_workload (same model, same dictionary)"""
    lengths = _lengths(seeds[0])
    parent, len_idx, levels, top = random_join_levels(n_tips, seeds[0])
    rates = synth.gamma_rates(synth.CFG2_ALPHA)
    seqs = _rows(simulate(n_tips, W, lengths, len_idx, levels, top, synth.CFG2_SUBST, synth.CFG2_FREQS, rates, seeds[1]))
    reads, _ = synth.make_reads(seqs, n_reads, read_len, 0.03, seeds[2])
    return {"newick": newick(n_tips, lengths, len_idx, levels, top), "labels": ["t%d" % i for i in range(n_tips)],
            "seqs": seqs, "reads": reads, "states": 4, "subst": synth.CFG2_SUBST, "freqs": synth.CFG2_FREQS,
            "rates": rates, "weights": np.full(4, 0.25), "depth": len(levels) + 1}


def flat_reads(n_tips, W, n_reads, read_len):
    """the "flat" input: every tip is one random base sequence with each column redrawn uniformly with
    probability 0.1 (RandomState(5)); reads cut from those tips.  Nearly every branch of the (unrelated) tree
    scores alike, so the dynamic rule keeps most of them: the input a per-candidate row pass cannot finish."""
    rng = np.random.RandomState(5)
    base = rng.randint(0, 4, W)
    tips = np.where(rng.random_sample((n_tips, W)) < 0.1, rng.randint(0, 4, (n_tips, W)), base[None, :]).astype(np.uint8)
    seqs = _rows(tips)
    reads, _ = synth.make_reads(seqs, n_reads, read_len, 0.03, 7)
    return seqs, reads
