"""Pure-numpy restatement of the RELL resampling that epa_dev_rell_support specifies (include/epa_dev.h), and the
brute-force site rows to feed it with.  No code of the product: the generator, the draws, the score and the tie rule
are written out from the specification.

  generator  Philox4x32-10, Random123 constants, key = (seed low word, seed high word)
  draws      replicate r of a query with stream id t and span n_q: draw d = output word d % 4 of counter
             (d / 4, r, t low word, t high word); site j = (word * n_q) >> 32
  score      0.0, then one fp64 add per draw in draw order (no centring, no reassociation)
  winner     largest score; ties to the smaller branch id, then to the smaller entry index
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcastable) or ints, key: two ints -> four uint64 arrays holding 32-bit words"""
    c = [np.asarray(x, np.uint64) & np.uint64(MASK) for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def draws(n_q, R, stream_id, seed):
    """-> int64 [R][n_q]: the site every draw of every replicate takes"""
    if n_q == 0:
        return np.zeros((R, 0), np.int64)
    t, seed = int(stream_id), int(seed)
    blocks = (n_q + 3) // 4
    ctr = (np.arange(blocks, dtype=np.uint64)[None, :], np.arange(R, dtype=np.uint64)[:, None], t & MASK, (t >> 32) & MASK)
    words = np.stack(philox4x32_10(ctr, (seed & MASK, (seed >> 32) & MASK)), axis=2).reshape(R, 4 * blocks)[:, :n_q]
    return ((words * np.uint64(n_q)) >> np.uint64(32)).astype(np.int64)


def rell_counts(rows_by_entry, spans, groups, stream_ids, R, seed, branch_ids):
    """rows_by_entry [n][>= span]: site values per entry; spans[q], stream_ids[q] per query; groups: {q: entry
    indices}; branch_ids [n] -> int64 [n]: the replicates every entry wins"""
    rows = np.asarray(rows_by_entry, np.float64)
    counts = np.zeros(len(rows), np.int64)
    for q, members in groups.items():
        members = sorted(int(i) for i in members)
        n_q = int(spans[q])
        j = draws(n_q, R, stream_ids[q], seed)
        score = np.zeros((R, len(members)))
        sub = rows[members][:, :n_q]
        for d in range(n_q):                       # one add per draw, in draw order
            score += sub[:, j[:, d]].T
        # the winner: the largest score, ties to the smaller branch id, then to the smaller entry index
        branch = np.array([int(branch_ids[i]) for i in members], np.int64)
        tied = score == score.max(axis=1)[:, None]
        best = np.argmin(np.where(tied, branch[None, :], np.iinfo(np.int64).max), axis=1)   # argmin: the first minimum
        counts[members] += np.bincount(best, minlength=len(members))
    return counts


def group_by_query(seq_ids):
    g = {}
    for i, q in enumerate(seq_ids):
        g.setdefault(int(q), []).append(i)
    return g


def multinomial_proportions(rows, R, rng):
    """plain resampling of one query's rows [E][n_q] with numpy's own generator: R replicates, site counts drawn as a
    multinomial, the replicate's score the count-weighted sum -> the proportion of replicates every entry wins (ties
    to the first entry; they do not occur with real-valued rows)"""
    rows = np.asarray(rows, np.float64)
    n_q = rows.shape[1]
    w = rng.multinomial(n_q, np.full(n_q, 1.0 / n_q), size=R)      # [R][n_q]
    win = np.argmax(w @ rows.T, axis=1)
    return np.bincount(win, minlength=len(rows)) / float(R)


def site_rows(bf, reads, branches, seq_ids, pendant, distal):
    """brute-force per-site lnL rows (BruteForce._star over each read's own window) -> (list of 1-d arrays, spans per entry)"""
    from brute_force import valid_range
    out, spans = [], []
    for i, (b, q) in enumerate(zip(branches, seq_ids)):
        read = reads[int(q)]
        lo, n = valid_range(read)
        out.append(np.asarray(bf._star(int(b), bf.tip_vectors(read)[lo:lo + n], float(pendant[i]), float(distal[i]), lo, n)))
        spans.append(n)
    return out, np.array(spans)


# ---- the input of the statistical checks (tests/test_rell_cpu.py, tests/test_gpu_rell.py)

STAT_R = 4096
STAT_SPAN = 30


def adjacent_branches(bf, b):
    """the branches that share a node with branch b"""
    index = {id(x): i for i, x in enumerate(bf.brs)}
    node = bf.brs[b]
    out = [index[id(k)] for k in node.kids] + [index[id(k)] for k in node.parent.kids if k is not node]
    if node.parent is not bf.root:
        out.append(index[id(node.parent)])
    return sorted(out)


def six_sigma(p, q, R):
    """six standard deviations of the difference of two binomial proportions of R trials each, plus one count"""
    m = (np.asarray(p) + np.asarray(q)) / 2.0
    return 6.0 * np.sqrt(2.0 * m * (1.0 - m) / R) + 1.0 / R


_STAT = {}


def stat_input():
    """D5 of tests/brute_cases.py: two 30-site windows (at the first site and in the middle, stepped right off a gap) of each of its reads of
    64 sites and more, every one on its best preplacement branch (BruteForce.preplace) and that branch's two best
    adjacent branches, pendant -ln 0.9, distal at the midpoint -> dict: reads, branch, seq (three entries per read,
    query-major), pendant, distal, rows [n][30] (brute force), cpu (default_rng multinomial proportions, STAT_R
    replicates).  Built once per process."""
    if _STAT:
        return _STAT
    import brute_cases as bc
    from brute_force import valid_range
    from gen_golden import DEFAULT_BL
    c, bf = bc.case("D5"), bc.brute("D5")
    reads = []
    for read in c["reads"]:
        lo, n = valid_range(read)
        if n >= 64:
            for off in (0, (n - STAT_SPAN) // 2):
                # a window must not begin or end on a gap of the read: step right until it spans 30 sites
                while valid_range(bc.windowed(read, lo + off, STAT_SPAN))[1] != STAT_SPAN:
                    off += 1
                reads.append(bc.windowed(read, lo + off, STAT_SPAN))
    table = bf.preplace(reads)
    branch, seq = [], []
    for q in range(len(reads)):
        b = int(np.argmax(table[q]))
        branch += [b] + sorted(adjacent_branches(bf, b), key=lambda x: -table[q, x])[:2]
        seq += [q] * 3
    branch, seq = np.array(branch), np.array(seq)
    pendant, distal = np.full(len(branch), DEFAULT_BL), bf.lengths[branch] / 2.0
    rows, spans = site_rows(bf, reads, branch, seq, pendant, distal)
    assert np.all(spans == STAT_SPAN)
    rows = np.stack(rows)
    rng = np.random.default_rng(20240607)
    cpu = np.concatenate([multinomial_proportions(rows[3 * q:3 * q + 3], STAT_R, rng) for q in range(len(reads))])
    for a in (branch, seq, pendant, distal, rows, cpu):
        a.setflags(write=False)
    _STAT.update(reads=reads, branch=branch, seq=seq, pendant=pendant, distal=distal, rows=rows, cpu=cpu)
    return _STAT
