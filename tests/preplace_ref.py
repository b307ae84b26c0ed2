"""Bit-exact expectation of preplacement rows, independent of the device and of the oracle -- test infrastructure of
tests/test_preplace_order_cpu.py and tests/test_gpu_preplace_edges.py.

The lookup table is read through the public entry point: a read whose window is the single site s with the character
x returns T[b][s][x] itself for every branch (a sum of one term; the pair path adds an exact +0.0).  With the table
extracted by such reads (extraction_reads, table_from_rows), expected_rows() sums the terms of any read in the order
preplace.hip, DESIGN.md and include/epa_dev.h promise -- ((t0 + t1) + (t2 + t3)) per complete group of four sites
counted from the window start, then the remaining singles -- in plain float64 numpy.  Nothing here knows how the table
was built, and no character -> column map is restated: tables are keyed by the code bytes epa.encode_queries produced
for the extraction reads.

Also here: the references and the deterministic read sets of the two test files, the restated dispatch conditions of
launch_preplace (instantiation), and the decoder of the segment-maximum keys (_seg_values).
"""
import functools

import numpy as np

from epa_ng_amd import synth

DNA_PLAIN, DNA_ANY, DNA_RARE = "ACGT", "N", "RYKMSWBDHV"
AA_PLAIN, AA_ANY, AA_AMBIG = synth.AA, "X", "BZ"
DNA_CAP, AA_CAP = 160, 128          # longest window of the single-chunk kernels (CH, CHS of preplace.hip)

# id -> (states, tips, W); B = 2 * tips - 3
REFS = {"N5": (4, 4, 97), "N67": (4, 35, 97), "N125": (4, 64, 385), "P9": (20, 6, 131), "P67": (20, 35, 131)}
_SEEDS = {"N5": 501, "N67": 502, "N125": 503, "P9": 504, "P67": 505}


# ---- the restated order ------------------------------------------------------------------------------------------------
def ordered_sum(terms):
    """terms [n][...] float64 in window order -> [...]: 0.0, + ((t0 + t1) + (t2 + t3)) per complete group of four from
    the window start, + the remaining singles one by one"""
    t = np.asarray(terms, np.float64)
    n = t.shape[0]
    s = np.zeros(t.shape[1:], np.float64)
    for g in range(0, n - n % 4, 4):
        s = s + ((t[g] + t[g + 1]) + (t[g + 2] + t[g + 3]))
    for i in range(n - n % 4, n):
        s = s + t[i]
    return s


def left_to_right_sum(terms):
    """a wrong order, for the CPU file's proof that the inputs tell orders apart: one term after the other"""
    t = np.asarray(terms, np.float64)
    s = np.zeros(t.shape[1:], np.float64)
    for i in range(t.shape[0]):
        s = s + t[i]
    return s


def shifted_sum(terms):
    """another wrong order: the groups of four start one site late (the first site is a single)"""
    t = np.asarray(terms, np.float64)
    n = t.shape[0]
    s = np.zeros(t.shape[1:], np.float64)
    if n:
        s = s + t[0]
    last = 1 + (n - 1) // 4 * 4 if n else 0
    for g in range(1, last, 4):
        s = s + ((t[g] + t[g + 1]) + (t[g + 2] + t[g + 3]))
    for i in range(last, n):
        s = s + t[i]
    return s


# ---- table extraction ----------------------------------------------------------------------------------------------------
def extraction_chars(states):
    return DNA_PLAIN + DNA_ANY + DNA_RARE if states == 4 else AA_PLAIN + AA_ANY + AA_AMBIG


def any_char(states):
    """the character whose column a gap inside a window takes"""
    return DNA_ANY if states == 4 else AA_ANY


def extraction_reads(W, chars):
    """one full-width read per (site, character), site-major: the character at the site, gaps elsewhere"""
    return ["-" * s + ch + "-" * (W - 1 - s) for s in range(W) for ch in chars]


def table_from_rows(rows, codes_full, W, chars, any_ch):
    """rows [W * len(chars)][B]: preplacement of extraction_reads(W, chars); codes_full: their full-width code rows
    -> table [W][code byte][B] (NaN where no extraction read has that byte).  The byte of a gap is read off the
    extraction reads' own rows and takes the column of `any_ch`."""
    rows = np.asarray(rows, np.float64)
    codes_full = np.asarray(codes_full)
    nch = len(chars)
    assert rows.shape[0] == W * nch and codes_full.shape == (W * nch, W)
    site = np.repeat(np.arange(W), nch)
    byte = codes_full[np.arange(W * nch), site]
    off = codes_full[np.arange(W * nch), (site + 1) % W]      # a gap: every other site of an extraction read
    gap = int(off[0])
    assert np.all(off == gap) and not np.any(byte == gap)
    assert all(len(set(byte[ci::nch].tolist())) == 1 for ci in range(nch))       # one byte per character
    assert len(set(byte[:nch].tolist())) == nch                                  # and one character per byte
    table = np.full((W, int(max(byte.max(), gap)) + 1, rows.shape[1]), np.nan)
    table[site, byte] = rows
    table[:, gap] = table[:, int(byte[chars.index(any_ch)])]
    return table


def expected_rows(table, codes_full, win_begin, win_span, order=ordered_sum):
    """table [W][code byte][B], the reads' full-width code rows and windows -> [Q][B], reads of equal span at once"""
    codes_full = np.asarray(codes_full)
    wb = np.asarray(win_begin, np.int64)
    ws = np.asarray(win_span, np.int64)
    out = np.empty((len(wb), table.shape[2]), np.float64)
    for n in np.unique(ws):
        idx = np.nonzero(ws == n)[0]
        cols = wb[idx, None] + np.arange(n)[None, :]                            # [R][n]
        terms = table[cols, codes_full[idx[:, None], cols]]                     # [R][n][B]
        out[idx] = order(np.moveaxis(terms, 1, 0))
    return out


# ---- which kernel a call runs (restates launch_preplace, csrc/preplace.hip) ------------------------------------------
NARROW = "k_preplace_pairs<false, 96, ROWL_NARROW>"
WIDE = "k_preplace_pairs<false, 288, ROWL_PACKED>"
PAIRS_ACC = "k_preplace_pairs<true, 96, ROWL_PACKED>"
SITES = "k_preplace_sites<24, false>"
SITES_ACC = "k_preplace_sites<24, true>"


def generic_instantiation(states, max_span):
    """the kernel of reads with rare IUPAC codes, and of everything under preplace_generic"""
    return "k_preplace<%d, %s>" % (16 if states == 4 else 24, "true" if max_span == 0 or max_span > 160 else "false")


def instantiation(states, Q, W, max_span, generic=False):
    """the instantiation launch_preplace picks for the rare-free reads of a call; max_span 0 = bound open"""
    if generic:
        return generic_instantiation(states, max_span)
    if states == 4:
        if max_span == 0 or max_span > 160:
            return PAIRS_ACC
        return NARROW if Q * 96 >= 1400 * W else WIDE
    assert states == 20
    return SITES_ACC if max_span == 0 or max_span > 128 else SITES


# ---- segment maxima --------------------------------------------------------------------------------------------------------
def _seg_values(keys):
    """order-preserving keys of the segment maxima (include/epa_dev.h) -> doubles; 0 (not written) -> NaN"""
    k = np.asarray(keys, np.uint64)
    pos = (k >> np.uint64(63)) == 1
    u = np.where(pos, k & np.uint64(0x7fffffffffffffff), ~k)
    v = u.view(np.float64).copy()
    v[k == 0] = np.nan
    return v


def segment_maxima(rows):
    """[Q][B] -> [Q][ceil(B / 64)]: the maximum of every 64-branch segment"""
    Q, B = rows.shape
    nseg = (B + 63) // 64
    pad = np.full((Q, nseg * 64), -np.inf)
    pad[:, :B] = rows
    return pad.reshape(Q, nseg, 64).max(axis=2)


# ---- references ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference_case(rid):
    """-> dict(newick, labels, seqs, states, subst, freqs, rates, W, B): random tree, simulated alignment, four gamma
    categories"""
    states, tips, W = REFS[rid]
    seed = _SEEDS[rid]
    subst, freqs = (synth.CFG2_SUBST, synth.CFG2_FREQS) if states == 4 else synth.aa_model(3)
    rates = synth.gamma_rates(0.7)
    root = synth.random_tree(tips, seed)
    labels, seqs = synth.simulate_msa(root, W, subst, freqs, rates, seed + 10)
    return dict(newick=synth.newick(root), labels=labels, seqs=seqs, states=states, subst=subst, freqs=freqs,
                rates=rates, W=W, B=2 * tips - 3)


def cap_of(states):
    return DNA_CAP if states == 4 else AA_CAP


# ---- read sets -------------------------------------------------------------------------------------------------------------
class ReadSet:
    """reads: full-width ASCII rows; windows: the intended (begin, span) of each; rare: which reads carry a rare
    IUPAC code (served by the generic kernel beside the fast path)"""

    def __init__(self, reads, windows, rare):
        self.reads, self.windows, self.rare = list(reads), [tuple(w) for w in windows], np.asarray(rare, bool)
        assert len(self.reads) == len(self.windows) == len(self.rare)

    def __len__(self):
        return len(self.reads)

    @property
    def max_span(self):
        return max(s for _, s in self.windows)

    def take(self, idx):
        return ReadSet([self.reads[i] for i in idx], [self.windows[i] for i in idx], self.rare[list(idx)])

    def first(self, n):
        return self.take(range(n))

    def reversed(self):
        return self.take(range(len(self) - 1, -1, -1))

    def times(self, k):
        """the whole set k times over: the copies of a read lie len(self) apart"""
        return ReadSet(self.reads * k, self.windows * k, np.tile(self.rare, k))


def _dress(case, windows, seed):
    """windows -> ReadSet on the reference: plain characters of a random tip; every third read has N / gap (X / gap)
    at a tenth of its inner sites, first and last site kept plain; DNA: every seventh read has one rare code"""
    rng = np.random.RandomState(seed)
    states, W, seqs = case["states"], case["W"], case["seqs"]
    any_ch = any_char(states)
    reads, rare = [], []
    for i, (b, n) in enumerate(windows):
        assert n >= 1 and 0 <= b and b + n <= W
        frag = list(seqs[rng.randint(len(seqs))][b:b + n])
        if i % 3 == 0 and n > 2:
            k = (n - 2 + 9) // 10
            for j, p in enumerate(rng.choice(np.arange(1, n - 1), size=k, replace=False)):
                frag[p] = any_ch if j % 2 == 0 else "-"
        is_rare = states == 4 and i % 7 == 3
        if is_rare:
            plain = [p for p in range(n) if frag[p] in DNA_PLAIN]
            frag[plain[rng.randint(len(plain))]] = DNA_RARE[rng.randint(len(DNA_RARE))]
        reads.append("-" * b + "".join(frag) + "-" * (W - b - n))
        rare.append(is_rare)
    return ReadSet(reads, windows, rare)


def _between(rng, W, n, parity):
    """a begin of the given parity strictly between 0 and W - n, or None"""
    c = [b for b in range(1, W - n) if b % 2 == parity]
    return c[rng.randint(len(c))] if c else None


@functools.lru_cache(maxsize=None)
def short_set(rid):
    """every span 1 .. min(cap, W), each at begin 0, at W - span, and at one even and one odd begin in between"""
    case = reference_case(rid)
    W, cap = case["W"], cap_of(case["states"])
    rng = np.random.RandomState(_SEEDS[rid] + 1000)
    windows = []
    for n in range(1, min(cap, W) + 1):
        begins = [0, W - n, _between(rng, W, n, 0), _between(rng, W, n, 1)]
        seen = []
        for b in begins:
            if b is not None and b not in seen:
                seen.append(b)
        windows += [(b, n) for b in seen]
    return _dress(case, windows, _SEEDS[rid] + 1001)


LONG_SPANS = {"N125": list(range(159, 164)) + list(range(319, 324)) + [383, 384, 385],
              "P9": list(range(127, 132)), "P67": list(range(127, 132)),
              "N5": list(range(93, 98)), "N67": list(range(93, 98))}


@functools.lru_cache(maxsize=None)
def long_set(rid):
    """LONG_SPANS, each at begin 0, at W - span, and at one begin of the other parity where it fits"""
    case = reference_case(rid)
    W = case["W"]
    windows = []
    for n in LONG_SPANS[rid]:
        begins = [0]
        if W - n not in begins:
            begins.append(W - n)
        if all(b % 2 == 0 for b in begins) and W - n >= 1:
            begins.append(1)
        windows += [(b, n) for b in begins]
    return _dress(case, windows, _SEEDS[rid] + 1002)


@functools.lru_cache(maxsize=None)
def sparse_set(rid):
    """40 reads of span 5 .. 20 whose starts lie only in [0, 8) and [W - 28, W - 20), both parities in each cluster:
    the groups of the 96- / 288-site buckets in between stay empty"""
    case = reference_case(rid)
    W = case["W"]
    rng = np.random.RandomState(_SEEDS[rid] + 1003)
    windows = []
    for i in range(40):
        base = 0 if i % 2 == 0 else W - 28
        windows.append((base + (i // 2) % 8, int(rng.randint(5, 21))))
    assert {b % 2 for b, _ in windows if b < 8} == {0, 1} == {b % 2 for b, _ in windows if b >= 8}
    return _dress(case, windows, _SEEDS[rid] + 1004)


TILED_DISTINCT, TILED_COPIES = 40, 1024 + 1


@functools.lru_cache(maxsize=None)
def tiled_distinct(rid):
    """the first 40 rare-free reads of short"""
    s = short_set(rid)
    return s.take([i for i in range(len(s)) if not s.rare[i]][:TILED_DISTINCT])


def tiled_set(rid):
    """tiled_distinct 1025 times over (41 000 reads): more than 1024 reads on one sort key, >= 40 groups"""
    return tiled_distinct(rid).times(TILED_COPIES)


FEW = (1, 15, 16, 17)


def few_set(rid, n):
    return short_set(rid).first(n)


@functools.lru_cache(maxsize=None)
def extraction_set(rid):
    case = reference_case(rid)
    chars = extraction_chars(case["states"])
    W = case["W"]
    reads = extraction_reads(W, chars)
    rare = [case["states"] == 4 and ch in DNA_RARE for _ in range(W) for ch in chars]
    return ReadSet(reads, [(s, 1) for s in range(W) for _ in chars], rare)


def narrow_factor(rid):
    """how many times over `short` reaches the narrow pair kernel on this reference (Q x 96 >= 1400 x W)"""
    W, n = reference_case(rid)["W"], len(short_set(rid))
    return (1400 * W + 96 * n - 1) // (96 * n)


# ---- the launches of the two test files -------------------------------------------------------------------------------
def set_names(rid):
    names = ["short", "long", "sparse", "tiled", "extraction"] + ["few%d" % n for n in FEW]
    if REFS[rid][0] == 4:
        names.append("short x %d" % narrow_factor(rid))
    return names


def read_set(rid, name):
    """-> (ReadSet of the distinct reads, copies): the set on the device is the distinct reads `copies` times over"""
    if name.startswith("short x"):
        return short_set(rid), narrow_factor(rid)
    if name == "tiled":
        return tiled_distinct(rid), TILED_COPIES
    if name.startswith("few"):
        return few_set(rid, int(name[3:])), 1
    return {"short": short_set, "long": long_set, "sparse": sparse_set, "extraction": extraction_set}[name](rid), 1


def variant_cases(rid):
    """(set name, Q, bound, instantiation the rare-free reads are meant for) of every fast launch on this reference:
    bound 0 = open; a bounded call passes the largest span of the set and exists where that fits a single chunk"""
    states = REFS[rid][0]
    out = []
    for name in set_names(rid):
        rs, copies = read_set(rid, name)
        Q = len(rs) * copies
        out.append((name, Q, 0, PAIRS_ACC if states == 4 else SITES_ACC))
        if rs.max_span > cap_of(states):
            continue
        if states == 20:
            want = SITES
        else:
            want = NARROW if name in ("tiled", "extraction") or name.startswith("short x") else WIDE
        out.append((name, Q, rs.max_span, want))
    return out
