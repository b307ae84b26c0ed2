"""Inputs of the brute-force parity tests (tests/test_brute_force_cpu.py pins the CPU checker on them,
tests/test_gpu_brute_force.py the device): one builder, so both files draw exactly the same trees, alignments, reads
and models.  Plain data generation plus a cache of the BruteForce objects; no likelihood code of the product.

Every configuration is the smallest shape that still reaches its code path:
  D  nucleotides, 12 tips (B = 21), 200 sites, 1 .. 16 free-rate categories with unequal weights, +I on even counts;
     read windows on both sides of every 32-site step of the Newton kernel's wave classes
  A  20 states, 8 tips (B = 13), 260 sites, 1 .. 9 categories (replicated, padded, NC = 8, general kernel)
  S  ladder trees deep enough that every site is rescaled (asserted by the tests), 4 Gamma categories
  L  a window beyond 1536 sites (the long-window kernel)
  X  branch lengths drawn from [1e-8, 20]: the two trees reach 9e-7 and 11.9

OPT_NAMES adds the inputs of the end-point tests (tests/test_endpoints_cpu.py, tests/test_gpu_endpoints.py), which
compare where the branch-length optimiser ENDS with BruteForce.optimise through the fixtures of tests/golden/endpoints:
  T4 / T4I  group D's shape with four unequal categories, pinv 0 / 0.2: the main tuned nucleotide kernel (one wave
            group) in span classes 0, 1, 2, 3 and the half-chunk classes 10, 11
  M / MI    8 tips (B = 13), 1600 sites, four unequal categories, pinv 0 / 0.2, windows on both sides of every step
            between span classes 3 .. 8 (1 / 2 / 4 / 8 waves per pair)
  AL        20 states, 6 tips, 420 sites, four categories, windows of 384, 385 and 420 residues.  A thorough call is
            dispatched by its LONGEST window, so all of AL (420) runs on the lane-per-site kernel with its HBM slab
            under the sliding rule and on the general kernel under --raxml-blo
  AL384     AL's tree and alignment with windows of 258, 383, 384 and 384 residues: the call's longest window is 384,
            the matrix-core kernel's last, under both rules
"""
import functools

import numpy as np

from epa_ng_amd import synth

D_CATS = (1, 2, 3, 5, 6, 7, 9, 13, 16)
D_READS = (1, 3, 30, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 200)
A_CATS = (1, 2, 3, 4, 6, 8, 9)
A_READS = (1, 30, 64, 65, 102, 103, 128, 129, 192, 193, 256, 257)

M_READS = (256, 257, 384, 385, 512, 513, 768, 769, 1024, 1025, 1536)
AL_READS = (384, 384, 385, 385, 420, 420)
AL384_READS = (258, 383, 384, 384)

NAMES = (["D%d" % c for c in D_CATS] + ["A%d" % c for c in A_CATS]
         + ["S4", "S20", "L", "Xlong", "Xshort"])
OPT_NAMES = ("T4", "T4I", "M", "MI", "AL", "AL384") + tuple(NAMES)

AMBIG = {4: "RYKMSWBDHVN-", 20: "BZX-"}


def free_rates(cats, seed):
    """+R-style categories: unequal weights, mean rate 1"""
    rng = np.random.RandomState(seed)
    rates = np.sort(rng.gamma(0.7, 1.5, cats)) + 1e-3
    weights = rng.dirichlet(np.full(cats, 4.0))
    return rates / np.sum(rates * weights), weights


def ladder(n_tips):
    """(...((t0,t1),t2)...) with every length 0.9 and a trifurcation on top: n_tips - 2 levels deep"""
    inner = "(t0:0.9,t1:0.9)"
    for i in range(2, n_tips - 2):
        inner = "(%s:0.9,t%d:0.9)" % (inner, i)
    return "(%s:0.9,t%d:0.9,t%d:0.9);" % (inner, n_tips - 2, n_tips - 1)


def random_seqs(n, W, states, rng):
    alphabet = np.frombuffer((synth.DNA if states == 4 else synth.AA).encode(), np.uint8)
    return [alphabet[rng.randint(0, states, W)].tobytes().decode() for _ in range(n)]


def decorate_tips(seqs, states, rng):
    """six ambiguity / gap characters at random columns of every tip, a 20-column gap run in one tip"""
    W = len(seqs[0])
    out = []
    for sq in seqs:
        sq = list(sq)
        for j in rng.choice(W, 6, replace=False):
            sq[j] = AMBIG[states][rng.randint(len(AMBIG[states]))]
        out.append(sq)
    t, j = rng.randint(len(seqs)), rng.randint(0, W - 20 + 1)
    out[t][j:j + 20] = "-" * 20
    return ["".join(sq) for sq in out]


def decorate_reads(reads, states, rng):
    """every third read: ambiguity codes and an internal gap strictly inside its window (the window's end columns
    stay plain characters, so the window itself does not move)"""
    out = []
    for i, r in enumerate(reads):
        if i % 3 == 1:
            cols = [j for j, ch in enumerate(r) if ch != "-"][1:-1]
            r = list(r)
            if len(cols) >= 8:
                g = rng.randint(0, len(cols) - 3)
                for j in cols[g:g + 3]:
                    r[j] = "-"
                for j in rng.choice(cols, 3, replace=False):
                    r[j] = AMBIG[states][rng.randint(len(AMBIG[states]))]
            elif cols:
                r[cols[len(cols) // 2]] = "-"
            r = "".join(r)
        out.append(r)
    return out


def windowed(seq, lo, n):
    return "-" * lo + seq[lo:lo + n] + "-" * (len(seq) - lo - n)


def _simulated(states, n_tips, W, read_lens, seed, **tree_kw):
    subst, freqs = (synth.CFG2_SUBST, synth.CFG2_FREQS) if states == 4 else synth.aa_model(3)
    root = synth.random_tree(n_tips, seed, **tree_kw)
    labels, clean = synth.simulate_msa(root, W, subst, freqs, synth.gamma_rates(0.7), seed + 1)
    rng = np.random.RandomState(seed + 2)
    reads = []
    for k, rl in enumerate(read_lens):
        reads += synth.make_reads(clean, 1, rl, 0.05, seed + 10 + k, states=states)[0]
    return dict(states=states, subst=subst, freqs=freqs, newick=synth.newick(root), labels=labels,
                seqs=decorate_tips(clean, states, rng), reads=decorate_reads(reads, states, rng))


def _ladder_case(states, n_tips, W, n_full, n_win, win, seed):
    subst, freqs = (synth.CFG2_SUBST, synth.CFG2_FREQS) if states == 4 else synth.aa_model(3)
    rng = np.random.RandomState(seed)
    seqs = decorate_tips(random_seqs(n_tips, W, states, rng), states, rng)
    reads = random_seqs(n_full + n_win, W, states, rng)
    for i in range(n_full, n_full + n_win):
        reads[i] = windowed(reads[i], rng.randint(0, W - win + 1), win)
    return dict(states=states, subst=subst, freqs=freqs, newick=ladder(n_tips), labels=["t%d" % i for i in range(n_tips)],
                seqs=seqs, reads=decorate_reads(reads, states, rng), rates=synth.gamma_rates(0.5),
                weights=np.full(4, 0.25), pinv=0.0)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: states, subst, freqs, newick, labels, seqs, reads, rates, weights, pinv, branch_step (thorough pairs
    on every branch_step-th branch), variants (tuple of dicts: the evaluator settings the device test runs)"""
    plain = dict(device_precompute=True, rate_scalers=False)
    host = dict(device_precompute=False, rate_scalers=False)
    if name[0] in "DA" and name[1:].isdigit():
        cats = int(name[1:])
        if name[0] == "D":
            c = _simulated(4, 12, 200, D_READS, 1000)
            c["pinv"] = 0.2 if cats % 2 == 0 else 0.0
            c["variants"] = (plain,) + ((host,) if cats in (5, 13) else ())
            if cats == 5:
                c["variants"] = (dict(plain, chunk=True), host, dict(plain, blocks=True))
        else:
            c = _simulated(20, 8, 260, A_READS, 2000)
            c["pinv"] = 0.15 if cats in (3, 8) else 0.0
            c["variants"] = (plain,)
            if cats == 4:
                c["variants"] = (dict(plain, chunk=True), dict(plain, options=(("aa_valu", 1),)))
        c["rates"], c["weights"] = free_rates(cats, 100 * c["states"] + cats)
        c["branch_step"] = 1
    elif name == "S4":
        c = _ladder_case(4, 200, 48, 6, 2, 20, 3000)
        c["branch_step"] = 9
        # per-rate scalers exist on the device-side precompute only: the host-CLV path keeps per-site scalers and a
        # context that asks for both is refused (EPA_ERR -8), which the device test asserts instead of a parity check
        c["variants"] = tuple(dict(device_precompute=dp, rate_scalers=rs, **({"refused": -8} if rs and not dp else {}))
                              for rs in (False, True) for dp in (True, False))
    elif name == "S20":
        c = _ladder_case(20, 90, 24, 4, 2, 10, 3100)
        c["branch_step"] = 5
        c["variants"] = tuple(dict(device_precompute=True, rate_scalers=rs) for rs in (False, True))
    elif name == "L":
        c = _simulated(4, 8, 1800, (90, 1536, 1537, 1700), 4000)
        c["rates"], c["weights"] = free_rates(4, 4004)
        c.update(pinv=0.1, branch_step=1, variants=(plain,))
    elif name == "Xlong":
        c = _simulated(4, 9, 130, (3, 3, 3, 3, 65, 65, 65, 65), 5000, mean_bl=3.0, lo=1e-8, hi=20.0)
        c["rates"], c["weights"] = free_rates(4, 5004)
        c.update(pinv=0.0, branch_step=1, variants=(plain,))
    elif name == "Xshort":
        c = _simulated(4, 9, 130, (3, 65), 5100, mean_bl=1e-5, lo=1e-8, hi=1.0)
        c["rates"], c["weights"] = free_rates(7, 5107)
        c.update(pinv=0.35, branch_step=1, variants=(plain,))
    elif name in ("T4", "T4I"):
        c = _simulated(4, 12, 200, D_READS, 1100)
        c["rates"], c["weights"] = free_rates(4, 1104)
        c.update(pinv=0.2 if name == "T4I" else 0.0, branch_step=1, variants=())
    elif name in ("M", "MI"):
        c = _simulated(4, 8, 1600, M_READS, 6000)
        c["rates"], c["weights"] = free_rates(4, 6004)
        c.update(pinv=0.2 if name == "MI" else 0.0, branch_step=1, variants=())
    elif name in ("AL", "AL384"):
        c = _simulated(20, 6, 420, AL_READS if name == "AL" else AL384_READS, 7000)
        c["rates"], c["weights"] = free_rates(4, 7004)
        c.update(pinv=0.0, branch_step=1, variants=())
    else:
        raise KeyError(name)
    c["name"] = name
    return c


@functools.lru_cache(maxsize=None)
def brute(name):
    """the BruteForce of a configuration, built once per process"""
    from brute_force import BruteForce
    c = case(name)
    return BruteForce(c["newick"], c["labels"], c["seqs"], c["states"], c["subst"], c["freqs"], c["rates"],
                      weights=c["weights"], pinv=c["pinv"])


def pair_lists(c, B):
    """(branch ids, read ids) of the configuration's thorough pairs, branch-major"""
    br = np.arange(0, B, c["branch_step"])
    Q = len(c["reads"])
    return np.repeat(br, Q), np.tile(np.arange(Q), len(br))


def variant_ids():
    return [(n, i) for n in NAMES for i in range(len(case(n)["variants"]))]


# ---- end-point tests: evaluator settings per configuration.  A variant is a setting of the DEVICE; the expected end
# points depend on the configuration, the rule ("sliding" / "raxml") and the lower length bound alone.
def opt_variants(name):
    """-> list of dicts: mode, min_branch, and the evaluator settings (device_precompute, rate_scalers, blocks,
    keep_eigenvalues, chunk, options) -- both rules on every configuration, the further settings on T4, A4, S4, S20"""
    base = dict(device_precompute=True, rate_scalers=False, min_branch=1e-4)
    extra = [{}]
    if name == "T4":
        extra += [dict(device_precompute=False), dict(blocks=True), dict(keep_eigenvalues=True),
                  dict(min_branch=1e-6), dict(chunk=True)]
    elif name == "A4":
        extra += [dict(blocks=True), dict(options=(("aa_valu", 1),))]
    elif name in ("S4", "S20"):
        extra += [dict(rate_scalers=True)]
    # aa_valu switches kernels under the sliding rule only: under --raxml-blo it would repeat the plain item
    return [dict(base, mode=mode, **e) for e in extra for mode in ("sliding", "raxml")
            if not (mode == "raxml" and e.get("options"))]


def opt_variant_ids():
    def label(v):
        tags = [k for k in ("blocks", "keep_eigenvalues", "chunk", "rate_scalers") if v.get(k)]
        tags += ["host"] if not v["device_precompute"] else []
        tags += ["min%g" % v["min_branch"]] if v["min_branch"] != 1e-4 else []
        tags += [k for k, _ in v.get("options", ())]
        return "-".join([v["mode"]] + tags)
    return [(n, i, "%s-%s" % (n, label(v))) for n in OPT_NAMES for i, v in enumerate(opt_variants(n))]


def endpoint_key(mode, min_branch):
    return "%s@%g" % (mode, min_branch)
