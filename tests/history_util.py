"""Inputs, probe and comparison of tests/test_gpu_call_history.py.

A PROBE is a fixed set of calls on fixed inputs (probe()).  Its answers on a context that has done nothing else are
the expected ones (fresh_probe(), computed once per reference and input form); a test then runs some HISTORY of other
calls on another new context over the same reference, runs the probe there and compares every output bit for bit
(assert_same()).  Data generation is epa_ng_amd.synth's; nothing here evaluates a likelihood."""
import numpy as np

import epa_ng_amd as epa
from epa_ng_amd import hostlib, synth

# window lengths on both sides of every span-class border of the Newton kernels (epa_span_class,
# epa_ng_amd/csrc/epa_dev_internal.hpp): 4 states 64 | 65..96 | 97..128 | 129..160 | 161..192 | 193..256, 20 states 64 | 128 | 192
DNA_SPANS = (1, 3, 37, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 256)
AA_SPANS = (1, 40, 64, 65, 128, 129, 192, 193, 200)
DNA_AMBIG = "RYKMSWBDHV"
AA_AMBIG = "BZX"

# name -> shape.  R4: B = 77 is two 64-branch segments and more branches than the 64 staging slots of the sorted
# selection; W = 260 holds the span classes 0, 10, 1, 11, 2 and 3.  R4B: the same reference in the blocked lookup layout
# with 64-branch blocks (two blocks per chunk body).  R20: 20 states, classes 0 .. 3 (matrix-core and lane-per-site kernel)
SHAPES = {"R4": dict(states=4, tips=40, W=260, blocks=False),
          "R4B": dict(states=4, tips=40, W=260, blocks=True),
          "R20": dict(states=20, tips=10, W=200, blocks=False)}

_REFS = {}


def reference(name):
    """-> dict(ref=hostlib.Reference, seqs, states, W, B, blocks), built once per name (R4 and R4B share theirs)"""
    sh = SHAPES[name]
    key = (sh["states"], sh["tips"], sh["W"])
    if key not in _REFS:
        if sh["states"] == 4:
            w = synth.dna_workload(sh["tips"], sh["W"], 1, 8, (301, 302, 303))
        else:
            w = synth.aa_workload(sh["tips"], sh["W"], 1, 8, (311, 312, 313))
        ref = hostlib.Reference(w["newick"], w["labels"], w["seqs"], states=sh["states"], subst=w["subst"],
                                freqs=w["freqs"], rates=w["rates"])
        assert ref.W == sh["W"] and ref.B == 2 * sh["tips"] - 3
        _REFS[key] = dict(ref=ref, seqs=w["seqs"], states=sh["states"], W=ref.W, B=ref.B)
    return dict(_REFS[key], blocks=sh["blocks"], name=name)


def new_context(name):
    """a context over reference `name` that has served no call yet"""
    r = reference(name)
    ev = r["ref"].evaluator(flags=epa.FLAG_LOOKUP_BLOCKS if r["blocks"] else 0)
    if r["blocks"]:
        ev.set_option("lookup_block", 64)
        assert ev.lookup_mode() == (epa.LOOKUP_BLOCKS, 64)
    return ev


def make_reads(name, spans, seed, marks=True):
    """one aligned ASCII row per entry of `spans`: that many consecutive columns of a random tip with 3 % substitutions,
    '-' elsewhere.  Read i starts on a column of parity i & 1; every fifth read ends at column W - 1.  marks: every
    fourth read (of three sites or more) carries one ambiguity code, every third one an 'N' ('X') or a gap INSIDE its
    window -- never at its ends, so that the encoder's window is the span asked for."""
    r = reference(name)
    W, seqs, states = r["W"], r["seqs"], r["states"]
    alphabet = synth.DNA if states == 4 else synth.AA
    ambig, any_code = (DNA_AMBIG, "N") if states == 4 else (AA_AMBIG, "X")
    rng = np.random.RandomState(seed)
    rows = []
    for i, n in enumerate(spans):
        n = int(n)
        assert 1 <= n <= W
        starts = [s for s in range(W - n + 1) if (s & 1) == (i & 1)] or list(range(W - n + 1))
        start = W - n if i % 5 == 0 else starts[rng.randint(len(starts))]
        tip = seqs[rng.randint(len(seqs))]
        frag = list(tip[start:start + n])
        for k in np.nonzero(rng.random_sample(n) < 0.03)[0]:
            frag[k] = alphabet[rng.randint(len(alphabet))]
        if marks and n >= 3:
            inner = list(range(1, n - 1))
            if i % 4 == 0:
                frag[inner.pop(rng.randint(len(inner)))] = ambig[(i // 4) % len(ambig)]
            if i % 3 == 0 and inner:
                frag[inner[rng.randint(len(inner))]] = any_code if (i // 3) & 1 else "-"
        rows.append("-" * start + "".join(frag) + "-" * (W - start - n))
    return rows


def forms(name, reads):
    """the three query forms of the same reads -> dict: "full" (aligned rows of W codes), "compact" (window rows) and,
    4 states only, "packed" (compact rows in the 4-bit wire format); each (codes, win_begin, win_span)"""
    states = reference(name)["states"]
    out = {"full": epa.encode_queries(states, reads), "compact": epa.encode_queries(states, reads, compact=True)}
    assert np.array_equal(out["full"][1], out["compact"][1]) and np.array_equal(out["full"][2], out["compact"][2])
    if states == 4:
        c, wb, ws = out["compact"]
        out["packed"] = (epa.pack_codes_4bit(c), wb, ws)
    return out


def first_rows(codes, n):
    """the first n code rows of any of the three forms"""
    if isinstance(codes, epa.Packed4):
        return epa.Packed4(np.ascontiguousarray(codes.data[:n]), codes.stride)
    return np.ascontiguousarray(codes[:n])


def head(form, n):
    """the first n reads of one (codes, win_begin, win_span)"""
    codes, wb, ws = form
    return first_rows(codes, n), wb[:n].copy(), ws[:n].copy()


_INPUTS = {}


def inputs(name):
    """the fixed inputs of reference `name` -> dict of forms() dicts:
      probe   48 reads (20 states: 24) over the span list, in ONE chunk (4 states: six classes in one Newton launch)
      big     600 reads with spans up to the longest (H1: grows every scratch buffer)
      small   3 reads of at most 64 sites
      mixed   40 reads over the span list, other reads than the probe's (the histories' everyday chunk)
      short   32 reads of at most 64 sites (one span class: the queued Newton launch runs)
      tiny    30 reads of 1 .. 3 sites (flat table rows: a query selects nearly every branch)
      mid     12 reads of 100 .. 160 sites (4 states: classes 1 and 11 only)
      ten     10 reads of at most 64 sites (H8)"""
    if name in _INPUTS:
        return _INPUTS[name]
    base = {"R4B": "R4"}.get(name, name)
    if base != name:
        _INPUTS[name] = inputs(base)
        return _INPUTS[name]
    spans = DNA_SPANS if reference(name)["states"] == 4 else AA_SPANS
    nprobe = 48 if reference(name)["states"] == 4 else 24
    rng = np.random.RandomState(5)
    sets = {"probe": [spans[i % len(spans)] for i in range(nprobe)],
            "big": [spans[k] for k in rng.randint(0, len(spans), 600)],
            "small": [1, 37, 64],
            "mixed": [spans[(5 * i + 1) % len(spans)] for i in range(40)],
            "short": [int(x) for x in rng.randint(20, 65, 32)],
            "tiny": [1 + i % 3 for i in range(30)],
            "mid": [100, 129, 128, 160, 113, 145, 101, 130, 127, 159, 120, 150],
            "ten": [int(x) for x in rng.randint(30, 65, 10)]}
    out = {}
    for k, (key, sp) in enumerate(sorted(sets.items())):
        out[key] = forms(name, make_reads(name, sp, 900 + k, marks=key not in ("tiny", "ten")))
        assert list(out[key]["full"][2]) == list(sp), key      # the encoder's windows are the spans asked for
    wb, ws = out["probe"]["full"][1:]
    assert {0, 1} <= set((wb & 1).tolist()) and int((wb + ws).max()) == reference(name)["W"]
    _INPUTS[name] = out
    return out


def grid_pairs(B, Q, step=5, seed=7):
    """every step-th pair of the B x Q grid (branch-major numbering) in a fixed shuffled order"""
    idx = np.arange(0, B * Q, step)
    idx = idx[np.random.RandomState(seed).permutation(len(idx))]
    p = np.zeros(len(idx), epa.PAIR_DTYPE)
    p["branch_id"], p["seq_id"] = idx // Q, idx % Q
    return p


def _counters(ev):
    s = ev.last_stats
    return np.array([s["rounds"], s["newton_evals"], s["reverts"]], np.uint64)


def _rows(out, key, pairs, res, ev=None):
    out[key + ".branch_id"] = np.array(pairs["branch_id"])
    out[key + ".seq_id"] = np.array(pairs["seq_id"])
    for f in ("lnl", "pendant_length", "distal_length"):
        out[key + "." + f] = np.array(res[f])
    if ev is not None:
        out[key + ".counters"] = _counters(ev)
    return out


def chunk_rows(pairs, res, ev=None):
    """the rows of one chunk body (place_chunk, or a slot's finish) as a dict of plain arrays"""
    return _rows({}, "place_chunk", pairs, res, ev)


def thorough_rows(ev, pairs, codes, wb, ws):
    return _rows({}, "thorough", pairs, ev.thorough(pairs, codes, wb, ws), ev)


def probe(ev, codes, wb, ws):
    """the probe on (codes, wb, ws) -> dict of arrays: the preplacement table; pairs, lnL, lengths and Newton counters
    of place_chunk (dynamic rule, max_span = 0) and of thorough on grid_pairs(); the pairs of select on the table;
    counts, rows, LWR and counters of place_all on the first 6 reads (filter_max = 7); 4 states: score_at at place_chunk's
    lengths"""
    Q, B = len(wb), ev.B
    out = {"preplace": ev.preplace(codes, wb, ws)}
    pairs, res = ev.place_chunk(codes, wb, ws, max_span=0, max_pairs=Q * B)
    _rows(out, "place_chunk", pairs, res, ev)
    out.update(thorough_rows(ev, grid_pairs(B, Q), codes, wb, ws))
    sel = ev.select(out["preplace"], Q)
    out["select.branch_id"], out["select.seq_id"] = np.array(sel["branch_id"]), np.array(sel["seq_id"])
    pa = ev.place_all(first_rows(codes, 6), wb[:6].copy(), ws[:6].copy(), filter_max=7)
    out["place_all.counts"] = np.array([len(t[0]) for t in pa], np.uint32)
    for k, f in enumerate(("branch_id", "lnl", "pendant_length", "distal_length", "lwr")):
        out["place_all." + f] = np.concatenate([t[k] for t in pa])
    out["place_all.counters"] = _counters(ev)
    if ev.s == 4:
        out["score_at.lnl"] = ev.score_at(pairs, res["pendant_length"], res["distal_length"], codes, wb, ws)
    return out


def assert_same(a, b, what=""):
    """every array of dict a equals its namesake in b BIT FOR BIT (floats compared as their bytes: -0.0 != 0.0, a NaN
    equals only the same NaN); on a mismatch the field and the first differing index are named"""
    assert sorted(a) == sorted(b), "%s: fields differ: %s / %s" % (what, sorted(a), sorted(b))
    for k in sorted(a):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, \
            "%s: field %s: %s %s against %s %s" % (what, k, x.dtype, x.shape, y.dtype, y.shape)
        if x.tobytes() == y.tobytes():
            continue
        xi, yi = x.reshape(-1), y.reshape(-1)
        bx = xi.view(np.uint8).reshape(len(xi), -1)
        by = yi.view(np.uint8).reshape(len(yi), -1)
        bad = np.flatnonzero((bx != by).any(axis=1))
        i = int(bad[0])
        raise AssertionError("%s: field %s differs at %d of %d entries, first at flat index %d (%s): %r against %r"
                             % (what, k, len(bad), len(xi), i, np.unravel_index(i, x.shape), xi[i], yi[i]))


def span_class(states, span):
    """epa_span_class (epa_ng_amd/csrc/epa_dev_internal.hpp) for windows of at most 256 sites"""
    assert 0 <= span <= 256
    if states != 4:
        return 0 if span <= 64 else 1 if span <= 128 else 2 if span <= 192 else 3
    if 64 < span <= 96:
        return 10
    if 128 < span <= 160:
        return 11
    return max((span + 63) // 64, 1) - 1


def check_not_vacuous(name, got):
    """the probe reaches what it is meant to reach: its ONE place_chunk holds pairs of every span class, the explicit
    list as well, every call ran Newton rounds, place_all kept a placement per read"""
    states = reference(name)["states"]
    ws = inputs(name)["probe"]["full"][2]
    want = {0, 10, 1, 11, 2, 3} if states == 4 else {0, 1, 2, 3}
    for key in ("place_chunk", "thorough"):
        assert {span_class(states, int(ws[q])) for q in got[key + ".seq_id"]} == want, key
        assert got[key + ".counters"][0] >= len(got[key + ".seq_id"]) and got[key + ".counters"][1] > 0, key
        assert np.all(np.isfinite(got[key + ".lnl"])), key
    assert set(got["place_chunk.seq_id"].tolist()) == set(range(len(ws)))
    assert np.all(got["place_all.counts"] >= 1) and got["place_all.counters"][0] >= 6 * reference(name)["B"]
    assert np.all(np.isfinite(got["preplace"]))


_FRESH = {}


def fresh_probe(name, form="full", options=()):
    """the probe's answers on a context that has done nothing else (options: (key, value) pairs set before it);
    computed once, shared by the tests and never modified"""
    key = (name, form, tuple(options))
    if key not in _FRESH:
        ev = new_context(name)
        for k, v in options:
            ev.set_option(k, v)
        _FRESH[key] = probe(ev, *inputs(name)["probe"][form])
        check_not_vacuous(name, _FRESH[key])
        for v in _FRESH[key].values():
            v.setflags(write=False)
        ev.close()
    return _FRESH[key]


_FRESH_CALLS = {}


def fresh_chunk(name, which, form="full", max_span=0):
    """place_chunk rows of input `which` on a context that has done nothing else (computed once)"""
    key = ("chunk", name, which, form, max_span)
    if key not in _FRESH_CALLS:
        ev = new_context(name)
        codes, wb, ws = inputs(name)[which][form]
        p, r = ev.place_chunk(codes, wb, ws, max_span=max_span, max_pairs=len(wb) * ev.B)
        _FRESH_CALLS[key] = chunk_rows(p, r, ev)
        ev.close()
    return _FRESH_CALLS[key]


def fresh_thorough(name, which, pairs, form="full", tag=""):
    """thorough rows of `pairs` over input `which` on a context that has done nothing else (computed once per tag)"""
    key = ("thorough", name, which, form, tag)
    if key not in _FRESH_CALLS:
        ev = new_context(name)
        _FRESH_CALLS[key] = thorough_rows(ev, pairs, *inputs(name)[which][form])
        ev.close()
    return _FRESH_CALLS[key]


def fresh_preplace(name, which, form="full"):
    key = ("preplace", name, which, form)
    if key not in _FRESH_CALLS:
        ev = new_context(name)
        _FRESH_CALLS[key] = {"preplace": ev.preplace(*inputs(name)[which][form])}
        ev.close()
    return _FRESH_CALLS[key]
