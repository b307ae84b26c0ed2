"""Profile queries on the device (include/epa_dev.h, "Profile queries"): reads given as per-site state likelihoods.

The checkers: the coded entry points (a 0/1 row that is a code's state set IS the coded query), the independent
log-space evaluator of tests/brute_force.py, which takes real-valued tip vectors as it stands (_star, _derivatives), and
k_score_at's profile instantiation for the preplacement kernel's shape edges.  Every bound is LNL_TOL = 1e-6, the
suite's device bound; the end points follow the rule of tests/endpoints_util.py.

  1. 0/1 rows are coded queries: T4 (4 states, 4 categories), D5I (5 +R categories, +I), A4 (20 states, 4 categories);
     reads with ambiguity codes and interior gaps.  score_at / site_lnl / thorough (general kernel, both BLO rules) bit
     for bit, the preplacement within LNL_TOL.
  2. real-valued rows (Phred scores 2 .. 41 through profile_from_phred, and dense random rows) against BruteForce on the
     same rows: score_at_profile, the site rows, preplace_profile; S4 is the rescaling ladder (every site rescaled).
     preplace_profile is score_at_profile at the default lengths.
  3. shape edges of k_preplace_profile: spans 1, 63, 64, 65, W at both ends of the alignment, B = 5 and 125, Q = 1 and
     67, NaN in the padding rows.
  4. thorough_profile ends where BruteForce.optimise ends on the same rows (span <= 64, span 129, +I).
  5. place_chunk_profile is its composition; overflow; a profile call leaves a following coded place_chunk alone.
  6. validation from host and device rows; the blocked lookup layout.

Largest differences measured on MI355X (the tests print them):

    test 1  |preplace_profile(0/1 rows) - preplace|            T4 6.8e-13, D5I 6.8e-13, A4 1.4e-12
    test 2  |device - brute force|, Phred and dense rows       score_at 1.3e-11, site rows 5.3e-12, preplacement 1.5e-11
                                                               (the largest on the ladder S4)
            |preplace_profile - score_at_profile|              3.6e-12
    test 3  |preplace_profile - score_at_profile|              9.1e-13 (B = 125), 1.1e-13 (B = 5)
    test 4  end points: every pair agrees (|dlnL| <= 4.5e-13, relative lengths <= 3.5e-14), rounds equal the brute force's
"""
import functools

import numpy as np
import pytest

import brute_cases as bc
import endpoints_util as eu
import epa_ng_amd as epa
import profile_util as pu
from epa_ng_amd import hostlib
from gen_golden import DEFAULT_BL, valid_range

pytestmark = pytest.mark.gpu

LNL_TOL = 1e-6


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "D5I":          # group D's shape: five free-rate categories, with +I
        return dict(bc.case("D5"), pinv=0.2, name="D5I")
    return bc.case(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    ref = hostlib.Reference(c["newick"], c["labels"], c["seqs"], states=c["states"], subst=c["subst"], freqs=c["freqs"],
                            rates=c["rates"], weights=c["weights"], pinv=c["pinv"])
    return ref, np.array([ref.branch(b)["length"] for b in range(ref.B)])


@functools.lru_cache(maxsize=None)
def evaluator(name, raxml=False, blocks=False, generic=False):
    ev = reference(name)[0].evaluator(raxml_blo=raxml, flags=epa.FLAG_LOOKUP_BLOCKS if blocks else 0)
    if generic:
        ev.set_option("thorough_generic", 1)
    return ev


@functools.lru_cache(maxsize=None)
def queries(name):
    c = case(name)
    return epa.encode_queries(c["states"], c["reads"], compact=True)


@functools.lru_cache(maxsize=None)
def brute(name):
    c = case(name)
    bf = pu.brute_of(c)
    ref, lengths = reference(name)
    assert bf.B == ref.B and np.array_equal(bf.lengths, lengths)          # same edge numbering
    return bf


@functools.lru_cache(maxsize=None)
def rows_of(name, kind):
    """profile rows [Q][stride][s] of the configuration's reads: "01" state sets, "phred" random scores 2 .. 41, "dense"
    random rows; padding rows are NaN"""
    c = case(name)
    codes, wb, ws = queries(name)
    if kind == "01":
        rows = pu.zero_one_rows(c["states"], codes, ws, fill=np.nan)
    elif kind == "phred":
        phred = np.random.RandomState(7).randint(2, 42, codes.shape).astype(np.uint8)
        rows = epa.profile_from_phred(c["states"], codes, phred, ws, out=np.full(codes.shape + (c["states"],), np.nan))
        assert np.array_equal(np.isnan(rows), np.isnan(pu.zero_one_rows(c["states"], codes, ws, fill=np.nan)))
    else:
        rows = pu.dense_rows(c["states"], codes.shape, 11)
        rows[np.arange(codes.shape[1])[None, :] >= ws[:, None]] = np.nan
    rows.setflags(write=False)
    return rows


def make_pairs(pb, ps):
    pairs = np.zeros(len(pb), epa.PAIR_DTYPE)
    pairs["branch_id"], pairs["seq_id"] = pb, ps
    return pairs


def all_pairs(B, Q):
    return np.repeat(np.arange(B), Q), np.tile(np.arange(Q), B)


# ---- 1. 0/1 rows are coded queries

@pytest.mark.parametrize("name", ["T4", "D5I", "A4"])
def test_zero_one_rows_are_coded_queries(name):
    c = case(name)
    _, lengths = reference(name)
    ev = evaluator(name)
    codes, wb, ws = queries(name)
    rows = rows_of(name, "01")
    assert any(set(r) & set(bc.AMBIG[c["states"]][:-1]) for r in c["reads"])        # ambiguity codes and interior gaps
    assert any("-" in r.strip("-") for r in c["reads"])
    Q = len(ws)
    pb, ps = all_pairs(ev.B, Q)
    rng = np.random.RandomState(3)
    pen = rng.choice([1e-4, DEFAULT_BL, 2.5], len(pb))
    dis = rng.choice([0.0, 0.3, 1.0], len(pb)) * lengths[pb]
    pairs = make_pairs(pb, ps)
    assert np.array_equal(ev.score_at_profile(pairs, pen, dis, rows, wb, ws), ev.score_at(pairs, pen, dis, codes, wb, ws))
    prox = 0.7 * lengths[pb]
    assert np.array_equal(ev.score_at_profile(pairs, pen, dis, rows, wb, ws, proximal=prox),
                          ev.score_at(pairs, pen, dis, codes, wb, ws, proximal=prox))
    coded_sites = ev.site_lnl(pairs, pen, dis, codes, wb, ws)
    assert np.array_equal(ev.site_lnl_profile(pairs, pen, dis, rows, wb, ws), coded_sites)
    assert coded_sites.shape == (len(pb), int(ws.max()))
    table, want = ev.preplace_profile(rows, wb, ws), ev.preplace(codes, wb, ws)
    d = float(np.max(np.abs(table - want)))
    print("\n%s: max |preplace_profile(0/1 rows) - preplace| %.3g" % (name, d))
    assert np.all(np.isfinite(table)) and d < LNL_TOL


@pytest.mark.parametrize("name", ["T4", "D5I", "A4"])
@pytest.mark.parametrize("raxml", [False, True], ids=["sliding", "raxml"])
def test_zero_one_rows_thorough_is_the_general_kernel(name, raxml):
    c = case(name)
    codes, wb, ws = queries(name)
    pb, ps = bc.pair_lists(c, reference(name)[0].B)
    pairs = make_pairs(pb[::2], ps[::2])
    coded = evaluator(name, raxml=raxml, generic=True)
    want = coded.thorough(pairs, codes, wb, ws)
    want_stats = dict(coded.last_stats)
    ev = evaluator(name, raxml=raxml)          # thorough_profile runs the general kernel whatever the option says
    got = ev.thorough_profile(pairs, rows_of(name, "01"), wb, ws)
    assert got.tobytes() == want.tobytes()
    assert ev.last_stats == want_stats and want_stats["rounds"] >= len(pairs)


# ---- 2. real-valued rows against the brute force

def brute_entries(name, rows, pb, ps, pen, dis):
    """-> (lnL [n], site rows [n][max span]) of BruteForce._star on the rows"""
    c, bf = case(name), brute(name)
    for q, r in enumerate(c["reads"]):
        bf.set_rows(r, rows[q])
    width = max(valid_range(r)[1] for r in c["reads"])
    sites = np.zeros((len(pb), width))
    for i, (b, q) in enumerate(zip(pb, ps)):
        r = c["reads"][q]
        lo, n = valid_range(r)
        sites[i, :n] = bf._star(int(b), bf.tip_vectors(r)[lo:lo + n], float(pen[i]), float(dis[i]), lo, n)
    return sites.sum(1), sites


@pytest.mark.parametrize("name,kind", [("T4", "phred"), ("T4", "dense"), ("D5I", "phred"), ("D5I", "dense"), ("A4", "phred"),
                                       ("A4", "dense"), ("S4", "phred"), ("S4", "dense")])
def test_real_valued_rows_against_the_brute_force(name, kind):
    c, bf = case(name), brute(name)
    _, lengths = reference(name)
    ev = evaluator(name)
    _, wb, ws = queries(name)
    rows = rows_of(name, kind)
    Q = len(ws)
    # score_at and the site rows, away from the default lengths
    br = np.array([0, bf.B // 2, bf.B - 1])
    pb, ps = np.repeat(br, Q), np.tile(np.arange(Q), len(br))
    pen = np.tile(np.array([0.02, DEFAULT_BL, 1.7]), len(pb))[:len(pb)]
    dis = np.tile(np.array([0.25, 0.5, 0.9, 0.0]), len(pb))[:len(pb)] * lengths[pb]
    want, want_sites = brute_entries(name, rows, pb, ps, pen, dis)
    pairs = make_pairs(pb, ps)
    got = ev.score_at_profile(pairs, pen, dis, rows, wb, ws)
    got_sites = ev.site_lnl_profile(pairs, pen, dis, rows, wb, ws)
    d_score, d_sites = float(np.max(np.abs(got - want))), float(np.max(np.abs(got_sites - want_sites)))
    # the preplacement: every branch at its midpoint, pendant DEFAULT_BL
    for q, r in enumerate(c["reads"]):
        bf.set_rows(r, rows[q])
    table = ev.preplace_profile(rows, wb, ws)
    d_pre = float(np.max(np.abs(table - bf.preplace(c["reads"]))))
    pb, ps = all_pairs(bf.B, Q)
    at_start = ev.score_at_profile(make_pairs(pb, ps), np.full(len(pb), DEFAULT_BL), lengths[pb] / 2.0, rows, wb, ws)
    d_tie = float(np.max(np.abs(table[ps, pb] - at_start)))
    print("\n%s %s: max |device - brute force| score_at %.3g, site rows %.3g, preplacement %.3g; |preplace_profile - "
          "score_at_profile| %.3g" % (name, kind, d_score, d_sites, d_pre, d_tie))
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(table))
    assert d_score < LNL_TOL and d_sites < LNL_TOL and d_pre < LNL_TOL and d_tie < LNL_TOL
    if name == "S4":           # the ladder: every site of the deep branches carries scaler counts
        assert float(table.max()) < -256 * np.log(2.0)


# ---- 3. shape edges of the preplacement kernel

@functools.lru_cache(maxsize=None)
def shape_reference(tips):
    W = 130
    c = bc._simulated(4, tips, W, (), 8100 + tips)
    rates, weights = bc.free_rates(4, 8104)
    ref = hostlib.Reference(c["newick"], c["labels"], c["seqs"], states=4, subst=c["subst"], freqs=c["freqs"], rates=rates,
                            weights=weights, pinv=0.0)
    assert ref.B == 2 * tips - 3 and ref.W == W
    return ref, ref.evaluator(), np.array([ref.branch(b)["length"] for b in range(ref.B)])


@pytest.mark.parametrize("tips,Q", [(4, 1), (4, 67), (64, 1), (64, 67)], ids=["B5-Q1", "B5-Q67", "B125-Q1", "B125-Q67"])
def test_preplace_profile_shape_edges(tips, Q):
    ref, ev, lengths = shape_reference(tips)
    W, B = ref.W, ref.B
    assert B == {4: 5, 64: 125}[tips]
    windows = [(lo, n) for n in (1, 63, 64, 65, W) for lo in sorted({0, W - n})]
    assert len(windows) == 9
    pick = [windows[(5 + i) % len(windows)] for i in range(Q)]          # Q = 1: 65 sites ending at W
    wb = np.array([w[0] for w in pick], np.uint32)
    ws = np.array([w[1] for w in pick], np.uint32)
    stride = W + 6
    rng = np.random.RandomState(100 + Q)
    codes = rng.choice([1, 2, 4, 8], (Q, stride)).astype(np.uint8)
    rows = epa.profile_from_phred(4, codes, rng.randint(2, 42, (Q, stride)).astype(np.uint8), np.full(Q, stride, np.uint32))
    rows[::3] = pu.dense_rows(4, (len(rows[::3]), stride), 5)
    rows[np.arange(stride)[None, :] >= ws[:, None]] = np.nan            # the padding is never read
    table = ev.preplace_profile(rows, wb, ws)
    assert table.shape == (Q, B) and np.all(np.isfinite(table))
    for n in sorted(set(ws.tolist())):                                   # stride == span: the same bits
        sel = np.flatnonzero(ws == n)
        tight = ev.preplace_profile(np.ascontiguousarray(rows[sel, :n]), wb[sel], ws[sel])
        assert np.array_equal(tight, table[sel]), n
    pb, ps = all_pairs(B, Q)
    at_start = ev.score_at_profile(make_pairs(pb, ps), np.full(len(pb), DEFAULT_BL), lengths[pb] / 2.0, rows, wb, ws)
    d = float(np.max(np.abs(table[ps, pb] - at_start)))
    print("\nB %d Q %d: max |preplace_profile - score_at_profile| %.3g" % (B, Q, d))
    assert d < LNL_TOL
    assert ev.kernel_ms("preplace_profile") >= 0


# ---- 4. end points

@pytest.mark.parametrize("name,reads,raxml", [("T4", (2, 3), False), ("T4", (2, 3), True), ("T4", (8,), False), ("T4I", (2, 5, 8), False)],
                         ids=["span<=64-sliding", "span<=64-raxml", "span129", "+I"])
def test_thorough_profile_end_points(name, reads, raxml):
    c, bf = case(name), brute(name)
    _, lengths = reference(name)
    _, wb, ws = queries(name)
    rows = rows_of(name, "phred")
    assert {int(ws[q]) for q in reads} == {"T4": {(2, 3): {30, 64}, (8,): {129}}, "T4I": {(2, 5, 8): {30, 96, 129}}}[name][reads]
    br = np.array([0, bf.B // 3, 2 * bf.B // 3, bf.B - 1])
    pb, ps = np.repeat(br, len(reads)), np.tile(np.array(reads), len(br))
    for q in reads:
        bf.set_rows(c["reads"][q], rows[q])
    ends = [bf.optimise(int(b), c["reads"][q], mode="raxml" if raxml else "sliding") for b, q in zip(pb, ps)]
    entry = {"branch": pb, "read": ps, "lnl": np.array([e["lnl"] for e in ends]), "pendant": np.array([e["pendant"] for e in ends]),
             "distal": np.array([e["distal"] for e in ends])}
    ev = evaluator(name, raxml=raxml)
    res = ev.thorough_profile(make_pairs(pb, ps), rows, wb, ws)
    args = (entry, res["lnl"], res["pendant_length"], res["distal_length"], lengths, LNL_TOL)
    st = eu.measure(*args)
    want_rounds = sum(e["rounds"] for e in ends)
    print("\n" + eu.line(name, "raxml" if raxml else "sliding", st), st["other_pairs"] or "",
          "| rounds device %d brute force %d" % (ev.last_stats["rounds"], want_rounds))
    eu.compare(*args)


# ---- 5. the chunk body

@pytest.mark.parametrize("name", ["T4", "A4"])
def test_place_chunk_profile_is_its_composition(name):
    ev = evaluator(name)
    codes, wb, ws = queries(name)
    rows = rows_of(name, "phred")
    Q = len(ws)
    table = ev.preplace_profile(rows, wb, ws)
    pairs = ev.select(table, Q, 0.99999)
    res = ev.thorough_profile(pairs, rows, wb, ws)
    assert 0 < len(pairs) < Q * ev.B
    got_pairs, got_res = ev.place_chunk_profile(rows, wb, ws, max_pairs=Q * ev.B)
    assert got_pairs.tobytes() == pairs.tobytes() and got_res.tobytes() == res.tobytes()
    assert ev.last_stats["pairs"] == len(pairs)
    # too little room, then enough
    with pytest.raises(epa.EpaError) as e:
        ev.place_chunk_profile(rows, wb, ws, max_pairs=len(pairs) - 1)
    assert e.value.code == -9
    again_pairs, again_res = ev.place_chunk_profile(rows, wb, ws, max_pairs=len(pairs))
    assert again_pairs.tobytes() == pairs.tobytes() and again_res.tobytes() == res.tobytes()
    # the coded chunk body after profile calls is a fresh context's
    after = ev.place_chunk(codes, wb, ws)
    fresh = reference(name)[0].evaluator().place_chunk(codes, wb, ws)
    assert after[0].tobytes() == fresh[0].tobytes() and after[1].tobytes() == fresh[1].tobytes()


# ---- 6. validation

FAULTS = {"negative": -0.25, "nan": np.nan, "zero row": 0.0, "tiny row": 2.0 ** -70}


def faulty(rows, q, j, what):
    out = np.array(rows)
    if what in ("zero row", "tiny row"):
        out[q, j, :] = FAULTS[what]
    else:
        out[q, j, 1] = FAULTS[what]
    return out


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("what", sorted(FAULTS))
def test_row_validation_names_query_and_position(what, on_device):
    import torch
    name = "T4"
    ev = evaluator(name)
    _, wb, ws = queries(name)
    rows = np.nan_to_num(rows_of(name, "phred"), nan=1.0)
    q, j = 5, int(ws[5]) - 2
    bad = faulty(rows, q, j, what)
    bad[q + 1, 3, :] = -1.0                                   # a later offender: the first one is named
    pairs, pen, dis = make_pairs([0, 1], [q, q + 1]), np.full(2, 0.1), np.zeros(2)
    arg = torch.from_numpy(bad).cuda() if on_device else bad
    calls = [lambda: ev.preplace_profile(arg, wb, ws), lambda: ev.score_at_profile(pairs, pen, dis, arg, wb, ws),
             lambda: ev.site_lnl_profile(pairs, pen, dis, arg, wb, ws), lambda: ev.thorough_profile(pairs, arg, wb, ws),
             lambda: ev.place_chunk_profile(arg, wb, ws)]
    for call in calls:
        with pytest.raises(epa.EpaError) as e:
            call()
        assert e.value.code == -1 and "query %d position %d" % (q, j) in str(e.value), str(e.value)
    # the same fault in a padding row is never read
    pad = faulty(rows, q, int(ws[q]), what)
    assert int(ws[q]) < rows.shape[1]
    arg = torch.from_numpy(pad).cuda() if on_device else pad
    assert np.array_equal(ev.preplace_profile(arg, wb, ws), ev.preplace_profile(rows, wb, ws))


def test_window_checks_and_empty_calls():
    name = "T4"
    ev = evaluator(name)
    _, wb, ws = queries(name)
    rows = np.nan_to_num(rows_of(name, "phred"), nan=1.0)
    with pytest.raises(epa.EpaError) as e:                     # a window longer than the stride
        ev.preplace_profile(np.ascontiguousarray(rows[:, :100]), wb, ws)
    assert e.value.code == -1 and "stride" in str(e.value)
    ws0 = ws.copy()
    ws0[2] = 0
    with pytest.raises(epa.EpaError) as e:
        ev.preplace_profile(rows, wb, ws0)
    assert e.value.code == -5
    wide = wb.copy()
    wide[1] = ev.W
    with pytest.raises(epa.EpaError) as e:
        ev.place_chunk_profile(rows, wide, ws)
    assert e.value.code == -4
    # an empty window is the empty sum for the entry calls, as for codes
    pairs, pen, dis = make_pairs([0, 0, 0], [1, 2, 3]), np.full(3, 0.1), np.zeros(3)
    got = ev.score_at_profile(pairs, pen, dis, rows, wb, ws0)
    assert got[1] == 0.0 and got[0] < 0.0 and got[2] < 0.0
    assert ev.score_at_profile(make_pairs([], []), np.zeros(0), np.zeros(0), rows, wb, ws).shape == (0,)
    assert len(ev.thorough_profile(make_pairs([], []), rows, wb, ws)) == 0


def test_blocked_layout():
    name = "T4"
    ev, blk = evaluator(name), evaluator(name, blocks=True)
    assert blk.lookup_mode()[0] == epa.LOOKUP_BLOCKS
    _, wb, ws = queries(name)
    rows = rows_of(name, "phred")
    for call in (lambda: blk.preplace_profile(rows, wb, ws), lambda: blk.place_chunk_profile(rows, wb, ws)):
        with pytest.raises(epa.EpaError) as e:
            call()
        assert e.value.code == -8 and "--memsave" in str(e.value)
    _, lengths = reference(name)
    pb, ps = all_pairs(ev.B, len(ws))
    pairs, pen, dis = make_pairs(pb, ps), np.full(len(pb), 0.3), 0.4 * lengths[pb]
    assert np.array_equal(blk.score_at_profile(pairs, pen, dis, rows, wb, ws), ev.score_at_profile(pairs, pen, dis, rows, wb, ws))
    assert np.array_equal(blk.site_lnl_profile(pairs, pen, dis, rows, wb, ws), ev.site_lnl_profile(pairs, pen, dis, rows, wb, ws))
    some = np.ascontiguousarray(pairs[::5])
    assert blk.thorough_profile(some, rows, wb, ws).tobytes() == ev.thorough_profile(some, rows, wb, ws).tobytes()
