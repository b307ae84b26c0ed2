"""Duplicate queries on the device (epa_dev_dedup_queries, epa_dev_place_chunk_dedup) against tests/dedup_ref.py: exact
integer equality of rep and first, in every layout (full-width, compact, compact 4-bit, full-width 4-bit), and the rows
of place_chunk_dedup against place_chunk, bit for bit.

References (tests/preplace_ref.py): N125 (4 states, B = 125, W = 385), P67 (20 states, B = 67, W = 131), and L5 (4 states,
B = 5, W = 1701) for the window of 1700 sites.  dedup_queries looks at codes and windows only, so its inputs are random
codes with everything outside the windows filled at random; the placement cases encode real reads.

  spans       1 .. 257 and 1700 on both begin parities: every number of 128-bit window chunks per lane group (1, 2, 4 .. 64
              lanes, and the loop beyond 64 chunks), windows that start on either nibble, tails of every length
  structures  Q = 63 .. 41 000: all identical, none, blocks, interleaved, one class of 90 % plus singletons
  collisions  dedup_key_bits = 0, 1, 3 and dedup_sort_bits = 0, 1, 3: every run holds many classes (of equal and of
              unequal full keys) and the answer must not move
"""
import functools

import numpy as np
import pytest

import dedup_ref as dr
import epa_ng_amd as epa
import history_util as hu
import preplace_ref as pr
from epa_ng_amd import hostlib, synth

pytestmark = pytest.mark.gpu

SPANS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257)


@functools.lru_cache(maxsize=None)
def case_of(rid):
    if rid != "L5":
        return pr.reference_case(rid)
    root = synth.random_tree(4, 601)
    rates = synth.gamma_rates(0.7)
    labels, seqs = synth.simulate_msa(root, 1701, synth.CFG2_SUBST, synth.CFG2_FREQS, rates, 611)
    return dict(newick=synth.newick(root), labels=labels, seqs=seqs, states=4, subst=synth.CFG2_SUBST,
                freqs=synth.CFG2_FREQS, rates=rates, W=1701, B=5)


_REF, _EV = {}, {}


def evaluator(rid, blocked=False, raxml=False):
    """one context per (reference, lookup layout, branch-length rule), shared by the tests of the module"""
    key = (rid, blocked, raxml)
    if key not in _EV:
        if rid not in _REF:
            c = case_of(rid)
            _REF[rid] = hostlib.Reference(c["newick"], c["labels"], c["seqs"], states=c["states"], subst=c["subst"],
                                          freqs=c["freqs"], rates=c["rates"])
        ev = _REF[rid].evaluator(raxml_blo=raxml, flags=epa.FLAG_LOOKUP_BLOCKS if blocked else 0)
        if blocked:
            ev.set_option("lookup_block", 64)
            assert ev.lookup_mode() == (epa.LOOKUP_BLOCKS, 64)
        _EV[key] = ev
    return _EV[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for ev in _EV.values():
        ev.close()
    _EV.clear()
    _REF.clear()


def dev_form(enc):
    codes, wb, ws = enc
    if isinstance(codes, dr.Packed):
        codes = epa.Packed4(np.ascontiguousarray(codes.data), codes.stride)
    return codes, wb, ws


def check_all_layouts(ev, windows, stride, fill="random", seed=0, want=None):
    """dedup_queries on every layout of the same chunk equals the restatement (of that layout, or `want`)"""
    W = ev.W
    encs = dr.layouts(windows, W, stride, ev.s == 4, fill=fill, seed=seed)
    assert len(encs) == (4 if ev.s == 4 else 2)
    for name, enc in encs.items():
        rep, first = ev.dedup_queries(*dev_form(enc))
        wr, wf = dr.dedup(*enc, W) if want is None else want
        assert rep.dtype == np.uint32 and first.dtype == np.uint32
        assert np.array_equal(first, wf), (name, first[:8], wf[:8])
        assert np.array_equal(rep, wr), (name, np.flatnonzero(rep != wr)[:8])
        dr.check_invariants(rep, first)
    return wr, wf


def stride_for(W, span):
    s = (max(span, 1) + 15) // 16 * 16
    return s + 16 if s == W else s


TOP = {4: 16, 20: 24}


# ---- smallest chunks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", ["N125", "P67"])
def test_smallest_chunks(rid):
    ev = evaluator(rid)
    rng = np.random.RandomState(1)
    a = rng.randint(0, TOP[ev.s], 21).astype(np.uint8)
    last, first_ = a.copy(), a.copy()
    last[-1] ^= 1
    first_[0] ^= 1
    e = np.zeros(0, np.uint8)
    cases = {"one": [(5, a)], "identical": [(5, a), (5, a)], "last code": [(5, a), (5, last)], "first code": [(5, a), (5, first_)],
             "begin, odd step": [(5, a), (6, a)], "begin, even step": [(5, a), (7, a)], "prefix": [(5, a), (5, a[:-1])],
             "prefix of one": [(5, a[:1]), (5, a[:2])], "empty": [(5, e), (5, e), (6, e), (5, e)], "empty and not": [(5, e), (5, a[:1])]}
    want = {"one": 1, "identical": 1, "empty": 2}
    for name, rows in cases.items():
        for fill in (0, "random"):
            rep, first = check_all_layouts(ev, rows, 32, fill=fill, seed=2)
            assert len(first) == want.get(name, 2), name
    assert ev.kernel_ms("dedup") > 0.0


def test_no_queries():
    ev = evaluator("N125")
    z = np.zeros(0, np.uint32)
    rep, first = ev.dedup_queries(np.zeros((0, 32), np.uint8), z, z)
    assert len(rep) == 0 and len(first) == 0
    p, r, rep, first = ev.place_chunk_dedup(np.zeros((0, 32), np.uint8), z, z)
    assert len(p) == len(r) == len(rep) == len(first) == 0


def test_a_window_past_the_alignment_is_refused():
    ev = evaluator("N125")
    codes = np.zeros((3, 32), np.uint8)
    with pytest.raises(epa.EpaError) as e:
        ev.dedup_queries(codes, np.array([0, ev.W - 3, 0], np.uint32), np.array([4, 4, 4], np.uint32))
    assert e.value.code == -4
    with pytest.raises(epa.EpaError) as e:      # longer than its compact row
        ev.dedup_queries(codes, np.array([0, 0, 0], np.uint32), np.array([4, 33, 4], np.uint32))
    assert e.value.code == -4
    rep, first = ev.dedup_queries(codes, np.array([0, 1, 0], np.uint32), np.array([4, 4, 4], np.uint32))
    assert rep.tolist() == [0, 1, 0] and first.tolist() == [0, 1]


# ---- ignored bytes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", ["N125", "P67"])
@pytest.mark.parametrize("span", [1, 20, 21, 64, 65])
def test_bytes_outside_the_window_are_ignored(rid, span):
    """compact padding, the pad nibble of odd rows (W is odd: full-width 4-bit rows; an odd stride: compact ones) and the
    columns around a full-width window: 0xFF / random in one row, zeros in its twin"""
    ev = evaluator(rid)
    rng = np.random.RandomState(span)
    a = rng.randint(0, TOP[ev.s], span).astype(np.uint8)
    for b in (0, 3, ev.W - span):
        for stride in (stride_for(ev.W, span), span | 1 if span > 1 else 3):
            for fill in ([0, 0xff, "random"], ["random", 0, 0xff]):
                rep, first = check_all_layouts(ev, [(b, a)] * 3, stride, fill=fill, seed=b)
                assert rep.tolist() == [0, 0, 0] and first.tolist() == [0]


# ---- spans: every load shape --------------------------------------------------------------------------------------------------
def span_rows(W, span, top, seed):
    """around one random window per begin parity: two copies, rows differing in the last / first / a middle code, the
    same codes two columns on, the prefix of span - 1 codes"""
    rng = np.random.RandomState(seed)
    rows = []
    for par in (0, 1):
        b = par if W - span >= par else 0
        if W - span - b >= 8:
            b += 2 * rng.randint((W - span - b) // 2 - 2)
        a = rng.randint(0, top, span).astype(np.uint8)
        rows += [(b, a), (b, a.copy())]
        for k in {span - 1, 0, span // 2}:
            v = a.copy()
            v[k] = (v[k] + 1) % top
            rows.append((b, v))
        if b + 2 + span <= W:
            rows.append((b + 2, a))
        if span > 1:
            rows.append((b, a[:-1]))
        rows.append((b, a))
    return rows


@pytest.mark.parametrize("rid,span", [("N125", s) for s in SPANS] + [("P67", s) for s in SPANS if s <= 131] + [("L5", 1700)])
def test_spans(rid, span):
    ev = evaluator(rid)
    rows = span_rows(ev.W, span, TOP[ev.s], span)
    assert {b & 1 for b, _ in rows} == {0, 1} or ev.W - span < 1
    for stride in {stride_for(ev.W, span), span if span != ev.W and span > 1 else span + 1}:
        rep, first = check_all_layouts(ev, rows, stride, seed=span)
        assert len(first) >= 4 and len(first) < len(rep)


# ---- class structures -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool(W):
    """41 000 pairwise different nucleotide windows of 30 .. 70 sites, shared by the tests and never modified"""
    return dr.distinct_windows(41000, W, (30, 37, 48, 64, 65, 70), 16, 11)


@pytest.mark.parametrize("Q", [63, 64, 65, 1000, 41000])
@pytest.mark.parametrize("name", dr.STRUCTURES)
def test_structures(name, Q):
    ev = evaluator("N125")
    ids = dr.structure(name, Q, seed=Q)
    rows = pool(ev.W)
    windows = [rows[i] for i in ids]
    # the expected answer from the construction (distinct ids are distinct rows); the restatement agrees on a prefix
    order = {}
    want_rep = np.array([order.setdefault(int(i), len(order)) for i in ids], np.uint32)
    want_first = np.unique(want_rep, return_index=True)[1].astype(np.uint32)
    enc = dr.layouts(windows[:2000], ev.W, 80, True, fill="random", seed=3)["packed"]
    assert np.array_equal(dr.dedup(*enc, ev.W)[0], want_rep[:2000])
    check_all_layouts(ev, windows, 80, seed=3, want=(want_rep, want_first))


def test_structures_twenty_states():
    ev = evaluator("P67")
    for name in dr.STRUCTURES:
        ids = dr.structure(name, 1000, seed=4)
        rows = dr.distinct_windows(int(ids.max()) + 1, ev.W, (8, 30, 64, 65, 100, 131), 24, 12)
        check_all_layouts(ev, [rows[i] for i in ids], 144, seed=5)


# ---- forced collisions -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option,bits", [("dedup_key_bits", 0), ("dedup_key_bits", 1), ("dedup_key_bits", 3),
                                         ("dedup_sort_bits", 0), ("dedup_sort_bits", 1), ("dedup_sort_bits", 3), ("dedup_sort_bits", 64)])
@pytest.mark.parametrize("name", ["distinct", "interleaved"])
@pytest.mark.parametrize("Q", [65, 600])
def test_forced_collisions_change_nothing(name, Q, option, bits):
    """few key bits: unequal rows with EQUAL keys share a run; few sort bits: rows with unequal full keys do"""
    ev = evaluator("N125")
    ids = dr.structure(name, Q)
    rows = pool(ev.W)
    default = {"dedup_key_bits": 64, "dedup_sort_bits": 32}[option]
    ev.set_option(option, bits)
    try:
        wr, wf = check_all_layouts(ev, [rows[i] for i in ids], 80, seed=6)
    finally:
        ev.set_option(option, default)
    assert len(wf) == (Q if name == "distinct" else max(2, Q // 8))


def test_key_bits_outside_0_to_64_are_refused():
    ev = evaluator("N125")
    for key in ("dedup_key_bits", "dedup_sort_bits"):
        for bad in (-1, 65):
            with pytest.raises(epa.EpaError):
                ev.set_option(key, bad)


# ---- host and device pointers ----------------------------------------------------------------------------------------------------------
def test_host_and_device_pointers_give_the_same_answer():
    import torch
    ev = evaluator("N125")
    ids = dr.structure("skewed", 1000, seed=8)
    rows = pool(ev.W)
    encs = dr.layouts([rows[i] for i in ids], ev.W, 80, True, fill="random", seed=9)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else a.dtype)).cuda()   # noqa: E731
    for name in ("compact", "packed", "full"):
        codes, wb, ws = dev_form(encs[name])
        want = ev.dedup_queries(codes, wb, ws)
        assert np.array_equal(want[0], dr.dedup(*encs[name], ev.W)[0])
        d_codes = epa.Packed4(dev(codes.data), codes.stride) if isinstance(codes, epa.Packed4) else dev(codes)
        d_wb, d_ws = dev(wb), dev(ws)
        Q = len(wb)
        got = ev.dedup_queries(d_codes, d_wb, d_ws, Q=Q)                       # device in, host out
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        for c, b, s in ((d_codes, d_wb, d_ws), (codes, wb, ws), (codes, d_wb, ws)):   # device out; mixed inputs
            d_rep = torch.full((Q,), -1, dtype=torch.int32, device="cuda")
            d_first = torch.full((Q,), -1, dtype=torch.int32, device="cuda")
            n = ev.dedup_queries(c, b, s, Q=Q, rep_out=d_rep, first_out=d_first)
            torch.cuda.synchronize()
            assert n == len(want[1])
            assert np.array_equal(d_rep.cpu().numpy().view(np.uint32), want[0])
            assert np.array_equal(d_first.cpu().numpy().view(np.uint32)[:n], want[1])
            assert np.all(d_first.cpu().numpy()[n:] == -1)


# ---- place_chunk_dedup ---------------------------------------------------------------------------------------------------------------------
PLACE_SPANS = {4: (1, 37, 64, 65, 96, 97, 129, 160, 161, 200, 64, 37), 20: (1, 40, 64, 65, 100, 128, 129, 131, 64, 40)}


@functools.lru_cache(maxsize=None)
def place_inputs(rid):
    """32 .. 40 reads: about a dozen distinct ones over the span classes of the Newton kernels, each 1 .. 6 times, shuffled;
    two of the distinct reads share window and all but one code -> {layout: (codes, win_begin, win_span)}, ids"""
    c = case_of(rid)
    rng = np.random.RandomState(21)
    spans = PLACE_SPANS[c["states"]]
    windows = [((7 * i + (i & 1)) % (c["W"] - n + 1), n) for i, n in enumerate(spans)]
    rs = pr._dress(c, windows, 22)
    reads = list(rs.reads)
    b, n = windows[2]
    twin = list(reads[2])
    twin[b + n - 1] = "A" if twin[b + n - 1] != "A" else "C"
    reads.append("".join(twin))
    counts = (1, 6, 2, 4, 3, 5, 1, 4, 2, 3, 1, 5, 3)[:len(reads)]
    ids = np.concatenate([np.full(n, i) for i, n in enumerate(counts)])
    ids = ids[rng.permutation(len(ids))]
    chunk = [reads[i] for i in ids]
    enc = {"full": epa.encode_queries(c["states"], chunk), "compact": epa.encode_queries(c["states"], chunk, compact=True)}
    if c["states"] == 4:
        cc, wb, ws = enc["compact"]
        enc["packed"] = (epa.pack_codes_4bit(cc), wb, ws)
    return enc, ids


def rows_of(codes, idx):
    if isinstance(codes, epa.Packed4):
        return epa.Packed4(np.ascontiguousarray(codes.data[idx]), codes.stride)
    return np.ascontiguousarray(codes[idx])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("rid", ["N125", "P67"])
@pytest.mark.parametrize("blocked", [False, True], ids=["resident", "blocked"])
@pytest.mark.parametrize("raxml", [False, True], ids=["sliding", "raxml_blo"])
@pytest.mark.parametrize("heur", ["dynamic", "fixed"])
def test_place_chunk_dedup_equals_place_chunk(rid, blocked, raxml, heur):
    ev = evaluator(rid, blocked, raxml)
    encs, ids = place_inputs(rid)
    ev.set_heuristic(heur, 0.1)
    try:
        for name, (codes, wb, ws) in encs.items():
            Q, ms = len(wb), int(ws.max())
            wr, wf = dr.dedup(dr.Packed(codes.data, codes.stride) if isinstance(codes, epa.Packed4) else codes, wb, ws, ev.W)
            assert len(wf) == len(set(ids.tolist())) < Q
            pd, rd, rep, first = ev.place_chunk_dedup(codes, wb, ws, max_span=ms, max_pairs=Q * ev.B)
            assert np.array_equal(rep, wr) and np.array_equal(first, wf)
            # the representatives alone, gathered on the host
            p1, r1 = ev.place_chunk(rows_of(codes, first), wb[first].copy(), ws[first].copy(), max_span=ms, max_pairs=Q * ev.B)
            assert len(pd) > len(first) and same_bits(pd, p1) and same_bits(rd, r1), name
            # the whole chunk: every query's rows are its class's rows
            p2, r2 = ev.place_chunk(codes, wb, ws, max_span=ms, max_pairs=Q * ev.B)
            by_class = {u: (pd["branch_id"][pd["seq_id"] == u], rd[pd["seq_id"] == u]) for u in range(len(first))}
            for q in range(Q):
                sel = p2["seq_id"] == q
                bc, rc = by_class[int(rep[q])]
                assert len(bc) >= 1 and same_bits(p2["branch_id"][sel], bc) and same_bits(r2[sel], rc), (name, q)
    finally:
        ev.set_heuristic("dynamic")


def test_device_buffers_for_place_chunk_dedup():
    import torch
    ev = evaluator("N125")
    codes, wb, ws = place_inputs("N125")[0]["packed"]
    Q, ms = len(wb), int(ws.max())
    pd, rd, rep, first = ev.place_chunk_dedup(codes, wb, ws, max_span=ms, max_pairs=Q * ev.B)
    cap = Q * ev.B
    d_pairs = torch.zeros(cap * 2, dtype=torch.int32, device="cuda")
    d_res = torch.zeros(cap * 3, dtype=torch.float64, device="cuda")
    d_rep = torch.zeros(Q, dtype=torch.int32, device="cuda")
    d_first = torch.zeros(Q, dtype=torch.int32, device="cuda")
    d_codes = epa.Packed4(torch.from_numpy(codes.data).cuda(), codes.stride)
    d_wb, d_ws = (torch.from_numpy(a.view(np.int32)).cuda() for a in (wb, ws))
    n, nu = ev.place_chunk_dedup(d_codes, d_wb, d_ws, Q=Q, max_span=ms, max_pairs=cap, pairs_out=d_pairs, results_out=d_res,
                                 rep_out=d_rep, first_out=d_first)
    torch.cuda.synchronize()
    assert (n, nu) == (len(pd), len(first))
    assert same_bits(d_pairs.cpu().numpy()[:2 * n].view(epa.PAIR_DTYPE), pd)
    assert same_bits(d_res.cpu().numpy()[:3 * n].view(epa.RESULT_DTYPE), rd)
    assert np.array_equal(d_rep.cpu().numpy().view(np.uint32), rep)
    assert np.array_equal(d_first.cpu().numpy().view(np.uint32)[:nu], first)


def test_an_empty_window_is_the_chunk_bodys_error():
    ev = evaluator("N125")
    codes, wb, ws = place_inputs("N125")[0]["compact"]
    ws = ws.copy()
    ws[[3, 17]] = 0
    with pytest.raises(epa.EpaError) as e:
        ev.place_chunk_dedup(codes, wb, ws)
    assert e.value.code == -5 and "Sequence 17 " in str(e.value)      # as place_chunk names it: the chunk's query
    with pytest.raises(epa.EpaError) as e2:
        ev.place_chunk(codes, wb, ws)
    assert str(e2.value) == str(e.value)


@pytest.mark.parametrize("blocked", [False, True], ids=["resident", "blocked"])
def test_pair_overflow_leaves_the_context_usable(blocked):
    ev = evaluator("N125", blocked)
    codes, wb, ws = place_inputs("N125")[0]["compact"]
    Q, ms = len(wb), int(ws.max())
    want = ev.place_chunk_dedup(codes, wb, ws, max_span=ms, max_pairs=Q * ev.B)
    with pytest.raises(epa.EpaError) as e:
        ev.place_chunk_dedup(codes, wb, ws, max_span=ms, max_pairs=len(want[3]) - 1)
    assert e.value.code == -9
    got = ev.place_chunk_dedup(codes, wb, ws, max_span=ms, max_pairs=Q * ev.B)
    assert all(same_bits(a, b) for a, b in zip(got, want))


# ---- call history ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", [("R4", "compact"), ("R4B", "packed"), ("R20", "full")])
def test_dedup_calls_leave_no_trace(name, form):
    """after dedup calls that grow and shrink the scratch, force collisions and overflow, the fixed probe of
    tests/history_util.py answers as on a fresh context, bit for bit"""
    ev = hu.new_context(name)
    inp = hu.inputs(name)
    try:
        for which in ("big", "small", "mixed"):
            codes, wb, ws = inp[which][form]
            twice = (rows_of(codes, np.r_[0:len(wb), 0:len(wb)]), np.tile(wb, 2), np.tile(ws, 2))
            rep, first = ev.dedup_queries(*twice)
            assert np.array_equal(rep[len(wb):], rep[:len(wb)]) and first.max() < len(wb)
            p, r, rep2, first2 = ev.place_chunk_dedup(*twice, max_pairs=2 * len(wb) * ev.B)
            assert np.array_equal(rep2, rep) and len(p) >= len(first)
        ev.set_option("dedup_key_bits", 1)
        codes, wb, ws = inp["mixed"][form]
        rep, first = ev.dedup_queries(codes, wb, ws)
        ev.set_option("dedup_key_bits", 64)
        assert np.array_equal(ev.dedup_queries(codes, wb, ws)[0], rep)
        with pytest.raises(epa.EpaError) as e:
            ev.place_chunk_dedup(codes, wb, ws, max_pairs=1)
        assert e.value.code == -9
        got = hu.probe(ev, *inp["probe"]["full"])
    finally:
        ev.close()
    hu.assert_same(got, hu.fresh_probe(name, "full"), "%s after dedup calls" % name)
