"""Every preplacement kernel instantiation against plain numpy, bit for bit, at the shape edges of the pieces around them
(pack kernels, counting sort, k_make_groups, item walk, 8-branch bursts) -- tests/preplace_ref.py holds the method and
the inputs, tests/test_preplace_order_cpu.py proves both on the CPU with the oracle in the device's place.

The lookup table is read off the device through the public entry point: under `preplace_generic` a read whose window is
one site s with character x returns T[b][s][x].  That table is within 1e-6 (the suite's device bound) of the oracle's;
from it, numpy sums the expected row of any read in the promised order ((t0 + t1) + (t2 + t3) per four sites from the
window start, then the singles).  Every read set of preplace_ref, under every setting -- generic kernel; fast path with
the bound open (accumulating kernels); fast path with preplace_bounded (narrow / wide pair kernel by Q,
k_preplace_sites<24, false>); the last two on the blocked layout with blocks of 64 branches; full-width and compact
code rows, 4-bit packing on N67 -- must return exactly those rows (np.array_equal; the device is never compared with
another device table), the segment maxima of the single-chunk kernels must be the maxima of those rows, and the row of
a read must not depend on the reads it is submitted with.  Each launch asserts the instantiation it is meant to reach
(preplace_ref.instantiation restates launch_preplace's conditions).

References (preplace_ref.REFS): B = 5 (one partial burst), 9 (a burst + 1), 67 (tiles of 16 leave 3, 64 + 3), 125
(64 + 61); W = 97, 131, 385, all odd; spans 1 .. W; 1 .. 41 000 reads.

What the file found: reads with a gap inside their window left the pair path for the generic kernel (the gap's code
had the symbol of the rare ambiguity codes): right rows, no segment maxima.  Fixed in k_pack_pairs' symbol tables;
test_a_gap_inside_the_window_stays_on_the_pair_path is the smallest case.

Measured on MI355X: largest |extracted table - oracle|, and the wall time of the slowest read set of the reference
under all its settings (test_every_setting_equals_numpy_bit_for_bit):

    reference   B     W     |table - oracle|   slowest set, all settings
    N5          5     97    1.2e-14            short x 4 (1528 reads, 6 launches): 0.01 s
    N67         67    97    6.2e-14            tiled (41 000 reads, 10 launches): 0.06 s
    N125        125   385   1.1e-12            tiled (41 000 reads, a 41 MB table per launch, 10 launches): 0.07 s
    P9          9     131   1.6e-13            tiled (6 launches): 0.01 s
    P67         67    131   4.2e-12            tiled (10 launches): 0.06 s

    test_extracted_table_is_the_oracles_to_the_device_bound: 1.5 s for the first reference (first context of the
    process: code objects, oracle build), 0.01 - 0.13 s for the others; test_segment_maxima_of_the_single_chunk_kernels,
    test_a_gap_inside_the_window_stays_on_the_pair_path and test_a_reads_row_does_not_depend_on_its_company: at most
    0.02 s per reference.  The whole file: 66 tests in 3.4 s.
"""
import functools
import time

import numpy as np
import pytest

import epa_ng_amd as epa
import preplace_ref as pr
from epa_ng_amd import hostlib
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

LNL_TOL = 1e-6
RIDS = list(pr.REFS)
BLOCKED = ("N67", "N125", "P67")           # references that also run on FLAG_LOOKUP_BLOCKS, lookup_block = 64
SET_CASES = [(rid, name) for rid in RIDS for name in pr.set_names(rid)]


class Ref:
    """one reference: its evaluators (resident, and blocked where listed) and the table extracted by the generic kernel"""

    def __init__(self, rid):
        c = self.case = pr.reference_case(rid)
        self.rid, self.states, self.W, self.B = rid, c["states"], c["W"], c["B"]
        self.ref = hostlib.Reference(c["newick"], c["labels"], c["seqs"], states=c["states"], subst=c["subst"],
                                     freqs=c["freqs"], rates=c["rates"])
        assert (self.ref.B, self.ref.W) == (self.B, self.W)
        self.ev = self.ref.evaluator()
        assert self.ev.lookup_mode() == (epa.LOOKUP_RESIDENT, 0)
        self.evb = None
        if rid in BLOCKED:
            self.evb = self.ref.evaluator(flags=epa.FLAG_LOOKUP_BLOCKS)
            self.evb.set_option("lookup_block", 64)
            assert self.evb.lookup_mode() == (epa.LOOKUP_BLOCKS, 64)
        ex = pr.extraction_set(rid)
        self.ex_enc = epa.encode_queries(self.states, ex.reads)
        self.ev.set_option("preplace_generic", 1)
        self.ex_rows = self.ev.preplace(*self.ex_enc)
        self.ev.set_option("preplace_generic", 0)
        self.table = pr.table_from_rows(self.ex_rows, self.ex_enc[0], self.W, pr.extraction_chars(self.states),
                                        pr.any_char(self.states))

    def close(self):
        for e in (self.ev, self.evb):
            if e is not None:
                e.close()


_REFS = {}


def ref_of(rid):
    if rid not in _REFS:
        _REFS[rid] = Ref(rid)
    return _REFS[rid]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for r in _REFS.values():
        r.close()
    _REFS.clear()
    inputs.cache_clear()


@functools.lru_cache(maxsize=None)
def inputs(rid, name):
    """-> (ReadSet of the distinct reads, copies, {layout: (codes, win_begin, win_span)} of the whole set, expected rows
    of the distinct reads)"""
    r = ref_of(rid)
    rs, copies = pr.read_set(rid, name)
    full = epa.encode_queries(r.states, rs.reads)
    assert [(int(a), int(b)) for a, b in zip(full[1], full[2])] == rs.windows
    want = pr.expected_rows(r.table, *full)
    assert not np.isnan(want).any()
    compact = epa.encode_queries(r.states, rs.reads, compact=True)
    encs = {"full": full, "compact": compact}
    if copies > 1:                 # the copies of a read lie len(rs) apart
        encs = {k: (np.tile(c, (copies, 1)), np.tile(b, copies), np.tile(s, copies)) for k, (c, b, s) in encs.items()}
    if (rid, name) == ("N67", "short"):
        c = encs["compact"]
        encs["4bit"] = (epa.pack_codes_4bit(c[0]), c[1], c[2])
    return rs, copies, encs, want


def assert_rows(got, want, copies, rs, what):
    """got [copies * n][B] against want [n][B], bit for bit; a failure names the differing (read, branch) cells"""
    n, B = want.shape
    g = got.reshape(copies, n, B)
    if np.array_equal(g, np.broadcast_to(want, g.shape)):
        return
    bad = np.argwhere(g != want[None])
    cells = [(int(k * n + i), rs.windows[i], int(b), float(g[k, i, b] - want[i, b])) for k, i, b in bad[:8]]
    branches = sorted({int(b) for b in bad[:, 2]})
    raise AssertionError("%s: %d of %d cells differ from numpy; reads %d, branches %s; first (read, (begin, span), "
                         "branch, got - want): %s" % (what, len(bad), g.size, len({(int(k), int(i)) for k, i, _ in bad}),
                                                     branches[:16], cells))


def assert_keys(keys, want, copies, rs, what):
    """segment-maximum keys of a single-chunk fast kernel: the maxima of the expected rows bit for bit on the rare-free
    reads, 0 (never written) on the reads the generic kernel served and beyond the last segment"""
    n, B = want.shape
    nseg = (B + 63) // 64
    k = keys.reshape(copies, n, -1)
    assert not k[:, :, nseg:].any(), what
    assert not k[:, rs.rare, :].any(), what
    vals = pr._seg_values(k[:, ~rs.rare, :nseg])
    assert not np.isnan(vals).any(), what
    mx = pr.segment_maxima(want)[~rs.rare]
    assert np.array_equal(vals, np.broadcast_to(mx, vals.shape)), (what, np.argwhere(vals != mx[None])[:8].tolist())


def fast_launches(r, name, rs, copies):
    """(label, evaluator, bound, instantiation) of the fast-path settings of one read set"""
    want = {(n, b > 0): v for n, _, b, v in pr.variant_cases(r.rid) if n == name}
    Q = len(rs) * copies
    out = []
    for lay, ev in (("resident", r.ev), ("blocked", r.evb)):
        if ev is None:
            continue
        for bound in (0, rs.max_span):
            if (name, bound > 0) not in want:
                continue                      # no bounded call: the spans do not fit a single chunk
            inst = pr.instantiation(r.states, Q, r.W, bound)
            assert inst == want[(name, bound > 0)], (r.rid, name, Q, bound)
            out.append(("%s %s %s bound %d: %s" % (r.rid, name, lay, bound, inst), ev, bound, inst))
    return out


# ---- the table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", RIDS)
def test_extracted_table_is_the_oracles_to_the_device_bound(rid):
    r = ref_of(rid)
    c = r.case
    o = Oracle(c["newick"], c["labels"], c["seqs"], c["states"], c["subst"], c["freqs"], c["rates"])
    assert pr.instantiation(r.states, len(r.ex_rows), r.W, 0, generic=True) == "k_preplace<%d, true>" % (16 if r.states == 4 else 24)
    d = float(np.max(np.abs(r.ex_rows - o.preplace(pr.extraction_set(rid).reads))))
    print("\n%s (B %d, W %d): largest |extracted table - oracle| %.3g over %d cells" % (rid, r.B, r.W, d, r.ex_rows.size))
    assert d < LNL_TOL
    assert np.all(np.isfinite(r.ex_rows))


# ---- every setting against numpy ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid,name", SET_CASES, ids=["%s-%s" % c for c in SET_CASES])
def test_every_setting_equals_numpy_bit_for_bit(rid, name):
    r = ref_of(rid)
    rs, copies, encs, want = inputs(rid, name)
    t0 = time.time()
    # generic kernel, bound open
    r.ev.set_option("preplace_generic", 1)
    try:
        for lay in ("full", "compact"):
            assert_rows(r.ev.preplace(*encs[lay]), want, copies, rs, "%s %s generic %s" % (rid, name, lay))
    finally:
        r.ev.set_option("preplace_generic", 0)
    # fast paths: accumulating (bound open) and single-chunk (bounded) kernels, resident and blocked
    n = 0
    for label, ev, bound, inst in fast_launches(r, name, rs, copies):
        for lay, enc in encs.items():
            what = "%s, %s rows" % (label, lay)
            if bound == 0:
                assert_rows(ev.preplace(*enc), want, copies, rs, what)
            else:
                got, keys = ev.preplace_bounded(*enc, bound, seg_keys=True)
                assert_rows(got, want, copies, rs, what)
                assert_keys(keys, want, copies, rs, what)
            n += 1
    print("\n%s %s: %d reads, %d fast launches + 2 generic, %.2f s" % (rid, name, len(rs) * copies, n, time.time() - t0))


# ---- segment maxima ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", RIDS)
def test_segment_maxima_of_the_single_chunk_kernels(rid):
    """B = 5: one segment shorter than a burst; 9: one segment; 67: 64 + 3; 125: 64 + 61"""
    r = ref_of(rid)
    seen = set()
    for name in ("short", "sparse", "few17") + tuple(n for n in pr.set_names(rid) if n.startswith("short x")):
        rs, copies, encs, want = inputs(rid, name)
        for label, ev, bound, inst in fast_launches(r, name, rs, copies):
            if bound == 0:
                continue
            got, keys = ev.preplace_bounded(*encs["compact"], bound, seg_keys=True)
            assert keys.shape == (len(rs) * copies, ((r.B + 63) // 64 + 7) // 8 * 8)
            assert_keys(keys, want, copies, rs, label)
            assert_rows(got, want, copies, rs, label)
            seen.add(inst)
    assert seen == ({pr.WIDE, pr.NARROW} if r.states == 4 else {pr.SITES})
    # a window above the bound is refused, whatever the kernel
    rs, copies, encs, want = inputs(rid, "short")
    with pytest.raises(epa.EpaError):
        r.ev.preplace_bounded(*encs["compact"], rs.max_span - 1)


@pytest.mark.parametrize("rid", [r for r in RIDS if pr.REFS[r][0] == 4])
def test_a_gap_inside_the_window_stays_on_the_pair_path(rid):
    """The smallest case of what this file found: k_pack_pairs gave the gap's code (0) the symbol of the rare ambiguity
    codes, so every read with a gap inside its window left the pair path for the generic kernel -- the right row, but
    no segment maxima, against the kernel's own description (windows of A/C/G/T/N-or-gap).  The gap's lookup column is
    N's; it takes N's symbol now."""
    r = ref_of(rid)
    seq = r.case["seqs"][0]
    reads = ["-" * 10 + seq[10] + "-" + seq[12] + "-" * (r.W - 13),               # a gap in a tail single
             "-" * 21 + seq[21:23] + "-" + seq[24:29] + "-" * (r.W - 29)]           # and in a pair word, odd start
    rs = pr.ReadSet(reads, [(10, 3), (21, 8)], [False, False])
    full = epa.encode_queries(4, reads)
    assert [(int(a), int(b)) for a, b in zip(full[1], full[2])] == rs.windows
    want = pr.expected_rows(r.table, *full)
    for ev in (r.ev, r.evb):
        if ev is None:
            continue
        for enc in (full, epa.encode_queries(4, reads, compact=True)):
            got, keys = ev.preplace_bounded(*enc, 8, seg_keys=True)
            assert_rows(got, want, 1, rs, rid)
            assert keys[:, 0].all()
            assert_keys(keys, want, 1, rs, rid)
            assert_rows(ev.preplace(*enc), want, 1, rs, rid)


# ---- independence of company ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", RIDS)
def test_a_reads_row_does_not_depend_on_its_company(rid):
    """the row of a read alone, in `short`, in `short` reversed and among the 41 000 of `tiled`: the same bits"""
    r = ref_of(rid)
    short = pr.short_set(rid)
    td = pr.tiled_distinct(rid)
    pick = list(range(0, 40, 4))                                   # ten of the 40 rare-free reads `tiled` repeats
    in_short = [short.reads.index(td.reads[i]) for i in pick]
    assert all(short.windows[j] == td.windows[i] for i, j in zip(pick, in_short))
    enc_s = epa.encode_queries(r.states, short.reads, compact=True)
    enc_r = epa.encode_queries(r.states, short.reversed().reads, compact=True)
    _, copies, encs_t, want_t = inputs(rid, "tiled")
    for bound in (0, short.max_span):
        def run(enc):
            return r.ev.preplace(*enc) if bound == 0 else r.ev.preplace_bounded(*enc, bound)
        rows_s, rows_r = run(enc_s), run(enc_r)
        rows_t = run(encs_t["compact"])
        for i, j in zip(pick, in_short):
            alone = run(epa.encode_queries(r.states, [td.reads[i]], compact=True))[0]
            what = (rid, bound, i, td.windows[i])
            assert np.array_equal(alone, want_t[i]), what
            assert np.array_equal(rows_s[j], alone), what
            assert np.array_equal(rows_r[len(short) - 1 - j], alone), what
            assert np.array_equal(rows_t[i], alone) and np.array_equal(rows_t[i + 40 * (copies - 1)], alone), what
            assert np.array_equal(rows_t[i::40], np.broadcast_to(alone, (copies, r.B))), what
