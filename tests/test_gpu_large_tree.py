"""GPU tests of references with more than 65 535 branches: 32 770 tips, B = 65 537, W = 96.

Context creation (from the tree and from host CLVs), the lookup build and the preplacement against the oracle;
the streaming selection kernel (k_select_stream) against the plain restatement of the reference's rules
(selection_ref.py) on crafted tables, on a tree-shaped table and on a "flat" table where the dynamic rule keeps
most of the row; the fused chunk body, epa_dev_place_all and the CLI.

Inputs (large_tree_gen.py; rehearsed on the CPU oracle's tables):
  tree-shaped  large_tree_gen.dna_workload(32770, 96, 64, 64, (201, 202, 203)): generation 1.0 s, 15 join levels,
               tree lnL -1041042.2155513722 (hostlib.Reference and Oracle agree to the last digit); the dynamic
               rule at 0.99999 keeps 761 pairs, 1 .. 139 per query (median 7), baseball keeps 7 .. 17; all 64 rows
               are selection_ref.robust, smallest margin 1.9e-8 against the suite's 1e-10.
  flat         large_tree_gen.flat_reads(32770, 96, 16, 64) on the same tree: dynamic at 0.9 keeps 1 .. 29 847 per
               query (184 120 pairs; all 16 rows robust, smallest margin 7.2e-8), at 0.99999 1 .. 63 407 per query
               (863 819 pairs; 16 of 16 robust, smallest margin 2.4e-10: close to the line, hence "at least 12").
Tolerances are the suite's: 1e-6 on lnL and lengths (test_gpu_parity.py), 1e-7 |lnL| on the tree lnL
(test_gpu_generic.py)."""
import json
import math
import subprocess
import time

import numpy as np
import pytest

import epa_ng_amd as epa
from epa_ng_amd import hostlib, synth
from oracle_lib import Oracle
import selection_ref as ref

import large_tree_gen as gen

pytestmark = pytest.mark.gpu

N_TIPS, W, B = 32770, 96, 65537
LNL_TOL = 1e-6
QS = (1, 33, 65)


class _Row:
    """one table row with its selection order and LWRs computed once.  The order is selection_ref.order's
    (lnL descending, branch id ascending) from a stable numpy sort -- 5 ms instead of 70 ms per row;
    test_numpy_order_is_the_restatements_order holds the two together."""

    def __init__(self, row, exact=False):
        self.row, self.exact = np.asarray(row, np.float64), exact
        self.o = np.lexsort((np.arange(len(self.row)), -self.row)).tolist()
        lw = ref.lwr(self.row)
        self.lw = [lw[i] for i in self.o]
        self.lnl = [float(self.row[i]) for i in self.o]

    def keep(self, mode, thr):
        if mode == "dynamic":
            n = ref.until_accumulated_reached(self.lw, thr)
        elif mode == "fixed":
            n = ref.until_top_percent(len(self.row), thr)
        else:
            n = ref.baseball_count(self.lnl)
        return self.o[:n]

    def margin(self, thr):
        """selection_ref.margin on the cached order and LWRs"""
        t = float(thr)
        s, c, m = 0.0, 0.0, math.inf
        for x in self.lw:
            if not s + c < t:
                break
            y = s + x
            c += (s - y) + x if abs(s) >= abs(x) else (x - y) + s
            s = y
            m = min(m, abs((s + c) - t))
        return m

    def robust(self, thr):
        return self.exact or self.margin(thr) > 1e-10


def _expect(keep):
    """per-query kept branch lists -> (branch, query) arrays in Work order"""
    b = np.concatenate([np.asarray(ks, np.int64) for ks in keep] + [np.zeros(0, np.int64)])
    q = np.repeat(np.arange(len(keep)), [len(ks) for ks in keep])
    o = np.lexsort((q, b))
    return b[o], q[o]


def _same(p, eb, eq):
    return np.array_equal(p["branch_id"], eb) and np.array_equal(p["seq_id"], eq)


@pytest.fixture(scope="module")
def big():
    w = gen.dna_workload(N_TIPS, W, 64, 64, (201, 202, 203))
    r = hostlib.Reference(w["newick"], w["labels"], w["seqs"], states=4, subst=w["subst"], freqs=w["freqs"],
                          rates=w["rates"])
    assert r.B == B
    ev = r.evaluator()
    o = Oracle(w["newick"], w["labels"], w["seqs"], 4, w["subst"], w["freqs"], w["rates"])
    enc = epa.encode_queries(4, w["reads"])
    lnl = ev.preplace(*enc)
    d = dict(w=w, ref=r, ev=ev, o=o, enc=enc, lnl=lnl, rows=None)
    yield d
    ev.close()
    d.clear()


def _rows(big):
    if big["rows"] is None:
        big["rows"] = [_Row(r) for r in big["lnl"]]
    return big["rows"]


def test_numpy_order_is_the_restatements_order():
    rows = ref.crafted_rows(2049)
    for _, r, _ in rows[:4]:
        assert _Row(r).o == ref.order(r)
        assert _Row(r).margin(0.9) == ref.margin(r, 0.9)


# ---- 1. contexts, lookup build, preplacement ---------------------------------------------------------------
def test_contexts_tree_lnl_and_preplacement_match_oracle(big):
    o, ev, reads = big["o"], big["ev"], big["w"]["reads"]
    olnl = o.preplace(reads)
    evh = big["ref"].evaluator(device_precompute=False)
    try:
        for e in (ev, evh):
            for b in (0, 65534, 65535, 65536):
                want = o.tree_lnl(b)
                assert abs(e.tree_logl(b) - want) < 1e-7 * abs(want), b
            lnl = e.preplace(*big["enc"])
            assert lnl.shape == (64, B)
            assert np.max(np.abs(lnl - olnl)) < LNL_TOL
            e.set_option("preplace_generic", 1)
            try:
                assert np.array_equal(e.preplace(*big["enc"]), lnl)
            finally:
                e.set_option("preplace_generic", 0)
    finally:
        evh.close()
    assert np.array_equal(big["lnl"], ev.preplace(*big["enc"]))


# ---- 2. crafted tables ---------------------------------------------------------------------------------------
def test_select_on_crafted_tables_equals_restatement(big):
    """test_gpu_selection_edges.py's crafted-table test at B = 65 537: ties (all equal, a group straddling the
    cutoff, pairs at ids 63|64, 255|256, B-1|0), the maximum at B-1, LWRs that underflow or are subnormal,
    thresholds crossed exactly, -g 0 / 1e-300 / 1 - 1e-16 / 1, -G values whose x * B rounds, the baseball strike
    box: the device's pair list equals the restatement element for element, from the bitmap and the staging rows"""
    ev = big["ev"]
    rows = [_Row(r, e) for _, r, e in ref.crafted_rows(B)]
    cases = [("dynamic", t) for t in ref.DYN_THRESHOLDS] + [("fixed", x) for x in ref.fixed_fractions(B)] + \
            [("baseball", 0.0)]
    tables = []
    for mode, thr in cases:
        use = [r for r in rows if mode != "dynamic" or r.robust(thr)]
        assert use, (mode, thr)
        keep = [use[i % len(use)].keep(mode, thr) for i in range(max(QS))]
        tables.append((np.array([use[i % len(use)].row for i in range(max(QS))]),
                       {Q: _expect(keep[:Q]) for Q in QS}))
    try:
        for sort in (0, 1):
            ev.set_option("select_sort", sort)
            for (mode, thr), (table, expect) in zip(cases, tables):
                ev.set_heuristic(mode, thr if mode == "fixed" else 0.0)
                for Q in QS:
                    p = ev.select(np.ascontiguousarray(table[:Q]), Q, thr if mode == "dynamic" else 0.99999,
                                  max_pairs=Q * B)
                    assert _same(p, *expect[Q]), (sort, mode, thr, Q, len(p), len(expect[Q][0]))
    finally:
        ev.set_option("select_sort", 0)
        ev.set_heuristic("dynamic")


# ---- 3. the fused chunk body -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,param", [("dynamic", 0.99999), ("fixed", 1e-4), ("baseball", 0.0)])
def test_chunk_body_equals_restatement_and_oracle(big, mode, param):
    """place_chunk, the staged two-slot loop and one chunk_launch_many group: the pair list equals the
    restatement on the device's own preplacement table on every robust row (at least 60 of 64); lnL and
    lengths of all pairs against the oracle, optimiser statistics equal"""
    ev, o, reads = big["ev"], big["o"], big["w"]["reads"]
    codes, wb, ws = big["enc"]
    Q = len(wb)
    rows = _rows(big)
    thr = param if mode == "dynamic" else 0.99999
    qs = [q for q in range(Q) if mode != "dynamic" or rows[q].robust(thr)]
    assert len(qs) >= 60
    keep = [rows[q].keep(mode, param) if q in qs else [] for q in range(Q)]
    eb, eq = _expect(keep)
    cap = Q * 256

    def check(p, r, q0, q1, stats):
        sel = np.isin(p["seq_id"], [q - q0 for q in qs])
        m = (eq >= q0) & (eq < q1)
        assert np.array_equal(p["branch_id"][sel], eb[m]) and np.array_equal(p["seq_id"][sel] + q0, eq[m])
        tl, tp, td = o.thorough(p["branch_id"], p["seq_id"] + q0, reads)
        assert np.max(np.abs(r["lnl"] - tl)) < LNL_TOL
        assert np.max(np.abs(r["pendant_length"] - tp) / np.maximum(1.0, tp)) < 1e-6
        assert np.max(np.abs(r["distal_length"] - td)) < 1e-6
        if stats is not None:
            for k in ("reverts", "rounds", "newton_evals"):
                assert stats[k] == o.last_stats[k], k

    ev.set_heuristic(mode, param if mode == "fixed" else 0.0)
    try:
        p, r = ev.place_chunk(codes, wb, ws, threshold=thr, max_pairs=cap)
        check(p, r, 0, Q, ev.last_stats)
        half = Q // 2
        parts = [(codes[:half], wb[:half], ws[:half]), (codes[half:], wb[half:], ws[half:])]
        bounds = [(0, half), (half, Q)]
        # the staged loop, both slots in flight
        for s, c in enumerate(parts):
            ev.chunk_stage(s, *c)
        for s in range(2):
            ev.chunk_launch_begin(s, threshold=thr, max_pairs=cap)
        for s in range(2):
            ev.chunk_launch_end(s)
        for s in range(2):
            ps, rs = ev.chunk_finish(s)
            check(ps, rs, *bounds[s], None)
        # one group launch over the two staged chunks
        for s, c in enumerate(parts):
            ev.chunk_stage(s, *c)
        ev.chunk_launch_many([0, 1], threshold=thr, max_pairs=cap, host_ordered=True)
        for s in range(2):
            ps, rs = ev.chunk_finish(s)
            check(ps, rs, *bounds[s], None)
    finally:
        ev.set_heuristic("dynamic")


# ---- 4. the flat input -----------------------------------------------------------------------------------------
def test_flat_input_selection_finishes_and_equals_restatement(big):
    """The dynamic rule keeps up to 63 407 of 65 537 branches per query here: one row pass per candidate is
    ~860 000 passes over a 524 KB row for the 0.99999 call alone.  The device calls of this test (context,
    preplacement, twelve selections) must finish inside 60 s; measured: see profiles/large_tree_select.md."""
    w = big["w"]
    seqs, reads = gen.flat_reads(N_TIPS, W, 16, 64)
    r = hostlib.Reference(w["newick"], w["labels"], seqs, states=4, subst=w["subst"], freqs=w["freqs"], rates=w["rates"])
    Q = len(reads)
    enc = epa.encode_queries(4, reads)
    dev_s = 0.0
    t0 = time.monotonic()
    ev = r.evaluator()
    try:
        lnl = ev.preplace(*enc)
        dev_s += time.monotonic() - t0
        rows = [_Row(x) for x in lnl]
        cases = []
        for thr, need in ((0.9, Q), (0.99999, 12)):
            qs = [q for q in range(Q) if rows[q].robust(thr)]
            assert len(qs) >= need, (thr, len(qs))
            keep = [rows[q].keep("dynamic", thr) for q in range(Q)]
            print("flat input, dynamic %r: kept per query %d .. %d, %d pairs, %d robust rows"
                  % (thr, min(map(len, keep)), max(map(len, keep)), sum(map(len, keep)), len(qs)))
            cases.append(("dynamic", thr, qs, keep))
        cases.append(("fixed", 0.5, list(range(Q)), [rows[q].keep("fixed", 0.5) for q in range(Q)]))
        assert all(len(k) == 32769 for k in cases[-1][3])
        for sort in (0, 1):
            ev.set_option("select_sort", sort)
            for mode, thr, qs, keep in cases:
                ev.set_heuristic(mode, thr if mode == "fixed" else 0.0)
                t0 = time.monotonic()
                p = ev.select(lnl, Q, thr if mode == "dynamic" else 0.99999, max_pairs=Q * B)
                dt = time.monotonic() - t0
                dev_s += dt
                print("flat input, %s %r, select_sort %d: %d pairs in %.3f s (select kernels %.3f ms)"
                      % (mode, thr, sort, len(p), dt, ev.kernel_ms("select")))
                sel = np.isin(p["seq_id"], qs)
                eb, eq = _expect([keep[q] if q in qs else [] for q in range(Q)])
                assert np.array_equal(p["branch_id"][sel], eb) and np.array_equal(p["seq_id"][sel], eq), (sort, mode, thr)
    finally:
        ev.set_option("select_sort", 0)
        ev.set_heuristic("dynamic")
        ev.close()
    print("flat input: device calls %.2f s" % dev_s)
    assert dev_s < 60.0


# ---- 5. --no-heur on the device -----------------------------------------------------------------------------------
def test_place_all_filter_equals_restatement(big):
    ev, (codes, wb, ws) = big["ev"], big["enc"]
    Q = 8
    codes, wb, ws = codes[:Q], wb[:Q], ws[:Q]
    allp = np.zeros(B * Q, epa.PAIR_DTYPE)
    allp["branch_id"] = np.repeat(np.arange(B), Q)
    allp["seq_id"] = np.tile(np.arange(Q), B)
    full = ev.thorough(allp, codes, wb, ws)["lnl"].reshape(B, Q)
    out = ev.place_all(codes, wb, ws, min_lwr=0.01, acc=False, filter_min=1, filter_max=7)
    for q in range(Q):
        exp = ref.filter_pquery(list(full[:, q]), list(range(B)), 0.01, False, 1, 7)
        bids, lnls, _, _, lwrs = out[q]
        assert bids.tolist() == [b for b, _ in exp], q
        assert np.array_equal(lnls, full[bids, q])
        assert np.max(np.abs(lwrs - np.array([x for _, x in exp]))) < 1e-12


# ---- 6. the CLI ----------------------------------------------------------------------------------------------------
def test_cli_paths_give_identical_jplace_and_report_the_path(big, tmp_path):
    w = big["w"]
    tf, sf, qf = tmp_path / "ref.tre", tmp_path / "ref.fasta", tmp_path / "q.fasta"
    tf.write_text(w["newick"] + "\n")
    sf.write_text("".join(">%s\n%s\n" % (l, s) for l, s in zip(w["labels"], w["seqs"])))
    qf.write_text("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(w["reads"])))
    model = "GTR{%s}+FU{%s}+G4{%r}" % ("/".join(map(repr, synth.CFG2_SUBST)), "/".join(map(repr, synth.CFG2_FREQS)),
                                         synth.CFG2_ALPHA)
    exe = hostlib.cli_exe()

    def run(name, *flags):
        d = tmp_path / name
        d.mkdir()
        sj = d / "stats.json"
        cmd = [exe, "-t", str(tf), "-s", str(sf), "-q", str(qf), "-m", model, "-w", str(d), "--stats-json", str(sj)]
        proc = subprocess.Popen(cmd + list(flags), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        try:
            out, _ = proc.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            proc.kill()
            proc.communicate()
            raise
        assert proc.returncode == 0, out
        doc = json.loads(open(d / "epa_result.jplace").read())
        doc.pop("metadata")
        return doc, json.loads(sj.read_text())

    a, sa = run("default")
    assert len(a["placements"]) == len(w["reads"])
    assert sa["chunk_path"] == "pipelined" and sa["device_chunk"] >= 1
    assert sa["queries"] == len(w["reads"]) and "loop_s" in sa
    b, sb = run("hostheur", "--host-heuristic")
    assert sb["chunk_path"] == "host"
    assert a == b
    c, sc = run("nopipe", "--no-pipeline")
    assert sc["chunk_path"] == "fused"
    assert a == c
