"""GPU tests of candidate selection and the --no-heur LWR filter at ties, underflow and kernel-class edges,
against the plain restatement of the reference (selection_ref.py): crafted tables through every k_select
class (Evaluator.select, bitmap and sorted-staging emit), a reference with duplicated taxa in cherries
through the fused chunk body (k_select_seg, the full-row kernels, a group launch) and epa_dev_place_all
(k_lwr_filter), and the CLI's device and host paths on the same input."""
import json
import subprocess

import numpy as np
import pytest

import epa_ng_amd as epa
from epa_ng_amd import hostlib, synth
from oracle_lib import Oracle
import selection_ref as ref

pytestmark = pytest.mark.gpu

# one reference per selection kernel class: B = 2n - 3 just past a boundary
# (k_select<2, 2, 4, 8, 16, 32, 64>, k_select_wg<32>, k_select_wg<64>, k_select_big<16>)
SIZES = [3, 63, 129, 257, 513, 1025, 2049, 4097, 8193, 16385]
QS = (1, 31, 33, 65)


@pytest.fixture(scope="module")
def evaluators():
    cache = {}

    def get(B):
        if B not in cache:
            n = (B + 3) // 2
            w = synth.dna_workload(n, 24, 2, 24, (201, 202, 203))
            r = hostlib.Reference(w["newick"], w["labels"], w["seqs"], states=4, subst=w["subst"],
                                  freqs=w["freqs"], rates=w["rates"])
            assert r.B == B
            cache[B] = (r, r.evaluator())
        return cache[B][1]
    yield get
    cache.clear()


def _expect(keep):
    """per-query kept branch lists -> (branch, query) arrays in Work order"""
    b = np.concatenate([np.asarray(ks, np.int64) for ks in keep] + [np.zeros(0, np.int64)])
    q = np.repeat(np.arange(len(keep)), [len(ks) for ks in keep])
    o = np.lexsort((q, b))
    return b[o], q[o]


class _Row:
    """one crafted row with its selection order and LWRs computed once"""

    def __init__(self, row, exact):
        self.row, self.exact = row, exact
        self.o = ref.order(row)
        lw = ref.lwr(row)
        self.lw = [lw[i] for i in self.o]
        self.lnl = [float(row[i]) for i in self.o]

    def keep(self, mode, thr):
        if mode == "dynamic":
            n = ref.until_accumulated_reached(self.lw, thr)
        elif mode == "fixed":
            n = ref.until_top_percent(len(self.row), thr)
        else:
            n = ref.baseball_count(self.lnl)
        return self.o[:n]


@pytest.mark.parametrize("B", SIZES)
def test_select_on_crafted_tables_equals_restatement(evaluators, B):
    """ties (all equal, a group straddling the cutoff, pairs at ids 63|64, 255|256, B-1|0), the maximum at B-1,
    LWRs that underflow or are subnormal, thresholds crossed exactly (0.25 steps), -g 0 / 1e-300 / 1 - 1e-16 / 1,
    -G values whose x * B rounds, baseball values exactly 3.0 below the best: the device's pair list equals the
    restatement element for element, for the three rules, from the bitmap and from the sorted staging rows"""
    ev = evaluators(B)
    rows = [_Row(r, e) for _, r, e in ref.crafted_rows(B)]
    cases = [("dynamic", t) for t in ref.DYN_THRESHOLDS] + [("fixed", x) for x in ref.fixed_fractions(B)] + \
            [("baseball", 0.0)]
    tables = []
    for mode, thr in cases:
        use = [r for r in rows if mode != "dynamic" or ref.robust(r.row, thr, r.exact)]
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
                    eb, eq = expect[Q]
                    assert np.array_equal(p["branch_id"], eb) and np.array_equal(p["seq_id"], eq), \
                        (B, sort, mode, thr, Q)
    finally:
        ev.set_option("select_sort", 0)
        ev.set_heuristic("dynamic")


# ---- a reference with duplicated taxa ------------------------------------------------------------------
def _tie_workload():
    """random tree of 40 tips; 6 of them become cherries of two identical sequences (3 at branch length
    1e-6, 3 at 0.05); reference tips with gap runs and IUPAC codes; reads copied from the duplicated taxa:
    short ones, long ones (>= 1000 columns: LWRs underflow) and mostly-N ones"""
    rng = np.random.RandomState(31)
    W = 1200
    root = synth.random_tree(40, 301)
    leaves = []

    def walk(n):
        if n.kids:
            for k in n.kids:
                walk(k)
        else:
            leaves.append(n)
    walk(root)
    dups, nxt = [], 40
    for j, leaf in enumerate(leaves[:6]):
        bl = 1e-6 if j < 3 else 0.05
        a, b = synth.Node(leaf.label), synth.Node("t%d" % nxt)
        a.length = b.length = bl
        leaf.kids, leaf.label = [a, b], None
        dups.append((a.label, b.label))
        nxt += 1
    rates = synth.gamma_rates(synth.CFG2_ALPHA)
    labels, seqs = synth.simulate_msa(root, W, synth.CFG2_SUBST, synth.CFG2_FREQS, rates, 302)
    seqs = dict(zip(labels, seqs))
    for a, b in dups:
        s = list(seqs[a])
        for st in rng.randint(0, W - 40, 3):                 # gap runs
            ln = rng.randint(5, 30)
            s[st:st + ln] = "-" * ln
        for k in rng.randint(0, W, 6):                        # IUPAC codes
            s[k] = "RYKMSWN"[rng.randint(7)]
        seqs[a] = seqs[b] = "".join(s)
    dup_labels = {x for d in dups for x in d}
    for lab in [l for l in labels if l not in dup_labels][:6]:   # gaps and codes in other tips as well
        s = list(seqs[lab])
        st = rng.randint(0, W - 50)
        s[st:st + 50] = "-" * 50
        s[rng.randint(W)] = "Y"
        seqs[lab] = "".join(s)
    reads = []
    for a, _ in dups:
        src = seqs[a].replace("-", "A")
        for ln in (80, 150):                                   # short
            st = rng.randint(0, W - ln)
            reads.append("-" * st + src[st:st + ln] + "-" * (W - st - ln))
        st = rng.randint(0, W - 1100)                          # long
        reads.append("-" * st + src[st:st + 1100] + "-" * (W - st - 1100))
        r = np.array(list(src))                                # mostly N
        r[rng.rand(W) < 0.95] = "N"
        reads.append("".join(r))
    model = "GTR{%s}+FU{%s}+G4{%r}" % ("/".join(map(repr, synth.CFG2_SUBST)), "/".join(map(repr, synth.CFG2_FREQS)),
                                         synth.CFG2_ALPHA)
    return dict(newick=synth.newick(root), labels=labels, seqs=[seqs[l] for l in labels], rates=rates,
                reads=reads, dups=dups, model=model)


@pytest.fixture(scope="module")
def ties():
    w = _tie_workload()
    r = hostlib.Reference(w["newick"], w["labels"], w["seqs"], states=4, subst=synth.CFG2_SUBST,
                          freqs=synth.CFG2_FREQS, rates=w["rates"])
    ev = r.evaluator()
    o = Oracle(w["newick"], w["labels"], w["seqs"], 4, synth.CFG2_SUBST, synth.CFG2_FREQS, w["rates"])
    codes, wb, ws = epa.encode_queries(4, w["reads"])      # aligned rows: the mostly-N reads span the width
    # branch id of every tip's pendant edge, from the numbered tree ("label:length{id}")
    import re
    edge = {lab: int(e) for lab, e in re.findall(r"(t\d+):[-0-9.e+]+\{(\d+)\}", r.numbered_newick())}
    pairs = [(edge[a], edge[b]) for a, b in w["dups"]]
    lnl = ev.preplace(codes, wb, ws)
    return dict(w=w, ref=r, ev=ev, o=o, enc=(codes, wb, ws), lnl=lnl, tied=pairs)


def test_duplicated_taxa_preplacement_is_tied_and_matches_oracle(ties):
    lnl = ties["lnl"]
    assert np.max(np.abs(lnl - ties["o"].preplace(ties["w"]["reads"]))) < 1e-6
    for a, b in ties["tied"]:
        assert np.array_equal(lnl[:, a], lnl[:, b]), (a, b)
    long_reads = range(2, len(lnl), 4)
    assert all(0.0 in ref.lwr(lnl[q]) for q in long_reads)        # long reads: LWRs underflow to 0


def _restated(lnl, thr, qs):
    keep = [ref.select_row(list(lnl[q]), "dynamic", thr) if q in qs else [] for q in range(len(lnl))]
    return _expect(keep)


def test_chunk_candidates_at_ties_equal_restatement(ties):
    """place_chunk through k_select_seg (default), the full-row kernel and the sorted staging path, and a
    two-slot group launch: the candidates of every query whose decision float64 rounding cannot flip
    equal the restatement on the device's own table; tied branches give bit-equal thorough results that
    match the oracle"""
    ev, lnl = ties["ev"], ties["lnl"]
    codes, wb, ws = ties["enc"]
    Q, B = len(wb), ties["ref"].B
    reads = ties["w"]["reads"]
    ev.set_heuristic("dynamic")
    for thr in (0.9, 0.99999, 1.0 - 1e-9):
        qs = {q for q in range(Q) if ref.robust(lnl[q], thr)}
        assert len(qs) >= Q // 2
        eb, eq = _restated(lnl, thr, qs)
        got = {}
        for name, opt in (("seg", None), ("full", "select_full_rows"), ("sort", "select_sort")):
            if opt:
                ev.set_option(opt, 1)
            try:
                got[name] = ev.place_chunk(codes, wb, ws, threshold=thr, max_pairs=Q * B)
            finally:
                if opt:
                    ev.set_option(opt, 0)
        half = Q // 2
        parts = [(codes[:half], wb[:half], ws[:half]), (codes[half:], wb[half:], ws[half:])]
        for s, c in enumerate(parts):
            ev.chunk_stage(s, *c)
        ev.chunk_launch_many([0, 1], threshold=thr, max_pairs=Q * B, host_ordered=True)
        grp = [ev.chunk_finish(s) for s in range(2)]
        for s, (p, r) in enumerate(grp):
            e = ev.place_chunk(*parts[s], threshold=thr, max_pairs=Q * B)
            assert np.array_equal(p, e[0]) and np.array_equal(r, e[1]), (thr, s)
        for name, (p, r) in got.items():
            assert np.array_equal(p, got["seg"][0]) and np.array_equal(r, got["seg"][1]), (thr, name)
            m = np.isin(p["seq_id"], sorted(qs))
            assert np.array_equal(p["branch_id"][m], eb) and np.array_equal(p["seq_id"][m], eq), (thr, name)
        p, r = got["seg"]
        tl, tp, td = ties["o"].thorough(p["branch_id"], p["seq_id"], reads)
        assert np.max(np.abs(r["lnl"] - tl)) < 1e-6
        assert np.max(np.abs(r["pendant_length"] - tp) / np.maximum(1.0, tp)) < 1e-6
        assert np.max(np.abs(r["distal_length"] - td)) < 1e-6
        at = {(int(b), int(q)): k for k, (b, q) in enumerate(zip(p["branch_id"], p["seq_id"]))}
        n_tied = 0
        for a, b in ties["tied"]:
            for q in range(Q):
                if (a, q) in at and (b, q) in at:
                    ra, rb = r[at[(a, q)]], r[at[(b, q)]]
                    assert ra["lnl"] == rb["lnl"] and ra["pendant_length"] == rb["pendant_length"] and \
                        ra["distal_length"] == rb["distal_length"], (a, b, q)
                    n_tied += 1
        assert n_tied > 0


@pytest.mark.parametrize("thresh,acc,mn,mx", [(0.01, False, 1, 7), (0.0, False, 10, 64), (0.5, False, 64, 64),
                                              (0.99, True, 5, 5), (0.9999, True, 1, 64)])
def test_place_all_filter_at_ties_equals_restatement(ties, thresh, acc, mn, mx):
    """epa_dev_place_all (k_lwr_filter) against compute_and_set_lwr + filter restated on the thorough lnLs of
    every pair: ties, top-ups into zero-LWR placements, filter_max 64, filter_min == filter_max; LWRs within
    1e-12 of the restatement's"""
    ev, (codes, wb, ws) = ties["ev"], ties["enc"]
    Q, B = len(wb), ties["ref"].B
    allp = np.zeros(B * Q, epa.PAIR_DTYPE)
    allp["branch_id"] = np.repeat(np.arange(B), Q)
    allp["seq_id"] = np.tile(np.arange(Q), B)
    full = ev.thorough(allp, codes, wb, ws)["lnl"].reshape(B, Q)
    out = ev.place_all(codes, wb, ws, min_lwr=thresh, acc=acc, filter_min=mn, filter_max=mx)
    checked = 0
    for q in range(Q):
        row = list(full[:, q])
        if acc and ref.margin(row, thresh) <= 1e-10:
            continue
        exp = ref.filter_pquery(row, list(range(B)), thresh, acc, mn, mx)
        bids, lnls, _, _, lwrs = out[q]
        assert bids.tolist() == [b for b, _ in exp], q
        assert np.array_equal(lnls, full[bids, q])
        assert np.max(np.abs(lwrs - np.array([w for _, w in exp]))) < 1e-12
        checked += 1
    assert checked >= Q // 2


# ---- the CLI: device and host paths give the same jplace -------------------------------------------------
def test_cli_device_and_host_paths_give_identical_jplace(ties, tmp_path):
    """--no-heur with --filter-max 64 (device filter) and 65 (host filter); -G 0.3 and -g 0 with and without
    --host-heuristic: the same jplace (the invocation aside).  The host-selection path writes its pqueries in
    more post-processing parts, and the parts are joined by "\n,\n" where a part's own pqueries are joined by
    ",\n": the documents are compared as parsed JSON, every value exactly"""
    w = ties["w"]
    tf, sf, qf = tmp_path / "ref.tre", tmp_path / "ref.fasta", tmp_path / "q.fasta"
    tf.write_text(w["newick"] + "\n")
    sf.write_text("".join(">%s\n%s\n" % (l, s) for l, s in zip(w["labels"], w["seqs"])))
    qf.write_text("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(w["reads"])))
    exe = hostlib.cli_exe()

    def run(name, *flags):
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run([exe, "-t", str(tf), "-s", str(sf), "-q", str(qf), "-m", w["model"], "-w", str(d)]
                           + list(flags), capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        doc = json.loads(open(d / "epa_result.jplace").read())
        doc.pop("metadata")
        return doc, doc["placements"]

    a, pa = run("nh64", "--no-heur", "--filter-min", "10", "--filter-max", "64")
    b, _ = run("nh65", "--no-heur", "--filter-min", "10", "--filter-max", "65")
    assert a == b
    assert len(pa) == len(w["reads"]) and all(len(p["p"]) >= 10 for p in pa)
    assert any(p["p"][-1][2] == 0.0 for p in pa)          # the top-ups reach zero-LWR placements
    g, pg = run("G", "-G", "0.3")
    assert g == run("Gh", "-G", "0.3", "--host-heuristic")[0] and len(pg) == len(w["reads"])
    g0, _ = run("g0", "-g", "0")
    assert g0 == run("g0h", "-g", "0", "--host-heuristic")[0]
