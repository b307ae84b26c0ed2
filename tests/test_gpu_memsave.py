"""GPU tests of the blocked lookup layout (EPA_FLAG_LOOKUP_BLOCKS / _AUTO, include/epa_dev.h): a context that keeps
only refT / scSum resident and rebuilds lookup / lookup2 per branch block inside every chunk body.

Every test first asserts that its context really is in the blocked layout (lookup_mode()).  References: a resident
context of the same reference (preplacement tables and candidate lists must be the same bits: the tables are a pure
function of refT, and a cell's summation order does not depend on the block size) and the CPU oracle with the suite's
tolerances (test_gpu_parity.py: 1e-6 on lnL and lengths).

Newton results with and without the cached starting vectors (refI: resident contexts read them, blocked contexts
compute them in the kernel) are NOT the same bits.  Measured on MI355X over every case of this file: the candidate
lists are identical, lnL differs by at most 3.4e-12 (|lnL| ~ 2e4: a few ulp), lengths by at most 2.5e-14 -- the
in-kernel path forms the inner CLV with the kernel's own fused operations, the lookup build with its own (DESIGN
section 4.3).  So blocked against resident is asserted at 1e-6 on lnL and 1e-6 relative on lengths, on every pair
(no exclusions), and the measured differences are printed."""
import json
import os
import subprocess

import numpy as np
import pytest

import epa_ng_amd as epa
from epa_ng_amd import hostlib, synth
from golden_util import GOLDEN, load_case
from oracle_lib import Oracle
from preplace_ref import _seg_values

import large_tree_gen as gen

pytestmark = pytest.mark.gpu

LNL_TOL = 1e-6
BLOCKS = epa.FLAG_LOOKUP_BLOCKS


def blocked(ref, blk=None, **kw):
    ev = ref.evaluator(flags=BLOCKS, **kw)
    if blk is not None:
        ev.set_option("lookup_block", blk)
    assert ev.lookup_mode() == (epa.LOOKUP_BLOCKS, blk if blk is not None else 1024)
    return ev


def resident(ref, **kw):
    ev = ref.evaluator(**kw)
    assert ev.lookup_mode() == (epa.LOOKUP_RESIDENT, 0)
    return ev


def reference_of(w, states=4, **kw):
    return hostlib.Reference(w["newick"], w["labels"], w["seqs"], states=states, subst=w["subst"], freqs=w["freqs"],
                             rates=w["rates"], **kw)


def with_rare_codes(reads, every=3, seed=77):
    """every `every`-th read gets a few two- and three-state ambiguity codes inside its window (k_preplace's queries)"""
    rng = np.random.RandomState(seed)
    out = []
    for i, r in enumerate(reads):
        if i % every == 0:
            pos = [j for j, ch in enumerate(r) if ch != "-"]
            r = list(r)
            for j in rng.choice(pos, size=min(3, len(pos)), replace=False):
                r[j] = "RYKMSWBDHV"[rng.randint(10)]
            r = "".join(r)
        out.append(r)
    return out


def assert_thorough_parity(res, o, pairs, reads, q0=0):
    tl, tp, td = o.thorough(pairs["branch_id"], pairs["seq_id"] + q0, reads)
    assert np.max(np.abs(res["lnl"] - tl)) < LNL_TOL
    assert np.max(np.abs(res["pendant_length"] - tp) / np.maximum(1.0, tp)) < 1e-6
    assert np.max(np.abs(res["distal_length"] - td)) < 1e-6


def report_vs_resident(what, r_blk, r_res):
    """blocked (starting vectors computed in the kernel) against resident (read from refI): the finding is printed,
    the caller asserts"""
    same = all(np.array_equal(r_blk[k], r_res[k]) for k in ("lnl", "pendant_length", "distal_length"))
    d = [float(np.max(np.abs(r_blk[k] - r_res[k]))) if len(r_blk) else 0.0 for k in ("lnl", "pendant_length", "distal_length")]
    print("%s: %d pairs, blocked vs resident bit-identical: %s (max |d| lnl %.3g pendant %.3g distal %.3g)"
          % (what, len(r_blk), same, d[0], d[1], d[2]))
    return same


def assert_same_results(what, r_blk, r_res):
    """blocked against resident Newton results: not the same bits (module docstring), so 1e-6 on lnL and 1e-6
    relative on the lengths, every pair"""
    report_vs_resident(what, r_blk, r_res)
    assert len(r_blk) == len(r_res)
    assert np.all(np.abs(r_blk["lnl"] - r_res["lnl"]) < LNL_TOL), what
    for k in ("pendant_length", "distal_length"):
        assert np.all(np.abs(r_blk[k] - r_res[k]) <= 1e-6 * np.abs(r_res[k])), (what, k)


# ---- 1. preplacement tables ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tips", [8, 512])      # B = 13 and 1021: not multiples of 64
def test_preplace_table_dna_bit_identical(n_tips):
    w = synth.dna_workload(n_tips, 600, 1500, 150, (31, 32, 33))
    ref = reference_of(w)
    assert ref.B == 2 * n_tips - 3 and ref.B % 64
    base = w["seqs"][1]
    long_reads = ["-" * 20 + base[20:20 + n] + "-" * (600 - 20 - n) for n in (161, 200, 333, 580)]   # spans above the chunk length
    reads = with_rare_codes(w["reads"]) + long_reads
    full = epa.encode_queries(4, reads)
    compact = epa.encode_queries(4, reads, compact=True)
    packed = (epa.pack_codes_4bit(compact[0]), compact[1], compact[2])
    evr = resident(ref)
    want = evr.preplace(*full)
    assert np.array_equal(evr.preplace(*compact), want)
    for blk in (64, 128, 1024):
        ev = blocked(ref, blk)
        for name, enc in (("full", full), ("compact", compact), ("4bit", packed)):
            got = ev.preplace(*enc)
            assert np.array_equal(got, want), (blk, name, float(np.max(np.abs(got - want))))
        assert ev.kernel_ms("lookup_block") > 0.0 and ev.kernel_ms("preplace") > 0.0 and ev.kernel_ms("lookup") < 0.0
        ev.set_option("preplace_generic", 1)
        assert np.array_equal(ev.preplace(*full), want), (blk, "generic")
        ev.set_option("preplace_generic", 0)
        # window errors found by the once-per-chunk prologue survive the block loop
        bad = full[2].copy()
        bad[len(bad) // 2] = 0
        with pytest.raises(epa.EpaError) as e:
            ev.preplace(full[0], full[1], bad)
        assert e.value.code == -5
        ev.build_lookup()                      # a no-op on a blocked context
        assert ev.kernel_ms("lookup") < 0.0
        ev.close()
    evr.close()


@pytest.mark.parametrize("n_tips", [96, 512])      # B = 189 and 1021
def test_preplace_single_chunk_kernels_table_and_segment_maxima(n_tips):
    """Evaluator.preplace leaves the span bound open and so always runs the accumulating pair kernel.  With the bound
    the fused chunk body passes (150 sites) the narrow kernel (9000 reads: Q x 96 >= 1400 x W) and the wide one (900
    reads) run: they write the table in 64-byte bursts at d_lnl + b0 and the segment maxima at segmax + b0 / 64.
    Every cell of the table and every key must be the resident context's."""
    w = synth.dna_workload(n_tips, 600, 9000, 150, (81, 82, 83))
    ref = reference_of(w)
    B = ref.B
    assert B % 64
    codes, wb, ws = epa.encode_queries(4, with_rare_codes(w["reads"], every=11), compact=True)
    evr = resident(ref)
    want = {}
    for n in (9000, 900):
        c = (codes[:n], wb[:n], ws[:n])
        tab, keys = evr.preplace_bounded(*c, 150, seg_keys=True)
        assert np.max(np.abs(tab - evr.preplace(*c))) < 1e-9          # the accumulating kernel's table
        vals = _seg_values(keys)[:, :(B + 63) // 64]
        written = ~np.isnan(vals)
        rare = np.arange(n) % 11 == 0                                  # served by k_preplace: no keys
        assert not written[rare].any() and written[~rare].all()
        pad = np.full((n, (B + 63) // 64 * 64), -np.inf)
        pad[:, :B] = tab
        assert np.array_equal(vals[~rare], pad.reshape(n, -1, 64).max(axis=2)[~rare])
        want[n] = (tab, keys)
    for blk in (64, 128, 1024):
        ev = blocked(ref, blk)
        for n in (9000, 900):
            tab, keys = ev.preplace_bounded(codes[:n], wb[:n], ws[:n], 150, seg_keys=True)
            assert np.array_equal(tab, want[n][0]), (blk, n, float(np.max(np.abs(tab - want[n][0]))))
            assert np.array_equal(keys, want[n][1]), (blk, n)
        ev.close()
    with pytest.raises(epa.EpaError):                                  # a window above the bound is refused
        evr.preplace_bounded(codes[:10], wb[:10], ws[:10], 100)
    evr.close()


def test_preplace_table_20_states_bit_identical():
    w = synth.aa_workload(70, 260, 400, 90, (41, 42, 43))
    ref = reference_of(w, states=20)
    assert ref.B == 137
    reads = w["reads"] + [w["seqs"][2]]       # one full-width window
    full = epa.encode_queries(20, reads)
    compact = epa.encode_queries(20, reads, compact=True)
    evr = resident(ref)
    want = evr.preplace(*full)
    for blk in (64, 128, 192):
        ev = blocked(ref, blk)
        assert np.array_equal(ev.preplace(*full), want), blk
        assert np.array_equal(ev.preplace(*compact), want), blk
        short = [i for i in range(len(reads)) if compact[2][i] <= 128]      # k_preplace_sites<24, false>
        cs = tuple(a[short] for a in compact)
        assert np.array_equal(ev.preplace_bounded(*cs, 128), evr.preplace_bounded(*cs, 128)), blk
        ev.set_option("preplace_generic", 1)
        assert np.array_equal(ev.preplace(*full), want), (blk, "generic")
        ev.close()
    evr.close()


def test_lookup_block_option_is_validated():
    w = synth.dna_workload(8, 100, 4, 50, (21, 22, 23))
    ref = reference_of(w)
    ev = blocked(ref)
    for bad in (0, -64, 100, 63):
        with pytest.raises(epa.EpaError) as e:
            ev.set_option("lookup_block", bad)
        assert e.value.code == -1
    ev.set_option("lookup_block", 128)
    assert ev.lookup_mode() == (epa.LOOKUP_BLOCKS, 128)
    ev.preplace(*epa.encode_queries(4, w["reads"]))
    with pytest.raises(epa.EpaError):          # the bank's block buffer exists now
        ev.set_option("lookup_block", 64)
    ev.close()
    evr = resident(ref)
    with pytest.raises(epa.EpaError) as e:
        evr.set_option("lookup_block", 64)
    assert e.value.code == -1
    evr.close()


# ---- 2. the fused chunk body -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid():
    """189 branches (three blocks of 64), reads with rare codes; 9000 reads of 150 sites on 600 columns take the narrow
    pair path (launch_preplace: Q x 96 >= 1400 x W), a 900-read chunk the wide one, max_span = 0 the accumulating one"""
    w = synth.dna_workload(96, 600, 9000, 150, (61, 62, 63))
    ref = reference_of(w)
    assert ref.B == 189
    reads = with_rare_codes(w["reads"], every=11)
    o = Oracle(w["newick"], w["labels"], w["seqs"], 4, w["subst"], w["freqs"], w["rates"])
    d = dict(w=w, ref=ref, reads=reads, o=o, enc=epa.encode_queries(4, reads, compact=True))
    yield d
    d.clear()


@pytest.mark.parametrize("mode,param,full_rows", [("dynamic", 0.99999, 0), ("dynamic", 0.99, 1), ("fixed", 0.02, 0),
                                                  ("baseball", 0.0, 0)])
def test_chunk_body_place_chunk_equals_resident_and_oracle(mid, mode, param, full_rows):
    ref, o, reads = mid["ref"], mid["o"], mid["reads"]
    codes, wb, ws = mid["enc"]
    thr = param if mode == "dynamic" else 0.99999
    evr = resident(ref)
    ev = blocked(ref, 64)
    for e in (evr, ev):
        e.set_heuristic(mode, param if mode == "fixed" else 0.0)
        e.set_option("select_full_rows", full_rows)
    # (reads, max_span): narrow, wide and accumulating pair kernels
    for n, max_span in ((9000, 150), (900, 150), (900, 0)):
        c = (codes[:n], wb[:n], ws[:n])
        pr, rr = evr.place_chunk(*c, threshold=thr, max_span=max_span, max_pairs=n * 64)
        pb, rb = ev.place_chunk(*c, threshold=thr, max_span=max_span, max_pairs=n * 64)
        assert len(pr) > n // 2
        assert np.array_equal(pb, pr), (n, max_span)
        assert_same_results("place_chunk %s %d reads max_span %d" % (mode, n, max_span), rb, rr)
        if n == 900:
            assert_thorough_parity(rb, o, pb, reads)
    ev.close()
    evr.close()


def test_chunk_body_slot_pipeline_and_groups(mid):
    ref, o, reads = mid["ref"], mid["o"], mid["reads"]
    codes, wb, ws = mid["enc"]
    n = 600
    chunks = [(codes[i * n:(i + 1) * n], wb[i * n:(i + 1) * n], ws[i * n:(i + 1) * n]) for i in range(4)]
    evr = resident(ref)
    want = [evr.place_chunk(*c, max_span=150, max_pairs=n * 64) for c in chunks]
    # EPA_CHUNK_HOST_ORDERED as the very first call of a cold context: nothing may depend on a lookup build elsewhere
    ev = blocked(ref, 64)
    ev.chunk_stage(3, *chunks[0])
    ev.chunk_launch(3, max_span=150, max_pairs=n * 64, host_ordered=True)
    p, r = ev.chunk_finish(3)
    assert np.array_equal(p, want[0][0])
    assert_same_results("host-ordered first call", r, want[0][1])
    assert_thorough_parity(r, o, p, reads)
    # two and three chunks in flight, each on a slot (and block buffer) of its own
    for depth in (2, 3):
        for s in range(depth):
            ev.chunk_stage(s, *chunks[s])
        for s in range(depth):
            ev.chunk_launch_begin(s, max_span=150, max_pairs=n * 64, host_ordered=True)
        for s in range(depth):
            ev.chunk_launch_end(s)
        for s in range(depth):
            p, r = ev.chunk_finish(s)
            assert np.array_equal(p, want[s][0]), (depth, s)
            assert_same_results("pipeline depth %d slot %d" % (depth, s), r, want[s][1])
            assert_thorough_parity(r, o, p, reads, q0=s * n)
    # one group launch over four small chunks
    for s in range(4):
        ev.chunk_stage(4 + s, *chunks[s])
    ev.chunk_launch_many([4, 5, 6, 7], max_span=150, max_pairs=4 * n * 64, host_ordered=True)
    for s in range(4):
        p, r = ev.chunk_finish(4 + s)
        assert np.array_equal(p, want[s][0]), s
        assert_same_results("group member %d" % s, r, want[s][1])
        assert_thorough_parity(r, o, p, reads, q0=s * n)
    ev.close()
    evr.close()


# ---- 3. one case per model / optimiser shape, blocked against the oracle -----------------------------------------
def _small_case(states, cats, pinv, seed):
    rng = np.random.RandomState(100 + cats)
    if cats == 4:
        rates, weights = synth.gamma_rates(0.7), None
    else:
        rates = np.sort(rng.gamma(0.7, 1.5, cats)) + 1e-3
        weights = rng.dirichlet(np.full(cats, 4.0))
        rates = rates / np.sum(rates * weights)
    subst, freqs = (synth.CFG2_SUBST, synth.CFG2_FREQS) if states == 4 else synth.aa_model(3)
    root = synth.random_tree(40, seed)
    labels, seqs = synth.simulate_msa(root, 260, subst, freqs, synth.gamma_rates(0.7), seed + 1)
    nw = synth.newick(root)
    reads, _ = synth.make_reads(seqs, 48, 150 if states == 4 else 90, 0.05, seed + 2, states=states)
    ref = hostlib.Reference(nw, labels, seqs, states=states, subst=subst, freqs=freqs, rates=rates, weights=weights,
                            pinv=pinv)
    return ref, (nw, labels, seqs, states, subst, freqs, rates), dict(weights=weights, pinv=pinv), reads


@pytest.mark.parametrize("name,states,cats,pinv,kw", [
    ("sliding", 4, 4, 0.0, {}), ("raxml_blo", 4, 4, 0.0, {"raxml_blo": True}), ("plus_I", 4, 4, 0.2, {}),
    ("8_categories", 4, 8, 0.0, {}), ("rate_scalers", 4, 4, 0.0, {"rate_scalers": True}),
    ("aa_8_categories", 20, 8, 0.0, {}), ("aa_raxml_blo", 20, 4, 0.0, {"raxml_blo": True})])
def test_blocked_shapes_against_oracle(name, states, cats, pinv, kw):
    ref, oargs, okw, reads = _small_case(states, cats, pinv, 7 + cats)
    o = Oracle(*oargs, rate_scalers=bool(kw.get("rate_scalers")), **okw)
    if kw.get("raxml_blo"):
        o.set_raxml_blo(True)
    ev = blocked(ref, 64, **kw)
    assert ref.B == 77                      # two blocks
    assert abs(ev.tree_logl(2) - o.tree_lnl(2)) < 1e-7 * abs(o.tree_lnl(2))
    codes, wb, ws = epa.encode_queries(states, reads, compact=True)
    lnl = ev.preplace(codes, wb, ws)
    assert np.max(np.abs(lnl - o.preplace(reads))) < LNL_TOL
    p, r = ev.place_chunk(codes, wb, ws)
    assert len(p) >= len(reads)
    assert_thorough_parity(r, o, p, reads)
    assert ev.last_stats["rounds"] == o.last_stats["rounds"]
    assert ev.last_stats["newton_evals"] == o.last_stats["newton_evals"]
    evr = resident(ref, **kw)
    assert np.array_equal(evr.preplace(codes, wb, ws), lnl)
    p2, r2 = evr.place_chunk(codes, wb, ws)
    assert np.array_equal(p2, p)
    assert_same_results(name, r, r2)
    ev.close()
    evr.close()


def test_place_all_allocates_no_block_buffer():
    ref, oargs, okw, reads = _small_case(4, 4, 0.0, 11)
    o = Oracle(*oargs, **okw)
    bank = epa.footprint(4, 4, ref.W, ref.B, flags=BLOCKS, block_branches=1024)["bank"]
    assert bank == 128 * 260 * (128 + 288)   # 13.8 MB: far above what eight queries need otherwise
    warm = blocked(ref)                      # code objects and the runtime's own buffers: not part of the measurement
    enc = epa.encode_queries(4, reads[:8], compact=True)
    warm.place_all(*enc)
    warm.preplace(*enc)
    warm.close()
    ev = blocked(ref)
    f0 = ev.mem_info()[0]
    out = ev.place_all(*enc, min_lwr=0.0, filter_max=64)
    f1 = ev.mem_info()[0]
    assert f0 - f1 < bank // 2, (f0 - f1, bank)
    ev.preplace(*enc)                        # the first preplacement brings the buffer
    f2 = ev.mem_info()[0]
    assert f1 - f2 >= 0.9 * bank, (f1 - f2, bank)
    allp = np.zeros(ref.B * 8, epa.PAIR_DTYPE)
    allp["branch_id"] = np.repeat(np.arange(ref.B), 8)
    allp["seq_id"] = np.tile(np.arange(8), ref.B)
    tl, _, _ = o.thorough(allp["branch_id"], allp["seq_id"], reads[:8])
    tl = tl.reshape(ref.B, 8)
    for q in range(8):
        bids, lnls = out[q][0], out[q][1]
        assert 1 <= len(bids) <= 64
        assert np.max(np.abs(lnls - tl[bids, q])) < LNL_TOL
    ev.close()


# ---- 4. / 5. memory, on the 32 770-tip x 96-site tree ---------------------------------------------------------------
N_TIPS, W_BIG, B_BIG = 32770, 96, 65537


@pytest.fixture(scope="module")
def big():
    w = gen.dna_workload(N_TIPS, W_BIG, 64, 64, (201, 202, 203))
    ref = reference_of(w)
    assert ref.B == B_BIG
    d = dict(w=w, ref=ref, enc=epa.encode_queries(4, w["reads"]))
    yield d
    d.clear()


def test_memory_drop_matches_footprint(big):
    ref, enc = big["ref"], big["enc"]
    fp_res = epa.footprint(4, 4, W_BIG, B_BIG, banks=1)
    fp_blk = epa.footprint(4, 4, W_BIG, B_BIG, flags=BLOCKS, banks=1)
    saved = fp_res["steady"] - fp_blk["steady"]
    assert saved > 3.3e9                      # tables + refI: about 3.4 GB
    warm = resident(ref)                      # first launches: code objects, the runtime's own buffers
    warm.place_chunk(*enc, max_pairs=64 * 4096)
    warm.close()

    def run(make):
        f0 = ev0.mem_info()[0]
        ev = make(ref)
        p, r = ev.place_chunk(*enc, max_pairs=64 * 4096)
        f1 = ev.mem_info()[0]
        ev.close()
        f2 = ev0.mem_info()[0]
        return f0 - f1, f0, f2, (p, r)

    ev0 = blocked(reference_of(synth.dna_workload(8, 100, 4, 50, (21, 22, 23))))   # a bystander to ask for free memory
    drop_res, a0, a2, out_res = run(resident)
    drop_blk, b0, b2, out_blk = run(blocked)
    ev0.close()
    print("free-memory drop: resident %d, blocked %d, difference %d, footprint predicts %d (resident %d, blocked %d); "
          "after destroy: %+d / %+d bytes against before" % (drop_res, drop_blk, drop_res - drop_blk, saved,
                                                             fp_res["steady"], fp_blk["steady"], a2 - a0, b2 - b0))
    assert drop_res - drop_blk >= 0.9 * saved
    assert drop_blk < drop_res
    # destroy gives everything back (slack: one per cent of the saving, for the allocator's granularity)
    assert a2 >= a0 - saved // 100 and b2 >= b0 - saved // 100
    assert np.array_equal(out_blk[0], out_res[0])
    assert_same_results("large tree", out_blk[1], out_res[1])


def test_auto_and_no_memory(big):
    ref, enc, w = big["ref"], big["enc"], big["w"]
    res = epa.footprint(4, 4, W_BIG, B_BIG, from_tree=True, banks=4)
    blk64 = epa.footprint(4, 4, W_BIG, B_BIG, flags=BLOCKS, from_tree=True, block_branches=64, banks=4)
    ev0 = blocked(reference_of(synth.dna_workload(8, 100, 4, 50, (21, 22, 23))))
    try:
        # no cap: the reference fits, auto stays resident
        ev = ref.evaluator(flags=epa.FLAG_LOOKUP_AUTO)
        assert ev.lookup_mode() == (epa.LOOKUP_RESIDENT, 0)
        ev.close()
        epa.set_mem_cap(res["peak"] - 1)
        ev = ref.evaluator(flags=epa.FLAG_LOOKUP_AUTO)
        assert ev.lookup_mode() == (epa.LOOKUP_BLOCKS, 1024)
        lnl = ev.preplace(*enc)
        o = Oracle(w["newick"], w["labels"], w["seqs"], 4, w["subst"], w["freqs"], w["rates"])
        assert np.max(np.abs(lnl - o.preplace(w["reads"]))) < LNL_TOL
        ev.close()
        # flags 0 do not look at the cap
        ev = ref.evaluator()
        assert ev.lookup_mode() == (epa.LOOKUP_RESIDENT, 0)
        assert np.array_equal(ev.preplace(*enc), lnl)
        ev.close()
        # a cap between the smallest and the default block size shrinks the block
        mid = epa.footprint(4, 4, W_BIG, B_BIG, flags=BLOCKS, from_tree=True, block_branches=512, banks=4)["peak"]
        epa.set_mem_cap(mid)
        ev = ref.evaluator(flags=epa.FLAG_LOOKUP_AUTO)
        assert ev.lookup_mode() == (epa.LOOKUP_BLOCKS, 512)
        assert np.array_equal(ev.preplace(*enc), lnl)
        ev.close()
        # below refT: nothing fits
        f0 = ev0.mem_info()[0]
        cap = res["reft"] - 1
        epa.set_mem_cap(cap)
        for flags in (epa.FLAG_LOOKUP_AUTO, BLOCKS):
            with pytest.raises(epa.EpaError) as e:
                ref.evaluator(flags=flags)
            assert e.value.code == epa.ERR_NO_MEMORY
            assert str(blk64["peak"]) in str(e.value) and str(cap) in str(e.value), str(e.value)
        assert abs(ev0.mem_info()[0] - f0) <= res["reft"] // 100     # nothing of the failed creates is left
    finally:
        epa.set_mem_cap(0)
        ev0.close()


# ---- 6. the CLI --------------------------------------------------------------------------------------------------------
def _cli(tmp, name, tree, msa, qf, model, *flags):
    d = tmp / name
    d.mkdir()
    sj = d / "stats.json"
    r = subprocess.run([hostlib.cli_exe(), "-t", str(tree), "-s", str(msa), "-q", str(qf), "-m", model, "-w", str(d),
                        "--stats-json", str(sj)] + list(flags), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    doc = json.loads(open(d / "epa_result.jplace").read())
    doc.pop("metadata")                      # the invocation line lives there
    return doc, json.loads(sj.read_text()), r.stdout


def test_cli_memsave_on_off_same_jplace(tmp_path):
    g = load_case("dna8_gtr_fu_g4")
    data = os.path.join(GOLDEN, "data")
    q8 = tmp_path / "q8.fasta"
    q8.write_text("".join(">%s\n%s\n" % (q["name"], q["seq"]) for q in g["queries"]))
    model8 = ("GTR{0.787874/1.821672/1.294006/0.698421/3.034135/1.0}+FU{0.256465/0.222535/0.308594/"
              "0.212406}+G4{0.478218}")
    w = synth.dna_workload(600, 400, 3000, 120, (71, 72, 73))
    tf, sf, qf = tmp_path / "ref.tre", tmp_path / "ref.fasta", tmp_path / "q.fasta"
    tf.write_text(w["newick"] + "\n")
    sf.write_text("".join(">%s\n%s\n" % (l, s) for l, s in zip(w["labels"], w["seqs"])))
    qf.write_text("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(w["reads"])))
    model = "GTR{%s}+FU{%s}+G4{%r}" % ("/".join(map(repr, synth.CFG2_SUBST)), "/".join(map(repr, synth.CFG2_FREQS)),
                                         synth.CFG2_ALPHA)
    cases = (("t8", os.path.join(data, "ref.tre"), os.path.join(data, "aln.fasta"), q8, model8, 13, ()),
             ("t8all", os.path.join(data, "ref.tre"), os.path.join(data, "aln.fasta"), q8, model8, 13, ("--no-heur",)),
             ("t600", tf, sf, qf, model, 1197, ("--chunk-size", "1000", "--device-min-chunk", "0")))
    for name, tree, msa, q, m, B, extra in cases:
        on, s_on, out_on = _cli(tmp_path, name + "_on", tree, msa, q, m, "--memsave", "on", *extra)
        off, s_off, out_off = _cli(tmp_path, name + "_off", tree, msa, q, m, "--memsave", "off", *extra)
        auto, s_auto, _ = _cli(tmp_path, name + "_auto", tree, msa, q, m, *extra)
        assert (s_on["lookup_mode"], s_on["lookup_block"]) == ("blocks", 1024)
        assert (s_off["lookup_mode"], s_off["lookup_block"]) == ("resident", 0)
        assert (s_auto["lookup_mode"], s_auto["lookup_block"]) == ("resident", 0)
        assert "Memory-saving mode: lookup tables in blocks of 1024 branches" in out_on
        assert "Memory-saving mode" not in out_off
        assert auto == off, name               # byte for byte: the same layout
        # blocked against resident: the same placements; numbers as close as the Newton results are (module docstring:
        # 1e-6 on lnL, 1e-6 relative on lengths) plus half a unit of the jplace's tenth decimal on either side
        assert {k: v for k, v in on.items() if k != "placements"} == {k: v for k, v in off.items() if k != "placements"}
        assert len(on["placements"]) == len(off["placements"])
        same_text = on == off
        if name != "t600":     # measured: the 8-taxon files come out byte-identical; only t600 needs the numeric comparison
            assert same_text, name
        for a, b in zip(on["placements"], off["placements"]):
            assert a["n"] == b["n"] and len(a["p"]) == len(b["p"]), (name, a["n"])
            for x, y in zip(a["p"], b["p"]):
                assert x[0] == y[0], (name, a["n"])                                       # edge
                assert abs(x[1] - y[1]) < LNL_TOL and abs(x[2] - y[2]) < 1e-6, (name, a["n"])   # lnL, LWR
                for i in (3, 4):                                                          # distal, pendant
                    assert abs(x[i] - y[i]) <= 1e-6 * abs(y[i]) + 1e-10, (name, a["n"], i)
        print("%s: jplace of --memsave on byte-identical to off: %s" % (name, same_text))
        assert s_on["queries"] == s_off["queries"] and s_on["pairs"] == s_off["pairs"]
