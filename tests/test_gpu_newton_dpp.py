"""The single-wave nucleotide Newton kernels broadcast their per-evaluation table from registers by DPP
(default) or read it through LDS (option newton_lds).  Both forms perform the same IEEE operations on the same
operands in the same order, so every result and every counter must be bit-identical: on the cfg2-shaped half-chunk
classes (windows of 65..96 and 129..160 sites) and on the full-chunk classes, with and without +I.  (--raxml-blo runs
on the LDS form either way; its cases check that the option leaves it alone.)"""
import numpy as np
import pytest

import epa_ng_amd as epa
from epa_ng_amd import hostlib, synth

pytestmark = pytest.mark.gpu

READ_LENGTHS = (40, 80, 120, 150, 180, 230)   # span classes 0, 10, 1, 11, 2, 3


def _run(ev, pairs, codes, wb, ws, lds):
    ev.set_option("newton_lds", lds)
    res = ev.thorough(pairs, codes, wb, ws)
    return res.copy(), dict(ev.last_stats)


@pytest.mark.parametrize("pinv,raxml_blo", [(0.0, False), (0.2, False), (0.0, True), (0.2, True)])
def test_dpp_table_equals_lds_table_bitwise(pinv, raxml_blo):
    root = synth.random_tree(40, 71)
    labels, seqs = synth.simulate_msa(root, 600, synth.CFG2_SUBST, synth.CFG2_FREQS, synth.gamma_rates(0.7), 72)
    nw = synth.newick(root)
    reads = []
    for k, rl in enumerate(READ_LENGTHS):
        r, _ = synth.make_reads(seqs, 12, rl, 0.04, 80 + k, states=4)
        reads += list(r)
    ref = hostlib.Reference(nw, labels, seqs, states=4, subst=synth.CFG2_SUBST, freqs=synth.CFG2_FREQS,
                            rates=synth.gamma_rates(0.7), pinv=pinv)
    codes, wb, ws = epa.encode_queries(4, reads, compact=True)
    classes = {10 if 64 < s <= 96 else 11 if 128 < s <= 160 else min((s + 63) // 64, 4) - 1 for s in ws}
    assert {0, 1, 2, 3, 10, 11} <= classes   # every single-wave span class (epa_span_class)
    ev = ref.evaluator(raxml_blo=raxml_blo)
    B, Q = ref.B, len(reads)
    pairs = np.zeros(B * Q, epa.PAIR_DTYPE)
    pairs["branch_id"] = np.repeat(np.arange(B), Q)
    pairs["seq_id"] = np.tile(np.arange(Q), B)
    pairs = pairs[::2].copy()
    res_dpp, st_dpp = _run(ev, pairs, codes, wb, ws, 0)
    res_lds, st_lds = _run(ev, pairs, codes, wb, ws, 1)
    res_again, _ = _run(ev, pairs, codes, wb, ws, 0)
    for f in ("lnl", "pendant_length", "distal_length"):
        assert np.all(np.isfinite(res_dpp[f]))
        assert np.array_equal(res_dpp[f], res_lds[f]), f
        assert np.array_equal(res_dpp[f], res_again[f]), f
    for k in ("rounds", "newton_evals", "reverts"):
        assert st_dpp[k] == st_lds[k], k
    assert st_dpp["newton_evals"] > 0


def test_newton_lds_is_a_known_option():
    root = synth.random_tree(8, 3)
    labels, seqs = synth.simulate_msa(root, 100, synth.CFG2_SUBST, synth.CFG2_FREQS, synth.gamma_rates(0.7), 4)
    ref = hostlib.Reference(synth.newick(root), labels, seqs, states=4, subst=synth.CFG2_SUBST, freqs=synth.CFG2_FREQS,
                            rates=synth.gamma_rates(0.7))
    ev = ref.evaluator()
    ev.set_option("newton_lds", 1)
    ev.set_option("newton_lds", 0)
