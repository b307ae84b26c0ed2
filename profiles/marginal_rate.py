"""Kernel time of epa_dev_marginal_like next to the epa_dev_score_at launches that evaluate the same grid, same box, same
context.

  python profiles/marginal_rate.py [--entries 20000] [--rounds 5] [--kx 8] [--kp 16] [--out FILE]

Two references: the cfg2 shape (synth: 512 tips x 1500 sites, 4 states x 4 categories, reads of 150 sites) and a
20-state one (synth.aa_workload: 256 tips x 500 sites, 4 categories, reads of 100 sites).  On each, one fused chunk body
selects candidate pairs; the first `entries` of them are the entries.  Rule: posterior_rule(mean branch length, kx, kp).
After one warm-up of each, `rounds` interleaved rounds of
  marginal_like(entries, rule)                                  -> kernel_ms("marginal")
  kx * kp score_at launches over the same entries, one per node -> the sum of their kernel_ms("score_at")
Both are HIP-event times (epa_dev_last_kernel_ms); medians over the rounds.  score_at is the yardstick: it is the code
a host loop over the nodes would run.  One JSON line per reference, with the largest |grid - score_at| of the warm-up."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--entries", type=int, default=20000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--kx", type=int, default=8)
ap.add_argument("--kp", type=int, default=16)
ap.add_argument("--out", default="")
args = ap.parse_args()

import numpy as np  # noqa: E402

import epa_ng_amd as epa  # noqa: E402
from epa_ng_amd import hostlib, synth  # noqa: E402


def measure(shape, states, w, read_len):
    n = args.entries
    codes, wb, ws = synth.make_reads_compact(w["seqs"], n, read_len, 0.03, 3, states=states)
    ref = hostlib.Reference(w["newick"], w["labels"], w["seqs"], states=states, subst=w["subst"], freqs=w["freqs"],
                            rates=w["rates"])
    ev = ref.evaluator()
    pairs, _ = ev.place_chunk(codes, wb, ws, max_span=read_len, max_pairs=n * 64)
    assert len(pairs) >= n            # every read has at least one candidate
    pairs = np.ascontiguousarray(pairs[:n])
    blen = np.array([ref.branch(b)["length"] for b in range(ref.B)])
    x, xw, p, pw = epa.posterior_rule(float(blen.mean()), args.kx, args.kp)
    length = blen[pairs["branch_id"]]

    def score_loop(grid=None):
        total = 0.0
        for i in range(args.kx):
            dis = x[i] * length
            for j in range(args.kp):
                lnl = ev.score_at(pairs, np.full(n, p[j]), dis, codes, wb, ws)
                total += ev.kernel_ms("score_at")
                if grid is not None:
                    grid[:, i, j] = lnl
        return total

    M, g = ev.marginal_like(pairs, codes, wb, ws, x, xw, p, pw, grid=True)      # warm-up of both, and a cross-check
    want = np.empty_like(g)
    score_loop(want)
    d = float(np.max(np.abs(g - want)))
    t_m, t_s = [], []
    for _ in range(args.rounds):
        ev.marginal_like(pairs, codes, wb, ws, x, xw, p, pw)
        t_m.append(ev.kernel_ms("marginal"))
        t_s.append(score_loop())
    med = statistics.median
    line = dict(shape=shape, states=states, categories=ev.c, branches=ref.B, entries=n, read_len=read_len, kx=args.kx,
                kp=args.kp, prior_mean=float(blen.mean()), rounds=args.rounds, marginal_ms=t_m, score_at_loop_ms=t_s,
                marginal_ms_median=med(t_m), score_at_loop_ms_median=med(t_s), ratio=med(t_s) / med(t_m),
                marginal_ns_per_grid_point=1e6 * med(t_m) / (n * args.kx * args.kp),
                score_at_ns_per_grid_point=1e6 * med(t_s) / (n * args.kx * args.kp), max_abs_grid_minus_score_at=d)
    print(json.dumps(line), flush=True)
    ev.close()
    return line


lines = [measure("cfg2", 4, synth.dna_workload(512, 1500, 1, 150, (1, 2, 3)), 150),
         measure("aa256x500", 20, synth.aa_workload(256, 500, 1, 100, (11, 12, 13)), 100)]
if args.out:
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
