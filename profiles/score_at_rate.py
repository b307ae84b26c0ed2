"""Kernel time of epa_dev_score_at next to the Newton launch on the same pairs, same box, same context.

  python profiles/score_at_rate.py [--reads 100000] [--rounds 3] [--out FILE]

cfg2 shape (synth: 512 tips x 1500 sites, B = 1021, reads of 150 sites): one fused chunk body selects the candidate
pairs and returns their optimised lengths; then, after one warm-up of each, `rounds` interleaved rounds of
  thorough(pairs)                         -> kernel_ms("thorough")   (Newton rounds + at least two scores per pair)
  score_at(pairs, returned lengths)       -> kernel_ms("score_at")   (one score per pair)
Both are HIP-event times around the kernels (epa_dev_last_kernel_ms), no copies included.  One JSON line at the end;
the largest |score_at - returned lnL| over the pairs is reported with it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=100000)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default="")
args = ap.parse_args()

import numpy as np  # noqa: E402

import epa_ng_amd as epa  # noqa: E402
from epa_ng_amd import hostlib, synth  # noqa: E402

w = synth.dna_workload(512, 1500, 1, 150, (1, 2, 3))
codes, wb, ws = synth.make_reads_compact(w["seqs"], args.reads, 150, 0.03, 3)
ref = hostlib.Reference(w["newick"], w["labels"], w["seqs"], states=4, subst=w["subst"], freqs=w["freqs"], rates=w["rates"])
ev = ref.evaluator()
pairs, res = ev.place_chunk(codes, wb, ws, max_span=150, max_pairs=args.reads * 64)
pairs = np.ascontiguousarray(pairs)
pen, dis = np.ascontiguousarray(res["pendant_length"]), np.ascontiguousarray(res["distal_length"])
ev.thorough(pairs, codes, wb, ws)                        # warm-up of both
lnl = ev.score_at(pairs, pen, dis, codes, wb, ws)
t_th, t_sc = [], []
for _ in range(args.rounds):
    ev.thorough(pairs, codes, wb, ws)
    t_th.append(ev.kernel_ms("thorough"))
    ev.score_at(pairs, pen, dis, codes, wb, ws)
    t_sc.append(ev.kernel_ms("score_at"))
n = len(pairs)
line = dict(shape="cfg2", reads=args.reads, pairs=n, rounds=args.rounds,
            thorough_ms=t_th, score_at_ms=t_sc, thorough_ms_median=statistics.median(t_th),
            score_at_ms_median=statistics.median(t_sc),
            thorough_ns_per_pair=1e6 * statistics.median(t_th) / n, score_at_ns_per_pair=1e6 * statistics.median(t_sc) / n,
            max_abs_dlnl=float(np.max(np.abs(lnl - res["lnl"]))))
print(json.dumps(line), flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(json.dumps(line) + "\n")
ev.close()
