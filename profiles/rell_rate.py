"""Kernel times of epa_dev_site_lnl and epa_dev_rell_support next to epa_dev_score_at on the same pairs, same box, same
context.

  python profiles/rell_rate.py [--reads 100000] [--rounds 3] [--replicates 1000] [--out FILE]

cfg2 shape (synth: 512 tips x 1500 sites, B = 1021, reads of 150 sites), as profiles/score_at_rate.py: one fused chunk
body selects the candidate pairs and returns their optimised lengths; then, after one warm-up of each, `rounds`
interleaved rounds of
  thorough(pairs)                        (not reported: score_at then follows the Newton launch as in score_at_rate.py)
  score_at(pairs, returned lengths)      -> kernel_ms("score_at")   one lnL per pair
  site_lnl(pairs, returned lengths)      -> kernel_ms("site_lnl")   150 site values per pair into a device buffer
  rell_support(pairs, ..., replicates)   -> kernel_ms("rell")       grouping + site rows + resampling, one support per pair
All are HIP-event times (epa_dev_last_kernel_ms); "rell" spans one host round trip (the group bounds).  One JSON line
at the end, with the largest |row sum - score_at| and the share of reads whose top support lies inside (0.05, 0.95)."""
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
ap.add_argument("--replicates", type=int, default=1000)
ap.add_argument("--out", default="")
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

import epa_ng_amd as epa  # noqa: E402,F401
from epa_ng_amd import hostlib, synth  # noqa: E402

w = synth.dna_workload(512, 1500, 1, 150, (1, 2, 3))
codes, wb, ws = synth.make_reads_compact(w["seqs"], args.reads, 150, 0.03, 3)
ref = hostlib.Reference(w["newick"], w["labels"], w["seqs"], states=4, subst=w["subst"], freqs=w["freqs"], rates=w["rates"])
ev = ref.evaluator()
pairs, res = ev.place_chunk(codes, wb, ws, max_span=150, max_pairs=args.reads * 64)
pairs = np.ascontiguousarray(pairs)
pen, dis = np.ascontiguousarray(res["pendant_length"]), np.ascontiguousarray(res["distal_length"])
n, pitch = len(pairs), int(ws.max())
rows = torch.empty((n, pitch), dtype=torch.float64, device="cuda")
lnl = ev.score_at(pairs, pen, dis, codes, wb, ws)                 # warm-up of all three
ev.site_lnl(pairs, pen, dis, codes, wb, ws, pitch=pitch, out=rows)
torch.cuda.synchronize()
d_sum = float(np.max(np.abs(rows.sum(1).cpu().numpy() - lnl)))
sup = ev.rell_support(pairs, pen, dis, codes, wb, ws, args.replicates)
t_sc, t_si, t_re = [], [], []
for _ in range(args.rounds):
    ev.thorough(pairs, codes, wb, ws)
    ev.score_at(pairs, pen, dis, codes, wb, ws)
    t_sc.append(ev.kernel_ms("score_at"))
    ev.site_lnl(pairs, pen, dis, codes, wb, ws, pitch=pitch, out=rows)
    t_si.append(ev.kernel_ms("site_lnl"))
    ev.rell_support(pairs, pen, dis, codes, wb, ws, args.replicates)
    t_re.append(ev.kernel_ms("rell"))
top = np.zeros(args.reads)
np.maximum.at(top, pairs["seq_id"], sup)
med = statistics.median
line = dict(shape="cfg2", reads=args.reads, pairs=n, rounds=args.rounds, replicates=args.replicates,
            score_at_ms=t_sc, site_lnl_ms=t_si, rell_ms=t_re, score_at_ms_median=med(t_sc), site_lnl_ms_median=med(t_si),
            rell_ms_median=med(t_re), site_lnl_gb_per_s=1e-6 * 8.0 * float(np.sum(ws[pairs["seq_id"]])) / med(t_si),
            rell_ns_per_pair=1e6 * med(t_re) / n, max_abs_rowsum_minus_score_at=d_sum,
            reads_with_top_support_undecided=float(np.mean((top > 0.05) & (top < 0.95))))
print(json.dumps(line), flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(json.dumps(line) + "\n")
ev.close()
