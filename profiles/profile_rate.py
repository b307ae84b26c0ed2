"""Chunk-body time of profile queries next to coded queries on the general Newton kernel, same box, same context.

  python profiles/profile_rate.py [--reads 20000] [--rounds 5] [--out FILE]

One reference of the bench's cfg2 shape (synth: 512 tips x 1500 sites, 4 states x 4 categories, reads of 150 sites).
The same reads go in twice: as column codes, and as the 0/1 profile rows of those codes (so both bodies select the same
candidates and run the same Newton work).  After one warm-up of each, `rounds` interleaved rounds of
  place_chunk_profile(rows)                              -> wall time, kernel_ms("preplace_profile"), kernel_ms("thorough")
  place_chunk(codes) with set_option("thorough_generic") -> wall time, kernel_ms("preplace"), kernel_ms("thorough")
All inputs and outputs are device buffers, so the wall time (host clock around a call that ends in a device
synchronise) is the chunk body without the transfer of the rows; the kernel times are HIP events
(epa_dev_last_kernel_ms).  Medians over the rounds.  The coded body on the general kernel is the yardstick: the Newton
kernel is the same code, the preplacement is what differs.  One JSON line, with the largest difference between the
warm-up's results where both bodies selected the same pairs."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=20000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

import epa_ng_amd as epa  # noqa: E402
from epa_ng_amd import hostlib, synth  # noqa: E402

READ_LEN = 150
n = args.reads
w = synth.dna_workload(512, 1500, 1, READ_LEN, (1, 2, 3))
codes, wb, ws = synth.make_reads_compact(w["seqs"], n, READ_LEN, 0.03, 3, states=4)
ref = hostlib.Reference(w["newick"], w["labels"], w["seqs"], states=4, subst=w["subst"], freqs=w["freqs"], rates=w["rates"])
ev = ref.evaluator()
ev.set_option("thorough_generic", 1)

# lookup column -> state set: column bits A=8 C=4 G=2 T=1, state order A C G T; column 0 ('-') is any state
masks = np.array([[1.0] * 4 if col == 0 else [(col >> 3) & 1, (col >> 2) & 1, (col >> 1) & 1, col & 1] for col in range(16)], np.float64)
rows = np.ascontiguousarray(masks[codes])
d_rows, d_codes = torch.from_numpy(rows).cuda(), torch.from_numpy(codes).cuda()
d_wb, d_ws = torch.from_numpy(wb.astype(np.int32)).cuda(), torch.from_numpy(ws.astype(np.int32)).cuda()
cap = n * 64
d_pairs = [torch.empty(cap * 2, dtype=torch.int32, device="cuda") for _ in range(2)]
d_res = [torch.empty(cap * 3, dtype=torch.float64, device="cuda") for _ in range(2)]


def profile_body():
    t = time.perf_counter()
    k = ev.place_chunk_profile(d_rows, d_wb, d_ws, Q=n, max_pairs=cap, pairs_out=d_pairs[0], results_out=d_res[0])
    torch.cuda.synchronize()
    return k, time.perf_counter() - t, ev.kernel_ms("preplace_profile"), ev.kernel_ms("thorough")


def coded_body():
    t = time.perf_counter()
    k = ev.place_chunk(d_codes, d_wb, d_ws, Q=n, max_span=READ_LEN, max_pairs=cap, pairs_out=d_pairs[1], results_out=d_res[1])
    torch.cuda.synchronize()
    return k, time.perf_counter() - t, ev.kernel_ms("preplace"), ev.kernel_ms("thorough")


kp, kc = profile_body()[0], coded_body()[0]          # warm-up of both, and a cross-check
same_pairs = kp == kc and bool(torch.equal(d_pairs[0][:2 * kp], d_pairs[1][:2 * kp]))
d_lnl = float((d_res[0][:3 * kp] - d_res[1][:3 * kp]).abs().max()) if same_pairs else None
t_p, t_c = [], []
for _ in range(args.rounds):
    t_p.append(profile_body()[1:])
    t_c.append(coded_body()[1:])
med = lambda rows_, i: statistics.median(r[i] for r in rows_)   # noqa: E731
line = dict(shape="cfg2", branches=ref.B, sites=ref.W, reads=n, read_len=READ_LEN, pairs=int(kp), pairs_coded=int(kc), rounds=args.rounds,
            same_pairs=same_pairs, max_abs_result_difference=d_lnl,
            profile_wall_s=[r[0] for r in t_p], coded_generic_wall_s=[r[0] for r in t_c],
            profile_wall_s_median=med(t_p, 0), coded_generic_wall_s_median=med(t_c, 0),
            profile_reads_per_s=n / med(t_p, 0), coded_generic_reads_per_s=n / med(t_c, 0),
            preplace_profile_ms_median=med(t_p, 1), preplace_coded_ms_median=med(t_c, 1),
            thorough_profile_ms_median=med(t_p, 2), thorough_coded_generic_ms_median=med(t_c, 2))
print(json.dumps(line), flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(json.dumps(line) + "\n")
ev.close()
del ev, ref
