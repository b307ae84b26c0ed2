"""What epa_dev_squash costs at 64 and at 512 samples of 2000 reads x 3 rows on a 2000-tip tree (profiles/krd_rate.py's
inputs), against the pair pass of epa_dev_krd on the same input.

  python profiles/squash_rate.py [--samples 64,512] [--rounds 5] [--step-seconds 240] [--out FILE]
  python profiles/squash_rate.py --shape S            (one shape, one JSON line: what the driver starts per shape)

The driver opens no device.  It starts one child process per shape, each under its own time limit, one after the other,
and stops at the first that fails or runs out of time: nothing is started on a device after a failure.

Per shape, after one warm-up, `rounds` calls with host arrays in and out; medians of the HIP-event timers "squash",
"squash_init" and, summed over the merge steps, "squash_argmin", "squash_merge", "squash_row"; "squash_loop_wall", the host's
wall clock around the merge loop; and "krd_pairs" of epa_dev_krd on the same input (five calls, median) as the yardstick.
Derived:
  row_over_krd_pairs      "squash_row" / "krd_pairs": the edge-term counts are about equal (S^2 / 2 x B), so the excess is
                          the price of the small grids late in the loop
  per_merge_us            ("squash" - "squash_init") / (S - 1)
  host_share_of_loop      1 - ("squash_argmin" + "squash_merge" + "squash_row") / "squash_loop_wall": the part of the loop's
                          wall clock in which no kernel of the loop ran -- the read-back, the wait for it and the launches
The first call is spot-checked: four merges per shape (steps 0, 1, the middle one and the last -- above 64 samples the
one at three quarters instead) recomputed by
tests/krd_ref.restate on the materialised pair (tests/squash_ref.materialise, members replayed from the device's own
merges), within tol."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--samples", default="64,512")
ap.add_argument("--shape", type=int, default=0)
ap.add_argument("--reads", type=int, default=2000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--tips", type=int, default=2000)
ap.add_argument("--step-seconds", type=int, default=240)
ap.add_argument("--out", default="")
args = ap.parse_args()

if not args.shape:
    runs = []
    for S in [int(v) for v in args.samples.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", str(S), "--reads", str(args.reads), "--rounds", str(args.rounds),
               "--tips", str(args.tips)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_seconds)
        except subprocess.TimeoutExpired:
            sys.exit("squash_rate: %d samples ran past %d s: stopping here" % (S, args.step_seconds))
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
            sys.exit("squash_rate: %d samples ended with status %d: stopping here" % (S, r.returncode))
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    line = dict(shape="synth.random_tree(%d, 1)" % args.tips, branches=runs[0]["branches"], reads_per_sample=args.reads, rows_per_read=3,
                rounds=args.rounds, runs=runs)
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    sys.exit(0)

import numpy as np  # noqa: E402

import edpl_ref as er  # noqa: E402
import epa_ng_amd as epa  # noqa: E402
import krd_ref as kr  # noqa: E402
import squash_ref as sr  # noqa: E402
from epa_ng_amd import synth  # noqa: E402

prox, dist, blen = er.from_synth(synth.random_tree(args.tips, 1))
B = len(blen)
H = 0.5 * np.array([[1.0, 1, 1, 1], [1, 1, -1, -1], [1, -1, 1, -1], [1, -1, -1, 1]])
clv = np.random.RandomState(3).uniform(0.1, 1.0, (2, B, 4, 1, 4))
ev = epa.Evaluator(4, [1.0], [1.0], [0.0, -4.0 / 3, -4.0 / 3, -4.0 / 3], H, H, [0.25] * 4, blen, list(clv[0]), list(clv[1]))
ev.set_topology(prox, dist)
med = statistics.median
K, S = 3, args.shape
rng = np.random.RandomState(5 + S)
n = S * args.reads * K
centre = rng.randint(B, size=S)
start = (centre[:, None] + np.rint(rng.normal(0.0, B / 16.0, size=(S, args.reads))).astype(np.int64)) % B
pairs = np.zeros(n, epa.PAIR_DTYPE)
pairs["branch_id"] = ((start[:, :, None] + np.arange(K)[None, None, :]) % B).ravel()
pairs["seq_id"] = np.repeat(np.arange(S), args.reads * K).astype(np.uint32)
distal = rng.uniform(size=n) * blen[pairs["branch_id"]]
weight = (rng.dirichlet(np.ones(K), size=S * args.reads) / args.reads).ravel()
order = rng.permutation(n)                                       # entries come in any order
pairs, distal, weight = pairs[order], distal[order], weight[order]

ma, mb, md, ms_ = ev.squash(pairs, distal, weight, S)             # warm-up, and the check
c = dict(branch=pairs["branch_id"], seq=pairs["seq_id"], distal=distal, weight=weight, S=S, blen=blen)
members = {s: [s] for s in range(S)}
for t in range(S - 1):
    members[S + t] = sorted(members[int(ma[t])] + members[int(mb[t])])
worst = 0.0
for t in sorted({0, 1, (S - 1) // 2, S - 2 if S <= 64 else 3 * (S - 1) // 4}):   # the last merge of 512 samples is 3 x 10^6 rows of Python
    m = sr.materialise(c, [members[int(ma[t])], members[int(mb[t])]])
    want = kr.restate(prox, dist, blen, m["branch"], m["seq"], m["distal"], m["weight"], 2)[0][0, 1]
    worst = max(worst, abs(md[t] - want) / kr.tol(m, 0, 1))
assert worst <= 1.0, worst

names = ("squash", "squash_init", "squash_argmin", "squash_merge", "squash_row", "squash_loop_wall")
ms = {k: [] for k in names + ("krd_pairs",)}
for _ in range(args.rounds):
    ev.squash(pairs, distal, weight, S)
    for k in names:
        ms[k].append(ev.kernel_ms(k))
for _ in range(args.rounds):
    ev.krd(pairs, distal, weight, S)
    ms["krd_pairs"].append(ev.kernel_ms("krd_pairs"))
m = {k: med(v) for k, v in ms.items()}
print(json.dumps(dict(samples=S, branches=B, entries=n, merges=S - 1, ms=ms, ms_median=m,
                      row_over_krd_pairs=m["squash_row"] / m["krd_pairs"],
                      per_merge_us=1e3 * (m["squash"] - m["squash_init"]) / (S - 1),
                      host_share_of_loop=1.0 - (m["squash_argmin"] + m["squash_merge"] + m["squash_row"]) / m["squash_loop_wall"],
                      monotone=bool(np.all(np.diff(md) >= 0.0)), max_error_over_tol_against_restate=worst)), flush=True)
ev.close()
