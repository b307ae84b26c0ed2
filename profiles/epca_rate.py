"""What epa_dev_epca costs at 64 and at 512 samples of 2000 reads x 3 rows on a 2000-tip tree (profiles/krd_rate.py's
inputs), K = 5, phase by phase, with numpy.linalg.eigh of the same Gram matrix on the host beside it for scale.

  python profiles/epca_rate.py [--samples 64,512] [--rounds 5] [--step-seconds 240] [--out FILE]
  python profiles/epca_rate.py --shape S            (one shape, one JSON line: what the driver starts per shape)

The driver opens no device.  It starts one child process per shape, each under its own `timeout -k 10`, one after the
other, and stops at the first that fails or runs out of time (the shapes chained with &&): nothing is started on a device
after a failure.

Per shape, after one warm-up, `rounds` calls with host arrays in and out; medians of the HIP-event timers "epca",
"epca_tables", "epca_gram", "epca_eig" (summed over the sweeps) and "epca_project"; "epca_loop_wall", the host's wall clock
around the Jacobi loop; the sweep count; and the median wall clock of numpy.linalg.eigh on the device's Gram matrix.
Derived:
  per_step_us            "epca_loop_wall" / (sweeps (m - 1)), m = S rounded up to even: what one step of two launches costs
  host_share_of_loop     1 - "epca_eig" / "epca_loop_wall": the part of the loop's wall clock in which no kernel of the loop ran
  dominant               the largest of the four phases
The warm-up call is checked: eigenvalue (S - 1) against eigh of the returned Gram matrix within tests/epca_ref.tol_jac."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--samples", default="64,512")
ap.add_argument("--shape", type=int, default=0)
ap.add_argument("--reads", type=int, default=2000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--tips", type=int, default=2000)
ap.add_argument("--components", type=int, default=5)
ap.add_argument("--step-seconds", type=int, default=240)
ap.add_argument("--out", default="")
args = ap.parse_args()

if not args.shape:
    runs = []
    for S in [int(v) for v in args.samples.split(",")]:
        cmd = ["timeout", "-k", "10", str(args.step_seconds), sys.executable, os.path.abspath(__file__), "--shape", str(S), "--reads",
               str(args.reads), "--rounds", str(args.rounds), "--tips", str(args.tips), "--components", str(args.components)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
            sys.exit("epca_rate: %d samples ended with status %d (124 / 137: past %d s): stopping here" % (S, r.returncode, args.step_seconds))
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    line = dict(shape="synth.random_tree(%d, 1)" % args.tips, branches=runs[0]["branches"], reads_per_sample=args.reads, rows_per_read=3,
                components=args.components, rounds=args.rounds, runs=runs)
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    sys.exit(0)

import numpy as np  # noqa: E402

import edpl_ref as er  # noqa: E402
import epa_ng_amd as epa  # noqa: E402
import epca_ref as pr  # noqa: E402
from epa_ng_amd import synth  # noqa: E402

prox, dist, blen = er.from_synth(synth.random_tree(args.tips, 1))
B = len(blen)
H = 0.5 * np.array([[1.0, 1, 1, 1], [1, 1, -1, -1], [1, -1, 1, -1], [1, -1, -1, 1]])
clv = np.random.RandomState(3).uniform(0.1, 1.0, (2, B, 4, 1, 4))
ev = epa.Evaluator(4, [1.0], [1.0], [0.0, -4.0 / 3, -4.0 / 3, -4.0 / 3], H, H, [0.25] * 4, blen, list(clv[0]), list(clv[1]))
ev.set_topology(prox, dist)
med = statistics.median
R, S, K = 3, args.shape, args.components
rng = np.random.RandomState(5 + S)
n = S * args.reads * R
centre = rng.randint(B, size=S)
start = (centre[:, None] + np.rint(rng.normal(0.0, B / 16.0, size=(S, args.reads))).astype(np.int64)) % B
pairs = np.zeros(n, epa.PAIR_DTYPE)
pairs["branch_id"] = ((start[:, :, None] + np.arange(R)[None, None, :]) % B).ravel()
pairs["seq_id"] = np.repeat(np.arange(S), args.reads * R).astype(np.uint32)
distal = rng.uniform(size=n) * blen[pairs["branch_id"]]
weight = (rng.dirichlet(np.ones(R), size=S * args.reads) / args.reads).ravel()
order = rng.permutation(n)                                       # entries come in any order
pairs, distal, weight = pairs[order], distal[order], weight[order]

eig, vec, proj, total, sweeps, gram = ev.epca(pairs, distal, weight, S, K, with_gram=True)     # warm-up, and the check
lam = np.linalg.eigvalsh(gram)[::-1]
worst = float(np.max(np.abs(eig * (S - 1) - np.maximum(lam[:K], 0.0))) / pr.tol_jac(gram, int(sweeps[0])))
assert worst <= 1.0, worst

names = ("epca", "epca_tables", "epca_gram", "epca_eig", "epca_project", "epca_loop_wall")
ms = {k: [] for k in names + ("host_eigh",)}
sw = []
for _ in range(args.rounds):
    out = ev.epca(pairs, distal, weight, S, K)
    sw.append(int(out[4][0]))
    for k in names:
        ms[k].append(ev.kernel_ms(k))
for _ in range(args.rounds):
    t0 = time.perf_counter()
    np.linalg.eigh(gram)
    ms["host_eigh"].append(1e3 * (time.perf_counter() - t0))
m = {k: med(v) for k, v in ms.items()}
steps = med(sw) * (S + (S & 1) - 1)
phases = ("epca_tables", "epca_gram", "epca_eig", "epca_project")
print(json.dumps(dict(samples=S, branches=B, entries=n, components=K, sweeps=sw, ms=ms, ms_median=m,
                      per_step_us=1e3 * m["epca_loop_wall"] / steps, host_share_of_loop=1.0 - m["epca_eig"] / m["epca_loop_wall"],
                      dominant=max(phases, key=lambda k: m[k]), fraction_of_variance=[float(v) for v in eig / total[0]],
                      max_error_over_tol_jac_against_eigh=worst)), flush=True)
ev.close()
