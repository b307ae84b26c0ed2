"""Rate of epa_dev_edpl in entries per second at 7 rows per object (what placement files hold) and at 1024 rows per object
(the pair pass as a 1024-iteration loop on 1024 work items), on a 2000-tip tree, and the register / scratch figures of its
kernels.

  python profiles/edpl_rate.py [--objects7 100000] [--objects1024 256] [--rounds 5] [--resources FILE] [--out FILE]
  python profiles/edpl_rate.py --resources-only [--out FILE]        (no device: the compiler's figures alone)

Input: synth.random_tree(2000, 1) with its branches numbered depth first (tests/edpl_ref.py, from_synth), so that branch
ids that are close are close on the tree; a context of four sites of random CLVs under JC69 (EDPL reads no CLV).  An object
of K rows sits on K consecutive branch ids from a random start, at random distal lengths, with Dirichlet weights.  Per
shape, after one warm-up, `rounds` calls with host arrays; the time is kernel_ms("edpl"), HIP events around grouping, point
pass, pair pass and per-query sum (the uploads and the read-back are outside).  The first call's results are checked against
brute() of tests/edpl_ref.py on 20 objects.
Resources: hipcc -Rpass-analysis=kernel-resource-usage on csrc/treepath.hip (device code only, nothing is linked), or the
JSON file of an earlier --resources-only run.  One JSON line at the end."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--objects7", type=int, default=100000)
ap.add_argument("--objects1024", type=int, default=256)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--tips", type=int, default=2000)
ap.add_argument("--resources", default="", help="JSON of an earlier --resources-only run instead of compiling")
ap.add_argument("--resources-only", action="store_true")
ap.add_argument("--out", default="")
args = ap.parse_args()


def resource_usage():
    """-> {kernel: {vgprs, sgprs, scratch_bytes_per_lane, waves_per_simd, lds_bytes}} of the kernels of treepath.hip"""
    from epa_ng_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build.HIPCC] + build.DEV_FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                                 os.path.join(build.CSRC, "treepath.hip"), "-o", os.path.join(tmp, "treepath.o")]
        text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "Occupancy [waves/SIMD]": "waves_per_simd", "LDS Size [bytes/block]": "lds_bytes"}
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = re.search(r"\d+(k_edpl_[a-z]+)E", m.group(1))
            cur = out.setdefault(name.group(1), {}) if name else None
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", line)
        if m and cur is not None and m.group(1) in keys:
            cur[keys[m.group(1)]] = int(m.group(2))
    return out


def finish(line):
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if args.resources_only:
    finish(dict(resources=resource_usage()))
    sys.exit(0)

import numpy as np  # noqa: E402

import edpl_ref as er  # noqa: E402
import epa_ng_amd as epa  # noqa: E402
from epa_ng_amd import synth  # noqa: E402

prox, dist, blen = er.from_synth(synth.random_tree(args.tips, 1))
B = len(blen)
H = 0.5 * np.array([[1.0, 1, 1, 1], [1, 1, -1, -1], [1, -1, 1, -1], [1, -1, -1, 1]])
clv = np.random.RandomState(3).uniform(0.1, 1.0, (2, B, 4, 1, 4))
ev = epa.Evaluator(4, [1.0], [1.0], [0.0, -4.0 / 3, -4.0 / 3, -4.0 / 3], H, H, [0.25] * 4, blen, list(clv[0]), list(clv[1]))
ev.set_topology(prox, dist)
rng = np.random.RandomState(5)
med = statistics.median
runs = []
for K, Q in ((7, args.objects7), (1024, args.objects1024)):
    start = rng.randint(B, size=Q)
    pairs = np.zeros(Q * K, epa.PAIR_DTYPE)
    pairs["branch_id"] = ((start[:, None] + np.arange(K)[None, :]) % B).ravel()
    pairs["seq_id"] = np.repeat(np.arange(Q), K).astype(np.uint32)
    distal = rng.uniform(size=Q * K) * blen[pairs["branch_id"]]
    weight = rng.dirichlet(np.ones(K), size=Q).ravel()
    edpl, rows = ev.edpl(pairs, distal, weight, Q, row_dist=True)                # warm-up, and the check
    pick = rng.choice(Q, min(Q, 20), replace=False)
    worst = 0.0
    for q in pick:
        sl = slice(q * K, (q + 1) * K)
        want_rows, want = er.brute(prox, dist, blen, pairs["branch_id"][sl], np.zeros(K, np.uint32), distal[sl], weight[sl], 1)
        worst = max(worst, float(np.max(np.abs(rows[sl] - want_rows))), abs(edpl[q] - want[0]))
    assert worst <= er.tol(prox, dist, blen, K), worst
    ms = []
    for _ in range(args.rounds):
        ev.edpl(pairs, distal, weight, Q, row_dist=True)
        ms.append(ev.kernel_ms("edpl"))
    runs.append(dict(rows_per_object=K, objects=Q, entries=Q * K, edpl_ms=ms, edpl_ms_median=med(ms),
                     entries_per_second=Q * K / (1e-3 * med(ms)), pair_terms_per_second=Q * K * K / (1e-3 * med(ms)),
                     max_abs_error_against_brute=worst))
resources = json.load(open(args.resources))["resources"] if args.resources else resource_usage()
finish(dict(shape="synth.random_tree(%d, 1)" % args.tips, branches=B, rounds=args.rounds, runs=runs, resources=resources))
ev.close()
