"""Rate of epa_dev_krd in edge terms per second (pairs of samples x branches) at 64 and at 512 samples of 2000 reads x 3 rows
on a 2000-tip tree, the split of its time into sort / tables / pair pass, and the register / scratch figures of its kernels.

  python profiles/krd_rate.py [--samples 64,512] [--reads 2000] [--rounds 5] [--resources FILE] [--out FILE]
  python profiles/krd_rate.py --resources-only [--out FILE]        (no device: the compiler's figures alone)

Input: synth.random_tree(2000, 1) with its branches numbered depth first (tests/edpl_ref.py, from_synth); a context of four
sites of random CLVs under JC69 (the call reads no CLV).  A read of 3 rows sits on 3 consecutive branch ids from a start
that is drawn around the sample's own centre (samples differ, reads of a sample cluster), at random distal lengths, with
Dirichlet weights; a sample's weights are normalised to 1.  Per shape, after one warm-up, `rounds` calls with host arrays;
the times are kernel_ms("krd") and, inside it, "krd_sort", "krd_tables" and "krd_pairs" (HIP events; the uploads and the
read-back are outside).  The first call's matrix is checked against restate() of tests/krd_ref.py, run on eight of the
samples by themselves (28 pairs), within its tol.  For scale, the time of restate() on the host for the first shape: its tables in full, its pair loop on 24 pairs and
scaled to all of them.
Resources: hipcc -Rpass-analysis=kernel-resource-usage on csrc/krd.hip (device code only, nothing is linked), or the JSON
file of an earlier --resources-only run.  One JSON line at the end."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--samples", default="64,512")
ap.add_argument("--reads", type=int, default=2000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--tips", type=int, default=2000)
ap.add_argument("--resources", default="", help="JSON of an earlier --resources-only run instead of compiling")
ap.add_argument("--resources-only", action="store_true")
ap.add_argument("--no-host", action="store_true", help="leave the host restatement's time out")
ap.add_argument("--out", default="")
args = ap.parse_args()


def resource_usage():
    """-> {kernel: {vgprs, sgprs, scratch_bytes_per_lane, waves_per_simd, lds_bytes}} of the kernels of krd.hip"""
    from epa_ng_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build.HIPCC] + build.DEV_FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                                 os.path.join(build.CSRC, "krd.hip"), "-o", os.path.join(tmp, "krd.o")]
        text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "Occupancy [waves/SIMD]": "waves_per_simd", "LDS Size [bytes/block]": "lds_bytes"}
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = re.search(r"\d+(k_krd_[a-z_]+)E", m.group(1))
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
import krd_ref as kr  # noqa: E402
from epa_ng_amd import synth  # noqa: E402

prox, dist, blen = er.from_synth(synth.random_tree(args.tips, 1))
B = len(blen)
H = 0.5 * np.array([[1.0, 1, 1, 1], [1, 1, -1, -1], [1, -1, 1, -1], [1, -1, -1, 1]])
clv = np.random.RandomState(3).uniform(0.1, 1.0, (2, B, 4, 1, 4))
ev = epa.Evaluator(4, [1.0], [1.0], [0.0, -4.0 / 3, -4.0 / 3, -4.0 / 3], H, H, [0.25] * 4, blen, list(clv[0]), list(clv[1]))
ev.set_topology(prox, dist)
rng = np.random.RandomState(5)
med = statistics.median
K = 3
runs, host = [], None
for S in [int(v) for v in args.samples.split(",")]:
    n = S * args.reads * K
    centre = rng.randint(B, size=S)
    start = (centre[:, None] + np.rint(rng.normal(0.0, B / 16.0, size=(S, args.reads))).astype(np.int64)) % B
    pairs = np.zeros(n, epa.PAIR_DTYPE)
    pairs["branch_id"] = ((start[:, :, None] + np.arange(K)[None, None, :]) % B).ravel()
    pairs["seq_id"] = np.repeat(np.arange(S), args.reads * K).astype(np.uint32)
    distal = rng.uniform(size=n) * blen[pairs["branch_id"]]
    weight = (rng.dirichlet(np.ones(K), size=S * args.reads) / args.reads).ravel()
    order = rng.permutation(n)                                   # entries come in any order
    pairs, distal, weight = pairs[order], distal[order], weight[order]
    krd = ev.krd(pairs, distal, weight, S)                       # warm-up, and the check
    # the check: eight of the samples by themselves through restate(), all 28 pairs
    pick = np.sort(rng.choice(S, 8, replace=False))
    keep = np.flatnonzero(np.isin(pairs["seq_id"], pick))
    sub_seq = np.searchsorted(pick, pairs["seq_id"][keep]).astype(np.uint32)
    c = dict(seq=sub_seq, S=8, blen=blen, W=np.ones(8))
    want, _, _ = kr.restate(prox, dist, blen, pairs["branch_id"][keep], sub_seq, distal[keep], weight[keep], 8)
    worst = max(abs(krd[pick[a], pick[b]] - want[a, b]) / kr.tol(c, a, b) for a in range(8) for b in range(a + 1, 8))
    assert worst <= 1.0, worst
    if host is None and not args.no_host:
        t0 = time.time()
        kr.restate(prox, dist, blen, pairs["branch_id"], pairs["seq_id"], distal, weight, S, pairs=[])
        t_tables = time.time() - t0
        sub = [(a, a + 1) for a in range(0, min(S - 1, 48), 2)]
        t0 = time.time()
        kr.restate(prox, dist, blen, pairs["branch_id"], pairs["seq_id"], distal, weight, S, pairs=sub)
        t_pairs = max(0.0, time.time() - t0 - t_tables)
        n_pairs = S * (S - 1) // 2
        host = dict(samples=S, tables_s=t_tables, pairs_timed=len(sub), pair_loop_s=t_pairs,
                    all_pairs_s_scaled=t_tables + t_pairs * n_pairs / len(sub))
    ms = {k: [] for k in ("krd", "krd_sort", "krd_tables", "krd_pairs")}
    for _ in range(args.rounds):
        ev.krd(pairs, distal, weight, S)
        for k in ms:
            ms[k].append(ev.kernel_ms(k))
    terms = S * (S - 1) // 2 * B
    runs.append(dict(samples=S, entries=n, pairs=S * (S - 1) // 2, edge_terms=terms, ms=ms, ms_median={k: med(v) for k, v in ms.items()},
                     edge_terms_per_second=terms / (1e-3 * med(ms["krd_pairs"])), max_error_over_tol_against_restate=worst))
resources = json.load(open(args.resources))["resources"] if args.resources else resource_usage()
finish(dict(shape="synth.random_tree(%d, 1)" % args.tips, branches=B, reads_per_sample=args.reads, rows_per_read=K,
            rounds=args.rounds, runs=runs, host_restate=host, resources=resources))
ev.close()
