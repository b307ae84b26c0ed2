"""Kernel time of epa_dev_rell_au (ten scales, `replicates` each) next to epa_dev_rell_support on the same entries, same
box, same context, and the register / LDS figures of the two resampling kernels.

  python profiles/rell_au_rate.py [--queries 100000] [--rounds 5] [--replicates 1000] [--resources FILE] [--out FILE]
  python profiles/rell_au_rate.py --resources-only [--out FILE]        (no device: the compiler's figures alone)

Input: that of profiles/rell_tests_rate.py -- the statistical input of the tests (tests/rell_ref.py, stat_input: 22
reads of 30 sites on D5, three entries each) tiled to `--queries` queries; every copy is a query of its own, so its
stream id and its replicates are its own.  After one warm-up of each, `rounds` interleaved rounds of
  rell_support(...)   -> kernel_ms("rell")      grouping + site rows + k_rell
  rell_au(...)        -> kernel_ms("rell_au")   grouping + site rows + k_rell_ms + k_rell_au_fit
Both are HIP-event times (epa_dev_last_kernel_ms) and span one host round trip (the group bounds).  The draw work of
rell_au is sum(scale) / 1000 = 9.5 passes of k_rell; grouping and site rows are paid once.
Resources: hipcc -Rpass-analysis=kernel-resource-usage on csrc/rell.hip (device code only, nothing is linked), or the
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
ap.add_argument("--queries", type=int, default=100000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--replicates", type=int, default=1000)
ap.add_argument("--entry-copies", type=int, default=1,
                help="every entry this many times: 3 x this entries per query (2 and more: several tiles, staged per scale and round)")
ap.add_argument("--resources", default="", help="JSON of an earlier --resources-only run instead of compiling")
ap.add_argument("--resources-only", action="store_true")
ap.add_argument("--out", default="")
args = ap.parse_args()


def resource_usage():
    """-> {kernel: {vgprs, sgprs, scratch_bytes_per_lane, waves_per_simd, lds_bytes}} for k_rell, k_rell_ms, k_rell_au_fit"""
    from epa_ng_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build.HIPCC] + build.DEV_FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                                 os.path.join(build.CSRC, "rell.hip"), "-o", os.path.join(tmp, "rell.o")]
        text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "Occupancy [waves/SIMD]": "waves_per_simd", "LDS Size [bytes/block]": "lds_bytes"}
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = re.search(r"\d+(k_rell(?:_ms|_au_fit)?)E", m.group(1))
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

import brute_cases as bc  # noqa: E402
import epa_ng_amd as epa  # noqa: E402
import rell_ref as rr  # noqa: E402
from epa_ng_amd import hostlib  # noqa: E402

s = rr.stat_input()
c = bc.case("D5")
ref = hostlib.Reference(c["newick"], c["labels"], c["seqs"], states=c["states"], subst=c["subst"], freqs=c["freqs"],
                        rates=c["rates"], weights=c["weights"], pinv=c["pinv"])
ev = ref.evaluator()
Q0 = len(s["reads"])
copies = (args.queries + Q0 - 1) // Q0
Q = copies * Q0
codes, wb, ws = epa.encode_queries(4, list(s["reads"]) * copies, compact=True)
pairs = np.zeros(3 * Q, epa.PAIR_DTYPE)
pairs["branch_id"] = np.tile(s["branch"], copies)
pairs["seq_id"] = (np.tile(s["seq"], copies) + np.repeat(np.arange(copies) * Q0, 3 * Q0)).astype(np.uint32)
pen, dis = np.tile(s["pendant"], copies), np.tile(s["distal"], copies)
E = 3 * args.entry_copies
if args.entry_copies > 1:       # query-major stays query-major: the query's three entries, then the same three again
    idx = (np.arange(Q)[:, None] * 3 + np.tile(np.arange(3), args.entry_copies)[None, :]).ravel()
    pairs, pen, dis = np.ascontiguousarray(pairs[idx]), pen[idx], dis[idx]
R = args.replicates
ev.rell_support(pairs, pen, dis, codes, wb, ws, R)                            # warm-up of both
got = ev.rell_au(pairs, pen, dis, codes, wb, ws, R)
assert np.all(got["counts"].reshape(10, Q, E).sum(axis=2) == R)
t_rell, t_au = [], []
for _ in range(args.rounds):
    ev.rell_support(pairs, pen, dis, codes, wb, ws, R)
    t_rell.append(ev.kernel_ms("rell"))
    ev.rell_au(pairs, pen, dis, codes, wb, ws, R)
    t_au.append(ev.kernel_ms("rell_au"))
med = statistics.median
resources = json.load(open(args.resources))["resources"] if args.resources else resource_usage()
fitted = ~np.isnan(got["fit"][:, 0])
finish(dict(shape="stat_input tiled", queries=Q, entries=len(pairs), entries_per_query=E, sites=rr.STAT_SPAN, replicates=R,
            scales=10, rounds=args.rounds,
            rell_ms=t_rell, rell_au_ms=t_au, rell_ms_median=med(t_rell), rell_au_ms_median=med(t_au),
            ratio_of_medians=med(t_au) / med(t_rell),
            rell_entry_replicates_per_s=len(pairs) * R / (1e-3 * med(t_rell)),
            rell_au_entry_replicates_per_s=len(pairs) * R * 10 / (1e-3 * med(t_au)),
            rell_au_ns_per_entry=1e6 * med(t_au) / len(pairs),
            queries_with_a_fitted_entry=float(np.mean(np.any(fitted.reshape(Q, E), axis=1))),
            resources=resources))
ev.close()
