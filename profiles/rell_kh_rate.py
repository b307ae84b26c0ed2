"""Kernel time of epa_dev_rell_kh (p_kh, p_wkh, p_wsh) next to epa_dev_rell_tests on the same entries, same box, same
context, same run, at 3, 7 and 12 entries per query (12: beyond the queries whose centred scores stay in registers), and
the register / LDS figures of the two instantiations of k_rell_kh.

  python profiles/rell_kh_rate.py [--queries 20000] [--rounds 5] [--replicates 1000] [--resources FILE] [--out FILE]
  python profiles/rell_kh_rate.py --resources-only [--out FILE]        (no device: the compiler's figures alone)

Input: the statistical input of the tests (tests/rell_ref.py, stat_input: 22 reads of 30 sites on D5, three entries
each) tiled to `--queries` queries; every copy is a query of its own, so its stream id and its replicates are its own.
K entries per query: the query's three entries in turn, copy c of an entry with its pendant length stretched by
1 + c / 10, so that no two rows are equal and no pair is skipped.  Per K, after one warm-up of each, `rounds`
interleaved rounds of
  rell_tests(...)   -> kernel_ms("rell_tests")   grouping + site rows + observed sums + k_rell_tests
  rell_kh(...)      -> kernel_ms("rell_kh")      grouping + site rows + observed sums + pair scales + thresholds + k_rell_kh
Both are HIP-event times (epa_dev_last_kernel_ms) and span one host round trip (the group bounds).
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
ap.add_argument("--queries", type=int, default=20000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--replicates", type=int, default=1000)
ap.add_argument("--entries", default="3,7,12", help="entries per query, one measurement each")
ap.add_argument("--resources", default="", help="JSON of an earlier --resources-only run instead of compiling")
ap.add_argument("--resources-only", action="store_true")
ap.add_argument("--out", default="")
args = ap.parse_args()


def resource_usage():
    """-> {kernel: {vgprs, sgprs, scratch_bytes_per_lane, waves_per_simd, lds_bytes}} for k_rell_tests, k_rell_pair_scale and
    the two instantiations of k_rell_kh"""
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
            name = re.search(r"\d+(k_rell_tests|k_rell_pair_scale|k_rell_kh)(E|ILb([01])E)", m.group(1))
            cur = None
            if name:
                spill = {None: "", "0": "<registers>", "1": "<spill>"}[name.group(3)]
                cur = out.setdefault(name.group(1) + spill, {})
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
R = args.replicates
med = statistics.median
runs = []
for K in (int(k) for k in args.entries.split(",")):
    # query-major: entry k of a query is entry k % 3 of the input's query, pendant stretched by 1 + (k // 3) / 10
    base = (np.arange(Q)[:, None] % Q0) * 3 + (np.arange(K) % 3)[None, :]
    pairs = np.zeros(Q * K, epa.PAIR_DTYPE)
    pairs["branch_id"] = s["branch"][base].ravel()
    pairs["seq_id"] = np.repeat(np.arange(Q), K).astype(np.uint32)
    pen = (s["pendant"][base] * (1.0 + (np.arange(K) // 3)[None, :] / 10.0)).ravel()
    dis = s["distal"][base].ravel()
    tests = ev.rell_tests(pairs, pen, dis, codes, wb, ws, R)                    # warm-up of both
    kh = ev.rell_kh(pairs, pen, dis, codes, wb, ws, R)
    assert np.all(kh["p_kh"] <= tests["p_sh"]) and np.all(kh["p_wkh"] <= kh["p_wsh"])
    t_tests, t_kh = [], []
    for _ in range(args.rounds):
        ev.rell_tests(pairs, pen, dis, codes, wb, ws, R)
        t_tests.append(ev.kernel_ms("rell_tests"))
        ev.rell_kh(pairs, pen, dis, codes, wb, ws, R)
        t_kh.append(ev.kernel_ms("rell_kh"))
    inside = lambda p: float(np.mean(np.any((p.reshape(Q, K) > 0) & (p.reshape(Q, K) < 1), axis=1)))   # noqa: E731
    runs.append(dict(entries_per_query=K, entries=len(pairs), rell_tests_ms=t_tests, rell_kh_ms=t_kh,
                     rell_tests_ms_median=med(t_tests), rell_kh_ms_median=med(t_kh), ratio_of_medians=med(t_kh) / med(t_tests),
                     rell_kh_ns_per_entry=1e6 * med(t_kh) / len(pairs),
                     queries_with_a_value_inside_0_1={key: inside(kh[key]) for key in ("p_kh", "p_wkh", "p_wsh")}))
resources = json.load(open(args.resources))["resources"] if args.resources else resource_usage()
finish(dict(shape="stat_input tiled", queries=Q, sites=rr.STAT_SPAN, replicates=R, rounds=args.rounds, runs=runs,
            resources=resources))
ev.close()
