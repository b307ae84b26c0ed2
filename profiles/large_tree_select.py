"""Kernel times of one fused chunk body on a large reference, by the library's HIP-event timers
(epa_dev_last_kernel_ms): "lookup", "preplace", "select", "thorough".  One process = one package and one tree
size; run_large_tree_select.sh alternates child processes of two packages (the change and its parent) on the
same seeds and large_tree_select_report.py turns their JSON lines into the table of large_tree_select.md.

  python profiles/large_tree_select.py --pkg-root DIR --tips N [--flat] [--reps 5] --tag NAME

Cases of a tree-shaped run: 20 000 reads (staging rows: the [B][Q/32] bitmap would be 164 MB), 8 000 reads
(bitmap: 65.5 MB), both dynamic at 0.99999, and -G 0.01 on 2 000 reads.  --flat: the flat input of
tests/large_tree_gen.py at Q = 16, selection alone, dynamic 0.9 / 0.99999 and -G 0.5."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--pkg-root", required=True)
ap.add_argument("--tips", type=int, required=True)
ap.add_argument("--width", type=int, default=300)
ap.add_argument("--read-len", type=int, default=150)
ap.add_argument("--flat", action="store_true")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--tag", default="")
args = ap.parse_args()

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
sys.path.insert(0, os.path.abspath(args.pkg_root))

import numpy as np  # noqa: E402

import epa_ng_amd as epa  # noqa: E402
from epa_ng_amd import hostlib  # noqa: E402
import large_tree_gen as gen  # noqa: E402

assert os.path.abspath(os.path.dirname(os.path.dirname(epa.__file__))) == os.path.abspath(args.pkg_root)
B = 2 * args.tips - 3


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def emit(case, **kw):
    print(json.dumps(dict(tag=args.tag, tips=args.tips, B=B, case=case, **kw)), flush=True)


t0 = time.monotonic()
if args.flat:
    W, rl = 96, 64
    w = gen.dna_workload(args.tips, W, 1, rl, (201, 202, 203))
    seqs, reads = gen.flat_reads(args.tips, W, 16, rl)
else:
    W, rl = args.width, args.read_len
    w = gen.dna_workload(args.tips, W, 20000, rl, (201, 202, 203))
    seqs, reads = w["seqs"], w["reads"]
ref = hostlib.Reference(w["newick"], w["labels"], seqs, states=4, subst=w["subst"], freqs=w["freqs"], rates=w["rates"])
ev = ref.evaluator()
codes, wb, ws = epa.encode_queries(4, reads, compact=not args.flat)
emit("setup", seconds=time.monotonic() - t0, lookup_ms=ev.kernel_ms("lookup"))

if args.flat:
    Q = len(reads)
    lnl = ev.preplace(codes, wb, ws)
    for mode, thr in (("dynamic", 0.9), ("dynamic", 0.99999), ("fixed", 0.5)):
        ev.set_heuristic(mode, thr if mode == "fixed" else 0.0)
        for sort in (0, 1):
            ev.set_option("select_sort", sort)
            ms, n = [], 0
            for _ in range(1 + args.reps):
                n = len(ev.select(lnl, Q, thr if mode == "dynamic" else 0.99999, max_pairs=Q * B))
                ms.append(ev.kernel_ms("select"))
            # bytes the selection streams per query: passes over a row of B doubles
            emit("flat %s %r sort=%d" % (mode, thr, sort), Q=Q, pairs=n, select_ms=med(ms[1:]), row_bytes=8 * B)
else:
    for name, Q, mode, thr, per in (("dyn20000", 20000, "dynamic", 0.99999, 64), ("dyn8000", 8000, "dynamic", 0.99999, 64),
                                    ("G0.01_2000", 2000, "fixed", 0.01, int(0.01 * B) + 2)):
        ev.set_heuristic(mode, thr if mode == "fixed" else 0.0)
        c, b, s = codes[:Q], wb[:Q], ws[:Q]
        t = {"select": [], "preplace": [], "thorough": []}
        n = 0
        for _ in range(1 + args.reps):
            p, _r = ev.place_chunk(c, b, s, threshold=thr if mode == "dynamic" else 0.99999, max_span=rl, max_pairs=Q * per)
            n = len(p)
            for k in t:
                t[k].append(ev.kernel_ms(k))
        emit(name, Q=Q, pairs=n, **{k + "_ms": med(v[1:]) for k, v in t.items()})
ev.close()
