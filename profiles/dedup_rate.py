"""What the duplicate search costs and what it saves: place_chunk_dedup next to place_chunk on the same chunk, same box,
same context.

  python profiles/dedup_rate.py [--reads 100000] [--rounds 7] [--factors 1,4,20] [--layout packed|compact] [--out FILE]

One reference of the bench's cfg2 shape (synth: 512 tips x 1500 sites, 4 states x 4 categories, reads of 150 sites).
For a duplication factor f the chunk holds reads / f distinct reads, each f times, shuffled (f = 1: no duplicates, the
search finds nothing and everything it does is overhead).  Rows travel as the CLI sends them: compact, 4-bit packed
(--layout compact: one byte per code).  All inputs and outputs are device buffers, so a wall time (host clock around a
call that ends in a device synchronise) is the call without transfers; "dedup" is the HIP-event timer of the search
(keys, sort, classes, scan, gather).  After a warm-up of both calls, `rounds` interleaved rounds; medians.
Per factor: dedup timer, wall of place_chunk_dedup, wall of place_chunk on the whole chunk, their ratio; from the
factor-1 leg the overhead as a share of the plain chunk body and the factor at which the search pays for itself
(overhead = plain wall x (1 - 1 / f), the chunk body taken as proportional to its reads).  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=100000)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--factors", default="1,4,20")
ap.add_argument("--layout", default="packed", choices=["packed", "compact"])
ap.add_argument("--out", default="")
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

import epa_ng_amd as epa  # noqa: E402
from epa_ng_amd import hostlib, synth  # noqa: E402

READ_LEN = 150
n = args.reads
w = synth.dna_workload(512, 1500, 1, READ_LEN, (1, 2, 3))
ref = hostlib.Reference(w["newick"], w["labels"], w["seqs"], states=4, subst=w["subst"], freqs=w["freqs"], rates=w["rates"])
ev = ref.evaluator()
cap = n * 64
d_pairs = [torch.empty(cap * 2, dtype=torch.int32, device="cuda") for _ in range(2)]
d_res = [torch.empty(cap * 3, dtype=torch.float64, device="cuda") for _ in range(2)]
d_rep = torch.empty(n, dtype=torch.int32, device="cuda")
d_first = torch.empty(n, dtype=torch.int32, device="cuda")
med = statistics.median
legs = []
for f in [int(x) for x in args.factors.split(",")]:
    distinct = n // f
    codes, wb, ws = synth.make_reads_compact(w["seqs"], distinct, READ_LEN, 0.03, 3, states=4)
    ids = np.random.RandomState(f).permutation(np.arange(n) % distinct)
    codes, wb, ws = np.ascontiguousarray(codes[ids]), wb[ids].copy(), ws[ids].copy()
    row_bytes = codes.shape[1]
    if args.layout == "packed":
        p = epa.pack_codes_4bit(codes)
        d_codes, row_bytes = epa.Packed4(torch.from_numpy(p.data).cuda(), p.stride), p.data.shape[1]
    else:
        d_codes = torch.from_numpy(codes).cuda()
    d_wb, d_ws = torch.from_numpy(wb.astype(np.int32)).cuda(), torch.from_numpy(ws.astype(np.int32)).cuda()

    def dedup_body():
        t = time.perf_counter()
        k, u = ev.place_chunk_dedup(d_codes, d_wb, d_ws, Q=n, max_span=READ_LEN, max_pairs=cap, pairs_out=d_pairs[0],
                                    results_out=d_res[0], rep_out=d_rep, first_out=d_first)
        torch.cuda.synchronize()
        return k, u, time.perf_counter() - t, ev.kernel_ms("dedup"), ev.kernel_ms("preplace"), ev.kernel_ms("thorough")

    def plain_body():
        t = time.perf_counter()
        k = ev.place_chunk(d_codes, d_wb, d_ws, Q=n, max_span=READ_LEN, max_pairs=cap, pairs_out=d_pairs[1], results_out=d_res[1])
        torch.cuda.synchronize()
        return k, time.perf_counter() - t, ev.kernel_ms("preplace"), ev.kernel_ms("thorough")

    kd, u = dedup_body()[:2]                    # warm-up of both, and a cross-check: the class rows fan out to the plain rows
    kp = plain_body()[0]
    mult = torch.bincount(d_rep.long(), minlength=u)
    fanned = int(mult[d_pairs[0][:2 * kd].view(-1, 2)[:, 1].long()].sum())
    t_d, t_p = [], []
    for _ in range(args.rounds):
        t_d.append(dedup_body()[2:])
        t_p.append(plain_body()[1:])
    wall_d, wall_p = med(r[0] for r in t_d), med(r[0] for r in t_p)
    legs.append(dict(factor=f, unique=int(u), pairs_dedup=int(kd), pairs_plain=int(kp), fanned_out_pairs=fanned,
                     rows_agree=fanned == kp, dedup_ms=med(r[1] for r in t_d), dedup_wall_ms=1e3 * wall_d,
                     plain_wall_ms=1e3 * wall_p, dedup_over_plain=wall_d / wall_p,
                     dedup_preplace_ms=med(r[2] for r in t_d), dedup_thorough_ms=med(r[3] for r in t_d),
                     plain_preplace_ms=med(r[1] for r in t_p), plain_thorough_ms=med(r[2] for r in t_p),
                     window_bytes_read=int(n * (READ_LEN * (4 if args.layout == "packed" else 8)) // 8), row_bytes=int(row_bytes),
                     dedup_wall_ms_all=[1e3 * r[0] for r in t_d], plain_wall_ms_all=[1e3 * r[0] for r in t_p]))
line = dict(shape="cfg2", branches=ref.B, sites=ref.W, reads=n, read_len=READ_LEN, layout=args.layout, rounds=args.rounds, legs=legs)
one = [g for g in legs if g["factor"] == 1]
if one:
    over = one[0]["dedup_wall_ms"] - one[0]["plain_wall_ms"]
    share = over / one[0]["plain_wall_ms"]
    line.update(factor1_overhead_ms=over, factor1_overhead_share_of_plain=share,
                factor1_dedup_timer_share_of_plain=one[0]["dedup_ms"] / one[0]["plain_wall_ms"],
                break_even_factor=(1.0 / (1.0 - share)) if 0.0 < share < 1.0 else None)
print(json.dumps(line), flush=True)
if args.out:
    with open(args.out, "w") as fo:
        fo.write(json.dumps(line) + "\n")
ev.close()
del ev, ref
