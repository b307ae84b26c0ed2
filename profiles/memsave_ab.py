"""Resident against blocked lookup layout (EPA_FLAG_LOOKUP_BLOCKS), same box, alternating child processes.

  python profiles/memsave_ab.py [--rounds 3] [--reps 5] [--shapes cfg2,big] [--out FILE]

Driver: for every shape, `rounds` rounds of one child process per variant, variants alternating inside a round
(resident, blocks of 1024, ... , resident, ...), every child under its own time limit; the first child that fails,
faults or times out ends the run (nothing else is started on the device).  Child (--child): builds the reference,
creates ONE context in the variant's layout, and for every case runs one warm-up and `reps` timed fused chunk bodies
(epa_dev_place_chunk); per repeat the library's HIP-event kernel times ("lookup_block", "preplace", "select",
"thorough": epa_dev_last_kernel_ms) and the wall time of the call.  One JSON line per (variant, case, round); the
driver prints median and min..max over all repeats of all rounds (the table of profiles/memsave.md).

Shapes:  cfg2  512 tips x 1500 sites (B = 1021), chunks of 100 000 and 5 000 reads of 150 sites; resident, blocks 1024
         big   32 770 tips x 96 sites (B = 65 537), chunks of 20 000 reads of 64 sites; resident, blocks 256 / 1024 / 4096
The Newton launch with and without refI is the "thorough" column of resident against blocked."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SHAPES = {"cfg2": dict(variants=[0, 1024], limit=240), "big": dict(variants=[0, 256, 1024, 4096], limit=300)}

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--shapes", default="cfg2,big")
ap.add_argument("--out", default="")
ap.add_argument("--child", default="")       # SHAPE:BLOCK (0 = resident)
ap.add_argument("--round", type=int, default=0)
args = ap.parse_args()


def child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import epa_ng_amd as epa
    from epa_ng_amd import hostlib, synth
    shape, blk = args.child.split(":")
    blk = int(blk)
    if shape == "cfg2":
        w = synth.dna_workload(512, 1500, 1, 150, (1, 2, 3))
        enc = synth.make_reads_compact(w["seqs"], 100000, 150, 0.03, 3)
        cases, span = (("100000 reads", 100000), ("5000 reads", 5000)), 150
    else:
        import large_tree_gen as gen
        w = gen.dna_workload(32770, 96, 20000, 64, (201, 202, 203))
        enc = epa.encode_queries(4, w["reads"], compact=True)
        cases, span = (("20000 reads", 20000),), 64
    ref = hostlib.Reference(w["newick"], w["labels"], w["seqs"], states=4, subst=w["subst"], freqs=w["freqs"], rates=w["rates"])
    t0 = time.perf_counter()
    ev = ref.evaluator(flags=epa.FLAG_LOOKUP_BLOCKS if blk else 0)
    if blk:
        ev.set_option("lookup_block", blk)
    assert ev.lookup_mode() == ((epa.LOOKUP_BLOCKS, blk) if blk else (epa.LOOKUP_RESIDENT, 0))
    create_s = time.perf_counter() - t0
    codes, wb, ws = enc
    fams = ("lookup_block", "preplace", "select", "thorough")
    for name, Q in cases:
        c = (codes[:Q], wb[:Q], ws[:Q])
        rows = []
        for i in range(1 + args.reps):
            t0 = time.perf_counter()
            p, _ = ev.place_chunk(*c, max_span=span, max_pairs=Q * 64)
            wall = (time.perf_counter() - t0) * 1e3
            if i:
                rows.append(dict(wall=wall, **{f: max(0.0, ev.kernel_ms(f)) for f in fams}))
        print(json.dumps(dict(shape=shape, block=blk, case=name, round=args.round, pairs=len(p), create_s=create_s,
                              lookup_once_ms=ev.kernel_ms("lookup"), free_bytes=ev.mem_info()[0], reps=rows)), flush=True)
    ev.close()


def driver():
    lines = []
    for shape in args.shapes.split(","):
        for rnd in range(args.rounds):
            for blk in SHAPES[shape]["variants"]:
                cmd = ["timeout", "-k", "10", str(SHAPES[shape]["limit"]), sys.executable, os.path.abspath(__file__), "--child",
                       "%s:%d" % (shape, blk), "--round", str(rnd), "--reps", str(args.reps)]
                r = subprocess.run(cmd, capture_output=True, text=True)
                if r.returncode != 0:     # a fault, an abort, a time limit: nothing more is started on the device
                    sys.stderr.write(r.stdout + r.stderr)
                    sys.exit("child %s:%d ended with status %d: stopping" % (shape, blk, r.returncode))
                lines += [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))
    keys = sorted({(x["shape"], x["case"], x["block"]) for x in lines})
    print("| shape | case | layout | wall ms | lookup_block ms | preplace ms | select ms | thorough ms | build share |")
    print("|---|---|---|---|---|---|---|---|---|")
    for shape, case, blk in keys:
        reps = [r for x in lines if (x["shape"], x["case"], x["block"]) == (shape, case, blk) for r in x["reps"]]

        def cell(k):
            v = [r[k] for r in reps]
            return "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))
        body = [r["lookup_block"] + r["preplace"] + r["select"] + r["thorough"] for r in reps]
        share = statistics.median([r["lookup_block"] / b for r, b in zip(reps, body)])
        print("| %s | %s | %s | %s | %s | %s | %s | %s | %.1f %% |" % (
            shape, case, "blocks of %d" % blk if blk else "resident", cell("wall"), cell("lookup_block"), cell("preplace"),
            cell("select"), cell("thorough"), 100.0 * share))
    for x in lines:
        if x["round"] == 0 and x["case"] == [y["case"] for y in lines if y["shape"] == x["shape"]][0]:
            print("%s %s: create %.2f s, one-off lookup build %.3f ms, free after the run %.2f GB"
                  % (x["shape"], "blocks of %d" % x["block"] if x["block"] else "resident", x["create_s"],
                     x["lookup_once_ms"], x["free_bytes"] / 1e9))


if args.child:
    child()
else:
    driver()
