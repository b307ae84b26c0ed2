#!/usr/bin/env python3
"""Generator of tests/golden/endpoints/*.json: where BruteForce.optimise (tests/brute_force.py) ends on the
configurations brute_cases.OPT_NAMES, under the sliding rule and --raxml-blo (T4 also with the lower length bound
1e-6, under both rules).  Uses the test suite's own Python alone: no oracle, no device, nothing outside the repository.

    python tests/gen_endpoints.py [-j PROCESSES] [NAME ...]

optimise costs 0.01 .. 0.2 s per pair, too slow for a GPU test, hence the committed files.  One file per configuration:
{"case", "thinning", "modes": {"<mode>@<min_branch>": {"pairs": [[branch, read] ...], "lnl", "pendant", "distal" (17
significant digits), "rounds", "reverted"}}}.

Thinning (the files are committed, so they are kept small, 2 .. 17 KB each): every read is
compared on PER_READ = 4 branches -- the first tip branch, the shortest and the longest branch of the tree, and further
candidates (the branches 0, step, 2 step, ... of brute_cases.pair_lists) taken cyclically from candidate q N / Q on, so
that the reads spread over the tree.
"""
import json
import multiprocessing
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import brute_cases as bc                                                              # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "endpoints")
PER_READ = 4
RULE = ("every read on %d branches: the first tip branch, the shortest and the longest branch, then candidates (branches 0, "
        "step, 2 step ...) cyclically from candidate q N / Q on") % PER_READ


def must_have(bf):
    tip = next(b for b, n in enumerate(bf.brs) if not n.kids)
    return sorted({tip, int(np.argmin(bf.lengths)), int(np.argmax(bf.lengths))})


def thinned_pairs(name):
    """-> [(branch, read)] branch-major"""
    c, bf = bc.case(name), bc.brute(name)
    cand = list(range(0, bf.B, c["branch_step"]))
    Q = len(c["reads"])
    pairs = set()
    for q in range(Q):
        mine = set(must_have(bf))
        for i in range(len(cand)):
            if len(mine) >= PER_READ:
                break
            mine.add(cand[(q * len(cand) // Q + i) % len(cand)])
        pairs |= {(b, q) for b in mine}
    return sorted(pairs)


def modes_of(name):
    return sorted({(v["mode"], v["min_branch"]) for v in bc.opt_variants(name)})


def work(job):
    name, mode, mn, pairs = job
    c, bf = bc.case(name), bc.brute(name)
    return [bf.optimise(b, c["reads"][q], mode=mode, min_branch=mn) for b, q in pairs]


def numbers(v):
    return "[" + ",".join("%.17g" % x for x in v) + "]"


def main():
    args = sys.argv[1:]
    procs = 4
    if args[:1] == ["-j"]:
        procs, args = int(args[1]), args[2:]
    names = args or list(bc.OPT_NAMES)
    os.makedirs(OUT, exist_ok=True)
    jobs, plan = [], {}
    for name in names:
        pairs = plan[name] = thinned_pairs(name)
        for mode, mn in modes_of(name):
            for i in range(0, len(pairs), 10):
                jobs.append((name, mode, mn, pairs[i:i + 10]))
    for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):   # matrices of 4 x 4 .. 20 x 20: library
        os.environ.setdefault(v, "1")                                        # threads only fight the worker processes
    with multiprocessing.get_context("spawn").Pool(procs) as pool:           # fresh interpreters: they read the above
        done = pool.map(work, jobs, chunksize=1)
    got = {}
    for job, res in zip(jobs, done):
        got.setdefault((job[0], job[1], job[2]), []).extend(res)
    for name in names:
        pairs = plan[name]
        parts = []
        for mode, mn in modes_of(name):
            r = got[(name, mode, mn)]
            assert len(r) == len(pairs)
            parts.append('"%s":{"pairs":%s,\n"lnl":%s,\n"pendant":%s,\n"distal":%s,\n"rounds":%s,\n"reverted":%s}'
                         % (bc.endpoint_key(mode, mn), json.dumps(pairs, separators=(",", ":")),
                            numbers(e["lnl"] for e in r), numbers(e["pendant"] for e in r),
                            numbers(e["distal"] for e in r), json.dumps([e["rounds"] for e in r], separators=(",", ":")),
                            json.dumps([int(e["reverted"]) for e in r], separators=(",", ":"))))
        text = '{"case":%s,\n"thinning":%s,\n"modes":{\n%s}}\n' % (json.dumps(name), json.dumps(RULE),
                                                               ",\n".join(parts))
        assert len(text) < 64 * 1024, (name, len(text))
        with open(os.path.join(OUT, name + ".json"), "w") as f:
            f.write(text)
        print(name, "pairs", len(pairs), "bytes", len(text), file=sys.stderr)


if __name__ == "__main__":
    main()
