"""epa-ng-amd --rescore FILE.jplace --edpl end to end through the executable.

40 reads of 120 sites are placed on a 24-tip tree; the result, with its first object cut down to one row, is rescored with
--edpl --precision 15.

  1. "exp_dist" and "edpl" are the last two fields, in "fields" and in every row.  Recomputed from the OUTPUT's own
     edge_num, distal_length and like_weight_ratio with brute() of tests/edpl_ref.py -- the topology parsed from the
     output's numbered Newick, which knows no root -- they agree within tol + 1e-14: the bound of tests/edpl_ref.py plus
     the printed precision (lengths, ratios and the two values travel through 15 digits).
  2. "edpl" is the same text on all rows of an object, 0 for an object of one row, and the like_weight_ratio-weighted
     mean of the object's exp_dist.
  3. with --rell 100 --posterior --edpl the two fields come last and the rest of the file is, byte for byte, the file
     written without --edpl.
"""
import json
import re

import numpy as np
import pytest

import edpl_ref as er
import rescore_util as ru
from epa_ng_amd import synth
from test_gpu_rell_cli import body
from test_gpu_rescore_cli import raw_rows

pytestmark = pytest.mark.gpu

EDPL = ["exp_dist", "edpl"]


def parse_numbered_newick(text):
    """'(a:0.1{0},(b:0.2{1},c:0.3{2})x:0.4{3},d:0.5{4});' -> (node_prox, node_dist, blen) indexed by edge number; the
    node above an edge is its proximal end (distal_length counts from the node below)"""
    edges = {}
    stack, nodes, closed = [], 0, None
    for tok in re.findall(r"[(),;]|[^(),;]+", text.strip()):
        if tok == "(":
            stack.append(nodes)
            nodes += 1
        elif tok == ")":
            closed = stack.pop()
            continue
        elif tok not in ",;":
            m = re.fullmatch(r"[^:]*:([-0-9.eE+]+)\{(\d+)\}", tok)
            if m is None:                       # the label of the top node: no edge above it
                assert closed is not None and not stack, tok
            else:
                if closed is None:              # a tip
                    closed = nodes
                    nodes += 1
                edges[int(m.group(2))] = (stack[-1], closed, float(m.group(1)))
        closed = None
    B = len(edges)
    assert sorted(edges) == list(range(B)) and nodes == B + 1
    prox, dist, blen = (np.array([edges[b][k] for b in range(B)], dt) for k, dt in ((0, np.uint32), (1, np.uint32), (2, np.float64)))
    return prox, dist, blen


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("edpl_cli")
    w = synth.dna_workload(24, 300, 40, 120, (41, 42, 43))
    tre, msa, qf = tmp / "ref.tre", tmp / "ref.fasta", tmp / "q.fasta"
    tre.write_text(w["newick"] + "\n")
    ru.write_fasta(msa, w["labels"], w["seqs"])
    ru.write_fasta(qf, ["r%d" % i for i in range(len(w["reads"]))], w["reads"])

    def run(tag, extra):
        out = tmp / tag
        out.mkdir()
        r = ru.run_cli(tre, msa, qf, out, extra)
        assert r.returncode == 0, r.stdout + r.stderr
        return out / "epa_result.jplace"

    placed = json.load(open(run("placed", ["--filter-min-lwr", "0.001"])))
    assert len(placed["placements"]) == 40
    placed["placements"][0]["p"] = placed["placements"][0]["p"][:1]
    jp = tmp / "in.jplace"
    jp.write_text(json.dumps(placed, indent=1))
    return dict(run=lambda tag, extra: run(tag, ["--rescore", jp] + list(extra)))


def test_fields_values_and_conventions(setup):
    path = setup["run"]("edpl15", ["--edpl", "--precision", 15])
    res = json.load(open(path))
    assert res["fields"] == ru.FIELDS + EDPL
    prox, dist, blen = parse_numbered_newick(res["tree"])
    assert len(blen) == 2 * 24 - 3
    text_rows = raw_rows(path)
    worst, multi, single = 0.0, 0, 0
    for pq, texts in zip(res["placements"], text_rows):
        rows = pq["p"]
        k = len(rows)
        assert all(len(r) == 7 for r in rows) and len(texts) == k
        assert len({t[6] for t in texts}) == 1                      # the object's value, the same text on every row
        branch = np.array([r[0] for r in rows], np.uint32)
        lwr, distal = np.array([r[2] for r in rows]), np.array([r[3] for r in rows])
        want_rows, want_edpl = er.brute(prox, dist, blen, branch, np.zeros(k, np.uint32), distal, lwr, 1)
        tol = er.tol(prox, dist, blen, k) + 1e-14
        for r, want in zip(rows, want_rows):
            worst = max(worst, abs(r[5] - want), abs(r[6] - want_edpl[0]))
            assert abs(r[5] - want) <= tol and abs(r[6] - want_edpl[0]) <= tol, (pq["n"], r, want, want_edpl[0], tol)
        assert abs(rows[0][6] - float(np.sum(lwr * np.array([r[5] for r in rows])))) <= tol
        if k == 1:
            single += 1
            assert rows[0][5] == 0.0 and rows[0][6] == 0.0
        else:
            multi += rows[0][6] > 1e-6
    print("\n--edpl: max |file - brute| %.3g over %d objects, %d of one row, %d spread over the tree" %
          (worst, len(res["placements"]), single, multi))
    assert single >= 1 and multi >= 3


def test_fields_come_last_and_nothing_else_changes(setup):
    every = setup["run"]("every", ["--rell", 100, "--posterior", "--edpl"])
    without = setup["run"]("without", ["--rell", 100, "--posterior"])
    assert json.load(open(every))["fields"] == ru.FIELDS + ["rell_support", "marginal_like", "post_prob"] + EDPL
    text = body(every)
    assert text.count(', "exp_dist", "edpl"]') == 1
    strip = lambda t: re.sub(r"(\n      \[[^\]\n]*), [-0-9.]+, [-0-9.]+\]", r"\1]", t)   # noqa: E731
    assert strip(text).replace(', "exp_dist", "edpl"]', "]") == body(without)


def test_all_fifteen_values_at_precision_70(setup):
    """Every optional field at once at --precision 70: rows of 15 numbers of more than 70 characters each, far beyond the
    writer's stack line.  The file is JSON, "fields" has 16 names, every number carries exactly 70 digits behind the
    point, and every value equals the same field of a --precision 15 run with the same flags within 5e-16 (half a unit
    of the fifteenth decimal) plus one ulp of the value."""
    import math
    flags = ["--rell", 100, "--rell-tests", "--au", "--kh", "--posterior", "--edpl"]
    p70 = setup["run"]("all70", flags + ["--precision", 70])
    p15 = setup["run"]("all15", flags + ["--precision", 15])
    res70, res15 = json.load(open(p70)), json.load(open(p15))
    assert len(res70["fields"]) == 16 and res70["fields"] == res15["fields"] and res70["fields"][-2:] == EDPL
    assert len(res70["placements"]) == len(res15["placements"]) == 40
    rows70, rows15 = raw_rows(p70), raw_rows(p15)
    worst, count = 0.0, 0
    for pq70, pq15, t70, t15 in zip(res70["placements"], res15["placements"], rows70, rows15):
        assert pq70["n"] == pq15["n"] and len(pq70["p"]) == len(pq15["p"]) == len(t70) == len(t15)
        for r70, r15, x70, x15 in zip(pq70["p"], pq15["p"], t70, t15):
            assert len(r70) == len(r15) == len(x70) == len(x15) == 16
            assert x70[0] == x15[0] and re.fullmatch(r"\d+", x70[0])
            for a, b, ta, tb in zip(r70[1:], r15[1:], x70[1:], x15[1:]):
                assert re.fullmatch(r"-?\d+\.\d{70}", ta), ta
                assert re.fullmatch(r"-?\d+\.\d{15}", tb), tb
                worst = max(worst, abs(a - b))
                count += 1
                assert abs(a - b) <= 5e-16 + math.ulp(a), (pq70["n"], ta, tb)
    print("\n--precision 70 against 15: max |difference| %.3g over %d values" % (worst, count))
    assert count >= 15 * 40
