"""epa-ng-amd --rescore FILE.jplace --posterior [--prior-mean M] [--posterior-nodes KX,KP] end to end through the
executable, on the nucleotide fixture under tests/golden/data: a normal run places the queries on every branch
(--no-heur, every row kept: 13 rows per placement object), its jplace is rescored with --posterior.

  1. "fields" ends with marginal_like, post_prob; with --rell 100 as well the order is rell_support, marginal_like,
     post_prob, and the columns before them are those of the run without --posterior.
  2. post_prob adds up to 1 per placement object and is the softmax of the object's marginal_like column.
  3. marginal_like of every row is Evaluator.marginal_like with posterior_rule(mean branch length) on the same edge and
     read, to the printed precision; --prior-mean and --posterior-nodes change the numbers the way the Python call with
     the same rule does.
  4. the result does not depend on --chunk-size.

Largest |marginal_like (ten printed digits) - Evaluator.marginal_like| measured on MI355X: 4.9e-11.
"""
import re

import numpy as np
import pytest

import epa_ng_amd as epa
import rescore_util as ru
from epa_ng_amd import hostlib
from test_gpu_rell_cli import body
from test_gpu_score_at import make_pairs
from test_rescore_cpu import MSA, QUERY, TREE

pytestmark = pytest.mark.gpu

PRINTED = 2e-10        # ten printed digits: half a unit of the last one, and the same again for the reader
FIELDS_P = ru.FIELDS + ["marginal_like", "post_prob"]
FIELDS_RP = ru.FIELDS + ["rell_support", "marginal_like", "post_prob"]


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("marginal_cli")
    placed = tmp / "placed"
    placed.mkdir()
    r = ru.run_cli(TREE, MSA, QUERY, placed, ["--no-heur", "--filter-min-lwr", "0", "--filter-max", "64"])
    assert r.returncode == 0, r.stdout + r.stderr
    jp = placed / "epa_result.jplace"

    def run(tag, extra):
        out = tmp / tag
        out.mkdir()
        r = ru.run_cli(TREE, MSA, QUERY, out, ["--rescore", jp] + list(extra))
        assert r.returncode == 0, r.stdout + r.stderr
        return out / "epa_result.jplace", r

    # the evaluator's view of the same inputs: the columns the executable keeps, the default model
    labels, seqs = ru.read_fasta(MSA)
    names, reads = ru.read_fasta(QUERY)
    keep = hostlib.premask(MSA, QUERY) == 0
    cut = lambda sq: "".join(np.array(list(sq))[keep])   # noqa: E731
    ref = hostlib.Reference(open(TREE).read().strip(), labels, [cut(s) for s in seqs], model="GTR+G")
    lengths = np.array([ref.branch(b)["length"] for b in range(ref.B)])
    return dict(tmp=tmp, jp=jp, run=run, ref=ref, ev=ref.evaluator(), names=names, reads=[cut(s) for s in reads],
                mean=float(lengths.mean()), posterior=run("posterior", ["--posterior"]))


def check_against_evaluator(s, path, rule, fields=FIELDS_P):
    res = ru.result(path.parent)
    assert res["fields"] == fields
    col = fields.index("marginal_like")
    codes, wb, ws = epa.encode_queries(4, s["reads"], compact=True)
    worst, rows_seen = 0.0, 0
    for pq in res["placements"]:
        q = s["names"].index(pq["n"][0])
        rows = pq["p"]
        assert all(len(row) == len(fields) for row in rows) and len(rows) == s["ref"].B
        edges = [row[0] for row in rows]
        want = s["ev"].marginal_like(make_pairs(edges, [q] * len(edges)), codes, wb, ws, *rule)
        got = np.array([row[col] for row in rows])
        worst = max(worst, float(np.max(np.abs(got - want))))
        assert np.all(np.abs(got - want) < PRINTED), (pq["n"], got, want)
        post = np.array([row[col + 1] for row in rows])
        e = np.exp(want - want.max())
        assert np.all(np.abs(post - e / e.sum()) < PRINTED)
        assert abs(post.sum() - 1.0) < PRINTED * len(rows)
        assert all(rows[i][2] >= rows[i + 1][2] for i in range(len(rows) - 1))      # still sorted by like_weight_ratio
        rows_seen += len(rows)
    assert rows_seen > len(res["placements"])
    return worst, res


def test_default_rule_equals_the_evaluator(setup):
    path, r = setup["posterior"]
    worst, res = check_against_evaluator(setup, path, epa.posterior_rule(setup["mean"]))
    print("\n--posterior: max |marginal_like - Evaluator.marginal_like| %.3g over %d objects" % (worst, len(res["placements"])))
    assert len(res["placements"]) == 2
    assert "warning" not in r.stderr


def test_without_the_flag_nothing_changes(setup):
    plain, _ = setup["run"]("plain", [])
    assert ru.result(plain.parent)["fields"] == ru.FIELDS
    # the --posterior file is the plain file plus two columns and two field names
    stripped = re.sub(r"(\n      \[[^\]\n]*), [-0-9.]+, [-0-9.]+\]", r"\1]", body(setup["posterior"][0]))
    assert stripped.replace(', "marginal_like", "post_prob"]', "]") == body(plain)


def test_with_rell_the_fields_follow_rell_support(setup):
    both, _ = setup["run"]("both", ["--posterior", "--rell", 100])
    check_against_evaluator(setup, both, epa.posterior_rule(setup["mean"]), fields=FIELDS_RP)
    rell, _ = setup["run"]("rell", ["--rell", 100])
    stripped = re.sub(r"(\n      \[[^\]\n]*), [-0-9.]+, [-0-9.]+\]", r"\1]", body(both))
    assert stripped.replace(', "marginal_like", "post_prob"]', "]") == body(rell)


def test_prior_mean_and_node_counts(setup):
    default = body(setup["posterior"][0])
    path, _ = setup["run"]("mean", ["--posterior", "--prior-mean", "0.25"])
    check_against_evaluator(setup, path, epa.posterior_rule(0.25))
    assert body(path) != default
    path, _ = setup["run"]("nodes", ["--posterior", "--posterior-nodes", "4,7"])
    check_against_evaluator(setup, path, epa.posterior_rule(setup["mean"], Kx=4, Kp=7))
    assert body(path) != default
    path, _ = setup["run"]("both_flags", ["--posterior", "--prior-mean", "0.02", "--posterior-nodes", "64,64"])
    check_against_evaluator(setup, path, epa.posterior_rule(0.02, Kx=64, Kp=64))
    # the default rule, spelled out
    path, _ = setup["run"]("spelled", ["--posterior", "--posterior-nodes", "8,16", "--prior-mean", repr(setup["mean"])])
    assert body(path) == default


def test_small_pendant_nodes_are_warned_about(setup):
    _, r = setup["run"]("tiny", ["--posterior", "--prior-mean", "1e-4"])
    assert "warning" in r.stderr and "1 / pendant" in r.stderr and "--prior-mean" in r.stderr


def test_chunk_size_does_not_matter(setup):
    path, _ = setup["run"]("chunk1", ["--posterior", "--chunk-size", 1])
    assert body(path) == body(setup["posterior"][0])
