"""epa-ng-amd --rescore FILE.jplace --rell N [--rell-seed S] end to end through the executable.

The input is a jplace written by hand for D5 of tests/brute_cases.py (as in tests/test_gpu_rescore_cli.py) with the 22
reads of 30 sites of the statistical tests (tests/rell_ref.py, stat_input): three rows per read on its best
preplacement branch and two adjacent ones, lengths that ten printed digits hold exactly (so a rescored file read again
carries the same doubles), the placement objects in reverse read order.

  1. --rell 200 appends the field "rell_support" to "fields" and to every row; the values are Evaluator.rell_support
     at the file's lengths with the placement object's index as the stream id; they add up to 1 per object.
  2. --chunk-size 1 and the default chunk size give the same file.
  3. the output, rescored again with --rell, reproduces itself (its rows are LWR-sorted: another entry order).
  4. without --rell the output has the five fields, and the --rell output is that file plus the sixth column: the
     flag changes nothing else.  Another --rell-seed gives other values.
  5. --rell / --rell-seed without --rescore exit non-zero and name the two-step workflow; --rell 0 is refused.
"""
import json
import re

import numpy as np
import pytest

import brute_cases as bc
import epa_ng_amd as epa
import rell_ref as rr
import rescore_util as ru
from epa_ng_amd import hostlib
from gen_golden import DEFAULT_BL
from test_gpu_rescore_cli import model_string
from test_gpu_score_at import make_pairs

pytestmark = pytest.mark.gpu

R = 200
FIELDS6 = ru.FIELDS + ["rell_support"]


def body(path):
    """the file's text without the line that records the command line"""
    text = open(path).read()
    assert text.count('"invocation"') == 1
    return re.sub(r'"metadata": \{"invocation": "[^"]*"\},', "", text)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rell_cli")
    c = bc.case("D5")
    assert c["pinv"] == 0.0
    tre, msa, qf = tmp / "ref.tre", tmp / "ref.fasta", tmp / "q.fasta"
    tre.write_text(c["newick"] + "\n")
    ru.write_fasta(msa, c["labels"], c["seqs"])
    # the 30-site reads of the statistical tests, each on its best preplacement branch and two adjacent ones (half of
    # them are undecided between their branches); one sequence the jplace does not name, with a character in every column
    stat = rr.stat_input()
    reads = list(stat["reads"])
    names = ["r%d" % i for i in range(len(reads))]
    W = len(reads[0])
    ru.write_fasta(qf, ["extra_full"] + names, ["".join("ACGT"[i % 4] for i in range(W))] + reads)
    keep = hostlib.premask(str(msa), str(qf)) == 0
    cut = lambda sq: "".join(np.array(list(sq))[keep])   # noqa: E731
    ref = hostlib.Reference(c["newick"], c["labels"], [cut(s) for s in c["seqs"]], model=model_string(c))
    ten = lambda x: float("%.10f" % x)                   # noqa: E731
    placements, rows_of = [], {}
    for q in range(len(reads)):
        rows = []
        for k, edge in enumerate(int(b) for b in stat["branch"][3 * q:3 * q + 3]):
            pendant = ten(DEFAULT_BL * (1.0 + 0.5 * k))
            distal = ten(0.5 * ref.branch(edge)["length"])
            assert distal <= ref.branch(edge)["length"]
            rows.append([edge, -1.0, 0.3, distal, pendant])
        rows_of[names[q]] = rows
        placements.append({"p": rows, "n": [names[q]]})
    placements = placements[::-1]
    jp = tmp / "in.jplace"
    jp.write_text(json.dumps(ru.jplace_doc(placements), indent=1))

    def run(tag, extra, jplace=jp):
        out = tmp / tag
        out.mkdir()
        r = ru.run_cli(tre, msa, qf, out, ["--rescore", jplace] + list(extra), model=model_string(c))
        assert r.returncode == 0, r.stdout + r.stderr
        return out / "epa_result.jplace"

    return dict(c=c, tmp=tmp, tre=tre, msa=msa, qf=qf, jp=jp, run=run, ref=ref, reads=[cut(r) for r in reads], names=names,
                rows_of=rows_of, order=[p["n"][0] for p in placements], rell=run("rell", ["--rell", R]))


def test_sixth_field_equals_the_evaluator(setup):
    s = setup
    res = json.load(open(s["rell"]))
    assert res["fields"] == FIELDS6
    assert [pq["n"][0] for pq in res["placements"]] == s["order"]
    codes, wb, ws = epa.encode_queries(4, s["reads"], compact=True)
    pb, ps, pen, dis = [], [], [], []
    for q, name in enumerate(s["names"]):
        for edge, _, _, distal, pendant in s["rows_of"][name]:
            pb.append(edge), ps.append(q), pen.append(pendant), dis.append(distal)
    stream_id = np.array([s["order"].index(name) for name in s["names"]], np.uint64)
    want = s["ref"].evaluator().rell_support(make_pairs(pb, ps), np.array(pen), np.array(dis), codes, wb, ws, R,
                                             stream_id=stream_id)
    want = {(ps[i], pb[i]): want[i] for i in range(len(pb))}
    undecided = 0
    for pq in res["placements"]:
        q = s["names"].index(pq["n"][0])
        assert all(len(row) == 6 for row in pq["p"])
        got = {(q, row[0]): row[5] for row in pq["p"]}
        assert len(got) == 3
        for key, v in got.items():
            assert abs(v - want[key]) < 1e-9, (key, v, want[key])
        assert abs(sum(got.values()) - 1.0) < 1e-9
        undecided += max(got.values()) < 1.0
    assert undecided >= 2
    # the default seed is 1
    assert body(s["run"]("seed1", ["--rell", R, "--rell-seed", 1])) == body(s["rell"])


def test_chunk_size_does_not_matter(setup):
    assert body(setup["run"]("chunk1", ["--rell", R, "--chunk-size", 1])) == body(setup["rell"])


def test_output_reproduces_itself(setup):
    again = setup["run"]("again", ["--rell", R], jplace=setup["rell"])
    assert body(again) == body(setup["rell"])


def test_without_the_flag_nothing_changes(setup):
    plain = setup["run"]("plain", [])
    assert json.load(open(plain))["fields"] == ru.FIELDS
    # the --rell file is the plain file plus the sixth column and the sixth field name
    stripped = re.sub(r"(\n      \[[^\]\n]*), [-0-9.]+\]", r"\1]", body(setup["rell"])).replace(', "rell_support"]', "]")
    assert stripped == body(plain)
    other = setup["run"]("seed2", ["--rell", R, "--rell-seed", 2])
    assert body(other) != body(setup["rell"])
    strip = lambda t: re.sub(r"(\n      \[[^\]\n]*), [-0-9.]+\]", r"\1]", t)   # noqa: E731
    assert strip(body(other)) == strip(body(setup["rell"]))


def test_misuse_is_refused(setup):
    s = setup
    out = s["tmp"] / "refused"
    out.mkdir()
    for extra in (["--rell", 100], ["--rell-seed", 3]):
        r = ru.run_cli(s["tre"], s["msa"], s["qf"], out, extra, model=model_string(s["c"]))
        assert r.returncode != 0
        assert "--rescore out.jplace --rell N" in r.stderr and "place first" in r.stderr, r.stderr
    for extra in (["--rell", 0], ["--rell", (1 << 20) + 1], ["--rell-seed", 3]):
        r = ru.run_cli(s["tre"], s["msa"], s["qf"], out, ["--rescore", s["jp"]] + extra, model=model_string(s["c"]))
        assert r.returncode != 0 and "--rell" in r.stderr, r.stderr
    assert not (out / "epa_result.jplace").exists()
