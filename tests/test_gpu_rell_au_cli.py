"""epa-ng-amd --rescore FILE.jplace --rell N --au end to end through the executable, on the input of
tests/test_gpu_rell_cli.py (22 reads of 30 sites, three rows each, the placement objects in reverse read order).

  1. the field "p_au" follows "rell_support" directly, in "fields" and in every row; with --rell-tests it follows "p_sh";
     with --posterior it stands before "marginal_like".
  2. the values are Evaluator.rell_au (the default scales, N replicates per scale) at the file's lengths with the placement
     object's index as the stream id: the same doubles after the round trip through the printed digits.
  3. --chunk-size 1 gives the same file.
  4. the file with the column removed is, byte for byte, the file written without --au: the flag changes nothing else.
"""
import json
import re

import numpy as np
import pytest

import epa_ng_amd as epa
from test_gpu_rell_cli import FIELDS6, R, body, setup  # noqa: F401  (setup: the module's fixture)
from test_gpu_score_at import make_pairs

pytestmark = pytest.mark.gpu

PRECISION = 10          # the executable's default number of printed digits


@pytest.fixture(scope="module")
def au_file(setup):  # noqa: F811
    return setup["run"]("au", ["--rell", R, "--au"])


def test_field_and_values_equal_the_evaluator(setup, au_file):  # noqa: F811
    s = setup
    res = json.load(open(au_file))
    assert res["fields"] == FIELDS6 + ["p_au"]
    assert [pq["n"][0] for pq in res["placements"]] == s["order"]
    codes, wb, ws = epa.encode_queries(4, s["reads"], compact=True)
    pb, ps, pen, dis = [], [], [], []
    for q, name in enumerate(s["names"]):
        for edge, _, _, distal, pendant in s["rows_of"][name]:
            pb.append(edge), ps.append(q), pen.append(pendant), dis.append(distal)
    stream_id = np.array([s["order"].index(name) for name in s["names"]], np.uint64)
    want = s["ref"].evaluator().rell_au(make_pairs(pb, ps), np.array(pen), np.array(dis), codes, wb, ws, R, stream_id=stream_id)
    at = {(ps[i], pb[i]): i for i in range(len(pb))}
    fitted = 0
    for pq in res["placements"]:
        q = s["names"].index(pq["n"][0])
        assert len(pq["p"]) == 3 and all(len(row) == 7 for row in pq["p"])
        for row in pq["p"]:
            i = at[(q, row[0])]
            # the printed digits read back: the same double as the evaluator's value through the same round trip
            assert row[6] == float("%.*f" % (PRECISION, want["p_au"][i])), (pq["n"], row, want["p_au"][i])
            assert 0.0 <= row[6] <= 1.0
            fitted += bool(not np.isnan(want["fit"][i, 0]) and 0.0 < row[6] < 1.0)
    assert fitted >= 2


def test_order_with_rell_tests_and_posterior(setup, au_file):  # noqa: F811
    au = json.load(open(au_file))
    tests = json.load(open(setup["run"]("au_tests", ["--rell", R, "--rell-tests", "--au"])))
    assert tests["fields"] == FIELDS6 + ["elw", "p_sh", "p_au"]
    every = json.load(open(setup["run"]("au_tests_post", ["--au", "--posterior", "--rell-tests", "--rell", R])))
    assert every["fields"] == FIELDS6 + ["elw", "p_sh", "p_au", "marginal_like", "post_prob"]
    post = json.load(open(setup["run"]("au_post", ["--rell", R, "--au", "--posterior"])))
    assert post["fields"] == FIELDS6 + ["p_au", "marginal_like", "post_prob"]
    for a, b, c, d in zip(every["placements"], tests["placements"], post["placements"], au["placements"]):
        assert a["n"] == b["n"] == c["n"] == d["n"]
        assert [row[:9] for row in a["p"]] == b["p"]
        assert [row[:6] + row[8:] for row in a["p"]] == c["p"]
        assert [row[:6] + row[8:9] for row in a["p"]] == d["p"]


def test_chunk_size_does_not_matter(setup, au_file):  # noqa: F811
    assert body(setup["run"]("au_chunk1", ["--rell", R, "--au", "--chunk-size", 1])) == body(au_file)
    assert body(setup["run"]("au_chunk5", ["--rell", R, "--au", "--chunk-size", 5])) == body(au_file)


def test_without_the_flag_nothing_changes(setup, au_file):  # noqa: F811
    strip = lambda t: re.sub(r"(\n      \[[^\]\n]*), [-0-9.]+\]", r"\1]", t)   # noqa: E731
    text = body(au_file)
    assert text.count(', "p_au"]') == 1
    assert strip(text).replace(', "p_au"]', "]") == body(setup["rell"])
