"""epa-ng-amd --rescore FILE.jplace --rell N --rell-tests end to end through the executable, on the input of
tests/test_gpu_rell_cli.py (22 reads of 30 sites, three rows each, the placement objects in reverse read order).

  1. the fields "elw" and "p_sh" follow "rell_support" directly, in "fields" and in every row; with --posterior the order
     is rell_support, elw, p_sh, marginal_like, post_prob.
  2. the values are Evaluator.rell_tests at the file's lengths with the placement object's index as the stream id, to
     the printed digits; elw adds up to 1 per object and some row of every object has p_sh = 1.
  3. --chunk-size 1 gives the same file.
  4. the file with the two columns removed is, byte for byte, the --rell-only file: the flag changes nothing else.
"""
import json
import re

import numpy as np
import pytest

import epa_ng_amd as epa
from test_gpu_rell_cli import FIELDS6, R, body, setup  # noqa: F401  (setup: the module's fixture)
from test_gpu_score_at import make_pairs

pytestmark = pytest.mark.gpu

FIELDS8 = FIELDS6 + ["elw", "p_sh"]


@pytest.fixture(scope="module")
def tests_file(setup):  # noqa: F811
    return setup["run"]("tests", ["--rell", R, "--rell-tests"])


def test_fields_and_values_equal_the_evaluator(setup, tests_file):  # noqa: F811
    s = setup
    res = json.load(open(tests_file))
    assert res["fields"] == FIELDS8
    assert [pq["n"][0] for pq in res["placements"]] == s["order"]
    codes, wb, ws = epa.encode_queries(4, s["reads"], compact=True)
    pb, ps, pen, dis = [], [], [], []
    for q, name in enumerate(s["names"]):
        for edge, _, _, distal, pendant in s["rows_of"][name]:
            pb.append(edge), ps.append(q), pen.append(pendant), dis.append(distal)
    stream_id = np.array([s["order"].index(name) for name in s["names"]], np.uint64)
    want = s["ref"].evaluator().rell_tests(make_pairs(pb, ps), np.array(pen), np.array(dis), codes, wb, ws, R, stream_id=stream_id)
    at = {(ps[i], pb[i]): i for i in range(len(pb))}
    inside = 0
    for pq in res["placements"]:
        q = s["names"].index(pq["n"][0])
        assert len(pq["p"]) == 3 and all(len(row) == 8 for row in pq["p"])
        for row in pq["p"]:
            i = at[(q, row[0])]
            for col, key in ((5, "support"), (6, "elw"), (7, "p_sh")):
                assert abs(row[col] - want[key][i]) < 1e-9, (pq["n"], row, key, want[key][i])
        assert abs(sum(row[6] for row in pq["p"]) - 1.0) < 1e-9
        assert max(row[7] for row in pq["p"]) == 1.0
        inside += any(0.0 < row[7] < 1.0 for row in pq["p"])
    assert inside >= 2


def test_order_with_posterior(setup, tests_file):  # noqa: F811
    both = json.load(open(setup["run"]("tests_post", ["--rell", R, "--rell-tests", "--posterior"])))
    assert both["fields"] == FIELDS8 + ["marginal_like", "post_prob"]
    post = json.load(open(setup["run"]("rell_post", ["--rell", R, "--posterior"])))
    assert post["fields"] == FIELDS6 + ["marginal_like", "post_prob"]
    tests = json.load(open(tests_file))
    for a, b, c in zip(both["placements"], post["placements"], tests["placements"]):
        assert a["n"] == b["n"] == c["n"]
        assert [row[:6] + row[8:] for row in a["p"]] == b["p"]
        assert [row[:8] for row in a["p"]] == c["p"]


def test_chunk_size_does_not_matter(setup, tests_file):  # noqa: F811
    assert body(setup["run"]("tests_chunk1", ["--rell", R, "--rell-tests", "--chunk-size", 1])) == body(tests_file)


def test_without_the_flag_nothing_changes(setup, tests_file):  # noqa: F811
    strip = lambda t: re.sub(r"(\n      \[[^\]\n]*), [-0-9.]+\]", r"\1]", t)   # noqa: E731
    text = body(tests_file)
    assert text.count(', "elw", "p_sh"]') == 1
    assert strip(strip(text)).replace(', "elw", "p_sh"]', "]") == body(setup["rell"])
