"""epa-ng-amd --rescore FILE.jplace --rell N --kh end to end through the executable, on the input of
tests/test_gpu_rell_cli.py (22 reads of 30 sites, three rows each, the placement objects in reverse read order).

  1. the fields "p_kh", "p_wkh", "p_wsh" follow "rell_support" directly, in "fields" and in every row; with --rell-tests
     and --au they follow "p_au"; with --posterior they stand before "marginal_like".
  2. the values are Evaluator.rell_kh at the file's lengths with the placement object's index as the stream id: the same
     doubles after the round trip through the printed digits.
  3. --chunk-size 1 gives the same file.
  4. the file with the three columns removed is, byte for byte, the file written without --kh: the flag changes nothing
     else.
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
KH = ["p_kh", "p_wkh", "p_wsh"]


@pytest.fixture(scope="module")
def kh_file(setup):  # noqa: F811
    return setup["run"]("kh", ["--rell", R, "--kh"])


def test_fields_and_values_equal_the_evaluator(setup, kh_file):  # noqa: F811
    s = setup
    res = json.load(open(kh_file))
    assert res["fields"] == FIELDS6 + KH
    assert [pq["n"][0] for pq in res["placements"]] == s["order"]
    codes, wb, ws = epa.encode_queries(4, s["reads"], compact=True)
    pb, ps, pen, dis = [], [], [], []
    for q, name in enumerate(s["names"]):
        for edge, _, _, distal, pendant in s["rows_of"][name]:
            pb.append(edge), ps.append(q), pen.append(pendant), dis.append(distal)
    stream_id = np.array([s["order"].index(name) for name in s["names"]], np.uint64)
    want = s["ref"].evaluator().rell_kh(make_pairs(pb, ps), np.array(pen), np.array(dis), codes, wb, ws, R, stream_id=stream_id)
    at = {(ps[i], pb[i]): i for i in range(len(pb))}
    inside = 0
    for pq in res["placements"]:
        q = s["names"].index(pq["n"][0])
        assert len(pq["p"]) == 3 and all(len(row) == 9 for row in pq["p"])
        for row in pq["p"]:
            i = at[(q, row[0])]
            for col, key in enumerate(KH):
                # the printed digits read back: the same double as the evaluator's value through the same round trip
                assert row[6 + col] == float("%.*f" % (PRECISION, want[key][i])), (pq["n"], row, key, want[key][i])
                assert 0.0 <= row[6 + col] <= 1.0
            inside += bool(0.0 < row[7] < 1.0 and 0.0 < row[8] < 1.0)
        assert max(row[6] for row in pq["p"]) == 1.0
    assert inside >= 2


def test_order_with_every_other_flag_and_nothing_else_changes(setup, kh_file):  # noqa: F811
    kh = json.load(open(kh_file))
    every = json.load(open(setup["run"]("kh_every", ["--kh", "--posterior", "--au", "--rell-tests", "--rell", R])))
    assert every["fields"] == FIELDS6 + ["elw", "p_sh", "p_au"] + KH + ["marginal_like", "post_prob"]
    for a, b in zip(every["placements"], kh["placements"]):
        assert a["n"] == b["n"]
        assert [row[:6] + row[9:12] for row in a["p"]] == b["p"]
    # the three columns removed: the file of --rell alone
    strip = lambda t: re.sub(r"(\n      \[[^\]\n]*), [-0-9.]+, [-0-9.]+, [-0-9.]+\]", r"\1]", t)   # noqa: E731
    text = body(kh_file)
    assert text.count(', "p_kh", "p_wkh", "p_wsh"]') == 1
    assert strip(text).replace(', "p_kh", "p_wkh", "p_wsh"]', "]") == body(setup["rell"])


def test_chunk_size_does_not_matter(setup, kh_file):  # noqa: F811
    assert body(setup["run"]("kh_chunk1", ["--rell", R, "--kh", "--chunk-size", 1])) == body(kh_file)
