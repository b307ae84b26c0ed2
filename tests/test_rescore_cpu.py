"""epa-ng-amd --rescore: what is refused before any device is touched.  None of these runs needs a GPU; on a machine
without one a run that got as far as creating the device context would end with the no-device message instead of the
message asserted here, so the file also shows that reading and validating the jplace comes first."""
import json
import os

import pytest

import epa_ng_amd as epa
from epa_ng_amd import hostlib
import rescore_util as ru

TREE = os.path.join(ru.DATA, "ref.tre")
MSA = os.path.join(ru.DATA, "aln.fasta")
QUERY = os.path.join(ru.DATA, "query.fasta")
# the fixture's tips on a bifurcating root
ROOTED = "((A:0.2,B:0.1):0.05,((C:0.1,H:0.1):0.05,(D:0.5,(E:0.5,(F:0.2,G:0.2):0.05):0.2):0.1):0.05);"


@pytest.fixture(scope="module")
def ref():
    labels, seqs = ru.read_fasta(MSA)
    r = hostlib.Reference(open(TREE).read().strip(), labels, seqs, model="GTR+G")
    assert r.B == 13
    return r


def rows(ref, distal_factor=0.5, pendant=0.1, edge=3):
    length = ref.branch(edge)["length"] if edge < ref.B else 0.1
    return [[edge, -1000.0, 1.0, distal_factor * length, pendant]]


def refused(tmp_path, doc_text, message, tree=TREE, extra=()):
    jp = tmp_path / "in.jplace"
    jp.write_text(doc_text)
    out = tmp_path / "out"
    out.mkdir()
    r = ru.run_cli(tree, MSA, QUERY, out, ["--rescore", jp] + list(extra))
    assert r.returncode == 1, r.stdout + r.stderr
    assert message in r.stderr, r.stderr
    assert "no HIP device" not in r.stderr
    assert not (out / "epa_result.jplace").exists()
    return r


def good_doc(ref):
    return ru.jplace_doc([{"p": rows(ref), "n": ["Rat"]}, {"p": rows(ref, edge=7), "n": ["Carp"]}])


def test_truncated_json(ref, tmp_path):
    text = json.dumps(good_doc(ref))
    r = refused(tmp_path, text[:len(text) // 2], "malformed JSON")
    assert "in.jplace" in r.stderr


def test_fields_without_pendant_length(ref, tmp_path):
    doc = good_doc(ref)
    doc["fields"] = ["edge_num", "likelihood", "like_weight_ratio", "distal_length", "other"]
    r = refused(tmp_path, json.dumps(doc), "pendant_length")
    assert "in.jplace" in r.stderr and "missing" in r.stderr


def test_edge_num_equal_to_the_branch_count(ref, tmp_path):
    doc = ru.jplace_doc([{"p": rows(ref, edge=ref.B), "n": ["Rat"]}])
    refused(tmp_path, json.dumps(doc), "edge_num %d" % ref.B)


def test_negative_pendant_length(ref, tmp_path):
    doc = ru.jplace_doc([{"p": rows(ref, pendant=-0.1), "n": ["Rat"]}])
    refused(tmp_path, json.dumps(doc), "pendant_length")


def test_distal_length_beyond_the_branch(ref, tmp_path):
    doc = ru.jplace_doc([{"p": rows(ref, distal_factor=1.5), "n": ["Rat"]}])
    refused(tmp_path, json.dumps(doc), "distal_length")


def test_two_names_in_one_n(ref, tmp_path):
    doc = ru.jplace_doc([{"p": rows(ref), "n": ["Rat", "Carp"]}])
    refused(tmp_path, json.dumps(doc), "exactly one name")


def test_rooted_tree_with_preserve_rooting_on(ref, tmp_path):
    tre = tmp_path / "rooted.tre"
    tre.write_text(ROOTED + "\n")
    refused(tmp_path, json.dumps(good_doc(ref)), "--preserve-rooting off", tree=tre)


@pytest.mark.parametrize("extra,message", [(["--no-heur"], "--no-heur"), (["--devices", "0,1"], "--devices"),
                                           (["--world", "2"], "--world")])
def test_flags_that_do_not_combine_with_rescore(ref, tmp_path, extra, message):
    r = refused(tmp_path, json.dumps(good_doc(ref)), message, extra=extra)
    assert "--rescore" in r.stderr


def test_distal_length_just_beyond_the_branch_is_clamped_not_refused(ref, tmp_path):
    """5e-7 over the branch's length is a writer's rounding: the reader lets it pass.  Without a GPU the run then ends at
    the device with the no-device message, which shows that the reader did not reject it."""
    if epa.device_count() > 0:
        want_rc, want = 0, ""
    else:
        want_rc, want = 1, "no HIP device"
    row = rows(ref)
    row[0][3] = ref.branch(3)["length"] + 5e-7
    jp = tmp_path / "in.jplace"
    jp.write_text(json.dumps(ru.jplace_doc([{"p": row, "n": ["Rat"]}])))
    r = ru.run_cli(TREE, MSA, QUERY, tmp_path, ["--rescore", jp])
    assert r.returncode == want_rc, r.stdout + r.stderr
    assert want in r.stderr and "distal_length" not in r.stderr
