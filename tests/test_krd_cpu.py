"""Kantorovich-Rubinstein distances without a device: the two references of tests/krd_ref.py against each other and
against what the distance must be in cases one can work out by hand, and the executable's refusals that need no device.

  1. restate() (rooted at node_prox[0]: pre-order ranks, prefix sums, two-pointer merge) and brute() (no root order: cuts,
     side masks from path sums, math.fsum) agree within tol(a, b) = 8 (B + n_a + n_b + 4) 2^-53 (W_a + W_b) sum(blen): all
     pairs on the trees with B <= 77, the special pairs plus 24 random ones on the 600-tip ladder and the 512-tip tree.
  2. two unit point masses are edpl_ref.brute's path distance apart.
  3. a sample against its copy moved by delta along one branch: delta x W.
  4. another root changes pairs of equal totals by less than tol and the pair with the 0.7 sample by more.
  5. clade_mass over the root's branches adds up to W; edge_mass over all branches does too.
  6. epa-ng-amd --krd: refused with -q, with --rescore, for duplicate sample names (before any file is read); for a file
     without like_weight_ratio, a bad multiplicity, an edge_num out of range and a sample of total mass 0 (after the tree
     is built, before a device is opened).
"""
import json
import subprocess

import numpy as np
import pytest

import edpl_ref as er
import krd_ref as kr
import rescore_util as ru
from epa_ng_amd import hostlib, synth


@pytest.mark.parametrize("name", er.TREES)
def test_restate_agrees_with_brute(name):
    c = kr.case(name)
    B, S = len(c["blen"]), c["S"]
    assert len(c["pairs"]) == S * (S - 1) // 2 if B <= 77 else len(c["pairs"]) >= 24 + 8
    worst = 0.0
    for a, b in c["pairs"]:
        d, t = abs(c["want"][a, b] - c["brute"][a, b]), c["tol"][a, b]
        worst = max(worst, d / t if t > 0 else (0.0 if d == 0.0 else np.inf))
        assert d <= t, (name, a, b, c["want"][a, b], c["brute"][a, b], t)
    print(name, "max |restate - brute| / tol %.3g over %d pairs" % (worst, len(c["pairs"])))
    ix = c["index"]
    assert c["want"][ix["r65"], ix["copy65"]] == 0.0 and c["brute"][ix["r65"], ix["copy65"]] == 0.0
    assert c["want"][ix["zeros"], ix["empty"]] == 0.0
    assert np.all(c["want"][~np.isnan(c["want"])] >= 0.0)
    assert c["want"][ix["unit_deep"], ix["unit_b0"]] > 1e6 * c["tol"][ix["unit_deep"], ix["unit_b0"]]
    if name == "ladder600":
        assert "every" in ix and B > 1024            # a sample with a point on every branch: ranks beyond one tile


@pytest.mark.parametrize("name", er.TREES)
def test_two_unit_points_are_their_path_distance_apart(name):
    c = kr.case(name)
    a, b = c["index"]["unit_deep"], c["index"]["unit_b0"]
    rows = [int(np.flatnonzero(c["seq"] == s)[0]) for s in (a, b)]
    row_dist, _ = er.brute(c["prox"], c["dist"], c["blen"], c["branch"][rows], [0, 0], c["distal"][rows], [0.0, 1.0], 1)
    for ref in (c["want"], c["brute"]):
        assert abs(ref[a, b] - row_dist[0]) <= c["tol"][a, b] + er.tol(c["prox"], c["dist"], c["blen"], 2)


def test_a_copy_shifted_along_one_branch():
    prox, dist, blen = er.tree("random40")
    B = len(blen)
    rng = np.random.RandomState(3)
    k = 12
    branch = rng.randint(B, size=k).astype(np.uint32)
    e = int(branch[0])
    branch[1] = e                                              # two of the sample's points on the branch that moves
    distal = rng.uniform(0.1, 0.5, k) * blen[branch]
    weight = rng.dirichlet(np.ones(k)) * 0.8
    delta = 0.25 * blen[e]
    moved = distal + np.where(branch == e, delta, 0.0)
    both = dict(branch=np.concatenate([branch, branch]), seq=np.repeat([0, 1], k).astype(np.uint32),
                distal=np.concatenate([distal, moved]), weight=np.concatenate([weight, weight]))
    want = delta * float(np.sum(weight[branch == e]))
    c = dict(both, S=2, blen=blen, W=np.array([0.8, 0.8]))
    got = kr.restate(prox, dist, blen, both["branch"], both["seq"], both["distal"], both["weight"], 2)[0][0, 1]
    bt = kr.Brute(prox, dist, blen)
    smp = [bt.sample(s, both["branch"][both["seq"] == s], both["distal"][both["seq"] == s], both["weight"][both["seq"] == s])
           for s in (0, 1)]
    assert want > 1e6 * kr.tol(c, 0, 1)
    assert abs(got - want) <= kr.tol(c, 0, 1) and abs(bt.pair(*smp) - want) <= kr.tol(c, 0, 1)


def test_another_root_changes_only_pairs_of_unequal_totals():
    c = kr.case("random40")
    t = er.rooted(c["prox"], c["dist"], c["blen"])
    inner = [v for v in range(len(c["blen"]) + 1) if v != t["root"] and t["level"][v] >= 2 and
             sum(int(v in (int(p), int(d))) for p, d in zip(c["prox"], c["dist"])) == 3]
    moved, _, _ = kr.restate(c["prox"], c["dist"], c["blen"], c["branch"], c["seq"], c["distal"], c["weight"], c["S"],
                             root=inner[0])
    bt = kr.Brute(c["prox"], c["dist"], c["blen"], root=inner[0])
    smp = {s: bt.sample(s, c["branch"][c["seq"] == s], c["distal"][c["seq"] == s], c["weight"][c["seq"] == s])
           for s in range(c["S"])}
    equal = unequal = 0
    for a, b in c["pairs"]:
        if abs(c["W"][a] - c["W"][b]) < 1e-12:
            equal += 1
            assert abs(moved[a, b] - c["want"][a, b]) <= c["tol"][a, b]
            assert abs(bt.pair(smp[a], smp[b]) - c["brute"][a, b]) <= c["tol"][a, b]
        elif c["index"]["w07"] in (a, b) and c["W"][a] > 0 and c["W"][b] > 0:
            unequal += 1
            assert abs(moved[a, b] - c["want"][a, b]) > c["tol"][a, b]
            assert abs(bt.pair(smp[a], smp[b]) - moved[a, b]) <= c["tol"][a, b]
    assert equal > 20 and unequal >= 5


@pytest.mark.parametrize("name", er.TREES)
def test_masses_add_up(name):
    c = kr.case(name)
    p = kr.preorder(c["prox"], c["dist"], c["blen"])
    mt = kr.mass_tol(c)[:, 0]
    assert np.all(np.abs(c["want_clade"][:, p["at_root"]].sum(axis=1) - c["W"]) <= mt)
    assert np.all(np.abs(c["want_edge"].sum(axis=1) - c["W"]) <= mt)
    assert np.all(c["want_clade"] >= c["want_edge"] - mt[:, None])


# ---- the executable: refusals that need no device

def krd_cli(args):
    return subprocess.run([hostlib.cli_exe()] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_krd_is_refused_with_a_query_file_rescore_and_duplicate_names(tmp_path):
    # no file of these exists: the refusals come before any of them is opened
    base = ["-t", tmp_path / "no.tre", "-s", tmp_path / "no.fasta", "-w", tmp_path]
    for extra, text in ((["--krd", "a.jplace,b.jplace", "-q", tmp_path / "no_q.fasta"], "-q is not supported with it"),
                        (["--krd", "a.jplace,b.jplace", "--rescore", "c.jplace"], "--rescore is not supported with it"),
                        (["--krd", "a.jplace,b.jplace", "--dedup"], "--dedup is not supported with it"),
                        (["--krd", "a.jplace,b.jplace", "--devices", "0,1"], "--devices with several GPUs is not supported with it"),
                        (["--krd", "a.jplace,b.jplace", "--rank", "0"], "--rank / --world / --comm-file are not supported with it"),
                        (["--krd", "x/a.jplace,y/a.jplace"], "both give the sample name 'a'"),
                        (["--krd-masses"], "--krd-masses adds the mass tables to the output of --krd")):
        r = krd_cli(base + extra)
        assert r.returncode == 1 and text in r.stderr, (extra, r.stdout + r.stderr)
        assert "file_check failed" not in r.stderr and not (tmp_path / "krd.tsv").exists()


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("krd_cpu")
    w = synth.dna_workload(12, 120, 4, 60, (51, 52, 53))
    tre, msa = tmp / "ref.tre", tmp / "ref.fasta"
    tre.write_text(w["newick"] + "\n")
    ru.write_fasta(msa, w["labels"], w["seqs"])
    return tmp, ["-t", tre, "-s", msa, "-w", tmp]


def doc(placements, fields=ru.FIELDS):
    return json.dumps({"version": 3, "fields": fields, "placements": placements, "tree": "unused;", "metadata": {}})


GOOD = [{"n": ["r0"], "p": [[1, -10.0, 0.75, 0.0, 0.1], [2, -11.0, 0.25, 0.0, 0.1]]}]


@pytest.mark.parametrize("label,text,message", [
    ("no_lwr", doc([{"n": ["r0"], "p": [[1, -10.0, 0.0, 0.1]]}], [f for f in ru.FIELDS if f != "like_weight_ratio"]),
     "bad.jplace: required field \"like_weight_ratio\" is missing"),
    ("bad_multiplicity", doc([{"nm": [["r0", 2.0], ["r1", -1.0]], "p": [[1, -10.0, 1.0, 0.0, 0.1]]}]),
     "bad.jplace: placement object 0: \"nm\" entry 1: the multiplicity of 'r1' is negative or not finite"),
    ("edge_out_of_range", doc(GOOD + [{"n": ["r1"], "p": [[1, -10.0, 0.5, 0.0, 0.1], [21, -10.0, 0.5, 0.0, 0.1]]}]),
     "bad.jplace: placement object 1: row 1: edge_num 21 is not a branch of the reference tree (21 branches)"),
    ("zero_mass", doc([{"nm": [["r0", 0.0]], "p": [[1, -10.0, 1.0, 0.0, 0.1]]}, {"n": ["r1"], "p": [[2, -10.0, 0.0, 0.0, 0.1]]}]),
     "sample 'bad' has a total mass of 0"),
    ("negative_lwr", doc([{"n": ["r0"], "p": [[1, -10.0, -0.5, 0.0, 0.1]]}]),
     "bad.jplace: placement object 0: row 0: like_weight_ratio"),
    ("distal_beyond", doc([{"n": ["r0"], "p": [[1, -10.0, 1.0, 50.0, 0.1]]}]),
     "bad.jplace: placement object 0: row 0: distal_length 50.000000 lies beyond the length of edge 1"),
])
def test_krd_refuses_bad_files_before_a_device_is_opened(reference, label, text, message):
    tmp, base = reference
    good, bad = tmp / "good.jplace", tmp / "bad.jplace"
    good.write_text(doc(GOOD))
    bad.write_text(text)
    r = krd_cli(base + ["--krd", "%s,%s" % (good, bad)])
    assert r.returncode == 1 and message in r.stderr, (label, r.stdout + r.stderr)
    assert not (tmp / "krd.tsv").exists()
