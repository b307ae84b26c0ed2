"""epa-ng-amd --krd A.jplace,B.jplace,C.jplace end to end through the executable.

40 reads of 120 sites are placed on a 24-tip tree; three samples are cut from the result: one whose objects carry "nm"
multiplicities, one whose objects list several names in "n" (as --dedup writes them), one plain.  --precision 15.

  1. krd.tsv: the header names the samples in file order, the matrix is symmetric with a zero diagonal, and every value
     agrees with restate() of tests/krd_ref.py on the same normalised masses -- the topology parsed from the placed
     file's numbered Newick -- within tol + (B + 1) 5e-16: the bound of tests/krd_ref.py plus the printed precision (the B
     branch lengths of the Newick and the value itself travel through 15 digits; |F_a - F_b| <= 1).
  2. --krd-masses: the columns are the edge numbers, every row of edge_masses.tsv adds up to 1, and so does
     clade_masses.tsv over the branches at the root; both agree with restate().
  3. a single file gives a 1 x 1 matrix.
"""
import json

import numpy as np
import pytest

import krd_ref as kr
import rescore_util as ru
from epa_ng_amd import synth
from test_gpu_edpl_cli import parse_numbered_newick
from test_krd_cpu import krd_cli

pytestmark = pytest.mark.gpu


def table(path):
    lines = open(path).read().splitlines()
    head = lines[0].split("\t")
    assert head[0] == "sample"
    rows = [ln.split("\t") for ln in lines[1:]]
    return head[1:], [r[0] for r in rows], np.array([[float(v) for v in r[1:]] for r in rows])


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("krd_cli")
    w = synth.dna_workload(24, 300, 40, 120, (41, 42, 43))
    tre, msa, qf = tmp / "ref.tre", tmp / "ref.fasta", tmp / "q.fasta"
    tre.write_text(w["newick"] + "\n")
    ru.write_fasta(msa, w["labels"], w["seqs"])
    ru.write_fasta(qf, ["r%d" % i for i in range(len(w["reads"]))], w["reads"])
    out = tmp / "placed"
    out.mkdir()
    r = ru.run_cli(tre, msa, qf, out, ["--filter-min-lwr", "0.001", "--precision", 15])
    assert r.returncode == 0, r.stdout + r.stderr
    placed = json.load(open(out / "epa_result.jplace"))
    pls = placed["placements"]
    assert len(pls) == 40 and placed["fields"] == ru.FIELDS
    samples = {
        "with_nm": [{"nm": [[pq["n"][0], float(1 + k % 3)], [pq["n"][0] + "_twin", 0.5]], "p": pq["p"]} for k, pq in enumerate(pls[:15])],
        "multi_n": [{"n": [pq["n"][0]] + ["%s_copy%d" % (pq["n"][0], j) for j in range(k % 4)], "p": pq["p"]}
                    for k, pq in enumerate(pls[10:30])],
        "plain": [{"n": pq["n"], "p": pq["p"]} for pq in pls[25:]],
    }
    files = []
    for name, objs in samples.items():
        path = tmp / "in" / (name + ".jplace")
        path.parent.mkdir(exist_ok=True)
        path.write_text(json.dumps(dict(placed, placements=objs), indent=1))
        files.append(path)
    # the same masses, as the executable must form them: multiplicity x like_weight_ratio over the total in file order
    branch, seq, distal, weight = [], [], [], []
    for s, objs in enumerate(samples.values()):
        rows = []
        for o in objs:
            mult = float(len(o["n"])) if "n" in o else 0.0
            for _, m in o.get("nm", []):
                mult = mult + m
            rows += [(r[0], r[3], mult * r[2]) for r in o["p"]]
        total = 0.0
        for _, _, m in rows:
            total = total + m
        branch += [r[0] for r in rows]
        distal += [r[1] for r in rows]
        weight += [r[2] / total for r in rows]
        seq += [s] * len(rows)
    prox, dist, blen = parse_numbered_newick(placed["tree"])
    distal = np.minimum(np.array(distal), blen[branch])          # the reader's clamp within its slack
    ent = dict(branch=np.array(branch, np.uint32), seq=np.array(seq, np.uint32), distal=distal, weight=np.array(weight), S=3,
               blen=blen, W=np.ones(3))
    base = ["-t", tre, "-s", msa, "--precision", 15]
    return dict(tmp=tmp, base=base, files=files, names=list(samples), prox=prox, dist=dist, blen=blen, ent=ent)


def test_matrix_against_the_restatement(setup):
    out = setup["tmp"] / "krd"
    out.mkdir()
    r = krd_cli(setup["base"] + ["-w", out, "--krd", ",".join(str(f) for f in setup["files"])])
    assert r.returncode == 0, r.stdout + r.stderr
    assert not (out / "edge_masses.tsv").exists() and not (out / "epa_result.jplace").exists()
    head, names, m = table(out / "krd.tsv")
    assert head == setup["names"] and names == setup["names"] and m.shape == (3, 3)
    assert np.array_equal(m, m.T) and np.all(np.diag(m) == 0.0)
    e = setup["ent"]
    want, _, _ = kr.restate(setup["prox"], setup["dist"], e["blen"], e["branch"], e["seq"], e["distal"], e["weight"], 3)
    for a in range(3):
        for b in range(a + 1, 3):
            assert abs(m[a, b] - want[a, b]) <= kr.tol(e, a, b) + (len(e["blen"]) + 1) * 5e-16, (a, b, m[a, b], want[a, b])
            assert m[a, b] > 1e-3
    for line in open(out / "krd.tsv").read().splitlines()[1:]:
        assert all(len(v.split(".")[1]) == 15 for v in line.split("\t")[1:])


def test_masses(setup):
    out = setup["tmp"] / "masses"
    out.mkdir()
    r = krd_cli(setup["base"] + ["-w", out, "--krd", ",".join(str(f) for f in setup["files"]), "--krd-masses"])
    assert r.returncode == 0, r.stdout + r.stderr
    e, B = setup["ent"], len(setup["blen"])
    cols, names, edge = table(out / "edge_masses.tsv")
    cols2, names2, clade = table(out / "clade_masses.tsv")
    assert cols == cols2 == [str(b) for b in range(B)] and names == names2 == setup["names"]
    mt = kr.mass_tol(e) + 5e-16                                   # the printed precision
    assert np.all(np.abs(edge.sum(axis=1) - 1.0) <= B * mt[:, 0])
    # the executable's root is one end of edge 0: exactly one of the two reproduces the clade masses
    hits = 0
    for root in (int(setup["prox"][0]), int(setup["dist"][0])):
        _, want_edge, want_clade = kr.restate(setup["prox"], setup["dist"], e["blen"], e["branch"], e["seq"], e["distal"],
                                              e["weight"], 3, pairs=[], root=root)
        assert np.all(np.abs(edge - want_edge) <= mt)
        if np.all(np.abs(clade - want_clade) <= mt):
            hits += 1
            at_root = kr.preorder(setup["prox"], setup["dist"], e["blen"], root)["at_root"]
            assert len(at_root) >= 2 and np.all(np.abs(clade[:, at_root].sum(axis=1) - 1.0) <= len(at_root) * mt[:, 0])
    assert hits == 1


def test_a_single_file_gives_a_one_by_one_matrix(setup):
    out = setup["tmp"] / "single"
    out.mkdir()
    r = krd_cli(setup["base"] + ["-w", out, "--krd", setup["files"][2]])
    assert r.returncode == 0, r.stdout + r.stderr
    head, names, m = table(out / "krd.tsv")
    assert head == names == ["plain"] and m.shape == (1, 1) and m[0, 0] == 0.0
