"""epa-ng-amd --krd A.jplace,B.jplace,C.jplace --squash end to end through the executable.

The three sample files are those of test_gpu_krd_cli.py's recipe (40 reads placed on a 24-tip tree; one sample with "nm"
multiplicities, one with several names per object, one plain), built in a fixture of this file's own.  --precision 15.

  1. krd.tsv is byte for byte the file written without --squash.
  2. squash.tsv and squash.newick equal squash_ref.table / newick fed with Evaluator.squash's arrays on the same masses:
     the context comes from the same host tree (hostlib.Reference of the same Newick and alignment), the masses are formed
     as the executable forms them (multiplicity x like_weight_ratio over the total in file order, distal lengths clamped
     to the branch).
  3. every branch length of squash.newick, recomputed from the distances of squash.tsv (height = distance / 2, branch =
     height(parent) - height(child)), agrees within the printed precision: 1e-15 for the three printed numbers involved
     (0.5e-15 for the length, 0.25e-15 for each halved distance) plus 4 x 2^-53 x the largest distance for the arithmetic.
  4. once more with --krd-masses: the same three files, and the mass tables of the run without --squash.
"""
import json
import re

import numpy as np
import pytest

import rescore_util as ru
import squash_ref as sr
from epa_ng_amd import hostlib, synth
from test_gpu_score_at import make_pairs
from test_krd_cpu import krd_cli

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("squash_cli")
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
    # the same masses, as the executable forms them: multiplicity x like_weight_ratio over the total in file order
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
    # the executable's own tree: the same Newick and alignment through the same host code
    ref = hostlib.Reference(w["newick"], w["labels"], w["seqs"], model="GTR+G")
    blen = np.array([ref.branch(b)["length"] for b in range(ref.B)])
    prox, dist, _ = ref.topology()
    ev = ref.evaluator()
    ev.set_topology(prox, dist)
    distal = np.minimum(np.array(distal), blen[branch])             # the reader's clamp within its slack
    merges = ev.squash(make_pairs(np.array(branch, np.uint32), np.array(seq, np.uint32)), distal, np.array(weight), 3)
    base = ["-t", tre, "-s", msa, "--precision", 15]
    runs = {}
    for label, extra in (("krd", []), ("squash", ["--squash"]), ("masses", ["--krd-masses"]), ("both", ["--squash", "--krd-masses"])):
        d = tmp / label
        d.mkdir()
        r = krd_cli(base + ["-w", d, "--krd", ",".join(str(f) for f in files)] + extra)
        assert r.returncode == 0, (label, r.stdout + r.stderr)
        runs[label] = d
    return dict(names=list(samples), merges=merges, runs=runs)


def test_krd_tsv_is_the_same_file(setup):
    plain = (setup["runs"]["krd"] / "krd.tsv").read_bytes()
    assert len(plain.splitlines()) == 4
    assert (setup["runs"]["squash"] / "krd.tsv").read_bytes() == plain
    assert not (setup["runs"]["krd"] / "squash.tsv").exists() and not (setup["runs"]["krd"] / "squash.newick").exists()
    assert not (setup["runs"]["squash"] / "edge_masses.tsv").exists()


def test_the_two_texts_against_the_restatement(setup):
    d = setup["runs"]["squash"]
    ma, mb, md, ms = setup["merges"]
    assert md[0] > 1e-3 and md[1] > 1e-3 and list(ms) == [2, 3]
    assert (d / "squash.tsv").read_text() == sr.table(setup["names"], setup["merges"], 15)
    assert (d / "squash.newick").read_text() == sr.newick(setup["names"], setup["merges"], 15)


def parse_newick(text):
    """-> {label: (parent label or None, branch length or None)} of a tree whose every node is labelled"""
    assert text.endswith(";\n")
    tokens = re.findall(r"[(),]|[^(),:;]+|:[^(),;]+", text[:-2])
    nodes, stack, last = {}, [[]], None
    for tok in tokens:
        if tok == "(":
            stack.append([])
        elif tok == ",":
            pass
        elif tok == ")":
            last = stack.pop()
        elif tok.startswith(":"):
            name = stack[-1][-1]
            nodes[name] = (None, float(tok[1:]), tok[1:])
        else:
            for kid in last or []:
                nodes[kid] = (tok,) + nodes[kid][1:]
            last = None
            stack[-1].append(tok)
            nodes.setdefault(tok, (None, None, None))
    return nodes


def test_branch_lengths_follow_from_the_table(setup):
    d = setup["runs"]["squash"]
    lines = (d / "squash.tsv").read_text().splitlines()
    assert lines[0] == "step\ta\tb\tdistance\tsize" and len(lines) == 3
    height = {n: 0.0 for n in setup["names"]}
    kids = {}
    for ln in lines[1:]:
        step, a, b, dist, size = ln.split("\t")
        assert len(dist.split(".")[1]) == 15
        height["cluster" + step] = float(dist) / 2
        kids["cluster" + step] = [a, b]
    nodes = parse_newick((d / "squash.newick").read_text())
    assert set(nodes) == set(height) and nodes["cluster1"][:2] == (None, None)
    bound = 1e-15 + 4 * 2.0 ** -53 * 2 * max(height.values())
    for name, (parent, length, text) in nodes.items():
        if parent is None:
            continue
        assert name in kids[parent] and len(text.split(".")[1]) == 15
        assert abs(length - (height[parent] - height[name])) <= bound, (name, parent, length, height[parent], height[name])
    assert [k for k in nodes if nodes[k][0] == "cluster1"] == kids["cluster1"]          # the smaller id first


def test_with_the_mass_tables(setup):
    both, squash, masses = (setup["runs"][k] for k in ("both", "squash", "masses"))
    for f in ("krd.tsv", "squash.tsv", "squash.newick"):
        assert (both / f).read_bytes() == (squash / f).read_bytes(), f
    for f in ("edge_masses.tsv", "clade_masses.tsv"):
        assert (both / f).read_bytes() == (masses / f).read_bytes(), f
