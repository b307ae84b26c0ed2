"""EDPL without a device: the two references of tests/edpl_ref.py against each other, what the bit-for-bit comparison of
tests/test_gpu_edpl.py can tell, the executable's refusal of --edpl without --rescore, and Tree::fill_topology.

  1. restate() (the header's specification, rooted at node_prox[0]) and brute() (path sums on the unrooted tree) agree
     within tol = 16 (h + k + 2) 2^-53 Dmax on every tree and object of the GPU tests: 3 tips, 4 tips (both with a
     1025-row object), a ladder of 600 tips, synth.random_tree(40, 71) and synth.random_tree(512, 1) with a tenth of its
     branches at length 0.
  2. restate() rooted at another inner node gives other BITS in at least one row_dist of the 40-tip case while staying
     within tol: a device that rooted elsewhere, or summed in another order, would be caught.
  3. epa-ng-amd --edpl without --rescore exits 1 with the two-step message before any file is read.
  4. Tree::fill_topology on a 9-tip tree: 2 n - 3 branches, every inner node of degree 3, every tip of degree 1 and at a
     distal end, tips numbered first.
"""
import subprocess

import numpy as np
import pytest

import edpl_ref as er
from epa_ng_amd import hostlib, synth


@pytest.mark.parametrize("name", er.TREES)
def test_restate_agrees_with_brute(name):
    c = er.case(name)
    assert set(c["rows_of"]) >= {0, 1, 2, 7, 64, 65} and (len(c["blen"]) > 5 or 1025 in c["rows_of"])
    rows = np.abs(c["want_rows"] - c["brute_rows"])
    per_q = np.abs(c["want_edpl"] - c["brute_edpl"])
    print(name, "max |restate - brute| / tol: row_dist %.3g, edpl %.3g" % (np.max(rows / c["tol_rows"]),
                                                                           np.max(per_q / c["tol_q"])))
    assert np.all(rows <= c["tol_rows"]) and np.all(per_q <= c["tol_q"])
    # the conventions: no entry and one entry give exactly 0, every distance is >= 0, something is far from 0
    assert c["want_edpl"][c["empty"]] == 0.0 and c["brute_edpl"][c["empty"]] == 0.0
    for q, k in enumerate(c["rows_of"]):
        if k == 1:
            assert c["want_edpl"][q] == 0.0 and np.all(c["want_rows"][c["seq"] == q] == 0.0)
    assert np.all(c["want_rows"] >= 0.0) and c["want_edpl"].max() > 100 * c["tol_q"].max()


def test_same_edge_rows_in_both_orders():
    c = er.case("random40")
    a, b = c["want_rows"][c["seq"] == 0], c["want_rows"][c["seq"] == 1]
    assert np.array_equal(a, b[::-1]) and c["want_edpl"][0] > 0.0
    # two points on one edge: |D_i - D_j| = half the edge here, weighted
    e = int(c["branch"][0])
    assert abs(a[0] - c["weight"][1] * 0.5 * c["blen"][e]) <= c["tol_rows"][0]


def test_another_root_changes_bits_not_values():
    c = er.case("random40")
    t = er.rooted(c["prox"], c["dist"], c["blen"])
    inner = [v for v in range(len(c["blen"]) + 1) if v != t["root"] and t["level"][v] >= 2 and
             sum(int(v in (int(p), int(d))) for p, d in zip(c["prox"], c["dist"])) == 3]
    rows, per_q = er.restate(c["prox"], c["dist"], c["blen"], c["branch"], c["seq"], c["distal"], c["weight"], c["Q"],
                             root=inner[0])
    assert np.all(np.abs(rows - c["want_rows"]) <= c["tol_rows"]) and np.all(np.abs(per_q - c["want_edpl"]) <= c["tol_q"])
    assert np.any(rows != c["want_rows"])


def test_edpl_without_rescore_is_refused(tmp_path):
    # no file of these exists: the refusal comes before any of them is opened
    r = subprocess.run([hostlib.cli_exe(), "-t", str(tmp_path / "no.tre"), "-s", str(tmp_path / "no.fasta"), "-q",
                        str(tmp_path / "no_q.fasta"), "-w", str(tmp_path), "--edpl"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "--edpl works on an existing result: place first, then run again with --rescore out.jplace --edpl" in r.stderr
    assert not (tmp_path / "epa_result.jplace").exists()


def test_fill_topology_of_a_nine_tip_tree():
    n = 9
    root = synth.random_tree(n, 5)
    labels = ["t%d" % i for i in range(n)]
    ref = hostlib.Reference(synth.newick(root), labels, ["ACGT"] * n, model="GTR+G")
    prox, dist, n_nodes = ref.topology()
    B = 2 * n - 3
    assert ref.B == B and len(prox) == len(dist) == B and n_nodes == B + 1 == 2 * n - 2
    degree = np.bincount(np.concatenate([prox, dist]), minlength=n_nodes)
    assert np.all(degree[:n] == 1) and np.all(degree[n:] == 3)
    assert np.all(prox >= n)                      # a tip is never the proximal end
    assert sorted(int(v) for v in dist if v < n) == list(range(n))
    assert np.all(prox != dist)
    # the branches that end in a tip carry the newick's tip lengths
    assert sorted(ref.branch(b)["length"] for b in range(B) if dist[b] < n) == sorted(k.length for k in _tips(root))
    # and the graph is one tree: both references accept it
    er.rooted(prox, dist, np.ones(B))


def _tips(node):
    out, todo = [], [node]
    while todo:
        nd = todo.pop()
        todo.extend(nd.kids)
        if not nd.kids:
            out.append(nd)
    return out
