"""epa-ng-amd --rescore FILE.jplace end to end through the executable.

  7. round trip: a normal run writes jplace A, --rescore A writes B: the same pqueries in the same order, the same
     edges, the same distal / pendant text, likelihood and like_weight_ratio within 1e-6 -- nucleotides (golden
     fixture, default model) and LG+G4 on the amino-acid fixture.  The lengths travel through 10 printed digits;
     largest |likelihood B - likelihood A| measured on MI355X: 4.7e-09 (nucleotides), 0 (LG+G4).
  8. a jplace written by hand for D5 and A4 of tests/brute_cases.py (written out as FASTA): fields in another order
     with an extra column, one pquery named through "nm", three rows per query on edges 0, 5 and B - 1 at lengths of
     the grid of tests/test_gpu_score_at.py, a query file that holds more sequences than the jplace names,
     --precision 12: every likelihood within 1e-6 of Oracle.score_at, LWRs the softmax over the pquery's own rows
     (1e-9), rows LWR-descending, the skipped sequences counted on stdout.
"""
import json
import os
import re

import numpy as np
import pytest

import brute_cases as bc
import rescore_util as ru
from epa_ng_amd import hostlib
from gen_golden import DEFAULT_BL
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

LNL_TOL = 1e-6


def raw_rows(path):
    """the text of every placement row of a jplace the product wrote, per pquery: [[edge, lnl, lwr, distal, pendant]]"""
    text = open(path).read()
    out = []
    for block in re.findall(r'\{"p": \[\n(.*?)\n\s*\],\n\s*"n"', text, re.S):
        out.append([[t.strip() for t in row.strip().strip("[],").split(",")] for row in block.split("\n")])
    return out


@pytest.mark.parametrize("open_filter", [False, True], ids=["default-filter", "open-filter"])
@pytest.mark.parametrize("kind", ["dna", "aa"])
def test_round_trip(kind, open_filter, tmp_path):
    """open-filter: run A keeps every candidate (--filter-min-lwr 0), so its LWRs are normalised over exactly the rows
    it prints and B's must equal them as they stand.  default-filter: A prints the rows above 0.01 of a list that was
    normalised before the filter; B, normalised over the rows it is given, must equal A's ratios renormalised."""
    if kind == "dna":
        files, model = ("ref.tre", "aln.fasta", "query.fasta"), None
    else:
        files, model = ("aa_ref.tre", "AA_aln.fasta", "AA_query.fasta"), "LG+G4"
    tree, msa, query = (os.path.join(ru.DATA, f) for f in files)
    a_dir, b_dir = tmp_path / "a", tmp_path / "b"
    a_dir.mkdir()
    b_dir.mkdir()
    r = ru.run_cli(tree, msa, query, a_dir, ["--filter-min-lwr", "0", "--filter-max", "64"] if open_filter else [], model=model)
    assert r.returncode == 0, r.stdout + r.stderr
    r = ru.run_cli(tree, msa, query, b_dir, ["--rescore", a_dir / "epa_result.jplace", "--stats-json", b_dir / "stats.json"],
                   model=model)
    assert r.returncode == 0, r.stdout + r.stderr
    assert json.load(open(b_dir / "stats.json"))["chunk_path"] == "rescore"
    A, B = ru.result(a_dir), ru.result(b_dir)
    assert A["fields"] == B["fields"] == ru.FIELDS and A["tree"] == B["tree"]
    assert [pq["n"] for pq in A["placements"]] == [pq["n"] for pq in B["placements"]] and len(A["placements"]) == 2
    ta, tb = raw_rows(a_dir / "epa_result.jplace"), raw_rows(b_dir / "epa_result.jplace")
    assert len(ta) == len(tb) == len(A["placements"])
    worst = 0.0
    for pa, pb, ra, rb in zip(A["placements"], B["placements"], ta, tb):
        assert len(pa["p"]) == len(pb["p"]) == len(ra) == len(rb) >= 1
        lwr_a = np.array([row[2] for row in pa["p"]])
        if not open_filter:
            lwr_a = lwr_a / lwr_a.sum()
        for i, (x, y) in enumerate(zip(pa["p"], pb["p"])):
            assert x[0] == y[0]                                           # same edge, same order
            assert ra[i][0] == rb[i][0] and ra[i][3:] == rb[i][3:]        # distal / pendant: the same text
            worst = max(worst, abs(x[1] - y[1]))
            assert abs(x[1] - y[1]) < LNL_TOL
            assert abs(lwr_a[i] - y[2]) < 1e-6
        assert abs(sum(y[2] for y in pb["p"]) - 1.0) < 1e-8
    print("\n%s round trip (open filter: %s): max |likelihood B - likelihood A| %.3g" % (kind, open_filter, worst))


def model_string(c):
    name = "GTR" if c["states"] == 4 else "PROTGTR"
    j = lambda v: "/".join(repr(float(x)) for x in v)   # noqa: E731
    return "%s{%s}+FU{%s}+R%d{%s}{%s}" % (name, j(c["subst"]), j(c["freqs"]), len(c["rates"]), j(c["rates"]), j(c["weights"]))


@pytest.mark.parametrize("name", ["D5", "A4"])
def test_hand_made_jplace(name, tmp_path):
    c = bc.case(name)
    assert c["pinv"] == 0.0
    reads = c["reads"]
    W = len(reads[0])
    tre, msa, qf = tmp_path / "ref.tre", tmp_path / "ref.fasta", tmp_path / "q.fasta"
    tre.write_text(c["newick"] + "\n")
    ru.write_fasta(msa, c["labels"], c["seqs"])
    # two sequences the jplace does not name; the first has a character in every column, so no column is masked for the queries' sake
    # (no 'N' among the amino acids: the column mask reads it as undetermined)
    alphabet = "ACGT" if c["states"] == 4 else "ARDCQEGHILKMFPSTWYV"
    full = "".join(alphabet[i % len(alphabet)] for i in range(W))
    names = ["extra_full"] + ["r%d" % i for i in range(len(reads))] + ["extra_last"]
    ru.write_fasta(qf, names, [full] + list(reads) + [reads[0]])
    # the executable still drops the columns that are undetermined in the whole REFERENCE (for amino acids the mask
    # reads N as undetermined, so a conserved asparagine column goes): the oracle gets the same columns
    keep = hostlib.premask(str(msa), str(qf)) == 0
    cut = lambda sq: "".join(np.array(list(sq))[keep])   # noqa: E731
    reads = [cut(r) for r in reads]
    o = Oracle(c["newick"], c["labels"], [cut(sq) for sq in c["seqs"]], c["states"], c["subst"], c["freqs"], c["rates"],
               weights=c["weights"])
    B = o.B
    # three rows per query: edges 0, 5, B - 1 at (pendant, distal fraction) of the grid, rotated from read to read
    lengths = [(1e-4, 0.0), (DEFAULT_BL, 0.3), (2.5, 1.0), (12.0, 0.3), (2.5, 0.0), (1e-4, 1.0)]
    fields = ["likelihood", "post_prob", "pendant_length", "edge_num", "like_weight_ratio", "distal_length"]
    placements, want = [], {}
    for q in range(len(reads)):
        rows = []
        for k, edge in enumerate((0, 5, B - 1)):
            pendant, frac = lengths[(q + k) % len(lengths)]
            distal = frac * o.branch_info(edge)[0]
            rows.append([-1.0, 0.5, pendant, edge, 0.3, distal])
            want[(q, edge)] = (pendant, distal)
        placements.append({"p": rows, "nm": [["r%d" % q, 2.0]]} if q == 1 else {"p": rows, "n": ["r%d" % q]})
    placements = placements[::-1]            # input order is not file order
    jp = tmp_path / "in.jplace"
    jp.write_text(json.dumps(ru.jplace_doc(placements, fields=fields), indent=1))
    out = tmp_path / "out"
    out.mkdir()
    r = ru.run_cli(tre, msa, qf, out, ["--rescore", jp, "--precision", "12"], model=model_string(c))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "2 sequences of the query file are not named" in r.stdout, r.stdout
    res = ru.result(out)
    assert res["fields"] == ru.FIELDS
    assert [pq["n"] for pq in res["placements"]] == [[pl["n"][0] if "n" in pl else pl["nm"][0][0]] for pl in placements]
    worst = 0.0
    for pq in res["placements"]:
        q = int(pq["n"][0][1:])
        rows = pq["p"]
        assert sorted(row[0] for row in rows) == [0, 5, B - 1]
        lnl = np.array([row[1] for row in rows])
        pen = np.array([want[(q, row[0])][0] for row in rows])
        dis = np.array([want[(q, row[0])][1] for row in rows])
        assert np.allclose([row[4] for row in rows], pen, rtol=0, atol=1e-12)
        assert np.allclose([row[3] for row in rows], dis, rtol=0, atol=1e-12)
        ref = o.score_at([row[0] for row in rows], [q] * 3, reads, pen, dis)
        worst = max(worst, float(np.max(np.abs(lnl - ref))))
        assert np.max(np.abs(lnl - ref)) < LNL_TOL
        e = np.exp(lnl - lnl.max())
        assert np.max(np.abs(np.array([row[2] for row in rows]) - e / e.sum())) < 1e-9
        assert all(rows[i][2] >= rows[i + 1][2] for i in range(2))
    print("\n%s hand-made jplace: max |likelihood - oracle| %.3g" % (name, worst))
