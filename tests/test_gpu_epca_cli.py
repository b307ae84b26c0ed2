"""epa-ng-amd --krd A.jplace,..,E.jplace --epca 3 end to end through the executable.

Five sample files follow test_gpu_squash_cli.py's recipe on a 40-tip reference: 40 reads are placed, and overlapping slices
of the placements become the samples (one with "nm" multiplicities, one with several names per object, three plain).
--precision 15.

  1. krd.tsv is byte for byte the file written without --epca, and no epca file appears without the flag.
  2. epca_eigenvalues.tsv, epca_projection.tsv and epca_edges.tsv equal hostlib.epca_texts of an Evaluator.epca call on the
     same masses: the context comes from the same host tree (hostlib.Reference of the same Newick and alignment), the masses
     are formed as the executable forms them (multiplicity x like_weight_ratio over the total in file order, distal
     lengths clamped to the branch).
  3. the refusals, by their texts, with exit status 1 and no file written.
  4. --epca with --squash --krd-masses writes all eight files, each the bytes of the run that asks for it alone.
"""
import json

import numpy as np
import pytest

import rescore_util as ru
from epa_ng_amd import hostlib, synth
from test_gpu_score_at import make_pairs
from test_krd_cpu import krd_cli

pytestmark = pytest.mark.gpu

EPCA_FILES = ("epca_eigenvalues.tsv", "epca_projection.tsv", "epca_edges.tsv")


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("epca_cli")
    w = synth.dna_workload(40, 300, 40, 120, (51, 52, 53))
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
        "with_nm": [{"nm": [[pq["n"][0], float(1 + k % 3)], [pq["n"][0] + "_twin", 0.5]], "p": pq["p"]} for k, pq in enumerate(pls[:12])],
        "multi_n": [{"n": [pq["n"][0]] + ["%s_copy%d" % (pq["n"][0], j) for j in range(k % 4)], "p": pq["p"]}
                    for k, pq in enumerate(pls[8:20])],
        "plain_a": [{"n": pq["n"], "p": pq["p"]} for pq in pls[16:28]],
        "plain_b": [{"n": pq["n"], "p": pq["p"]} for pq in pls[24:36]],
        "plain_c": [{"n": pq["n"], "p": pq["p"]} for pq in pls[30:]],
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
    pca = ev.epca(make_pairs(np.array(branch, np.uint32), np.array(seq, np.uint32)), distal, np.array(weight), 5, 3)
    base = ["-t", tre, "-s", msa, "--precision", 15]
    runs = {}
    for label, extra in (("krd", []), ("epca", ["--epca", "3"]), ("squash", ["--squash"]), ("masses", ["--krd-masses"]),
                         ("all", ["--squash", "--epca", "3", "--krd-masses"])):
        d = tmp / label
        d.mkdir()
        r = krd_cli(base + ["-w", d, "--krd", ",".join(str(f) for f in files)] + extra)
        assert r.returncode == 0, (label, r.stdout + r.stderr)
        runs[label] = d
    return dict(names=list(samples), pca=pca, runs=runs, base=base, files=files, tmp=tmp, B=ref.B)


def test_krd_tsv_is_the_same_file(setup):
    plain = (setup["runs"]["krd"] / "krd.tsv").read_bytes()
    assert len(plain.splitlines()) == 6
    assert (setup["runs"]["epca"] / "krd.tsv").read_bytes() == plain
    assert not any((setup["runs"]["krd"] / f).exists() for f in EPCA_FILES)
    assert sorted(p.name for p in setup["runs"]["epca"].iterdir()) == sorted(EPCA_FILES + ("krd.tsv",))


def test_the_three_texts_against_the_writer(setup):
    d = setup["runs"]["epca"]
    ev, vec, proj, total, sweeps = setup["pca"]
    assert ev[0] > ev[1] > ev[2] > 0.0 and total[0] >= ev.sum() * (1 - 1e-12) and 1 <= sweeps[0] < 30
    want = hostlib.epca_texts(setup["names"], ev, total, vec, proj, precision=15)
    for f, text in zip(EPCA_FILES, want):
        assert (d / f).read_text() == text, f
    lines = (d / "epca_edges.tsv").read_text().splitlines()
    assert lines[0] == "edge_num\tpc1\tpc2\tpc3" and [ln.split("\t")[0] for ln in lines[1:]] == [str(b) for b in range(setup["B"])]
    assert (d / "epca_projection.tsv").read_text().splitlines()[1].startswith("with_nm\t")
    frac = [float(ln.split("\t")[2]) for ln in (d / "epca_eigenvalues.tsv").read_text().splitlines()[1:]]
    assert 0.0 < sum(frac) <= 1.0 + 1e-12 and len(frac) == 3


def test_refusals_write_nothing(setup):
    files = ",".join(str(f) for f in setup["files"])
    d = setup["tmp"] / "refused"
    d.mkdir()
    many = ",".join("f%d.jplace" % i for i in range(1025))
    for extra, text in ((["--epca", "2"], "--epca finds the principal components of the samples of --krd and needs it"),
                        (["--krd", str(setup["files"][0]), "--epca", "1"], "--epca: principal components take 2 .. 1024 samples (1 given)"),
                        (["--krd", many, "--epca", "1"], "--epca: principal components take 2 .. 1024 samples (1025 given)"),
                        (["--krd", files, "--epca", "0"], "--epca 0: 5 samples have 1 .. 4 components"),
                        (["--krd", files, "--epca", "5", "--squash", "--krd-masses"], "--epca 5: 5 samples have 1 .. 4 components")):
        r = krd_cli(setup["base"] + ["-w", d] + extra)
        assert r.returncode == 1 and text in r.stderr, (extra[-3:], r.stdout + r.stderr[-400:])
        assert list(d.iterdir()) == []


def test_with_squash_and_the_mass_tables(setup):
    runs = setup["runs"]
    assert len(list(runs["all"].iterdir())) == 8
    for f in EPCA_FILES + ("krd.tsv",):
        assert (runs["all"] / f).read_bytes() == (runs["epca"] / f).read_bytes(), f
    for f in ("squash.tsv", "squash.newick"):
        assert (runs["all"] / f).read_bytes() == (runs["squash"] / f).read_bytes(), f
    for f in ("edge_masses.tsv", "clade_masses.tsv"):
        assert (runs["all"] / f).read_bytes() == (runs["masses"] / f).read_bytes(), f
