"""Edge PCA without a device: the cases of tests/epca_ref.py are decided, the two restatements agree, and the writer of
epa-ng-amd --epca.

  1. decided cases.  For every case whose components are compared and every compared (non-null) k < K: the gap from
     lambda'_k to its nearest neighbour is >= 10^6 tol_eig; lambda'_k is >= 10^6 times the null threshold; every entry of
     edge_vec[k] whose |value| is within twice the vector's Davis-Kahan bound of the largest has the sign of the largest
     (edges of the ladder with no mass between them carry bit-equal columns, hence equal entries: whichever of them the
     tie rule names on the device, sigma_k is the same).  A null component stays null under the device's error: lambda'_k + tol_eig is below the
     threshold (or G is exactly zero).
  2. epca_ref.jacobi against numpy.linalg.eigh: eigenvalues within tol_jac, vectors within the Davis-Kahan bound, fewer
     than 30 sweeps everywhere.
  3. the exact case really is exact: G by math.fsum equals Xc @ Xc.T bit for bit.
  4. the Gram route and the textbook route agree: on random40 / 17 samples the eigenvalues of restate() against the
     non-zero spectrum of the E x E covariance matrix by eigh, within tol_eig / (S - 1).
  5. hostlib.epca_texts against string restatements of the three files, with a null component, total_var == 0 and
     precision 0 among them; the refusals of the command line, which come before any file is read.
"""
import math

import numpy as np
import pytest

import epca_ref as pr
from epa_ng_amd import hostlib
from test_krd_cpu import krd_cli


@pytest.mark.parametrize("name", pr.COMPONENT_CASES)
def test_every_case_is_decided(name):
    c = pr.case(name)
    S, K, B, lam = c["S"], c["K"], len(c["blen"]), c["lam"]
    _, _, sweeps = pr.sorted_jacobi(c["G"])
    te = pr.tol_eig(c["G"], sweeps, B)
    gap = pr.gaps(lam)
    compared = 0
    for k in range(K):
        if c["null"][k]:
            assert lam[0] == 0.0 or abs(lam[k]) + te < pr.NULL_REL * lam[0], (name, k, lam[k], te, lam[0])
            assert not c["edge_vec"][k].any() and not c["proj"][:, k].any()
            continue
        compared += 1
        assert gap[k] >= 1e6 * te, (name, k, gap[k], te)
        assert lam[k] >= 1e6 * pr.NULL_REL * lam[0], (name, k, lam[k], lam[0])
        v = c["edge_vec"][k]
        near = v[np.abs(v) >= np.abs(v).max() - 2 * pr.davis_kahan(te, gap[k])]
        assert np.all(near > 0.0), (name, k, near)
        assert abs(np.linalg.norm(c["edge_vec"][k]) - 1.0) <= 8 * te / lam[k] + 8 * pr.U
        assert not c["edge_vec"][k][c["excluded"]].any()
    print(name, "S", S, "sweeps", sweeps, "compared", compared, "smallest gap / tol_eig %.3g" % (gap[:K].min() / te if te else np.inf))
    assert compared == {"tips3": 0, "tips4": 1}.get(name, K)


@pytest.mark.parametrize("name", sorted(pr.CASES))
def test_jacobi_restatement_against_eigh(name):
    c = pr.case(name)
    S, G, lam, vec = c["S"], c["G"], c["lam"], c["vec"]
    lj, vj, sweeps = pr.sorted_jacobi(G)
    assert 1 <= sweeps < pr.MAX_SWEEPS
    tj = pr.tol_jac(G, sweeps)
    assert np.all(np.abs(lj - lam) <= tj), (name, np.max(np.abs(lj - lam)), tj)
    assert np.all(np.abs(vj.T @ vj - np.eye(S)) <= 16 * S * sweeps * pr.U)
    gap = pr.gaps(lam)
    for k in range(min(max(c["K"], 1), S - 1)):
        if pr.is_null(lam, k):
            continue
        sg = 1.0 if vj[:, k] @ vec[:, k] >= 0 else -1.0
        assert np.linalg.norm(sg * vj[:, k] - vec[:, k]) <= pr.davis_kahan(tj, gap[k]), (name, k)
    if name == "tips3":
        assert sweeps == 1 and not G.any()


def test_the_exact_case_is_exact():
    c = pr.case("exact")
    assert np.all(c["weight"] * 1024 == np.round(c["weight"] * 1024))
    G = c["Xc"] @ c["Xc"].T
    assert np.array_equal((G + 0.0).view(np.uint64), (c["G"] + 0.0).view(np.uint64))
    # every value is a multiple of 2^-30 below 2^20: any order of the additions is exact
    assert np.all(np.ldexp(c["Xc"], 15) == np.round(np.ldexp(c["Xc"], 15))) and np.abs(c["Xc"]).max() < 4.0
    mean, xc = pr.centre(c["X"])
    assert np.array_equal(xc, c["Xc"]) and np.array_equal(mean * c["S"], c["X"].sum(0))


def test_gram_and_covariance_routes_agree():
    c = pr.case("random40_s17")
    S, B = c["S"], len(c["blen"])
    cov = c["Xc"].T @ c["Xc"] / (S - 1)
    top = np.linalg.eigvalsh(cov)[::-1]
    _, _, sweeps = pr.sorted_jacobi(c["G"])
    bound = pr.tol_eig(c["G"], sweeps, B) / (S - 1)
    assert np.all(np.abs(top[:S - 1] - c["lam"][:S - 1] / (S - 1)) <= bound)
    assert np.all(np.abs(top[S - 1:]) <= bound)
    assert np.array_equal(c["eigenvalue"], np.maximum(c["lam"][:c["K"]], 0.0) / (S - 1))
    assert abs(c["total_var"] - top.sum()) <= bound * B


def writer_inputs(which):
    if which in ("tips4", "tips3", "random40_s3"):     # tips4: null components; tips3: total_var == 0
        c = pr.case(which)
        return ["s%d" % s for s in range(c["S"])], c["eigenvalue"], c["total_var"], c["edge_vec"], c["proj"]
    names = ["left", "right", "third one"]
    return names, [2.5, 1.0 / 3.0], 3.0, [[0.5, -0.5, 0.0, 1.0 / 3.0], [0.0, 0.0, 2.0 / 3.0, -0.125]], [[1.5, -2.5], [0.5, 0.25], [-2.0, 2.25]]


@pytest.mark.parametrize("precision", [0, 6, 15])
@pytest.mark.parametrize("which", ["tips3", "tips4", "random40_s3", "made_up"])
def test_host_writer_against_the_restatement(which, precision):
    names, ev, total, vec, proj = writer_inputs(which)
    got = hostlib.epca_texts(names, ev, total, vec, proj, precision=precision)
    want = pr.texts(names, ev, total, vec, proj, precision)
    assert got == want
    K = len(ev)
    assert got[0].splitlines()[0] == "component\teigenvalue\tfraction" and len(got[0].splitlines()) == K + 1
    assert got[1].splitlines()[0] == "sample" + "".join("\tpc%d" % (k + 1) for k in range(K))
    assert [ln.split("\t")[0] for ln in got[2].splitlines()[1:]] == [str(b) for b in range(np.shape(vec)[1])]
    if which == "tips3":
        assert float(total) == 0.0 and got[0].splitlines()[1].split("\t")[2] == "%.*f" % (precision, 0.0)
    if which == "tips4":
        assert all(ln.split("\t")[2:] == ["%.*f" % (precision, 0.0)] * (K - 1) for ln in got[1].splitlines()[1:])
    if which == "made_up" and precision == 6:
        assert got[0] == "component\teigenvalue\tfraction\n1\t2.500000\t0.833333\n2\t0.333333\t0.111111\n"
        assert got[1].splitlines()[3] == "third one\t-2.000000\t2.250000"
        assert got[2].splitlines()[4] == "3\t0.333333\t-0.125000"


def test_host_writer_refuses_bad_shapes():
    with pytest.raises(RuntimeError, match="epca: 2 components: 2 samples have 1 .. 1"):
        hostlib.epca_texts(["a", "b"], [1.0, 0.5], 1.5, np.zeros((2, 3)), np.zeros((2, 2)))
    with pytest.raises(RuntimeError, match="epca: 1 samples"):
        hostlib.epca_texts(["a"], [1.0], 1.0, np.zeros((1, 3)), np.zeros((1, 1)))


def test_epca_is_refused_before_any_file_is_read(tmp_path):
    base = ["-t", tmp_path / "no.tre", "-s", tmp_path / "no.fasta", "-w", tmp_path]
    many = ",".join("f%d.jplace" % i for i in range(1025))
    for extra, text in ((["--epca", "2"], "--epca finds the principal components of the samples of --krd and needs it"),
                        (["--krd", "a.jplace", "--epca", "1"], "--epca: principal components take 2 .. 1024 samples (1 given)"),
                        (["--krd", many, "--epca", "1"], "--epca: principal components take 2 .. 1024 samples (1025 given)"),
                        (["--krd", "a.jplace,b.jplace,c.jplace", "--epca", "0"], "--epca 0: 3 samples have 1 .. 2 components"),
                        (["--krd", "a.jplace,b.jplace,c.jplace", "--epca", "3", "--squash"], "--epca 3: 3 samples have 1 .. 2 components"),
                        (["--krd", "a.jplace,b.jplace,c.jplace", "--epca", "two"], "--epca two: 3 samples have 1 .. 2 components")):
        r = krd_cli(base + extra)
        assert r.returncode == 1 and text in r.stderr, (extra[-3:], r.stdout + r.stderr[-400:])
        assert "file_check failed" not in r.stderr
        assert not any((tmp_path / f).exists() for f in ("krd.tsv", "epca_eigenvalues.tsv", "epca_projection.tsv", "epca_edges.tsv"))
