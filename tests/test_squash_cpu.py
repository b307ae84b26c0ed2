"""Squash clustering without a device: the restated loop of tests/squash_ref.py, the host writer of squash.tsv and
squash.newick, and the executable's refusals.

  1. every step of squash_ref.restate is DECIDED on the five trees of krd_ref.case and on case65: runner-up - winner >=
     1000 tol_step, or both distances are exactly 0.0 and the tie rule gives the recorded pair.  This is the condition
     under which comparing the device's merge decisions with a restatement that agrees within a tolerance means anything.
     No step is left out.
  2. the winning distances agree with krd_ref.Brute on the materialised pair within tol: every step where B <= 77, steps
     0, 1, the last and four others otherwise.
  3. the linkage is well formed: every id is a child once, a < b, the sizes add up, the last size is S.
  4. the host writer (libepa_host's squash_texts) against squash_ref.newick / table as strings: 2 and 5 samples, an
     inversion that yields a negative branch length, precisions 0, 6 and 15; what is no linkage is refused.
  5. epa-ng-amd --squash: refused without --krd, with one file, for a sample name with '(' and one with a blank, before any
     file is read.
"""
import numpy as np
import pytest

import squash_ref as sr
from epa_ng_amd import hostlib
from test_krd_cpu import krd_cli


@pytest.mark.parametrize("name", sr.CASES)
def test_every_step_is_decided(name):
    steps, _ = sr.run(name)
    c = sr.case(name)
    assert len(steps) == c["S"] - 1
    worst = np.inf
    for t, s in enumerate(steps):
        if s["d"] == 0.0 and s["runner"] == 0.0:
            continue                                              # an exact tie: restate's argmin applied the tie rule
        gap = s["runner"] - s["d"]
        if s["tol_step"] > 0:
            worst = min(worst, gap / s["tol_step"])
        assert gap >= 1000.0 * s["tol_step"], (name, t, s)
    print(name, "smallest gap / tol_step over the decided steps: %.3g; exact ties at steps %s; monotone: %s" %
          (worst, [t for t, s in enumerate(steps) if s["d"] == 0.0 and s["runner"] == 0.0],
           all(x["d"] <= y["d"] for x, y in zip(steps[:-1], steps[1:]))))
    if name != "case65":
        ix = c["index"]                                           # the two exact ties every case starts with
        assert (steps[0]["a"], steps[0]["b"]) == tuple(sorted((ix["empty"], ix["zeros"]))) and steps[0]["d"] == 0.0
        assert (steps[1]["a"], steps[1]["b"]) == tuple(sorted((ix["r65"], ix["copy65"]))) and steps[1]["d"] == 0.0


@pytest.mark.parametrize("name", sr.CASES)
def test_winning_distances_agree_with_brute(name):
    steps, members = sr.run(name)
    n = len(steps)
    if len(sr.case(name)["blen"]) <= 77:
        chosen = range(n)
    else:
        chosen = sorted({0, 1, n - 1} | {int(t) for t in np.random.RandomState(n).choice(np.arange(2, n - 1), 4, replace=False)})
    worst = 0.0
    for t in chosen:
        s = steps[t]
        got = sr.brute_step(name, members[s["a"]], members[s["b"]])
        worst = max(worst, abs(got - s["d"]) / s["tol"] if s["tol"] > 0 else (0.0 if got == s["d"] else np.inf))
        assert abs(got - s["d"]) <= s["tol"], (name, t, got, s)
    print(name, "max |restate - brute| / tol %.3g over %d steps" % (worst, len(list(chosen))))


@pytest.mark.parametrize("name", sr.CASES)
def test_linkage_is_well_formed(name):
    steps, members = sr.run(name)
    S = sr.case(name)["S"]
    size = {s: 1 for s in range(S)}
    children = []
    for t, s in enumerate(steps):
        assert s["a"] < s["b"] < S + t
        size[S + t] = size[s["a"]] + size[s["b"]]
        assert s["size"] == size[S + t] == len(members[S + t])
        children += [s["a"], s["b"]]
    assert sorted(children) == list(range(2 * S - 2)) and steps[-1]["size"] == S
    assert members[2 * S - 2] == list(range(S))


WRITER_CASES = {
    "two": (["left", "right"], ([0], [1], [0.75], [2])),
    "five": (["s0", "s1", "s2", "s3", "s4"], ([1, 0, 2, 6], [3, 4, 5, 7], [0.125, 0.3, 1.0 / 3.0, 2.5], [2, 2, 3, 5])),
    # cluster3 = (a, b) is nearer to c than a was to b: a negative branch above it
    "inversion": (["a", "b", "c"], ([0, 2], [1, 3], [0.5, 0.3125], [2, 3])),
    "zeros": (["u", "v", "w"], ([0, 2], [1, 3], [0.0, 0.0], [2, 3])),
}


@pytest.mark.parametrize("precision", [0, 6, 15])
@pytest.mark.parametrize("which", sorted(WRITER_CASES))
def test_host_writer_against_the_restatement(which, precision):
    names, merges = WRITER_CASES[which]
    table, newick = hostlib.squash_texts(names, *merges, precision=precision)
    assert table == sr.table(names, merges, precision)
    assert newick == sr.newick(names, merges, precision)
    assert newick.endswith(")cluster%d;\n" % (len(names) - 2)) and newick.count("(") == len(names) - 1
    if which == "inversion" and precision:
        assert ":-0.09375" in newick                             # height 0.15625 - 0.25
    if which == "two" and precision == 6:
        assert table == "step\ta\tb\tdistance\tsize\n0\tleft\tright\t0.750000\t2\n"
        assert newick == "(left:0.375000,right:0.375000)cluster0;\n"


def test_host_writer_refuses_what_is_no_linkage():
    for a, b in (([0, 0], [1, 3]), ([1, 2], [0, 3]), ([0, 2], [1, 4])):
        with pytest.raises(RuntimeError, match="squash: step"):
            hostlib.squash_texts(["a", "b", "c"], a, b, [0.1, 0.2], [2, 3])


def test_squash_is_refused_before_any_file_is_read(tmp_path):
    base = ["-t", tmp_path / "no.tre", "-s", tmp_path / "no.fasta", "-w", tmp_path]
    for extra, text in ((["--squash"], "--squash clusters the samples of --krd and needs it"),
                        (["--krd", "a.jplace", "--squash"], "--squash: clustering needs two samples at least"),
                        (["--krd", "a.jplace,x/b(1).jplace", "--squash"], "--squash: the sample name 'b(1)'"),
                        (["--krd", "a.jplace,my sample.jplace", "--squash", "--krd-masses"], "--squash: the sample name 'my sample'")):
        r = krd_cli(base + extra)
        assert r.returncode == 1 and text in r.stderr, (extra, r.stdout + r.stderr)
        assert "file_check failed" not in r.stderr
        assert not any((tmp_path / f).exists() for f in ("krd.tsv", "squash.tsv", "squash.newick"))
