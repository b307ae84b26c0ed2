"""epa-ng-amd --dedup end to end through the executable.

The reads are windows cut from the two queries of the golden nucleotide fixture: a few dozen distinct reads, each 1 to 9
times, shuffled, written as aligned FASTA and as binary fasta (synth.write_query_files; names q0000000 .. in file order).
The expected classes are tests/dedup_ref.py's on the encoded chunk.
  1. --dedup writes one placement object per class in order of first appearance, "n" = the class's names in file order,
     and the text of every object's "p" is, byte for byte, the "p" of each of its names in the plain run of the same file;
     --stats-json carries the two counts.
  2. classes are per chunk: a read that occurs in two chunks gives two objects.
  3. what the loop does not do is refused by name, before any output file exists.
  4. without --dedup nothing changes: one name per object, no "dedup" in the statistics, the same bytes from run to run.
"""
import json
import os
import re

import numpy as np
import pytest

import dedup_ref as dr
import epa_ng_amd as epa
import rescore_util as ru
from epa_ng_amd import synth

pytestmark = pytest.mark.gpu

FILES = tuple(ru.DATA + "/" + f for f in ("ref.tre", "aln.fasta", "query.fasta"))
OBJECT = re.compile(r'\{"p": \[\n(.*?)\n      \],\n    "n": \[(.*?)\]\n    \}', re.S)


def distinct_reads():
    """the fixture's two queries and 34 windows cut from them -> (codes [36][stride], win_begin, win_span, W), compact"""
    _, seqs = ru.read_fasta(FILES[2])
    W = len(seqs[0])
    rng = np.random.RandomState(31)
    reads = list(seqs)
    for k in range(34):
        n = int(rng.randint(40, 200))
        lo = int(rng.randint(0, W - n + 1))
        reads.append("-" * lo + seqs[k % len(seqs)][lo:lo + n] + "-" * (W - lo - n))
    reads = [r for r in reads if r.strip("-")]
    codes, wb, ws = epa.encode_queries(4, reads, compact=True)
    return codes, wb, ws, W


def duplicated(seed, counts=range(1, 10)):
    """-> (codes, win_begin, win_span) of the shuffled chunk, W"""
    codes, wb, ws, W = distinct_reads()
    rng = np.random.RandomState(seed)
    ids = np.concatenate([np.full(counts[i % len(counts)], i) for i in range(len(wb))])
    ids = ids[rng.permutation(len(ids))]
    return (np.ascontiguousarray(codes[ids]), wb[ids].copy(), ws[ids].copy()), W


def write_queries(tmp_path, enc, W):
    fa, bf = tmp_path / "reads.fasta", tmp_path / "reads.bfast"
    n = synth.write_query_files(str(fa), str(bf), [enc], W)
    return {"fasta": fa, "bfast": bf}, ["q%07d" % i for i in range(n)]


def run(tmp_path, tag, query, extra=()):
    out = tmp_path / tag
    out.mkdir()
    r = ru.run_cli(FILES[0], FILES[1], query, out, extra)
    assert r.returncode == 0, r.stdout + r.stderr
    text = open(out / "epa_result.jplace").read()
    objects = [(p, json.loads("[" + n + "]")) for p, n in OBJECT.findall(text)]
    assert len(objects) == len(json.loads(text)["placements"])
    return text, objects


def classes_of(enc, W, names, lo=0, hi=None):
    """the expected "n" lists of the chunk enc[lo:hi]"""
    codes, wb, ws = enc
    hi = len(wb) if hi is None else hi
    rep, first = dr.dedup(codes[lo:hi], wb[lo:hi], ws[lo:hi], W)
    return [[names[lo + q] for q in np.flatnonzero(rep == u)] for u in range(len(first))]


@pytest.mark.parametrize("kind", ["fasta", "bfast"])
def test_one_object_per_class_with_the_plain_runs_rows(tmp_path, kind):
    enc, W = duplicated(41)
    files, names = write_queries(tmp_path, enc, W)
    want = classes_of(enc, W, names)
    assert 30 <= len(want) < len(names) and max(len(c) for c in want) == 9 and min(len(c) for c in want) == 1
    _, plain = run(tmp_path, "plain", files[kind])
    assert [n for _, n in plain] == [[x] for x in names]
    p_of = {n[0]: p for p, n in plain}
    _, dd = run(tmp_path, "dedup", files[kind], ["--dedup", "--stats-json", tmp_path / "stats.json"])
    assert [n for _, n in dd] == want
    for p, ns in dd:
        for n in ns:
            assert p == p_of[n], n
    stats = json.load(open(tmp_path / "stats.json"))
    assert stats["dedup"] == {"reads": len(names), "unique": len(want)} and stats["chunk_path"] == "dedup"
    assert stats["queries"] == len(names)


@pytest.mark.parametrize("extra", [[], ["--memsave", "on"], ["--raxml-blo", "-G", "0.2"], ["--baseball-heur"]],
                         ids=["default", "memsave", "raxml_fixed", "baseball"])
def test_classes_are_per_chunk(tmp_path, extra):
    enc, W = duplicated(43, counts=(2, 1, 3))
    files, names = write_queries(tmp_path, enc, W)
    Q, per = len(names), 25
    want = [c for lo in range(0, Q, per) for c in classes_of(enc, W, names, lo, min(Q, lo + per))]
    assert len(want) > len(classes_of(enc, W, names))          # some read occurs in two chunks: two objects
    _, plain = run(tmp_path, "plain", files["fasta"], ["--chunk-size", per] + extra)
    p_of = {n[0]: p for p, n in plain}
    _, dd = run(tmp_path, "dedup", files["fasta"], ["--dedup", "--chunk-size", per] + extra)
    assert [n for _, n in dd] == want
    assert all(p == p_of[n] for p, ns in dd for n in ns)


def test_what_the_loop_does_not_do_is_refused(tmp_path):
    enc, W = duplicated(45, counts=(1, 2))
    files, names = write_queries(tmp_path, enc, W)
    fq = tmp_path / "reads.fastq"
    with open(fq, "w") as f:
        f.write("@r\n%s\n+\n%s\n" % ("A" * W, "I" * W))
    jp = tmp_path / "in.jplace"
    jp.write_text(json.dumps(ru.jplace_doc([])))
    cases = [(["--devices", "0,1"], files["fasta"], "--devices"), (["--rank", "0", "--world", "2"], files["fasta"], "--rank"),
             (["--no-heur"], files["fasta"], "--no-heur"), (["--rescore", jp], files["fasta"], "--rescore"),
             ([], fq, "FASTQ"), (["--no-pipeline"], files["fasta"], "--no-pipeline"),
             (["--host-heuristic"], files["fasta"], "--host-heuristic"), (["--device-min-chunk", "10"], files["fasta"], "--device-min-chunk")]
    for k, (extra, query, word) in enumerate(cases):
        out = tmp_path / ("refused%d" % k)
        out.mkdir()
        r = ru.run_cli(FILES[0], FILES[1], query, out, ["--dedup"] + extra)
        assert r.returncode != 0, (extra, r.stdout)
        assert "--dedup" in r.stderr and word in r.stderr and "not supported with it" in r.stderr, (extra, r.stderr)
        assert os.listdir(out) == [], extra


def test_without_the_flag_nothing_changes(tmp_path):
    enc, W = duplicated(47, counts=(1, 3))
    files, names = write_queries(tmp_path, enc, W)
    strip = lambda t: re.sub(r'"invocation": "[^"]*"', "", t)   # noqa: E731  (the command line names the output directory)
    a, plain = run(tmp_path, "a", files["fasta"])
    b, _ = run(tmp_path, "b", files["fasta"], ["--stats-json", tmp_path / "stats.json"])
    assert strip(a) == strip(b)
    assert [n for _, n in plain] == [[x] for x in names]
    stats = json.load(open(tmp_path / "stats.json"))
    assert "dedup" not in stats and stats["chunk_path"] != "dedup"
    d, _ = run(tmp_path, "d", files["fasta"], ["--dedup"])
    assert strip(d) != strip(a)
