"""epa-ng-amd -q reads.fastq end to end through the executable: an aligned FASTQ is placed as per-site state likelihoods.

The reads are the two queries of the golden nucleotide fixture and four windows cut from them, with random Phred
scores 2 .. 41, in chunks of four (two chunk bodies).
  1. every jplace row's likelihood is Evaluator.score_at_profile at the row's printed lengths on the rows that
     profile_from_phred makes of the same reads and scores (the comparison of tests/test_gpu_rescore_cli.py: the
     lengths travel through the printed digits, bound 1e-6); LWRs are the softmax of the pquery's rows where no
     row was filtered; --stats-json names the query kind.
  2. with every score 93 (error rate 5e-10) each read keeps the best edge of the coded run on the same reads as FASTA.
"""
import json

import numpy as np
import pytest

import epa_ng_amd as epa
import rescore_util as ru
from epa_ng_amd import hostlib

pytestmark = pytest.mark.gpu

LNL_TOL = 1e-6
FILES = tuple(ru.DATA + "/" + f for f in ("ref.tre", "aln.fasta", "query.fasta"))


def fixture_reads():
    labels, seqs = ru.read_fasta(FILES[2])
    W = len(seqs[0])
    names, reads = list(labels), list(seqs)
    for k, (lo, n) in enumerate(((0, 70), (W - 130, 130), (200, 64), (301, 65))):
        src = seqs[k % len(seqs)]
        names.append("%s_w%d" % (labels[k % len(seqs)], k))
        reads.append("-" * lo + src[lo:lo + n] + "-" * (W - lo - n))
    return names, reads


def write_fastq(path, names, reads, quals):
    with open(path, "w") as f:
        for n, r, q in zip(names, reads, quals):
            f.write("@%s\n%s\n+\n%s\n" % (n, r, q))


def test_fastq_rows_are_score_at_profile(tmp_path):
    names, reads = fixture_reads()
    rng = np.random.RandomState(17)
    scores = [rng.randint(2, 42, len(r)) for r in reads]
    fq = tmp_path / "reads.fastq"
    write_fastq(fq, names, reads, ["".join(chr(33 + int(s)) for s in sc) for sc in scores])
    out = tmp_path / "out"
    out.mkdir()
    r = ru.run_cli(FILES[0], FILES[1], fq, out, ["--chunk-size", "4", "--filter-min-lwr", "0", "--filter-max", "64",
                                                 "--stats-json", out / "stats.json"])
    assert r.returncode == 0, r.stdout + r.stderr
    stats = json.load(open(out / "stats.json"))
    assert stats["query_kind"] == "profile" and stats["chunk_path"] == "profile" and stats["queries"] == len(reads)
    res = ru.result(out)
    assert res["fields"] == ru.FIELDS and [pq["n"] for pq in res["placements"]] == [[n] for n in names]
    # the same reference, reads and scores through the Python surface; the executable drops the masked columns first
    keep = hostlib.premask(FILES[1], str(fq)) == 0
    cut = lambda s: "".join(np.array(list(s))[keep])   # noqa: E731
    ref_labels, ref_seqs = ru.read_fasta(FILES[1])
    ref = hostlib.Reference(open(FILES[0]).read().strip(), ref_labels, [cut(s) for s in ref_seqs], model="GTR+G")
    ev = ref.evaluator()
    codes, wb, ws = epa.encode_queries(4, [cut(rd) for rd in reads], compact=True)
    phred = np.zeros(codes.shape, np.uint8)
    for q, sc in enumerate(scores):
        sc = sc[keep]
        phred[q, :ws[q]] = sc[wb[q]:wb[q] + ws[q]]
    rows = epa.profile_from_phred(4, codes, phred, ws)
    worst = 0.0
    for q, pq in enumerate(res["placements"]):
        p = np.array(pq["p"])
        assert len(p) >= 1 and np.all(p[:-1, 2] >= p[1:, 2])              # LWR descending
        pairs = np.zeros(len(p), epa.PAIR_DTYPE)
        pairs["branch_id"], pairs["seq_id"] = p[:, 0].astype(np.uint32), q
        want = ev.score_at_profile(pairs, p[:, 4], p[:, 3], rows, wb, ws)
        worst = max(worst, float(np.max(np.abs(p[:, 1] - want))))
        assert np.max(np.abs(p[:, 1] - want)) < LNL_TOL
        e = np.exp(p[:, 1] - p[:, 1].max())
        assert np.max(np.abs(p[:, 2] - e / e.sum())) < 1e-8
    print("\nFASTQ run: max |likelihood - score_at_profile at the printed lengths| %.3g" % worst)


def test_scores_of_93_keep_the_coded_best_edge(tmp_path):
    names, reads = fixture_reads()
    fq, fa = tmp_path / "reads.fastq", tmp_path / "reads.fasta"
    write_fastq(fq, names, reads, ["~" * len(r) for r in reads])
    ru.write_fasta(fa, names, reads)
    best = {}
    for kind, query in (("profile", fq), ("coded", fa)):
        out = tmp_path / kind
        out.mkdir()
        r = ru.run_cli(FILES[0], FILES[1], query, out)
        assert r.returncode == 0, r.stdout + r.stderr
        res = ru.result(out)
        assert [pq["n"] for pq in res["placements"]] == [[n] for n in names]
        best[kind] = [(pq["p"][0][0], pq["p"][0][1]) for pq in res["placements"]]
    assert [b[0] for b in best["profile"]] == [b[0] for b in best["coded"]]
    d = max(abs(a[1] - b[1]) for a, b in zip(best["profile"], best["coded"]))
    print("\nscores of 93: max |likelihood of the best edge, FASTQ run - FASTA run| %.3g" % d)
