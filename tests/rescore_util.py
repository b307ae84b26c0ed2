"""Shared by the --rescore tests: the golden nucleotide fixture, jplace documents written by hand and one way of
running the executable."""
import json
import os
import subprocess

from epa_ng_amd import hostlib

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
FIELDS = ["edge_num", "likelihood", "like_weight_ratio", "distal_length", "pendant_length"]


def read_fasta(path):
    """-> (labels, sequences)"""
    labels, seqs = [], []
    for line in open(path):
        line = line.strip()
        if line.startswith(">"):
            labels.append(line[1:])
            seqs.append("")
        elif line:
            seqs[-1] += line.upper()
    return labels, seqs


def write_fasta(path, labels, seqs):
    with open(path, "w") as f:
        for l, s in zip(labels, seqs):
            f.write(">%s\n%s\n" % (l, s))


def jplace_doc(placements, fields=FIELDS, tree="unused;"):
    return {"tree": tree, "placements": placements, "metadata": {"invocation": "by hand"}, "version": 3,
            "fields": list(fields)}


def run_cli(tree, msa, query, outdir, extra=(), model=None):
    """-> CompletedProcess of epa-ng-amd on the given files"""
    cmd = [hostlib.cli_exe(), "-t", str(tree), "-s", str(msa), "-q", str(query), "-w", str(outdir)]
    if model:
        cmd += ["-m", model]
    return subprocess.run(cmd + [str(x) for x in extra], capture_output=True, text=True, timeout=300)


def result(outdir):
    return json.load(open(os.path.join(str(outdir), "epa_result.jplace")))
