"""Profile queries, the parts that need no device: epa_profile_from_phred against a numpy restatement, the aligned-FASTQ
reader, the flag combinations the CLI refuses with a FASTQ query, and the self-consistency of the brute-force evaluator
that the device tests (tests/test_gpu_profile.py) use as their oracle for real-valued rows.
"""
import os
import subprocess

import numpy as np
import pytest

import brute_cases as bc
import epa_ng_amd as epa
import profile_util as pu
from epa_ng_amd import hostlib
from gen_golden import DEFAULT_BL, valid_range


# ---- epa_profile_from_phred

@pytest.mark.parametrize("states", [4, 20])
def test_profile_from_phred_against_numpy(states):
    rng = np.random.RandomState(states)
    Q, stride, ncols = 9, 40, {4: 16, 20: 24}[states]
    codes = rng.randint(0, ncols, (Q, stride)).astype(np.uint8)
    phred = rng.randint(0, 94, (Q, stride)).astype(np.uint8)
    phred[0, :4] = [0, 1, 93, 40]
    pure_col = {4: 8, 20: 0}[states]                    # 'A' in both alphabets
    codes[0, :4] = pure_col
    ws = rng.randint(1, stride + 1, Q).astype(np.uint32)
    ws[0], ws[1] = stride, 1
    sentinel = -7.0
    got = epa.profile_from_phred(states, codes, phred, ws, out=np.full((Q, stride, states), sentinel))
    want = pu.phred_rows(states, codes, phred, ws, fill=sentinel)
    pad = np.arange(stride)[None, :] >= ws[:, None]
    assert np.all(got[pad] == sentinel)                 # untouched padding, bit for bit
    masks = pu.column_masks(states)[codes]
    zero_one = (masks.sum(2) != 1) & ~pad
    assert zero_one.any() and np.array_equal(got[zero_one], masks[zero_one])         # state sets, bit for bit
    noisy = (masks.sum(2) == 1) & ~pad
    assert noisy.any()
    rel = np.abs(got[noisy] - want[noisy]) / want[noisy]
    print("\n%d states: %d rows with an error rate, max relative difference to numpy %.3g" % (states, noisy.sum(), rel.max()))
    assert rel.max() <= 1e-15
    # Phred 0 hits the cap (s - 1) / s: every state equally likely
    cap = (states - 1.0) / states
    assert got[0, 0, 0] == 1.0 - cap and np.all(got[0, 0, 1:] == cap / (states - 1.0))
    assert abs(got[0, 0].sum() - 1.0) < 1e-15
    # Phred 1 (eps 0.794) is above the cap of four states and below that of twenty; Phred 93 keeps all but 5e-10
    assert got[0, 1, 0] == 1.0 - cap if states == 4 else abs(got[0, 1, 0] - (1.0 - 10.0 ** -0.1)) < 1e-15
    assert abs(got[0, 2, 1] * (states - 1) / 10.0 ** -9.3 - 1.0) <= 1e-15 and abs(got[0, 2, 0] - (1.0 - 10.0 ** -9.3)) < 1e-15
    assert np.allclose(got[noisy].sum(1), 1.0, rtol=0, atol=1e-15)


def test_profile_from_phred_refuses():
    codes = np.full((2, 8), 8, np.uint8)
    ws = np.full(2, 8, np.uint32)
    phred = np.full((2, 8), 30, np.uint8)
    phred[1, 5] = 94
    with pytest.raises(epa.EpaError) as e:
        epa.profile_from_phred(4, codes, phred, ws)
    assert e.value.code == -1 and "query 1 position 5" in str(e.value) and "94" in str(e.value)
    codes[1, 5] = 10                                    # 'R': the score is ignored at an ambiguity code
    rows = epa.profile_from_phred(4, codes, phred, ws)
    assert np.array_equal(rows[1, 5], [1.0, 0.0, 1.0, 0.0])
    ws[1] = 5                                           # ... and beyond the span
    codes[1, 5] = 8
    epa.profile_from_phred(4, codes, phred, ws)
    codes[0, 0] = 16
    with pytest.raises(epa.EpaError) as e:
        epa.profile_from_phred(4, codes, phred, ws)
    assert e.value.code == -6 and "query 0 position 0" in str(e.value)
    with pytest.raises(epa.EpaError) as e:
        epa.profile_from_phred(4, np.full((1, 4), 8, np.uint8), np.zeros((1, 4), np.uint8), np.array([5], np.uint32))
    assert e.value.code == -1


# ---- the brute force as an oracle for rows: no device

@pytest.mark.parametrize("name", ["D5", "D6", "A3"])
def test_star_with_zero_one_rows_is_score_at(name):
    c, bf = bc.case(name), bc.brute(name)
    for q in (1, 4, len(c["reads"]) - 1):
        read = c["reads"][q]
        lo, n = valid_range(read)
        tipv = pu.column_masks(c["states"])[epa.encode_queries(c["states"], [read], compact=False)[0][0]][lo:lo + n]
        assert np.array_equal(tipv, bf.tip_vectors(read)[lo:lo + n])
        for b in (0, bf.B - 1):
            got = float(bf._star(b, tipv, DEFAULT_BL, 0.3 * bf.lengths[b], lo, n).sum())
            assert got == bf.score_at(b, read, DEFAULT_BL, 0.3 * bf.lengths[b])


@pytest.mark.parametrize("name", ["D5", "D6", "A3"])             # D6 and A3 carry +I: the invariant term is added once
def test_star_is_linear_in_the_rows(name):
    c, bf = bc.case(name), bc.brute(name)
    read = c["reads"][5]
    lo, n = valid_range(read)
    rows = pu.dense_rows(c["states"], (1, n), 3)[0]
    b = bf.B // 2
    base = bf._star(b, rows, 0.2, 0.5 * bf.lengths[b], lo, n)
    twice = np.array(rows)
    twice[7] *= 2.0
    moved = bf._star(b, twice, 0.2, 0.5 * bf.lengths[b], lo, n) - base
    if bf.pinv == 0.0:
        assert abs(moved[7] - np.log(2.0)) < 1e-12
    else:                      # log((1 - p) 2 L + c) - log((1 - p) L + c): ln 2 only where the site is not invariant
        inv = bf.invariant_state[lo + 7] >= 0
        assert (abs(moved[7] - np.log(2.0)) < 1e-12) == (not inv)
        assert 0.0 < moved[7] <= np.log(2.0) + 1e-12
    assert np.all(np.delete(moved, 7) == 0.0)
    # a sum of two rows is the sum of the likelihoods (with +I: of their variable parts)
    other = pu.dense_rows(c["states"], (1, n), 4)[0]
    la, lb, lab = (np.exp(bf._star(b, r, 0.2, 0.5 * bf.lengths[b], lo, n)) for r in (rows, other, rows + other))
    cinv = np.exp(bf.log_cinv[lo:lo + n]) if bf.pinv > 0.0 else 0.0
    assert np.allclose(lab - cinv, (la - cinv) + (lb - cinv), rtol=1e-10, atol=0)


# ---- the aligned-FASTQ reader

def write_fastq(path, names, reads, quals):
    with open(path, "w") as f:
        for n, r, q in zip(names, reads, quals):
            f.write("@%s\n%s\n+\n%s\n" % (n, r, q))


def test_fastq_reader_round_trip(tmp_path):
    names = ["read one", "r2/1", "third"]
    reads = ["--ACGTNRY-", "ACGT--ACGT", "-----T----"]
    quals = ["!!I5?#~+A!", "~~~~~~~~~~", "!!!!!J!!!!"]
    src, dst = tmp_path / "in.fastq", tmp_path / "out.fastq"
    write_fastq(src, names, reads, quals)
    assert hostlib.fastq_copy(src, dst) == 3
    assert dst.read_text() == src.read_text()
    # lower case, blank lines between records, a repeated name on the '+' line and CRLF line ends are read as the same records
    loose = tmp_path / "loose.fastq"
    loose.write_text("".join("\n@%s\r\n%s\r\n+%s\r\n%s\r\n" % (n, r.lower(), n, q) for n, r, q in zip(names, reads, quals)))
    assert hostlib.fastq_copy(loose, dst) == 3
    assert dst.read_text() == src.read_text()


def test_fastq_reader_refuses(tmp_path):
    src, dst = tmp_path / "in.fastq", tmp_path / "out.fastq"
    write_fastq(src, ["a", "b", "c"], ["ACGT-", "ACGT-", "ACGT-"], ["IIIII", "IIII", "IIIII"])
    with pytest.raises(RuntimeError) as e:                 # the width mismatch names the record
        hostlib.fastq_copy(src, dst)
    assert "record 2" in str(e.value) and "'b'" in str(e.value) and "5" in str(e.value) and "4" in str(e.value)
    write_fastq(src, ["a"], ["ACGT"], ["II I"])
    with pytest.raises(RuntimeError) as e:
        hostlib.fastq_copy(src, dst)
    assert "record 1" in str(e.value) and "Phred+33" in str(e.value)
    src.write_text("@a\nACGT\n+\n")
    with pytest.raises(RuntimeError) as e:
        hostlib.fastq_copy(src, dst)
    assert "record 1" in str(e.value) and "incomplete" in str(e.value)
    src.write_text(">a\nACGT\n")
    with pytest.raises(RuntimeError):
        hostlib.fastq_copy(src, dst)


# ---- what the CLI refuses with a FASTQ query, before any device is opened

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")


@pytest.mark.parametrize("flags,named", [(["--devices", "0,1"], "--devices"), (["--rank", "0", "--world", "2"], "--rank"),
                                         (["--world", "1"], "--world"), (["--comm-file", "x"], "--comm-file"),
                                         (["--no-heur"], "--no-heur"), (["--rescore", "some.jplace"], "--rescore"),
                                         (["--memsave", "on"], "--memsave on"), (["--host-heuristic"], "--host-heuristic"),
                                         (["--device-min-chunk", "10"], "--device-min-chunk")],
                         ids=lambda v: v if isinstance(v, str) else None)
def test_cli_refuses_with_a_fastq_query(flags, named, tmp_path):
    fq = tmp_path / "reads.fastq"
    write_fastq(fq, ["a"], ["ACGT"], ["IIII"])
    # neither tree nor alignment exists: the refusal comes before any file is parsed, let alone a device opened
    cmd = [hostlib.cli_exe(), "-t", str(tmp_path / "no.tre"), "-s", str(tmp_path / "no.fasta"), "-q", str(fq), "-w", str(tmp_path)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "EPA_RANK", "EPA_WORLD",
                                                            "EPA_COMM_FILE")}
    env.update(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run(cmd + flags, capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 1, r.stdout + r.stderr
    assert named in r.stderr and "FASTQ" in r.stderr, r.stderr
    assert not (tmp_path / "epa_result.jplace").exists()
    # the same flags with a FASTA query get past this check (and fail on the missing tree instead)
    fa = tmp_path / "reads.fasta"
    fa.write_text(">a\nACGT\n")
    cmd[cmd.index("-q") + 1] = str(fa)
    r = subprocess.run(cmd + flags, capture_output=True, text=True, timeout=60, env=env)
    assert "FASTQ" not in r.stderr
