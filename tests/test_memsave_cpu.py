"""CPU tests of the memory-saving lookup layout: the footprint and plan functions of include/epa_dev.h (pure host
arithmetic, no device), the chunk loop's memory clamp with block buffers, and the CLI's --memsave argument."""
import subprocess

import pytest

import epa_ng_amd as epa
from epa_ng_amd import hostlib

MISC_KEYS = ("reft", "scsum", "lookup", "lookup2", "refi", "misc")


def _fp(*a, **k):
    f = epa.footprint(*a, **k)
    assert f["reference"] == sum(f[k_] for k_ in MISC_KEYS)
    return f


def test_footprint_cfg2_to_the_byte():
    # n = 512 tips -> B = 1021 branches, W = 1500, 4 states, 4 categories
    B, W, c, s = 2 * 512 - 3, 1500, 4, 4
    f = _fp(s, c, W, B)
    assert f["reft"] == 8 * 2 * B * c * s * W == 392_064_000
    assert f["scsum"] == 4 * B * W == 6_126_000
    assert f["lookup"] == 8 * B * W * 16 == 196_032_000
    assert f["lookup2"] == 8 * B * 2 * ((W + 1) // 2) * 36 == 441_072_000
    assert f["refi"] == 8 * B * c * s * W + B * W == 196_032_000 + 1_531_500
    # the table's megabytes
    assert [round(f[k] / 1e6) for k in ("reft", "scsum", "lookup", "lookup2")] == [392, 6, 196, 441]
    assert f["bank"] == 0 and f["steady"] == f["reference"] == f["peak"]
    # blocked: only refT + scSum stay; one block of 1024 branches holds the whole tree
    g = _fp(s, c, W, B, flags=epa.FLAG_LOOKUP_BLOCKS, banks=2)
    assert (g["reft"], g["scsum"]) == (f["reft"], f["scsum"])
    assert g["lookup"] == g["lookup2"] == g["refi"] == 0
    assert g["bank"] == 1024 * W * 16 * 8 + 1024 * 2 * 750 * 36 * 8
    assert g["steady"] == g["reference"] + 2 * g["bank"]


def test_footprint_bytes_per_branch_site():
    W = 1500
    for s, res, blk in ((4, 805, 260), (20, 2117, 1284)):
        B = 2 * 100_000 - 3
        f = _fp(s, 4, W, B)
        g = _fp(s, 4, W, B, flags=epa.FLAG_LOOKUP_BLOCKS, banks=0)
        assert abs(f["reference"] / (B * W) - res) < 0.01
        assert abs(g["reference"] / (B * W) - blk) < 0.01
    # the issue's example: 100 000 tips x 1500 columns, nucleotides, resident: 241 GB
    assert 241e9 < _fp(4, 4, W, 199_997)["reference"] < 242e9


@pytest.mark.parametrize("s,c_in,c", [(4, 3, 4), (4, 5, 8), (4, 1, 4), (4, 2, 4), (4, 8, 8), (4, 13, 16), (20, 8, 8),
                                      (20, 1, 4), (20, 3, 4), (20, 6, 8), (20, 9, 9)])
def test_footprint_category_padding(s, c_in, c):
    B, W = 77, 333   # odd W
    f = _fp(s, c_in, W, B)
    assert f["reft"] == 8 * 2 * B * c * s * W
    assert f["scsum"] == 4 * B * W
    assert f["lookup"] == 8 * B * W * (16 if s == 4 else 24)
    assert f["lookup2"] == (8 * B * 2 * 167 * 36 if s == 4 else 0)    # ceil(333 / 2) = 167
    tuned = c == 4 or (s == 4 and c % 4 == 0) or (s == 20 and c == 8)
    assert f["refi"] == ((8 * B * c * s * W + B * W) if tuned else 0)
    g = _fp(s, c_in, W, B, flags=epa.FLAG_LOOKUP_BLOCKS, block_branches=64, banks=3)
    assert g["bank"] == 64 * W * (16 if s == 4 else 24) * 8 + (64 * 2 * 167 * 36 * 8 if s == 4 else 0)
    assert g["steady"] == g["reference"] + 3 * g["bank"]
    # a block buffer never holds more rows than the tree has, rounded up to 64
    assert _fp(s, c_in, W, B, flags=epa.FLAG_LOOKUP_BLOCKS, block_branches=1024)["bank"] == g["bank"] * 2


def test_footprint_per_rate_scalers_keep_caller_categories():
    # per-rate scaler rows of the caller cannot be padded: 5 categories stay 5 (general kernel, no refI)
    f = _fp(4, 5, 100, 13, flags=0x2)
    assert f["reft"] == 8 * 2 * 13 * 5 * 4 * 100 and f["refi"] == 0
    # from a tree they are padded, and the precompute's per-side counts are per category
    t = _fp(4, 5, 100, 13, flags=0x2, from_tree=True)
    assert t["reft"] == 8 * 2 * 13 * 8 * 4 * 100
    n = 8
    assert t["create_temp"] == n * 100 + 32 * 3 * (n - 2) + 4 * 2 * 13 * 8 * 100 + 4 * 13
    assert t["peak"] == max(t["steady"], t["reference"] + t["create_temp"])


def test_footprint_rejects_bad_shapes():
    for args in ((5, 4, 100, 13), (4, 0, 100, 13), (4, 17, 100, 13), (4, 4, 0, 13), (4, 4, 100, 0)):
        with pytest.raises(epa.EpaError):
            epa.footprint(*args)
    with pytest.raises(epa.EpaError):
        epa.footprint(4, 4, 100, 13, flags=epa.FLAG_LOOKUP_BLOCKS, block_branches=100)


SHAPE = (4, 4, 96, 65537)   # the 32 770-tip x 96-site tree of the large-tree tests


def test_lookup_plan_steps():
    banks = 4
    res = _fp(*SHAPE, banks=banks)
    assert epa.lookup_plan(res["peak"], *SHAPE, banks=banks) == (epa.LOOKUP_RESIDENT, 0)
    assert epa.lookup_plan(10 * res["peak"], *SHAPE, banks=banks) == (epa.LOOKUP_RESIDENT, 0)
    # one byte short of resident: blocks of 1024
    assert epa.lookup_plan(res["peak"] - 1, *SHAPE, banks=banks) == (epa.LOOKUP_BLOCKS, 1024)
    # forced blocks although resident would fit
    assert epa.lookup_plan(10 * res["peak"], *SHAPE, flags=epa.FLAG_LOOKUP_BLOCKS, banks=banks) == (epa.LOOKUP_BLOCKS, 1024)
    # the block shrinks in steps of 64 down to 64: exactly at each size's peak it is chosen, one byte below the next
    for blk in range(1024, 0, -64):
        need = _fp(*SHAPE, flags=epa.FLAG_LOOKUP_BLOCKS, block_branches=blk, banks=banks)["peak"]
        assert epa.lookup_plan(need, *SHAPE, banks=banks) == (epa.LOOKUP_BLOCKS, blk)
        if blk > 64:
            assert epa.lookup_plan(need - 1, *SHAPE, banks=banks) == (epa.LOOKUP_BLOCKS, blk - 64)
    low = _fp(*SHAPE, flags=epa.FLAG_LOOKUP_BLOCKS, block_branches=64, banks=banks)
    for usable in (low["peak"] - 1, low["reft"] + low["scsum"] - 1, low["reft"], 0):
        with pytest.raises(epa.EpaError) as e:
            epa.lookup_plan(usable, *SHAPE, banks=banks)
        assert e.value.code == epa.ERR_NO_MEMORY
        assert str(low["peak"]) in str(e.value) and str(usable) in str(e.value)   # needed and usable bytes


def test_lookup_plan_monotone():
    for shape in (SHAPE, (4, 4, 1500, 1021), (20, 4, 700, 1021), (4, 4, 300, 13)):
        for from_tree in (False, True):
            top = _fp(*shape, from_tree=from_tree, banks=4)["peak"]
            last = (-1, 0)
            for i in range(0, 401):
                usable = top * i // 380
                try:
                    mode, blk = epa.lookup_plan(usable, *shape, from_tree=from_tree, banks=4)
                    rank = (1, 0) if mode == epa.LOOKUP_RESIDENT else (0, blk)
                except epa.EpaError as e:
                    assert e.code == epa.ERR_NO_MEMORY
                    rank = (-1, 0)
                assert rank >= last, (shape, usable, rank, last)
                last = rank
            assert last == (1, 0)


def test_chunk_reads_with_block_buffers():
    B, slots = 65537, 4
    bank = _fp(4, 4, 96, B, flags=epa.FLAG_LOOKUP_BLOCKS, banks=1)["bank"]
    assert bank == 1024 * 96 * (128 + 288)
    for free in (1 << 28, 1 << 30, 3 << 30, 1 << 34):
        wanted = 1 << 30
        plain = hostlib.device_chunk_reads(free, B, slots, wanted)
        blocked = hostlib.device_chunk_reads(free, B, slots, wanted, bank_bytes=bank)
        # the banks' bytes come off the free memory, nothing else changes
        assert blocked == hostlib.device_chunk_reads(max(0, free - slots * bank), B, slots, wanted)
        assert blocked <= plain
        if free >= 1 << 30:
            assert 1 < blocked < plain
    # resident (no bank): the existing function, bit for bit
    assert hostlib.device_chunk_reads(1 << 30, B, slots, 50000, 0, 0) == hostlib.device_chunk_reads(1 << 30, B, slots, 50000)
    assert hostlib.device_chunk_reads(1 << 20, B, slots, 5000, bank_bytes=bank) == 1


def test_cli_memsave_argument():
    exe = hostlib.cli_exe()
    r = subprocess.run([exe, "--memsave", "bogus"], capture_output=True, text=True)
    assert r.returncode == 1
    assert "--memsave" in r.stderr and "bogus" in r.stderr and "auto,on,off" in r.stderr
    for v in ("auto", "on", "off"):   # accepted: the run then stops at the missing input files (usage, exit 1)
        r = subprocess.run([exe, "--memsave", v], capture_output=True, text=True)
        assert r.returncode == 1 and "--memsave:" not in r.stderr
    h = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert h.returncode == 0 and "--memsave auto|on|off" in h.stdout
