"""Fixtures of the end-point tests (tests/golden/endpoints/*.json, written by tests/gen_endpoints.py) and the rule by
which an optimiser's end points are compared with them.  Shared by tests/test_endpoints_cpu.py (the C oracle) and
tests/test_gpu_endpoints.py (the device); no likelihood code.

The rule uses the suite's existing numbers only:
  agreeing pair   pendant and distal equal the fixture's to 1e-6 relative, floor 1e-9 (sweep_util.lengths_differ) and
                  lnL within lnl_tol of the fixture's (1e-6 for the device, 1e-8 for the CPU oracle);
  any other pair  lnL within sweep_util.FLAT_LNL_TOL = 1e-4 of the fixture's, and at most n // 100 of them per
                  configuration and mode (sweep_util.FLAT_MAX_FRACTION);
  every pair      finite values, pendant > 0, 0 <= distal <= branch length.
"""
import functools
import json
import os

import numpy as np

from sweep_util import FLAT_LNL_TOL, FLAT_MAX_FRACTION, lengths_differ

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "endpoints")


@functools.lru_cache(maxsize=None)
def load(name):
    """-> {"case", "thinning", "modes": {key: {"branch", "read", "lnl", "pendant", "distal", "rounds", "reverted"}}},
    the columns as numpy arrays; key = brute_cases.endpoint_key(mode, min_branch)"""
    with open(os.path.join(DIR, name + ".json")) as f:
        g = json.load(f)
    assert g["case"] == name
    for e in g["modes"].values():
        pairs = np.array(e.pop("pairs"), np.int64).reshape(-1, 2)
        e["branch"], e["read"] = pairs[:, 0], pairs[:, 1]
        for k in ("lnl", "pendant", "distal"):
            e[k] = np.array(e[k], np.float64)
        e["rounds"] = np.array(e["rounds"], np.int64)
        e["reverted"] = np.array(e["reverted"], bool)
        assert len({len(e[k]) for k in ("branch", "lnl", "pendant", "distal", "rounds", "reverted")}) == 1
    return g


def lookup(entry, branches, reads):
    """rows of a fixture entry for the given (branch, read) pairs -> (index into the entry, found mask)"""
    at = {(int(b), int(q)): i for i, (b, q) in enumerate(zip(entry["branch"], entry["read"]))}
    idx = np.array([at.get((int(b), int(q)), -1) for b, q in zip(branches, reads)], np.int64)
    return idx, idx >= 0


def compare(entry, lnl, pendant, distal, branch_lengths, lnl_tol, rows=None):
    """applies the rule to results given in the entry's pair order (or for its `rows`) -> dict of the figures; raises
    AssertionError where the rule is broken"""
    st = measure(entry, lnl, pendant, distal, branch_lengths, lnl_tol, rows)
    assert st["sane"], "non-finite value, pendant <= 0 or distal outside [0, branch length]"
    assert st["max_dlnl_other"] <= FLAT_LNL_TOL, st
    assert st["other"] <= st["cap"], st
    return st


def measure(entry, lnl, pendant, distal, branch_lengths, lnl_tol, rows=None):
    """the figures of the rule without asserting: n, other (pairs that do not agree), cap, sane, max_dlnl (agreeing
    pairs), max_rel_pendant / max_rel_distal (agreeing pairs, relative with the rule's 1e-3 floor), max_dlnl_other,
    broken (True where compare() would raise)"""
    rows = np.arange(len(entry["lnl"])) if rows is None else np.asarray(rows)
    lnl, pendant, distal = (np.asarray(a, np.float64) for a in (lnl, pendant, distal))
    xl, xp, xd = entry["lnl"][rows], entry["pendant"][rows], entry["distal"][rows]
    length = np.asarray(branch_lengths)[entry["branch"][rows]]
    sane = bool(np.all(np.isfinite(lnl)) and np.all(np.isfinite(pendant)) and np.all(np.isfinite(distal))
                and np.all(pendant > 0.0) and np.all(distal >= 0.0) and np.all(distal <= length))
    with np.errstate(invalid="ignore"):
        dl = np.abs(lnl - xl)
        agree = ~lengths_differ(pendant, distal, xp, xd) & (dl <= lnl_tol)
        rp = np.abs(pendant - xp) / np.maximum(1e-3, np.abs(xp))
        rd = np.abs(distal - xd) / np.maximum(1e-3, np.abs(xd))
    n, other = len(rows), int((~agree).sum())
    mx = lambda a: float(np.max(a)) if len(a) else 0.0          # noqa: E731
    st = {"n": n, "other": other, "cap": n // int(round(1.0 / FLAT_MAX_FRACTION)), "sane": sane, "max_dlnl": mx(dl[agree]),
          "max_rel_pendant": mx(rp[agree]), "max_rel_distal": mx(rd[agree]), "max_dlnl_other": mx(dl[~agree]),
          "other_pairs": [(int(entry["branch"][r]), int(entry["read"][r])) for r in rows[~agree]]}
    st["broken"] = not (sane and st["max_dlnl_other"] <= FLAT_LNL_TOL and other <= st["cap"])
    return st


def line(name, key, st):
    return ("%-6s %-14s %4d pairs, %d not agreeing (cap %d), agreeing pairs: max |dlnL| %.2g, rel. pendant %.2g, "
            "rel. distal %.2g; others: max |dlnL| %.2g"
            % (name, key, st["n"], st["other"], st["cap"], st["max_dlnl"], st["max_rel_pendant"], st["max_rel_distal"],
               st["max_dlnl_other"]))
