"""Where the inputs and outputs of the post-placement entry points live: epa_dev_score_at, _site_lnl, _marginal_like,
_rell_support, _rell_tests and _rell_au take every array from host or device memory and write every output to either.
The other tests of these calls pass host arrays (marginal_like's M once into a device buffer); here the SAME call is
made with other memory and must give the same bits.

Inputs: the 22 reads x 30 sites x three entries of the statistical checks (rell_ref.stat_input, D5: 4 states) and A4's
reads (20 states) with three entries each; 257 replicates; explicit stream ids; a 3 x 5 rule.

  1. same call, different memory: all-host arrays against pairs, lengths, windows, codes (and stream ids) in device
     tensors with every output a device tensor pre-filled with NaN (the counts with 0xffffffff).
  2. mixed outputs, through the C ABI: rell_tests with support on the device, elw and p_sh on the host; rell_au with
     counts on the device, p_au and fit on the host, and with fit alone; marginal_like with M on the device and the
     grid on the host.
  3. history: each of these calls is followed by a call of another member of the family on the same context (host
     arrays); then the first call's outputs are read again, and the first call made again gives the same bits.  The
     six share the staging buffer of their host outputs, and marginal_like keeps its rule and grid values where the
     others keep their branch lengths.
"""
import functools

import numpy as np
import pytest
import torch

import brute_cases as bc
import epa_ng_amd as epa
import rell_ref as rr
from epa_ng_amd.api import _ptr
from history_util import assert_same
from test_gpu_rell import entry_lists
from test_gpu_score_at import evaluator, make_pairs, queries

pytestmark = pytest.mark.gpu

R, SEED = 257, 11
SCALES = 10                      # the default scales of rell_au
KINDS = ("score_at", "site_lnl", "marginal_like", "rell_support", "rell_tests", "rell_au")
# the call that follows each kind in the history check: marginal_like after a call that staged lengths and the reverse
FOLLOWER = {"score_at": "marginal_like", "site_lnl": "rell_au", "marginal_like": "rell_tests",
            "rell_support": "marginal_like", "rell_tests": "rell_au", "rell_au": "score_at"}
CASES = [(name, kind) for name in ("D5", "A4") for kind in KINDS]


@functools.lru_cache(maxsize=None)
def rule():
    r = epa.posterior_rule(0.05, Kx=3, Kp=5)
    for a in r:
        a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def host_input(name):
    """-> dict of host arrays: pairs, pen, dis, codes, wb, ws, sid"""
    if name == "D5":
        s = rr.stat_input()
        codes, wb, ws = epa.encode_queries(4, s["reads"], compact=True)
        assert len(ws) == 22 and np.all(np.asarray(ws) == rr.STAT_SPAN)
        pb, ps, pen, dis = s["branch"], s["seq"], s["pendant"], s["distal"]
    else:
        bf = bc.brute(name)
        codes, wb, ws = queries(name)
        pb, ps, pen, dis = entry_lists(bf.B, bf.lengths, [3] * len(ws))
    assert len(pb) == 3 * len(ws)
    a = dict(pairs=make_pairs(pb, ps), pen=np.ascontiguousarray(pen, dtype=np.float64),
             dis=np.ascontiguousarray(dis, dtype=np.float64), codes=codes, wb=wb, ws=ws,
             sid=np.arange(len(ws), dtype=np.uint64) + 5)
    for v in a.values():
        v.setflags(write=False)
    return a


def device_input(name):
    a = host_input(name)
    cu = lambda x, t: torch.from_numpy(np.array(x).view(t)).cuda()  # noqa: E731
    return dict(pairs=cu(a["pairs"], np.int32).reshape(-1, 2), pen=cu(a["pen"], np.float64), dis=cu(a["dis"], np.float64),
                codes=cu(a["codes"], np.uint8), wb=cu(a["wb"], np.int32), ws=cu(a["ws"], np.int32), sid=cu(a["sid"], np.int64))


def shapes(name, kind):
    """output name -> (shape, dtype), in the order of the C signature's output arguments"""
    a = host_input(name)
    n, pitch = len(a["pairs"]), int(np.max(a["ws"]))
    f = np.float64
    return {"score_at": {"lnl": ((n,), f)},
            "site_lnl": {"rows": ((n, pitch), f)},
            "marginal_like": {"M": ((n,), f), "grid": ((n, 3, 5), f)},
            "rell_support": {"support": ((n,), f)},
            "rell_tests": {"support": ((n,), f), "elw": ((n,), f), "p_sh": ((n,), f)},
            "rell_au": {"p_au": ((n,), f), "counts": ((SCALES, n), np.uint32), "fit": ((n, 2), f)}}[kind]


def buffers(name, kind, where):
    """where: output name -> "host" | "dev" (a name left out is not asked for) -> pre-filled buffers"""
    out = {}
    for key, (shape, dtype) in shapes(name, kind).items():
        if key not in where:
            continue
        if dtype == np.uint32:
            out[key] = (np.full(shape, 0xffffffff, np.uint32) if where[key] == "host" else
                        torch.full(shape, -1, dtype=torch.int32, device="cuda"))
        else:
            out[key] = (np.full(shape, np.nan) if where[key] == "host" else
                        torch.full(shape, float("nan"), dtype=torch.float64, device="cuda"))
    return out


def read(name, kind, out):
    """the buffers as host arrays of the outputs' own dtypes"""
    torch.cuda.synchronize()
    got = {}
    for key, buf in out.items():
        dtype = shapes(name, kind)[key][1]
        got[key] = np.array(buf if isinstance(buf, np.ndarray) else buf.cpu().numpy()).view(dtype)
    return got


def call(ev, kind, a, out):
    """one call of `kind` on inputs a into the buffers `out`: the Evaluator's method where it takes every output from the
    caller, else the C entry point"""
    n, Q = len(a["pairs"]), len(a["wb"])
    entries = (a["pairs"], a["pen"], a["dis"], a["codes"], a["wb"], a["ws"])
    if kind == "score_at":
        ev.score_at(*entries, out=out["lnl"])
    elif kind == "site_lnl":
        ev.site_lnl(*entries, pitch=out["rows"].shape[1], out=out["rows"])
    elif kind == "rell_support":
        ev.rell_support(*entries, R, seed=SEED, stream_id=a["sid"], out=out["support"])
    else:
        ev._layout(a["codes"])
        o = lambda key: _ptr(out.get(key))  # noqa: E731
        head = (ev.h, _ptr(a["pairs"]), _ptr(a["pen"]), _ptr(a["dis"]), None, n)
        query = (_ptr(a["codes"]), _ptr(a["wb"]), _ptr(a["ws"]), Q)
        if kind == "marginal_like":
            x, xw, p, pw = rule()
            ev._check(ev.L.epa_dev_marginal_like(ev.h, _ptr(a["pairs"]), n, _ptr(x), _ptr(xw), len(x), _ptr(p), _ptr(pw), len(p),
                                                 *query, o("M"), o("grid")))
        elif kind == "rell_tests":
            ev._check(ev.L.epa_dev_rell_tests(*head, *query, _ptr(a["sid"]), R, SEED, o("support"), o("elw"), o("p_sh")))
        else:
            ev._check(ev.L.epa_dev_rell_au(*head, *query, _ptr(a["sid"]), R, SEED, None, 0, o("p_au"), o("counts"), o("fit")))


def all_host(name, kind):
    return {key: "host" for key in shapes(name, kind)}


@functools.lru_cache(maxsize=None)
def expected(name, kind):
    """the outputs of the all-host call, computed once and never modified"""
    out = buffers(name, kind, all_host(name, kind))
    call(evaluator(name, "plain"), kind, host_input(name), out)
    got = read(name, kind, out)
    for key, v in got.items():
        v.setflags(write=False)
        if v.dtype == np.float64 and key != "fit":           # fit is NaN where the fallback applies
            assert np.all(np.isfinite(v)), (name, kind, key)
    return got


def check_with_history(name, kind, a, where):
    """the call with inputs a and the outputs placed as `where` gives the all-host bits; so do its buffers after a call
    of another member of the family, and so does the same call made again after that one"""
    ev = evaluator(name, "plain")
    want = {key: expected(name, kind)[key] for key in where}
    what = "%s %s %s" % (name, kind, sorted(where.items()))
    out = buffers(name, kind, where)
    call(ev, kind, a, out)
    assert_same(read(name, kind, out), want, what)
    other = FOLLOWER[kind]
    follow = buffers(name, other, all_host(name, other))
    call(ev, other, host_input(name), follow)
    assert_same(read(name, other, follow), expected(name, other), what + ", then " + other)
    assert_same(read(name, kind, out), want, what + ", read again after " + other)
    again = buffers(name, kind, where)
    call(ev, kind, a, again)
    assert_same(read(name, kind, again), want, what + ", called again after " + other)


@pytest.mark.parametrize("name,kind", CASES, ids=["%s-%s" % c for c in CASES])
def test_same_call_different_memory(name, kind):
    check_with_history(name, kind, device_input(name), {key: "dev" for key in shapes(name, kind)})


MIXED = [("rell_tests", dict(support="dev", elw="host", p_sh="host")),
         ("rell_au", dict(counts="dev", p_au="host", fit="host")),
         ("rell_au", dict(fit="host")),
         ("marginal_like", dict(M="dev", grid="host"))]


@pytest.mark.parametrize("name", ["D5", "A4"])
@pytest.mark.parametrize("kind,where", MIXED, ids=["%s-%s" % (k, "+".join("%s_%s" % kv for kv in sorted(w.items()))) for k, w in MIXED])
def test_mixed_outputs(name, kind, where):
    check_with_history(name, kind, host_input(name), where)
    if kind == "rell_au" and len(where) == 1:
        # the comparison is not one of fallback values only
        assert np.any(np.isfinite(expected(name, kind)["fit"]))
