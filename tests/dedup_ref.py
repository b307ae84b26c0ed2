"""Restatement of "Duplicate queries" (include/epa_dev.h) in numpy and a dict, and the inputs of the dedup tests.

Two queries of a chunk are identical when win_begin, win_span and the codes of the win_span window positions are equal;
nothing else of a row is looked at.  Classes are numbered in order of first appearance: first[u] is the smallest query
of class u, rep[q] the class of query q.  dedup() reaches that by keying a dict on (begin, span, bytes(window codes));
window_codes() decodes the three layouts itself:

  full-width   codes [Q][W]: the window of query q is columns win_begin[q] .. win_begin[q] + win_span[q] - 1
  compact      codes [Q][stride], stride != W: the window is columns 0 .. win_span[q] - 1
  4-bit        Packed(data [Q][(len + 1) // 2], len): two codes per byte, the earlier one in the high nibble, rows of
               len = W (full-width) or len = stride (compact) codes

Nothing here touches the device or the library."""
import collections

import numpy as np

Packed = collections.namedtuple("Packed", "data stride")   # the fields of epa_ng_amd.Packed4


def window_codes(codes, win_begin, win_span, W):
    """-> list of Q uint8 arrays: the codes of every query's window, whatever the layout"""
    packed = hasattr(codes, "stride")
    data = np.asarray(codes.data if packed else codes)
    row_len = int(codes.stride) if packed else int(data.shape[1])
    out = []
    for q in range(len(win_begin)):
        b, n = int(win_begin[q]), int(win_span[q])
        assert b + n <= W and n <= row_len
        c0 = b if row_len == W else 0
        cols = np.arange(c0, c0 + n)
        if packed:
            byte = data[q, cols // 2]
            out.append(np.where(cols % 2 == 0, byte >> 4, byte & 15).astype(np.uint8))
        else:
            out.append(np.array(data[q, cols], np.uint8))
    return out


def dedup(codes, win_begin, win_span, W):
    """-> (rep uint32 [Q], first uint32 [n_unique])"""
    classes = {}
    rep, first = [], []
    for q, w in enumerate(window_codes(codes, win_begin, win_span, W)):
        key = (int(win_begin[q]), int(win_span[q]), w.tobytes())
        if key not in classes:
            classes[key] = len(first)
            first.append(q)
        rep.append(classes[key])
    return np.array(rep, np.uint32), np.array(first, np.uint32)


def check_invariants(rep, first):
    """first strictly increasing, rep[first[u]] == u, rep covers exactly the classes, no query before its class's first"""
    rep, first = np.asarray(rep, np.int64), np.asarray(first, np.int64)
    assert np.all(np.diff(first) > 0)
    assert np.array_equal(rep[first], np.arange(len(first)))
    if len(rep):
        assert rep.min() == 0 and rep.max() == len(first) - 1
        assert np.all(first[rep] <= np.arange(len(rep)))


def pack4(rows):
    """[Q][len] codes 0 .. 15 -> [Q][(len + 1) // 2] bytes, the earlier code in the high nibble, pad nibble 0"""
    rows = np.asarray(rows, np.uint8)
    assert rows.max(initial=0) < 16
    if rows.shape[1] & 1:
        rows = np.concatenate([rows, np.zeros((len(rows), 1), np.uint8)], axis=1)
    return ((rows[:, 0::2] << 4) | rows[:, 1::2]).astype(np.uint8)


def layouts(windows, W, stride, four_bit, fill=0, seed=0):
    """windows: list of (begin, uint8 codes of the window).  -> dict name -> (codes, win_begin, win_span): "full",
    "compact" and, with four_bit (codes 0 .. 15), "packed" (compact) and "packed_full" (full-width), all of the same
    queries.  Everything OUTSIDE the windows -- the columns around a full-width window, the bytes from span to stride,
    the pad nibble of an odd row -- is filled per row by `fill`: an int (0 .. 255: that byte, or its low nibble), or
    "random"; a list gives one such fill per row."""
    Q = len(windows)
    rng = np.random.RandomState(seed)
    fills = fill if isinstance(fill, (list, tuple)) else [fill] * Q
    top = 16 if four_bit else 256
    assert stride != W and all(len(w) <= stride and b + len(w) <= W for b, w in windows)
    wb = np.array([b for b, _ in windows], np.uint32)
    ws = np.array([len(w) for _, w in windows], np.uint32)

    def blank(q, n):
        f = fills[q]
        return rng.randint(0, top, n).astype(np.uint8) if f == "random" else np.full(n, int(f) % top, np.uint8)

    Wp, Sp = W + (W & 1), stride + (stride & 1)   # with the pad nibble of an odd 4-bit row
    full = np.stack([blank(q, Wp) for q in range(Q)]) if Q else np.zeros((0, Wp), np.uint8)
    comp = np.stack([blank(q, Sp) for q in range(Q)]) if Q else np.zeros((0, Sp), np.uint8)
    for q, (b, w) in enumerate(windows):
        full[q, b:b + len(w)] = w
        comp[q, :len(w)] = w
    out = {"full": (np.ascontiguousarray(full[:, :W]), wb, ws), "compact": (np.ascontiguousarray(comp[:, :stride]), wb, ws)}
    if four_bit:
        out["packed"] = (Packed(pack4(comp), stride), wb, ws)
        out["packed_full"] = (Packed(pack4(full), W), wb, ws)
    return out


# ---- class structures of the GPU tests: which distinct row every query is ------------------------------------------------
STRUCTURES = ("identical", "distinct", "blocks", "interleaved", "skewed")


def structure(name, Q, seed=0):
    """-> int array [Q]: the id of the distinct row query q carries"""
    q = np.arange(Q)
    if name == "identical":
        return np.zeros(Q, np.int64)
    if name == "distinct":
        return q
    if name == "blocks":            # AAAA BBBB ...
        return q // 4
    if name == "interleaved":       # ABAB ... over max(2, Q / 8) rows
        return q % max(2, Q // 8)
    if name == "skewed":            # one class of 90 % of the chunk plus singletons, shuffled
        ids = np.where(q < (9 * Q) // 10, 0, q)
        return ids[np.random.RandomState(seed).permutation(Q)]
    raise ValueError(name)


def distinct_windows(n, W, spans, top, seed):
    """n pairwise different (begin, codes) windows: row i has span spans[i % len(spans)] (at least 8), a begin of parity
    i & 1 where the alignment leaves room, random codes below `top`, and i written into its first eight codes in base 4
    (codes 1 .. 4), which makes the rows of one (begin, span) differ"""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        s = int(spans[i % len(spans)])
        assert 8 <= s <= W and i < 4 ** 8
        par = i & 1 if W - s >= 1 else 0
        b = par + 2 * rng.randint((W - s - par) // 2 + 1)
        w = rng.randint(0, top, s).astype(np.uint8)
        w[:8] = [1 + (i >> (2 * k)) % 4 for k in range(8)]
        out.append((b, w))
    return out
