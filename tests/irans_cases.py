"""The cases that pin the irans32 device coder (csrc/rans_gpu.hip) to its definition tools/irans_ref.py at
production lane counts: table sets, symbol streams and decoder piece plans, all deterministic from seeds.  No GPU and no torch
device use here; tests/test_irans_cases_host.py checks on the reference alone that the cases hold what they claim, and
tests/test_gpu_irans_domain.py runs them through the kernels.

Domain.  The cases keep |sym - offset| < 2^30 (escape magnitudes k < 2^29, so raw = 2k or 2k + 1 < 2^30 and still reaches
the eight-digit class raw >= 2^28).  The coder's stated domain is |sym - offset| < 2^31: beyond it the 32-bit ``raw`` of an
escape wraps, in the reference as in the kernel, and the symbol does not come back.

Table sets are (cdf rows, sizes, offsets) as tools/irans_ref.py takes them: rows are lists of Python ints, all of the set's
stride (short rows zero-padded), so the same object feeds the reference and, through ``arrays``, the device tables.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import irans_ref as R  # noqa: E402

TABLE_SETS = ("gaussian", "ladder0", "ladder32", "edge")
PATTERNS = ("none", "sparse", "dense", "all", "lanes", "magnitudes")
PLANS = ("whole", "tiny", "round_edges", "at_escapes")
N32 = 131109                     # K = 32, not a multiple of 32: the last round is short
MAX_K = 1 << 29                  # escape magnitudes k < MAX_K: |sym - offset| < 2^30

# the edge set's rows as frequency lists, the escape slot last
EDGE_ESCAPE_ONLY, EDGE_BIG_ONE, EDGE_ONE_BIG, EDGE_ONES, EDGE_POW2, EDGE_RANDOM, EDGE_BUCKETS = range(7)
EDGE_OFFSETS = [5, 0, -1, -127, 3, -150, 17]


def _edge_freqs():
    g = np.random.default_rng(950)
    rnd = g.integers(1, 400, 300).tolist()
    rnd[0] = 65536 - sum(rnd[1:])                                       # the remainder on slot 0
    assert rnd[0] >= 1
    return [[65536],                                                    # escape only: sizes == 2, freq == 65536
            [65535, 1],                                                 # the dearest escape slot
            [1, 65535],                                                 # the dearest regular slot
            [1] * 255 + [65536 - 255],
            [1 << k for k in range(15, -1, -1)] + [1],                  # 32768 ... 2, 1, 1
            rnd,                                                        # odd and even frequencies; the widest row
            [255, 257] * 127 + [255, 256, 1]]                           # every slot boundary 1 off a multiple of 256


def _pad(rows):
    w = max(len(r) for r in rows)
    return [[int(v) for v in r] + [0] * (w - len(r)) for r in rows]


@functools.lru_cache(maxsize=None)
def tables(name):
    """-> (cdf rows, sizes, offsets) of one of TABLE_SETS."""
    if name == "gaussian":
        from test_irans_host import _gaussian_tables
        cdf, sizes, offs, _ = _gaussian_tables()
    elif name in ("ladder0", "ladder32"):
        from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import residual
        t = residual.tables(int(name[6:]))
        cdf, sizes, offs = t.cdf.tolist(), t.sizes.tolist(), t.offsets.tolist()
    elif name == "edge":
        freqs = _edge_freqs()
        cdf = [np.concatenate([[0], np.cumsum(f)]).tolist() for f in freqs]
        sizes, offs = [len(f) + 1 for f in freqs], list(EDGE_OFFSETS)
        assert all(r[-1] == 65536 for r in cdf) and max(sizes) == max(len(r) for r in cdf)   # the widest row fills the stride
    else:
        raise ValueError(name)
    return _pad(cdf), [int(v) for v in sizes], [int(v) for v in offs]


def arrays(tabs):
    """(cdf (ncdf, stride), sizes, offsets) int32 arrays of a table set, as irans.DeviceTables takes them."""
    return tuple(np.asarray(a, dtype=np.int32) for a in tabs)


def escapes(tabs, sym, idx):
    """Boolean array: symbol i codes the escape slot of its row."""
    _, sizes, offs = tabs
    idx = np.asarray(idx)
    v = np.asarray(sym, dtype=np.int64) - np.asarray(offs, dtype=np.int64)[idx]
    return (v < 0) | (v >= np.asarray(sizes, dtype=np.int64)[idx] - 2)


def escape_raw(tabs, sym, idx):
    """The 32-bit raw value of every symbol (0 where it does not escape), as irans_ref.codes computes it."""
    _, sizes, offs = tabs
    idx = np.asarray(idx)
    v = np.asarray(sym, dtype=np.int64) - np.asarray(offs, dtype=np.int64)[idx]
    maxv = np.asarray(sizes, dtype=np.int64)[idx] - 2
    return np.where(v < 0, -2 * v - 1, np.where(v >= maxv, 2 * (v - maxv), 0)) & 0xFFFFFFFF


def digits(raw):
    """nb of a raw value: the number of 4-bit digits the escape codes after its count digit."""
    raw = np.asarray(raw, dtype=np.int64)
    nb = np.zeros(raw.shape, dtype=np.int64)
    for k in range(8):
        nb += (raw >> (4 * k)) != 0
    return nb


# the raw values the ``magnitudes`` pattern cycles through: raw == 0 (nb == 0: the symbol exactly at offset + max_value),
# then for every nb in 1..8 and both parities (odd: negative symbol, even: positive) the lowest and the highest raw of that
# digit count.  That holds 0xF | 0x10 and 0xFFFFFFF | 0x10000000, where the digit count changes; nb == 8 ends at the domain.
def magnitude_raws():
    out = [0]
    for nb in range(1, 9):
        lo, hi = 1 << (4 * (nb - 1)), min(1 << (4 * nb), 2 * MAX_K) - 1
        for parity in (1, 0):
            a = lo if lo & 1 == parity else lo + 1
            b = hi if hi & 1 == parity else hi - 1
            out += [a, b, (a, b)]                                       # (a, b): a random one of that parity in between
    return out


def _lane_mask(n, K):
    """The ``lanes`` pattern's escape mask and, per round, the structure it was given (a name or "")."""
    rounds = (n + K - 1) // K
    m = np.zeros(rounds * K, dtype=bool).reshape(rounds, K)
    kind = [""] * rounds
    for r in range(rounds):
        c = r % 8
        if c == 0:
            m[r, 0], kind[r] = True, "first"
        elif c == 2:
            m[r, K - 1], kind[r] = True, "last"
        elif c == 3 and K > 1:
            e = (r // 8) % (K - 1)
            m[r, e] = m[r, e + 1] = True
            kind[r] = "pair"
        elif c in (4, 6):
            m[r, :], kind[r] = True, "every"
        else:
            kind[r] = "free"                                            # 1, 5, 7: escape-free, so 4..7 alternate
    m = m.reshape(-1)[:n].copy()
    m[0] = m[n - 1] = True                                              # the stream's first and last symbols escape
    return m, kind


def stream(tabs, n, pattern, seed):
    """-> (sym, idx): lists of n Python ints.  Rows are drawn uniformly, but a symbol that is not to escape gets a row with a
    regular slot (the escape-only row codes nothing else; it takes a quarter of the escapes instead), so every row is used
    and ``none`` uses every row but that one.  Regular symbols are
    drawn half from the row's own distribution and half uniformly over its regular slots (so slots of frequency 1 are hit);
    escapes are exactly the pattern's mask."""
    cdf, sizes, offs = tabs
    g = np.random.default_rng([seed, n, PATTERNS.index(pattern)])
    maxv = np.asarray(sizes, dtype=np.int64) - 2
    offs = np.asarray(offs, dtype=np.int64)
    K = R.lanes(n)
    if pattern == "none":
        esc = np.zeros(n, dtype=bool)
    elif pattern == "sparse":
        esc = g.integers(0, 200, n) == 0
    elif pattern == "dense":
        esc = g.random(n) < 0.3
    elif pattern == "all":
        esc = np.ones(n, dtype=bool)
    elif pattern == "lanes":
        esc = _lane_mask(n, K)[0]
    elif pattern == "magnitudes":
        esc = g.integers(0, 8, n) == 0
    else:
        raise ValueError(pattern)
    idx = g.integers(0, len(sizes), n)
    regular = np.flatnonzero(maxv > 0)
    fix = ~esc & (maxv[idx] == 0)
    idx[fix] = regular[g.integers(0, regular.size, int(fix.sum()))]
    only = np.flatnonzero(maxv == 0)
    if only.size:                                                       # and a quarter of the escapes go to it: sparse hits it too
        move = esc & (g.integers(0, 4, n) == 0)
        idx[move] = only[g.integers(0, only.size, int(move.sum()))]
    sym = np.zeros(n, dtype=np.int64)
    for r in regular:
        p = np.flatnonzero(~esc & (idx == r))
        row = np.asarray(cdf[r][:maxv[r] + 1], dtype=np.int64)
        own = np.searchsorted(row, g.integers(0, row[-1], p.size), side="right") - 1
        flat = g.integers(0, maxv[r], p.size)
        sym[p] = np.where(g.integers(0, 2, p.size) == 0, own, flat) + offs[r]
    p = np.flatnonzero(esc)
    if pattern == "magnitudes":
        raws = magnitude_raws()
        raw = np.zeros(p.size, dtype=np.int64)
        for j, want in enumerate(raws):
            q = np.arange(j, p.size, len(raws))
            if isinstance(want, tuple):
                raw[q] = want[0] + 2 * g.integers(0, (want[1] - want[0]) // 2 + 1, q.size)
            else:
                raw[q] = want
        neg, k = raw & 1 == 1, raw >> 1
    else:
        small = g.integers(0, 10, p.size) != 0
        k = np.where(small, g.integers(0, 8, p.size), g.integers(0, 1 << g.integers(0, 30, p.size)))
        neg = g.integers(0, 2, p.size) == 1
    sym[p] = np.where(neg, -1 - k, maxv[idx[p]] + k) + offs[idx[p]]
    assert int(np.abs(sym - offs[idx]).max(initial=0)) < 1 << 30
    return sym.tolist(), idx.tolist()


def pieces(n, K, kind, seed, esc=None):
    """-> the cut points [0, ..., n] of a split of [0, n) into consecutive decoder pieces.  ``at_escapes`` needs esc, the
    stream's escape mask."""
    g = np.random.default_rng([seed, n, PLANS.index(kind)])
    cuts, head = [0], min(n, 64 * K)
    if kind == "whole":
        return [0, n]
    if kind == "tiny":
        while cuts[-1] < head:
            cuts.append(cuts[-1] + int(g.integers(1, 8)))
    elif kind == "round_edges":
        steps, j = (K - 1, K, K + 1, 1), 0
        while cuts[-1] < head:
            cuts.append(cuts[-1] + max(1, steps[j % 4]))
            j += 1
    elif kind == "at_escapes":
        for e in np.flatnonzero(esc)[:200].tolist():
            cuts += [c for c in (e, e + 1) if c > cuts[-1]]
    else:
        raise ValueError(kind)
    while cuts[-1] < n:
        cuts.append(cuts[-1] + int(g.integers(1, 5001)))
    cuts = [c for c in cuts if c < n] + [n]
    assert len(cuts) < 2000 and all(b > a for a, b in zip(cuts, cuts[1:]))
    return cuts


@functools.lru_cache(maxsize=None)
def case(tset, pattern, n, seed):
    """-> (sym, idx, the reference's stream) of one case, computed once per process and shared; treat as read-only."""
    tabs = tables(tset)
    sym, idx = stream(tabs, n, pattern, seed)
    return sym, idx, R.encode(sym, idx, *tabs)


def worst_case(n):
    """The format's dearest stream: every symbol -2^31 on the edge set's row [65535, 1] (an escape slot of frequency 1, a count
    digit and eight digits: 16 + 4 + 32 bits = 6.5 bytes per symbol).  Outside the stated domain; used for its size only."""
    return [-(1 << 31)] * n, [EDGE_BIG_ONE] * n
