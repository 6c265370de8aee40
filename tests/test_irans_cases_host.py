"""CPU: the cases of tests/irans_cases.py, checked through the definition tools/irans_ref.py alone -- every (table set,
pattern) round-trips at K = 32 and holds the structures it claims (the floors below keep a GPU test from passing on an empty
case; they are not measurements); three deliberately wrong coders are told from the right one by the cases meant to catch
them -- and the library's host helpers of the device coder: the reciprocal table, the decoder's LUT, the capacity bound."""
import bisect
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import irans_cases as IC  # noqa: E402
from irans_cases import R  # noqa: E402

from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import _lib  # noqa: E402

N = IC.N32
SEED = 1


def _rounds(mask, K):
    """(rounds, K) boolean view of a per-symbol mask, the short last round padded with False."""
    m = np.zeros(-(-mask.size // K) * K, dtype=bool)
    m[:mask.size] = mask
    return m.reshape(-1, K)


# ------------------------------------------------------------------------------------------------ 1. the cases
@pytest.mark.parametrize("pattern", IC.PATTERNS)
@pytest.mark.parametrize("tset", IC.TABLE_SETS)
def test_case_round_trips_and_holds_what_it_claims(tset, pattern):
    tabs = IC.tables(tset)
    cdf, sizes, offs = tabs
    sym, idx, st = IC.case(tset, pattern, N, SEED)
    K = R.lanes(N)
    assert K == 32 and len(sym) == len(idx) == N
    assert R.decode(st, idx, *tabs) == sym
    esc = IC.escapes(tabs, sym, idx)
    v = np.asarray(sym, dtype=np.int64) - np.asarray(offs, dtype=np.int64)[idx]
    assert int(np.abs(v).max()) < 1 << 30                               # the cases' domain
    hits = np.bincount(idx, minlength=len(sizes))
    usable = np.asarray(sizes) > 2 if pattern == "none" else np.ones(len(sizes), dtype=bool)   # escape-only row: escapes only
    assert int(hits[usable].min()) >= 100 and int(hits[~usable].sum()) == 0, hits.tolist()
    per_round = _rounds(esc, K).sum(1)
    if pattern == "none":
        assert not esc.any()
    elif pattern == "sparse":
        assert N // 400 <= int(esc.sum()) <= N // 100
    elif pattern == "dense":
        assert int((per_round >= 2).sum()) * 2 >= per_round.size
    elif pattern == "all":
        assert esc.all()
    elif pattern == "lanes":
        m = _rounds(esc, K)[:-1]                                        # the short last round aside
        one = m.sum(1) == 1
        pair = (m.sum(1) == 2) & (m[:, :-1] & m[:, 1:]).any(1)
        every, free = m.all(1), ~m.any(1)
        assert int((one & m[:, 0]).sum()) >= 16 and int((one & m[:, K - 1]).sum()) >= 16
        assert int(pair.sum()) >= 16 and len(set(np.argmax(m[pair], 1).tolist())) == K - 1      # every e in 0..K-2
        assert int((every[:-1] & free[1:]).sum()) >= 16 and int((free[:-1] & every[1:]).sum()) >= 16
        assert esc[0] and esc[-1]
    elif pattern == "magnitudes":
        raw = IC.escape_raw(tabs, sym, idx)[esc]
        nb = IC.digits(raw)
        for k in range(1, 9):
            for parity in (0, 1):                                       # even: positive symbol, odd: negative
                assert int(((nb == k) & (raw & 1 == parity)).sum()) >= 8, (k, parity)
        assert int((raw == 0).sum()) >= 8                               # nb == 0: the positive boundary symbol only
        for want in (0xF, 0x10, 0xFFFFFFF, 0x10000000):
            assert int((raw == want).sum()) >= 8, hex(want)
    if tset == "edge" and pattern != "none":
        i = np.asarray(idx)
        for r in (IC.EDGE_BIG_ONE, IC.EDGE_ONE_BIG):
            assert (esc & (i == r)).any() and (pattern == "all" or (~esc & (i == r)).any())


def test_the_edge_set_holds_the_arithmetic_edges():
    cdf, sizes, offs = IC.tables("edge")
    freqs = [np.diff(cdf[r][:sizes[r]]) for r in range(len(sizes))]
    allf = np.concatenate(freqs)
    assert allf.min() == 1 and allf.max() == 65536 and sizes[IC.EDGE_ESCAPE_ONLY] == 2
    assert max(sizes) == len(cdf[0])                                    # the widest row fills the stride
    pow2 = (allf & (allf - 1)) == 0
    assert pow2.any() and (~pow2 & (allf & 1 == 1)).any() and (~pow2 & (allf & 1 == 0)).any()
    edges = np.asarray(cdf[IC.EDGE_BUCKETS][1:sizes[IC.EDGE_BUCKETS] - 1])
    # boundaries at 256 b - 1 and 256 b alternately: cum = 256 b - 1, 256 b and 256 b + 1 fall in up to three slots, every b
    assert set(((edges + 1) // 256).tolist()) >= set(range(1, 256)) and set((edges % 256).tolist()) == {0, 255}
    assert min(offs) < 0 and 0 in offs and max(offs) > 0


def test_piece_plans():
    K = 32
    esc = IC.escapes(IC.tables("edge"), *IC.case("edge", "lanes", N, SEED)[:2])
    for kind in IC.PLANS:
        cuts = IC.pieces(N, K, kind, 3, esc)
        assert cuts[0] == 0 and cuts[-1] == N and len(cuts) < 2000
        d = np.diff(cuts)
        assert d.min() >= 1
        head = d[np.asarray(cuts[:-1]) < 64 * K - 8]
        if kind == "whole":
            assert cuts == [0, N]
        elif kind == "tiny":
            assert head.max() <= 7 and set(head.tolist()) == set(range(1, 8))
            a, b = np.asarray(cuts[:-1]) % K, np.asarray(cuts[1:]) - np.asarray(cuts[:-1]) // K * K
            assert int(((a > 0) & (b < K)).sum()) >= 100                # pieces that start and end inside one round
        elif kind == "round_edges":
            assert set(head.tolist()) == {K - 1, K, K + 1, 1}
        elif kind == "at_escapes":
            first = np.flatnonzero(esc)[:200]
            assert set(first.tolist()) <= set(cuts) and set((first + 1).tolist()) <= set(cuts)


# ------------------------------------------------------------------------------------------------ 2. wrong coders
def _encode_two_phase(symbols, indexes, cdf, sizes, offsets):
    """The byte order DESIGN.md 7.1.2 rejects: per round of K symbols all regular codes, then the escaped lanes' bypass digits
    (the encoder being the reverse).  irans_ref.encode otherwise."""
    n = len(symbols)
    K = R.lanes(n)
    x = [R.RANS_L] * K
    stack = bytearray()

    def put(j, start, freq):
        s = x[j]
        x_max = ((R.RANS_L >> R.PREC) << 8) * freq
        while s >= x_max:
            stack.append(s & 0xFF)
            s >>= 8
        x[j] = ((s // freq) << R.PREC) + (s % freq) + start
    for r0 in range((n - 1) // K * K, -1, -K):
        cs = [(i % K, R.codes(symbols[i], int(indexes[i]), cdf, sizes, offsets)) for i in range(min(n, r0 + K) - 1, r0 - 1, -1)]
        for j, c in cs:
            for start, freq in reversed(c[1:]):
                put(j, start, freq)
        for j, c in cs:
            put(j, *c[0])
    return b"".join(struct.pack("<I", v) for v in x) + bytes(reversed(stack))


def _wrong(variant, monkeypatch, sym, idx, tabs):
    """The bytes of a deliberately wrong coder: 'cap16' (lanes capped at 16), 'neg' (negative escapes coded as raw = -2 v, not
    -2 v - 1) or 'two_phase'."""
    if variant == "two_phase":
        return _encode_two_phase(sym, idx, *tabs)
    with monkeypatch.context() as m:
        if variant == "cap16":
            m.setattr(R, "MAX_LANES", 16)
        else:
            codes = R.codes

            def wrong_codes(s, ci, cdf, sizes, offsets):
                v = int(s) - int(offsets[ci])
                # raw = -2 v is what the positive symbol max_value - v codes
                return codes(int(offsets[ci]) + int(sizes[ci]) - 2 - v if v < 0 else s, ci, cdf, sizes, offsets)
            m.setattr(R, "codes", wrong_codes)
        return R.encode(sym, idx, *tabs)


SMALL = (4095, 8192, 65537, 131071)                                     # K = 1, 2, 16, 16


def test_the_two_phase_order_is_the_reference_without_escapes():
    tabs = IC.tables("edge")
    for n, pattern in ((8192, "none"), (N, "none")):
        sym, idx, st = IC.case("edge", pattern, n, SEED)
        assert _encode_two_phase(sym, idx, *tabs) == st


CATCHES = {"cap16": ("dense", "none"),                                  # K = 32: any case catches it
           "neg": ("magnitudes", "dense"),                              # cases with negative escapes
           "two_phase": ("lanes", "dense")}                             # rounds with escapes before other lanes' bytes


@pytest.mark.parametrize("tset", IC.TABLE_SETS)
def test_wrong_coders_are_told_from_the_right_one(tset, monkeypatch):
    tabs = IC.tables(tset)
    for variant, patterns in CATCHES.items():
        for pattern in patterns:
            sym, idx, st = IC.case(tset, pattern, N, SEED)
            assert _wrong(variant, monkeypatch, sym, idx, tabs) != st, (variant, pattern)
    sym, idx, st = IC.case(tset, "none", N, SEED)                       # without escapes only the lane count shows
    assert _wrong("two_phase", monkeypatch, sym, idx, tabs) == st and _wrong("neg", monkeypatch, sym, idx, tabs) == st
    assert R.MAX_LANES == 32 and R.encode(sym, idx, *tabs) == st        # the reference is itself again


def test_capped_lanes_agree_below_131072():
    tabs = IC.tables("edge")
    for n in SMALL:
        sym, idx, st = IC.case("edge", "dense", n, SEED)
        with pytest.MonkeyPatch.context() as m:
            m.setattr(R, "MAX_LANES", 16)
            assert R.encode(sym, idx, *tabs) == st, n


# ------------------------------------------------------------------------------------------------ 3. host helpers
def test_rcp_table_divides_exactly():
    """For every f in [2, 65536]: ((x * rcp[f]) >> 32) >> (ceil(log2 f) - 1) == x // f at the edges of the encoder's range
    (x < 2^31; (f << 15) - 1 is the largest state the encoder ever divides)."""
    rcp = np.zeros(65537, dtype=np.uint32)
    _lib.check(_lib.load().lldwt_irans_rcp_table(rcp.ctypes.data_as(C.c_void_p)), "irans_rcp_table")
    assert rcp[0] == 0 and rcp[1] == 0
    f = np.arange(2, 65537, dtype=np.uint64)
    r = rcp[2:].astype(np.uint64)
    shift = np.ceil(np.log2(f.astype(np.float64))).astype(np.uint64)
    assert ((np.uint64(1) << shift) >= f).all() and ((np.uint64(1) << (shift - np.uint64(1))) < f).all()
    top = np.uint64((1 << 31) - 1)
    kmax = top // f                                                     # the largest k with k f < 2^31 (2^31 - 1 itself counts)
    xs = [np.zeros_like(f), np.ones_like(f), f - np.uint64(1), f, f + np.uint64(1), (f << np.uint64(15)) - np.uint64(1),
          np.full_like(f, top)]
    for d in range(3):
        k = np.maximum(kmax - np.uint64(d), np.uint64(1))
        xs += [k * f - np.uint64(1), k * f]
    for x in xs:
        assert int(x.max()) < 1 << 31
        got = ((x * r) >> np.uint64(32)) >> (shift - np.uint64(1))
        bad = np.flatnonzero(got != x // f)
        assert bad.size == 0, (int(f[bad[0]]), int(x[bad[0]]), int(got[bad[0]]))


@pytest.mark.parametrize("tset", IC.TABLE_SETS)
def test_lut_is_its_definition(tset):
    """lut[r][b] = the largest slot s <= max_value with cdf[r][s] <= 256 b, b in 0..256."""
    cdf, sizes, offs = IC.arrays(IC.tables(tset))
    cdf = np.ascontiguousarray(cdf)
    lut = np.full((cdf.shape[0], 257), -9, dtype=np.int32)
    pv = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(_lib.load().lldwt_irans_lut(pv(cdf), cdf.shape[0], cdf.shape[1], pv(sizes), pv(lut)), "irans_lut")
    rows = IC.tables(tset)[0]
    for r in range(cdf.shape[0]):
        maxv = int(sizes[r]) - 2
        want = [bisect.bisect_right(rows[r], 256 * b, 0, maxv + 1) - 1 for b in range(257)]
        assert lut[r].tolist() == want, r


@pytest.mark.parametrize("n", [1, 4096, 8192])
def test_worst_case_stream_fits_the_capacity(n):
    """No symbol costs more than 16 + 4 + 32 bits = 6.5 bytes (an escape slot of frequency 1, one count digit, eight digits),
    so capacity 8 n + 144 covers every stream of valid tables."""
    sym, idx = IC.worst_case(n)
    st = R.encode(sym, idx, *IC.tables("edge"))
    cap = int(_lib.load().lldwt_irans_capacity(n))
    assert cap == 8 * n + 144
    assert len(st) <= cap
    # 6.5 n and the rounding of x / freq (under 0.01 bit per code), the K final states, and the states' start at 2^23
    assert len(st) <= 6.51 * n + 4 * R.lanes(n) + 8
    assert len(st) >= 6.4 * n                                           # and this stream does cost the maximum
