"""Pure-Python definition of the interleaved rANS stream format (coder ``irans32``).

This module is the normative statement of the format: the HIP coder (csrc/rans_gpu.hip) must write the bytes
``encode`` writes and pop the symbols ``Decoder`` pops.  It is slow (one Python step per code) and is used by the tests and
as the specification, never by the package.

Tables are compressai's: cdf (ncdf, stride) int32 rows of 16-bit cumulative frequencies, sizes[i] = used entries of row i
(max_value = sizes[i] - 2 is the escape slot), offsets[i] = symbol value of slot 0.
"""
import bisect
import struct

PREC = 16                      # CDF precision (bits)
RANS_L = 1 << 23               # lower bound of a lane state; states live in [L, 2^31)
BYPASS_BITS = 4
BYPASS_FREQ = 1 << (PREC - BYPASS_BITS)
MAX_BYPASS = (1 << BYPASS_BITS) - 1
MAX_BYPASS_DIGITS = 8          # 32 bits of raw value; more digits in a stream is a corrupt stream
MAX_LANES = 32


def lanes(n):
    """K = clamp(2^floor(log2(n / 4096)), 1, 32): the number of lanes of a stream of n symbols."""
    q = n >> 12
    if q < 2:
        return 1
    return min(MAX_LANES, 1 << (q.bit_length() - 1))


def codes(sym, ci, cdf, sizes, offsets):
    """The (start, freq) codes of one symbol in decoding order: the regular code, then (escape) the bypass digits."""
    row = cdf[ci]
    max_value = int(sizes[ci]) - 2
    value = int(sym) - int(offsets[ci])
    raw = 0
    if value < 0:
        raw = (-2 * value - 1) & 0xFFFFFFFF
        value = max_value
    elif value >= max_value:
        raw = (2 * (value - max_value)) & 0xFFFFFFFF
        value = max_value
    out = [(int(row[value]), int(row[value + 1]) - int(row[value]))]
    if value == max_value:
        nb = 0
        while nb * BYPASS_BITS < 32 and (raw >> (nb * BYPASS_BITS)) != 0:
            nb += 1
        v = nb
        while v >= MAX_BYPASS:
            out.append((MAX_BYPASS << 12, BYPASS_FREQ))
            v -= MAX_BYPASS
        out.append((v << 12, BYPASS_FREQ))
        for j in range(nb):
            out.append((((raw >> (j * BYPASS_BITS)) & MAX_BYPASS) << 12, BYPASS_FREQ))
    return out


def encode(symbols, indexes, cdf, sizes, offsets):
    """symbols, indexes: sequences of n ints -> stream bytes.  Symbol i goes to lane i mod K; the symbols are coded from
    last to first, each symbol's codes from last to first, renormalisation bytes pushed on one shared stack."""
    n = len(symbols)
    K = lanes(n)
    x = [RANS_L] * K
    stack = bytearray()
    for i in range(n - 1, -1, -1):
        j = i % K
        s = x[j]
        for start, freq in reversed(codes(symbols[i], int(indexes[i]), cdf, sizes, offsets)):
            x_max = ((RANS_L >> PREC) << 8) * freq
            while s >= x_max:
                stack.append(s & 0xFF)
                s >>= 8
            s = ((s // freq) << PREC) + (s % freq) + start
        x[j] = s
    return b"".join(struct.pack("<I", v) for v in x) + bytes(reversed(stack))


class CorruptStream(ValueError):
    pass


class Decoder:
    """Pops symbols in coding order; ``pop(indexes)`` may be called with any split of [0, n) into consecutive ranges."""

    def __init__(self, stream, n, cdf, sizes, offsets):
        self.buf, self.n = bytes(stream), n
        self.cdf, self.sizes, self.offsets = cdf, sizes, offsets
        self.K = lanes(n)
        self.bad = len(self.buf) < 4 * self.K
        self.x = [struct.unpack_from("<I", self.buf, 4 * j)[0] if not self.bad else 0 for j in range(self.K)]
        self.cur = 4 * self.K
        self.pos = 0

    def _byte(self):
        if self.cur >= len(self.buf):
            self.bad = True
            return 0
        b = self.buf[self.cur]
        self.cur += 1
        return b

    def _code(self, j, start, freq):
        s = self.x[j]
        s = (freq * (s >> PREC) + (s & 0xFFFF) - start) & 0xFFFFFFFF     # 32-bit arithmetic, as the kernel
        if s < 1 << 7:                          # a valid stream never goes below 2^7 here (at most two bytes follow)
            raise CorruptStream("corrupt stream (state underflow)")
        while s < RANS_L:
            s = (s << 8) | self._byte()
        self.x[j] = s

    def _digit(self, j):
        v = (self.x[j] & 0xFFFF) >> 12
        self._code(j, v << 12, BYPASS_FREQ)
        return v

    def pop(self, indexes):
        out = []
        for ci in indexes:
            ci = int(ci)
            j = self.pos % self.K
            row = self.cdf[ci]
            max_value = int(self.sizes[ci]) - 2
            cum = self.x[j] & 0xFFFF
            s = min(max_value, bisect.bisect_right(row, cum, 0, max_value + 2) - 1)   # largest slot with row[s] <= cum
            self._code(j, int(row[s]), int(row[s + 1]) - int(row[s]))
            value = s
            if s == max_value:
                v = self._digit(j)
                nb = v
                while v == MAX_BYPASS and nb <= MAX_BYPASS_DIGITS:
                    v = self._digit(j)
                    nb += v
                if nb > MAX_BYPASS_DIGITS:
                    raise CorruptStream("corrupt stream (bypass length %d)" % nb)
                raw = 0
                for k in range(nb):
                    raw |= self._digit(j) << (k * BYPASS_BITS)
                value = raw >> 1
                value = -value - 1 if raw & 1 else value + max_value
            out.append(value + int(self.offsets[ci]))
            self.pos += 1
        if self.pos > self.n:
            raise CorruptStream("corrupt stream (more symbols popped than coded)")
        return out

    def finish(self):
        """After the n-th symbol: every lane back at L and the cursor at the end, else CorruptStream."""
        if self.bad or self.pos != self.n or any(v != RANS_L for v in self.x) or self.cur != len(self.buf):
            raise CorruptStream("corrupt stream")


def decode(stream, indexes, cdf, sizes, offsets):
    d = Decoder(stream, len(indexes), cdf, sizes, offsets)
    out = d.pop(indexes)
    d.finish()
    return out
