"""The residual layer of the codec: lossless and near-lossless coding on top of the decoded base image.

A unit is one image of an LLDW container or the in-image rectangle of one tile of an LLDT container.  With xh the base
layer's decoded uint8 RGB of the unit, x the original and d the bound (0 = lossless), the layer codes per pixel and channel
q = sign(r) * ((|r| + d) // (2d + 1)), r = x - xh, and the decoder returns clamp(xh + q * (2d + 1), 0, 255), so that
|out - x| <= d.  The context of a symbol (channel, and one of 8 activity classes of xh around the pixel) is a function of
xh alone; each of a unit's 24 contexts is coded with one of a ladder of 64 two-sided geometric tables, chosen by the encoder
from the context's histogram and written into the container.  One stream per (unit, channel), in raster order, coded by
the base container's coder.  The device work is csrc/residual.hip (ops.resid_analyse / resid_contexts / resid_apply); the
tables, the scale choice and the containers' bytes are host work.
"""
import zlib

import numpy as np

CLASSES = 8
CONTEXTS = 3 * CLASSES
LADDER_ID = 1
LADDER_SIZE = 64
MAX_NEAR = 32
_MASK64 = (1 << 64) - 1
_CS_MOD = 65521
_TABLES = {}
# units of one kernel / coder call: bounds the int32 symbol and index arrays (12 bytes per pixel each) and the stream count
_MAX_PIXELS_PER_CALL = 1 << 24
_MAX_UNITS_PER_CALL = 8192


def check_near(near):
    """The ``near`` argument of the encoders -> int in [0, MAX_NEAR] (ValueError naming near)."""
    if isinstance(near, bool) or not isinstance(near, (int, np.integer)) or not 0 <= int(near) <= MAX_NEAR:
        raise ValueError("near must be None or an integer in [0, %d]: 0 is lossless, d > 0 bounds the error of every sample "
                         "by d (got %r)" % (MAX_NEAR, near))
    return int(near)


def symbol_range(d):
    """Q: the symbols of bound d lie in [-Q, Q]."""
    return (255 + d) // (2 * d + 1)


def quantise(r, d):
    """The layer's quantiser on integer residuals r = x - xh (numpy int array or int) -> q."""
    r = np.asarray(r, dtype=np.int64)
    return np.sign(r) * ((np.abs(r) + d) // (2 * d + 1))


def reconstruct(xh, q, d):
    """clamp(xh + q * (2d + 1), 0, 255) on integer arrays."""
    return np.clip(np.asarray(xh, dtype=np.int64) + np.asarray(q, dtype=np.int64) * (2 * d + 1), 0, 255)


def checksum(u8):
    """The unit checksum of a uint8 array in HWC raster order: sum_i (byte_i + 1) * (1 + i mod 65521) mod 2^64."""
    b = np.ascontiguousarray(u8, dtype=np.uint8).reshape(-1).astype(np.uint64)
    w = (np.arange(b.size, dtype=np.uint64) % np.uint64(_CS_MOD)) + np.uint64(1)
    with np.errstate(over="ignore"):
        return int(((b + np.uint64(1)) * w).sum(dtype=np.uint64)) & _MASK64


class Tables:
    """The ladder of bound d as the coders' host tables: cdf (64, 2Q+3) int32, sizes, offsets, and what the encoder's scale
    choice needs (neg_log2 (64, 2Q+1) float64: the ideal length in bits of each symbol under each table)."""

    def __init__(self, d):
        from .ans import pmf_to_quantized_cdf
        self.d, self.Q = d, symbol_range(d)
        Q = self.Q
        q = np.arange(-Q, Q + 1, dtype=np.float64)
        rows = []
        for s in range(LADDER_SIZE):
            b = 0.05 * 1600.0 ** (s / 63.0)
            p = np.exp(-np.abs(q) / b)
            p = (p / p.sum()).astype(np.float32)
            # full support: every q in [-Q, Q] has a slot, so the layer never escapes; the coders' tables end with the
            # escape slot (cdf_length - 2), which gets the smallest frequency the quantiser gives (1)
            rows.append(pmf_to_quantized_cdf(np.concatenate([p, np.zeros(1, dtype=np.float32)]), 16))
        self.cdf = np.asarray(rows, dtype=np.int32)                                   # (64, 2Q + 3)
        self.sizes = np.full(LADDER_SIZE, 2 * Q + 3, dtype=np.int32)
        self.offsets = np.full(LADDER_SIZE, -Q, dtype=np.int32)
        freq = np.diff(self.cdf.astype(np.int64), axis=1)[:, :2 * Q + 1]
        self.neg_log2 = -np.log2(freq.astype(np.float64) / 65536.0)
        self.crc = zlib.crc32(self.cdf.astype("<i4").tobytes()) & 0xFFFFFFFF


def tables(d):
    """The Tables of bound d, built once per process (host only: the library's pmf_to_quantized_cdf is host code)."""
    if d not in _TABLES:
        _TABLES[d] = Tables(d)
    return _TABLES[d]


def choose_scales(hist, tab):
    """hist: (..., 2Q+1) integer counts of q + Q per context -> (...) uint8: per context the lowest ladder index that
    minimises the ideal code length sum_q hist[q] * -log2 p_s(q) under the quantised tables (float64); 0 for an empty one.
    Each context is costed on its own, over the span of its non-empty bins (an empty bin adds an exact 0): 64 numpy sums over
    rows of one fresh contiguous array, whose summation order is a function of that span alone.  So the choice cannot depend
    on which units share a call, which a matrix product over all contexts of a call would not promise."""
    h = np.asarray(hist, dtype=np.float64)
    rows = h.reshape(-1, h.shape[-1])
    s = np.zeros(len(rows), dtype=np.uint8)
    for k in np.flatnonzero(rows.any(axis=1)):
        nz = np.flatnonzero(rows[k])
        lo, hi = nz[0], nz[-1] + 1
        s[k] = np.argmin((tab.neg_log2[:, lo:hi] * rows[k, lo:hi]).sum(axis=1))       # first minimum: the lowest index
    return s.reshape(h.shape[:-1])


def _group_units(grid, tiles):
    """Units by rectangle size (at most four sizes in a grid), then cut to the per-call bounds -> list of lists of positions
    into ``tiles``."""
    from . import ops
    by = {}
    for k, t in enumerate(tiles):
        by.setdefault(ops.resid_unit_size(grid, t), []).append(k)
    calls = []
    for (uh, uw), ks in by.items():
        step = max(1, min(_MAX_UNITS_PER_CALL, _MAX_PIXELS_PER_CALL // (uh * uw)))
        calls += [ks[a:a + step] for a in range(0, len(ks), step)]
    return calls


def encode_units(x, xh, grid, tiles, d, coder):
    """x, xh: (B,H,W,3) uint8 device tensors (originals, base reconstructions); grid = (H, W, th, tw, ny, nx); tiles: the
    unit indexes -> per unit, in the order of ``tiles``: dict(cs_xh, cs_x, scales (24 bytes), streams [3 bytes objects]).
    cs_x is 0 for d > 0.  One host round trip per call group for the histograms (the scale choice is host float64), then
    the coder's own."""
    import torch
    from . import irans, ops
    from .ans import encode_streams
    H, W = grid[0], grid[1]
    region = (0, 0, H, W)
    tab = tables(d)
    out = [None] * len(tiles)
    for ks in _group_units(grid, tiles):
        grp = [tiles[k] for k in ks]
        sym, _, hist, cs_xh, cs_x = ops.resid_analyse(x, xh, grid, region, grp, d)
        scales = choose_scales(hist.cpu().numpy(), tab).reshape(len(grp), CONTEXTS)
        idx, _ = ops.resid_contexts(xh, grid, region, grp, torch.from_numpy(scales).to(x.device))
        if coder == "gpu":
            streams = irans.encode(sym, idx, irans.device_tables(tab, x.device))
        else:
            streams = encode_streams(sym.cpu().numpy(), idx.cpu().numpy(), tab.cdf, tab.sizes, tab.offsets)
        a, b = cs_xh.cpu().tolist(), cs_x.cpu().tolist()
        for j, k in enumerate(ks):
            out[k] = dict(cs_xh=a[j] & _MASK64, cs_x=(b[j] & _MASK64) if d == 0 else 0, scales=scales[j].tobytes(),
                          streams=[bytes(s) for s in streams[3 * j:3 * j + 3]])
    return out


def decode_units(buf, grid, region, tiles, units, d, coder):
    """Refines, in place, the units ``tiles`` of buf, a (B,h,w,3) uint8 device buffer holding the base reconstruction of the
    region (y0, x0, h, w) (every unit inside it).  units: per tile dict(cs_xh, cs_x, scales, streams) as parsed.
    ValueError("reconstruction check: ...") when a unit's base reconstruction has not the checksum the encoder stored
    (raised before anything is applied) or, for d = 0, when the refined unit has not the original's."""
    import torch
    from . import irans, ops
    from .ans import decode_streams
    tab = tables(d)
    calls = _group_units(grid, tiles)

    def contexts(ks):
        scales = np.frombuffer(b"".join(units[k]["scales"] for k in ks), dtype=np.uint8).reshape(len(ks), CONTEXTS)
        return ops.resid_contexts(buf, grid, region, [tiles[k] for k in ks], torch.from_numpy(scales.copy()).to(buf.device))
    # every unit's base is checked before any unit changes.  Only the checksums outlive this pass: the indexes are 12 bytes
    # per pixel, and holding those of every group would undo the bound of _MAX_PIXELS_PER_CALL, so with more than one group
    # they are made again below (one more read of the group's pixels; a context looks at its own unit only, so the units
    # refined in between change nothing).
    first = [contexts(ks) for ks in calls[:1]]
    sums = [c[1] for c in first] + [contexts(ks)[1] for ks in calls[1:]]
    keep = first[0][0] if len(calls) == 1 else None
    del first
    for ks, cs_xh in zip(calls, sums):
        for k, got in zip(ks, cs_xh.cpu().tolist()):
            if got & _MASK64 != units[k]["cs_xh"]:
                raise ValueError("reconstruction check: the base layer of unit %d decoded to other bytes than the encoder's "
                                 "(checksum %016x, the container holds %016x); the residual cannot be applied"
                                 % (tiles[k], got & _MASK64, units[k]["cs_xh"]))
    for ks in calls:
        grp = [tiles[k] for k in ks]
        idx = keep if keep is not None else contexts(ks)[0]
        streams = [s for k in ks for s in units[k]["streams"]]
        if coder == "gpu":
            dec = irans.Decoder(streams, int(idx.shape[1]), irans.device_tables(tab, buf.device), buf.device)
            sym = dec.pop(idx)
            dec.finish()
        else:
            sym = torch.from_numpy(decode_streams(streams, idx.cpu().numpy(), tab.cdf, tab.sizes, tab.offsets)).to(buf.device)
        _, cs_out = ops.resid_apply(buf, grid, region, grp, d, sym.contiguous())
        if d == 0:
            for k, t, got in zip(ks, grp, cs_out.cpu().tolist()):
                if got & _MASK64 != units[k]["cs_x"]:
                    raise ValueError("reconstruction check: the refined unit %d has not the original's checksum (%016x, the "
                                     "container holds %016x)" % (t, got & _MASK64, units[k]["cs_x"]))
    return buf
