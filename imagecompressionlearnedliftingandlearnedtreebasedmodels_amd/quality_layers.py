"""The quality layers of the codec: SNR scalability on top of a base container coded at a step q.

Layer j (1 .. m) brings every coefficient of the levels 0 .. L-2 -- those that carry a step -- from the step
q_{j-1} to q_j = q / 3^j.  A mid-tread bin of width q_{j-1} around v splits exactly into three bins of width q_j centred at
v - q_j, v, v + q_j, so the quantisers nest and a layer's alphabet is t in {-1, 0, +1}:

    encoder   t = clamp(rint((y - v_{j-1}) * inv_q_j), -1, 1),  v_j = v_{j-1} + t * q_j        (fp32, product rounded, then added)
    decoder   v_j = v_{j-1} + t * q_j

with v_0 the base's dequantised level and (q_j, inv_q_j) = ops.layer_pair(n, j).  The context of a symbol is a function of the
decoded base alone: per level one parallel evaluation of the coded layer's own model on v_0 gives (sigma, mu) of every
coefficient (``level_params``), reused by every layer, and layer j codes t with the table row (idx, a),

    idx = #(table[:63] < max(sigma * inv_q_{j-1}, 0.11)),   a = min(|rint((v_{j-1} - mu) * inv_q_{j-1})|, K),   K = 8,

mirrored (-t is coded) where that integer is negative.  Row (idx, a) holds the probabilities of t for a zero-mean Gaussian of
the scale table's entry idx, in units of the previous step, restricted to the bin [a - 1/2, a + 1/2] cut in three (``Tables``).
One stream per (layer, plane, unit, level), raster order with channels outermost, coded by the base container's coder.  The
device work is csrc/layers.hip (ops.layer_encode / layer_rows / layer_apply); the tables are host work, and the container
(LLDP) lives in codec.py.
"""
import math
import zlib

import numpy as np

K = 8                                # bell positions 0 .. K have a row of their own; farther bins share row K
MAX_LAYERS = 4
SCALES = 64                          # the scale table of the coded layers: 64 log-spaced scales from 0.11 to 256
_SCALES_MIN, _SCALES_MAX = 0.11, 256.0
_UNDERFLOW = 1e-280                  # a bin whose Gaussian mass is below this is coded with the uniform row
_TABLES = []


def scale_table():
    """The 64 scales as float64: exp(linspace(log 0.11, log 256, 64)), the values of LiftingBasedDWT_net.get_scale_table."""
    return np.exp(np.linspace(math.log(_SCALES_MIN), math.log(_SCALES_MAX), SCALES))


def bin_masses(s, a):
    """The Gaussian masses (float64) of the three thirds of the bin [a - 1/2, a + 1/2] under N(0, s^2), a >= 0 an integer ->
    [P(t = -1), P(t = 0), P(t = +1)], not normalised.  Every mass on the positive side is the difference of two erfc values of
    the tail-side arguments, so a bin far out in the tail loses no digits to cancellation; the third that straddles zero
    (a = 0, t = 0) is an erf."""
    r = 1.0 / (s * math.sqrt(2.0))
    tail = lambda lo, hi: 0.5 * (math.erfc(lo * r) - math.erfc(hi * r))
    if a == 0:
        side = tail(1.0 / 6.0, 0.5)
        return [side, math.erf(r / 6.0), side]
    return [tail(a + (t - 0.5) / 3.0, a + (t + 0.5) / 3.0) for t in (-1, 0, 1)]


def quantise_row(p, symmetric):
    """Three probabilities -> three 16-bit frequencies, each >= 1, that sum to 65 535: the coders' tables end with an escape
    slot, which takes the one remaining count and is never coded.  floor(p * 65535) with a floor of 1, the sum fixed on the
    largest entry -- on the middle one for a symmetric row (a = 0), whose middle entry is the largest."""
    f = [max(1, int(math.floor(v * 65535.0))) for v in p]
    k = 1 if symmetric else max(range(3), key=lambda i: (f[i], -i))            # first of the largest
    f[k] += 65535 - sum(f)
    return f


class Tables:
    """The rows of the quality layers as the coders' host tables, laid out like residual.Tables: cdf (64 (K+1), 5) int32, row
    idx * (K + 1) + a = [0, f(-1), f(-1) + f(0), 65535, 65536]; sizes 5 (three symbols, the escape slot and the end), offsets
    -1.  freq (64, K+1, 3) are the frequencies, crc the CRC32 of cdf as little-endian int32 (the LLDP header field)."""

    def __init__(self):
        sc = scale_table()
        freq = np.empty((SCALES, K + 1, 3), dtype=np.int64)
        for i in range(SCALES):
            for a in range(K + 1):
                p = bin_masses(float(sc[i]), a)
                tot = sum(p)
                p = [v / tot for v in p] if tot > _UNDERFLOW else [1.0 / 3.0] * 3
                freq[i, a] = quantise_row(p, a == 0)
        self.freq = freq
        rows = freq.reshape(-1, 3)
        cdf = np.zeros((rows.shape[0], 5), dtype=np.int64)
        cdf[:, 1:4] = np.cumsum(rows, axis=1)
        cdf[:, 4] = 65536
        self.cdf = cdf.astype(np.int32)
        self.sizes = np.full(rows.shape[0], 5, dtype=np.int32)
        self.offsets = np.full(rows.shape[0], -1, dtype=np.int32)
        self.crc = zlib.crc32(self.cdf.astype("<i4").tobytes()) & 0xFFFFFFFF


def tables():
    """The Tables, built once per process (host only, no library)."""
    if not _TABLES:
        _TABLES.append(Tables())
    return _TABLES[0]


def check_layers(layers):
    """The ``layers`` argument of the encoders -> m in [0, MAX_LAYERS] (None -> 0).  ValueError naming layers otherwise."""
    if layers is None:
        return 0
    if isinstance(layers, bool) or not isinstance(layers, (int, np.integer)) or not 0 <= int(layers) <= MAX_LAYERS:
        raise ValueError("layers must be None or an integer in [0, %d]: the number of quality layers over the base (got %r)"
                         % (MAX_LAYERS, layers))
    return int(layers)


def check_step_divides(n, m):
    """A base step n / 16 under m layers: the finest step q / 3^m must stay at or above 1 / 16 (ValueError naming both)."""
    if n < 3 ** m:
        raise ValueError("layers and step: %d layers divide the step by %d, which needs a step of at least %d / 16 (n / 3^m >= 1; "
                         "the step is %d / 16)" % (m, 3 ** m, 3 ** m, n))


def _table63(dev):
    import torch
    from .graphs.models.LiftingBasedDWT_net import get_scale_table
    return get_scale_table().to(dev).float()[:63].contiguous()


def level_params(em, i, v0):
    """(sigma, mu) of every coefficient of level i from ONE parallel evaluation of the coded layer's own model on the decoded
    base: em: the per-plane entropy layers; v0: the base's dequantised levels indexed by level (finest first; entries below the
    level a reduced decode stops at may be None) -> (P,B,2G,h,w), sigma on the even and mu on the odd channels.
      onlyEZWT      _level_params on the parent level, the call the base makes;
      ZTBlock       the four ops.ztblock_phase launches on the COMPLETE decoded level (the base runs them on the level as
                    decoded so far), each phase's result placed at its positions;
      conditioned2  _tree_context of the parent and ops.cgp16_params on the complete decoded level (the base steps along a
                    wavefront); cgp widths the register chain does not take are refused (NotImplementedError).
    Encoder and decoder make the same call on the same values, so the result need not equal the base's own parameters."""
    import torch
    from . import ops
    from .graphs.models import LiftingBasedDWT_net as net
    from .graphs.models.entropy_coding import ZT_PHASES
    cls, L = type(em[0]), len(v0)
    if not 0 <= i <= L - 2:
        raise ValueError("layers: level %d carries no step (the levels 0 .. %d do)" % (i, L - 2))
    parent, lev = v0[i + 1].contiguous(), v0[i].contiguous()
    with torch.no_grad():
        if cls is net.onlyEZWT:
            return cls._level_params(em, i, parent).contiguous()
        if cls is net.DWTConditioned2EntropyLayerZTBlock:
            cls._require_clrch1(em)
            packs = cls._phase_packs(em, L - i - 2)
            P, B, G, H, W = lev.shape
            out = torch.empty(P, B, 2 * G, H, W, device=lev.device, dtype=torch.float32)
            for k, (r, c) in enumerate(ZT_PHASES):
                out[:, :, :, r::2, c::2] = ops.ztblock_phase(parent, lev, packs[k], k + 1)
            return out
        if cls is net.DWTConditioned2EntropyLayerZTsepSubbands:
            plc, packed, _, ksize, bits = cls._tree_context(em, i, parent, lev.shape[2])
            if packed[1] is None:
                raise NotImplementedError("layers: the quality layers evaluate conditioned2ZTsepSubbands on the split-fp16 "
                                          "register chain, which is built for the cgp widths 93 -> 162 -> 54 -> 18 -> 2 only")
            return ops.cgp16_params(plc.contiguous(), lev, packed[1], ksize, bits)
    raise NotImplementedError("layers: %s is not a coded entropy layer" % cls.__name__)


def encode_units(em, y, v0, n, m, coder):
    """The m quality layers of a group of units.  em: the per-plane entropy layers; y: the coefficients per level (finest
    first, (P,B,G,h,w) each); v0: the base's dequantised levels (compress_planes' q_list); n: the base step is n / 16; coder:
    "host" or "gpu" (or entropy_coding.ESTIMATE) -> (streams, v): streams[j - 1][i][p][b] the stream of layer j, level i,
    plane p, unit b; v[j - 1][i] the level at the step of layer j, which decode_units reproduces bit for bit."""
    from . import ops
    from .graphs.models import entropy_coding as ec
    L, tab = len(y), tables()
    check_step_divides(n, m)
    streams = [[None] * (L - 1) for _ in range(m)]
    vs = [[None] * (L - 1) for _ in range(m)]
    for i in range(L - 1):
        params = level_params(em, i, v0)
        v, yi = v0[i].contiguous(), y[i].contiguous()
        P, B, G, h, w = v.shape
        t63 = _table63(v.device)
        for j in range(1, m + 1):
            sym, row, v = ops.layer_encode(yi, v, params, t63, ops.layer_pair(n, j - 1), ops.layer_pair(n, j), K)
            sink = ec._make_sink(coder, P, B, tab, None, G * h * w, v.device)
            sink.step(row.reshape(P, B, G * h * w, 1), sym.reshape(P, B, G * h * w, 1))
            streams[j - 1][i] = sink.flush()
            vs[j - 1][i] = v
    return streams, vs


def decode_units(em, v0, streams, n, j, coder, first_level=0):
    """The first j layers of a group of units applied to the decoded base.  v0: the base's dequantised levels indexed by level
    (decompress_planes' list; entries below first_level may be None); streams: as encode_units returns them (at least j
    layers; the entries of levels below first_level are never read) -> the list v0 with the levels first_level .. L-2 replaced
    by their values at the step of layer j."""
    from . import ops
    from .graphs.models import entropy_coding as ec
    L, tab = len(v0), tables()
    check_step_divides(n, j)
    out = list(v0)
    if j == 0:
        return out
    for i in range(int(first_level), L - 1):
        params = level_params(em, i, v0)
        v = v0[i].contiguous()
        P, B, G, h, w = v.shape
        t63 = _table63(v.device)
        for jj in range(1, j + 1):
            row, sign = ops.layer_rows(v, params, t63, ops.layer_pair(n, jj - 1), K)
            sink = ec._make_sink(coder, P, B, tab, streams[jj - 1][i], G * h * w, v.device)
            sym = sink.step(row.reshape(P, B, G * h * w, 1))
            sink.finish()
            v = ops.layer_apply(v, sym.int().contiguous(), sign, ops.layer_pair(n, jj))
        out[i] = v
    return out
