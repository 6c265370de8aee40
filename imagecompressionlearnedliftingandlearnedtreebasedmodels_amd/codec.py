"""Standalone image codec: uint8 RGB images <-> self-describing byte containers (one per image).

``encode_images(net, images)`` and ``decode_images(net, blobs)`` wrap the coded entropy layers
(conditioned2ZTsepSubbands, onlyEZWT, DWTConditioned2EntropyLayerZTBlock) of a ``LiftingBasedDWTNetWrapper`` in eval mode.
The decoder needs nothing but the container and a net with the same weights: the shapes, the model identity and the
coding arithmetic are in the header and are checked on the host before any GPU work.  ``read_header`` is CPU only.

Container format, version 1 (all integers little-endian):

    magic             4 bytes   b"LLDW"
    format version    u8        1
    entropy layer     u8        1 conditioned2ZTsepSubbands, 2 onlyEZWT, 3 DWTConditioned2EntropyLayerZTBlock
    netType           u8        1 CDF97, 2 LiftingBasedNeuralWaveletv4
    dwtlevels L       u8
    H, W              u32, u32  size of the original image
    numerics version  u16       CODING_NUMERICS_VERSION of the encoder
    arithmetic        u8 length + ASCII: canonical "key=value,..." of the switches that select the coding arithmetic
    weights digest    16 bytes  sha256 of the parameters (weights_digest), first 16 bytes
    stream count      u8        3 * (L + 1)
    stream lengths    LEB128 varints, one per stream
    payload           the rANS streams, plane-major; per plane: xe, then xo finest -> coarsest
    CRC32             u32       zlib.crc32 of every byte before it

The streams are coded by the host range coder (rans64, csrc/rans.hip) unless the arithmetic string holds a ``coder`` key:
``coder=irans32`` selects the interleaved device coder (``encode_images(..., coder="gpu")``).  The key is
absent for the host coder, so host-coded containers are those of the format as first defined, byte for byte.

The image is coded at the padded size padded_size(H, W) (replicate-edge padding, lifting_dwt_nets.padded_size) and
cropped back to H x W after decoding.

Tiled coding (``encode_tiled`` / ``decode_tiled``): a large image is cut into a grid of ny x nx tiles of
th x tw (tile_grid), each coded as an independent image -- its streams are byte-identical to those of
``encode_images(net, padded_tile)`` -- and a region decodes from the tiles it touches.  Tiled container, version 1:

    magic             4 bytes   b"LLDT"
    format version    u8        1
    entropy layer, netType, dwtlevels   u8 x 3, as LLDW
    H, W              u32, u32  size of the original image
    th, tw            u32, u32  tile size (padded_size(th, tw) == (th, tw))
    ny, nx            u16, u16  grid (ceil(H / th), ceil(W / tw))
    numerics version  u16
    arithmetic, weights digest          as LLDW
    streams per tile  u8        3 * (L + 1)
    stream lengths    LEB128 varints, tile-major in raster order of (ty, tx); inside a tile the LLDW order
    payload           the streams in the same order
    CRC32             u32       zlib.crc32 of every byte before it

Lapped tiles (``encode_tiled(..., overlap=ov)``): neighbouring tiles share a band of ov pixels, both code
it, and the decoder cross-fades the two reconstructions with a linear ramp (lap_weights) whose weights sum to exactly 1, so
a border's step becomes a ramp.  Every tile is still an independent image with the streams of ``encode_images``.  Such a
frame has its own container, version 1 (overlap == 0 writes LLDT as before):

    magic             4 bytes   b"LLDO"
    format version    u8        1
    ... the LLDT fields up to ny, nx (the grid at the stride (th - overlap, tw - overlap), tile_grid_lapped)
    overlap           u16       a power of two, 2^L <= overlap <= min(th, tw) / 2
    numerics version .. CRC32   as LLDT

Reduced-resolution decoding (``decode_images(..., reduce=k)``, ``decode_tiled(..., reduce=k)``): for
0 <= k <= L the output is the image at 1/2^k of each side, ceil(H / 2^k) x ceil(W / 2^k).  Only the xe streams and the xo
streams of levels k .. L-1 are decoded (the streams of finer levels are never handed to a coder), the inverse transform runs
for the top L-k levels, and the LL band at level k is brought to the image's scale by lifting_dwt_nets.ll_affine before the
colour conversion.  reduce=0 is the full decode.  ``reduce_bytes`` gives, per factor, the header plus stream bytes such a
decode reads.  The container format is the same.

Lossless and near-lossless coding (``encode_images(..., near=d)``, ``encode_tiled(..., near=d)``): a residual
layer over the decoded base image (residual.py, csrc/residual.hip).  near=0 returns the input bit for bit, near=d in 1..32
bounds the error of every sample by d; near=None writes the containers above, byte for byte.  A unit is the image of an LLDW
base or the in-image rectangle of one tile of an LLDT base (lapped bases are refused).  Refined container, version 1:

    magic             4 bytes   b"LLDR"
    format version    u8        1
    near d            u8        0 lossless, 1..32 the bound
    classes           u8        8 activity classes per channel (24 contexts per unit)
    ladder id         u8        1 (64 two-sided geometric tables, b_s = 0.05 * 1600^(s/63))
    table CRC32       u32       zlib.crc32 of the quantised ladder of d as little-endian int32 (residual.Tables.cdf)
    base length       LEB128
    base container    the complete LLDW or LLDT container, as encode_images / encode_tiled write it without ``near``
    unit count        u32       1 over LLDW, ny * nx over LLDT
    per unit          cs(xh) u64, cs(x) u64 (0 when d > 0), 24 u8 table indexes (context c * 8 + a), units in tile order
    stream lengths    LEB128 varints, 3 per unit (R, G, B)
    payload           the streams in the same order, coded by the base container's coder
    CRC32             u32       zlib.crc32 of every byte before it

Variable-rate coding (``encode_images(..., step=q)`` / ``target_bytes=T``, the same on ``encode_tiled``): the
levels 0 .. L-2 of a coded layer, whose Gaussian parameters are conditioned on an already decoded parent, are quantised with
a step q = n / 16, n an integer in [4, 1024]: symbol = round((y - mu) / q), value = symbol * q + mu, the table entered with
sigma / q.  xe and the coarsest level keep the unit step.  The step is one more key of the arithmetic string, ``step=<n>``,
absent at n = 16: ``step=None`` and ``step=1`` write the containers above byte for byte, no container type changes, and the
decoders read the step from the header (``hdr["step"]``, a float; on the nested base header of an LLDR).  ``target_bytes=T``
searches the quarter-octave grid STEP_GRID for the finest step whose container is at most T bytes, one image (or one tiled
frame) at a time.

Rate-distortion optimised quantisation (``encode_images(..., rdo=rho)``, the same on ``encode_tiled``): where
a step applies, the encoder moves a coefficient one level toward zero when rho * q^2 * (bits saved) exceeds the squared error
that adds, judged with the exact integer code lengths of the level's tables.  rho = m / 64, m an integer in [1, 256]
(ln 2 / 6 = 0.1155 is the high-rate slope; 13 / 64 is a good start).  It is an encoder's choice alone: nothing is recorded, no
header key, the decoders are untouched and never learn of it; ``rdo=None`` and ``rdo=0`` write the bytes above.  It composes
with ``step``, ``target_bytes`` (probes and real encodes both run with it), ``near``, tiles and both coders.

Region-of-interest coding (``encode_images(..., step_map=M)``, the same on ``encode_tiled``): a step per block
of 2^L x 2^L pixels instead of one per image.  M is (hb, wb) = (ceil(H / 2^L), ceil(W / 2^L)) steps, each n / 16 with n in
[4, 1024] (``check_step_map``; ``step_map_from_regions`` paints one from rectangles).  The coefficient at (y, x) of a subband of
level l <= L-2 takes the step of block (min(y >> s, hb - 1), min(x >> s, wb - 1)), s = L - 1 - l, with the arithmetic of 7.1.6
and 7.1.7 per coefficient; xe and the coarsest level keep the unit step.  The map travels in a wrapping container, version 1:

    magic             4 bytes   b"LLDQ"
    format version    u8        1
    block log2        u8        L of the inner container
    hb, wb            u16, u16  ceil(H / 2^L), ceil(W / 2^L) of the inner container's H, W
    map CRC32         u32       zlib.crc32 of the hb * wb values n as little-endian u16, raster order
    run count         LEB128
    runs              (LEB128 length >= 1, u16 n) each, raster order, maximal: adjacent runs differ
    inner length      LEB128
    inner container   a complete LLDW, LLDT, LLDO or LLDR container
    CRC32             u32       zlib.crc32 of every byte before it

The base container (of an LLDR: its nested base) carries one more arithmetic key, ``qmap=<8 hex digits of the map CRC>``, and no
``step`` key: the map holds every step.  The key binds base and map; a base with the key is refused without its wrapper, and
an LLDQ whose key and map disagree is refused.  ``step_map`` composes with ``coder``, ``rdo``, ``near``, ``tile`` and ``overlap``
(a tile codes with the slice of the map at its origin, clamped as above) and excludes ``step`` and ``target_bytes``.  The
decoders take an LLDQ wherever they take its inner container, with ``region``, ``reduce`` and ``refine``.

Quality-targeted coding (``encode_images(..., target_psnr=P)`` / ``target_msssim=M``, the same on ``encode_tiled``, DESIGN.md
7.1.9): the encoder searches STEP_GRID for a step whose decoded image meets the target while the next coarser grid step does
not -- the coarsest step that meets it where quality falls monotonically along the grid.  PSNR is judged in integers: the exact
SSE of the bytes the decoder would write (lldwt_ycc_tiles_sq_err on the encoder's own reconstruction) against
``psnr_sse_bound(P, H, W)``.  At most 7 probes without a range coder, then one real encode; the container is that of
``step=<chosen>`` byte for byte and records nothing.  Excludes ``step``, ``step_map``, ``target_bytes`` and ``near``.

Quality layers (``encode_images(..., step=q, layers=m)``, the same on ``encode_tiled``, DESIGN.md 7.1.10, quality_layers.py): SNR
scalability.  The container holds the unchanged base of ``step=q`` plus m refinement layers; layer j brings every coefficient of
the levels 0 .. L-2 from the step q / 3^(j-1) to q / 3^j with one symbol of {-1, 0, +1}, coded under tables conditioned on the
decoded base alone, so a layer decodes in a few parallel launches per level.  ``decode_images`` / ``decode_tiled(..., layers=j)``
decode the base plus the first j layers (default: all), ``layer_bytes`` gives the bytes each prefix reads and ``truncate_layers``
cuts a container to a prefix.  Layered container, version 1:

    magic             4 bytes   b"LLDP"
    format version    u8        1
    m                 u8        the number of layers, 1..4, with n / 3^m >= 1 for the base step n / 16
    K                 u8        8: bell positions 0 .. K have a table row each
    table CRC32       u32       zlib.crc32 of the quantised rows as little-endian int32 (quality_layers.Tables.cdf)
    base length       LEB128
    base container    the complete LLDW or LLDT container, as encode_images / encode_tiled write it without ``layers``
    unit count        u32       1 over LLDW, ny * nx over LLDT
    stream lengths    LEB128 varints, layer-major; per layer unit-major in tile order; per unit 3 (L - 1): plane-major, levels 0 .. L-2
    payload           the streams in the same order, coded by the base container's coder
    CRC32             u32       zlib.crc32 of every byte before it

``layers`` composes with ``coder``, ``step``, ``rdo``, tiles, ``region``, ``tiles_per_call`` and ``reduce`` (the levels the decode
reaches are refined, finer levels' streams are never touched) and excludes ``near``, ``step_map``, ``overlap > 0`` and the three
targets; ``layers=None`` and ``layers=0`` write the containers above byte for byte.

Chroma formats (``encode_images(..., chroma="420" | "400")``, the same on ``encode_tiled``): "420" codes Y at
full size and Cb, Cr at half size -- 1.5 planes of coefficients instead of 3; "400" codes a (B,H,W,1) greyscale image as one
plane.  With pd = lifting_dwt_nets.padded_dims, a 4:2:0 image (or tile share) of H x W codes chroma planes of (Hc, Wc) =
pd(ceil(H / 2), ceil(W / 2)) and a luma plane of (2 Hc, 2 Wc) (``chroma_sizes``).  A chroma sample is ((c00 + c01) + (c10 +
c11)) * 0.25 over its 2 x 2 pixels; the decoder interpolates with the weights 3/4 and 1/4 toward the nearer and the farther
sample, clamped at the tile's own plane (csrc/chroma.hip; tests/chroma_ref.py states both in torch).  Plane p is coded by the
net's plane p alone, so its streams are those of ``encode_strings_planes([nets[p]], x_p)``.  The format is one more key of the
arithmetic string, ``chroma=420`` or ``chroma=400``, absent for "444": ``chroma=None`` and ``"444"`` write the containers above
byte for byte, there is no new container type, the stream count is 3 (L + 1) for 4:2:0 and L + 1 for 4:0:0, and a parsed
header holds ``chroma`` only when the key is present (readers use ``hdr.get("chroma", "444")``).  Composes with ``coder``,
``step``, ``target_bytes``, ``rdo``, tiles, ``region``, ``tiles_per_call`` and ``reduce``; excludes ``near``, ``layers``,
``step_map``, ``overlap > 0`` and the quality targets, and LLDR / LLDQ / LLDP / LLDO containers over such a base are refused.

Sample depth (``encode_images(..., depth=d)``, the same on ``encode_tiled``): d in 9..16 codes ``torch.uint16``
tensors of d-bit samples, (B,H,W,3) or with ``chroma="400"`` (B,H,W,1).  A sample is v / M with M = 2^d - 1 in fp32, a true
division, followed by exactly the colour expressions of the uint8 kernels; the decoder stores floor((c + 0.5) * M + 0.5) as
uint16 (csrc/depth.hip; tests/depth_ref.py states both in torch).  A sample above M is a ValueError naming depth, found by the
input kernels.  The depth is one more key of the arithmetic string, ``depth=<d>``, absent for 8: ``depth=None`` and ``8`` take
uint8 and write the containers above byte for byte, and a parsed header holds ``depth`` only when the key is present (readers
use ``hdr.get("depth", 8)``; the pinned header fixtures hold exactly the keys they held).  Nothing below
the image boundary changes, so a depth-16 image holding v8 * 257 has the streams of the uint8 image v8 (65535 = 255 * 257).
Composes with ``coder``, ``step``, ``target_bytes``, ``rdo``, ``chroma``, tiles, ``region``, ``tiles_per_call`` and ``reduce``;
excludes ``near``, ``layers``, ``step_map``, ``overlap > 0`` and the quality targets, and LLDR / LLDQ / LLDP / LLDO containers
over such a base are refused.

Centroid reconstruction (``decode_images`` / ``decode_tiled(..., recon="centroid")``): a decoder's choice that
costs no bits and changes no container.  Every decoder above puts a coefficient at the centre of its bin, sym * q + mu; under
the Gaussian (sigma, mu) the entropy model assigns to it the mean-square-optimal value is the bin's conditional mean, which
lies toward mu.  For every level 0 .. L-2 the decode reaches, ``quality_layers.level_params`` on the decoded base gives (sigma,
mu) and ``ops.gauss_centroid`` (csrc/recon.hip) moves the values, never out of their bins, with the step in force: the header's
step, the step of the last quality layer decoded, or the block's step of an LLDQ map.  xe and the coarsest level stay as
decoded.  ``recon=None`` and ``"centre"`` are the decode as ever, bit for bit.  Composes with every container and decoder
argument above except a residual layer that is applied: LLDR with ``refine=True`` at full resolution is a ValueError naming
recon and near (the residual was taken against the centre reconstruction); ``refine=False`` is allowed.

``decode_images`` / ``decode_tiled`` take LLDR over LLDW / LLDT; ``refine=False`` returns the base decode, and reduce > 0
decodes the base only (the residual lives at full resolution).  A region decodes the base and residual streams of the tiles it
touches only.  The decoder compares cs(xh) with its own reconstruction before it applies anything and raises
ValueError("reconstruction check: ...") on a mismatch.
"""
import hashlib
import struct
import zlib

MAGIC = b"LLDW"
FORMAT_VERSION = 1
# Bump whenever a change alters the bits of any kernel on the coding context path (the tree-context pair, the crop-stack
# conv engine path, lldwt_cgp16_wavefront_step, lldwt_ztblock_phase, the rate tables, the range coder): a container
# written before such a change must be refused, not silently mis-decoded.
CODING_NUMERICS_VERSION = 1

LAYER_CODES = {"conditioned2ZTsepSubbands": 1, "onlyEZWT": 2, "DWTConditioned2EntropyLayerZTBlock": 3}
NETTYPE_CODES = {"CDF97": 1, "LiftingBasedNeuralWaveletv4": 2}
_LAYER_NAMES = {v: k for k, v in LAYER_CODES.items()}
_NETTYPE_NAMES = {v: k for k, v in NETTYPE_CODES.items()}
_FIXED = struct.Struct("<4sBBBBIIH")          # magic .. numerics version
TILED_MAGIC = b"LLDT"
TILED_FORMAT_VERSION = 1
_TFIXED = struct.Struct("<4sBBBBIIIIHHH")     # magic .. H, W, th, tw, ny, nx, numerics version
LAPPED_MAGIC = b"LLDO"
LAPPED_FORMAT_VERSION = 1
_OFIXED = struct.Struct("<4sBBBBIIIIHHHH")    # magic .. H, W, th, tw, ny, nx, overlap, numerics version
REFINED_MAGIC = b"LLDR"
REFINED_FORMAT_VERSION = 1
_RFIXED = struct.Struct("<4sBBBBI")            # magic, version, near, classes, ladder id, table CRC32
_RUNIT = struct.Struct("<QQ24s")               # cs(xh), cs(x), the 24 table indexes
# the base containers: magic -> (format version, fixed struct)
_BASE = {MAGIC: (FORMAT_VERSION, _FIXED), TILED_MAGIC: (TILED_FORMAT_VERSION, _TFIXED),
         LAPPED_MAGIC: (LAPPED_FORMAT_VERSION, _OFIXED)}
MAPPED_MAGIC = b"LLDQ"
MAPPED_FORMAT_VERSION = 1
_QFIXED = struct.Struct("<4sBBHHI")            # magic, version, block log2, hb, wb, map CRC32
LAYERED_MAGIC = b"LLDP"
LAYERED_FORMAT_VERSION = 1
_PFIXED = struct.Struct("<4sBBBI")             # magic, version, m, K, table CRC32
_PLANES = 3
# coder name of the API -> value of the arithmetic string's "coder" key (None: the key is absent)
CODER_KEYS = {"host": None, "gpu": "irans32"}
_CODER_NAMES = {v: k for k, v in CODER_KEYS.items() if v is not None}


# quantisation step: q = n / STEP_DENOM, n an integer in [STEP_N_MIN, STEP_N_MAX]; the arithmetic string's
# "step" key holds n and is absent at n = STEP_DENOM (the unit step)
STEP_DENOM, STEP_N_MIN, STEP_N_MAX = 16, 4, 1024
# the candidate steps of a byte target: n_k = round(16 * 2^(k / 4)), k = -8 .. 24 (a quarter octave apart, 0.25 .. 64)
STEP_GRID_K = (-8, 24)
STEP_GRID = tuple(int(round(STEP_DENOM * 2.0 ** (k / 4.0))) for k in range(STEP_GRID_K[0], STEP_GRID_K[1] + 1))


# ------------------------------------------------------------------------------------------------ byte level (host only)
def check_step(step):
    """A quantisation step of the API -> n, the integer with step == n / 16 (None -> 16).  ValueError naming step unless the
    value is exactly n / 16 with n in [4, 1024]."""
    if step is None:
        return STEP_DENOM
    try:
        n = float(step) * STEP_DENOM
    except (TypeError, ValueError):
        raise ValueError("step must be a number (got %r)" % (step,)) from None
    if not (n == n and STEP_N_MIN <= n <= STEP_N_MAX and n == int(n)):
        raise ValueError("step must be n / %d with an integer n in [%d, %d], i.e. a multiple of %g in [%g, %g] (got %r)"
                         % (STEP_DENOM, STEP_N_MIN, STEP_N_MAX, 1.0 / STEP_DENOM, STEP_N_MIN / STEP_DENOM,
                            STEP_N_MAX / STEP_DENOM, step))
    return int(n)


# rate-distortion optimised quantisation: the Lagrangian rho = m / RDO_DENOM in units of q^2 per bit
RDO_DENOM, RDO_M_MAX = 64, 256


def check_rdo(rdo):
    """The Lagrangian of the API -> m, the integer with rdo == m / 64 (None and 0 -> 0: off).  ValueError naming rdo unless
    the value is exactly m / 64 with m in [1, 256]."""
    if rdo is None:
        return 0
    try:
        m = float(rdo) * RDO_DENOM
    except (TypeError, ValueError):
        raise ValueError("rdo must be a number (got %r)" % (rdo,)) from None
    if m == 0:
        return 0
    if not (m == m and 1 <= m <= RDO_M_MAX and m == int(m)):
        raise ValueError("rdo must be m / %d with an integer m in [1, %d], i.e. a multiple of %g in [%g, %g], or 0 / None for "
                         "off (got %r)" % (RDO_DENOM, RDO_M_MAX, 1.0 / RDO_DENOM, 1.0 / RDO_DENOM, RDO_M_MAX / RDO_DENOM, rdo))
    return int(m)


# adaptive quantisation: the strength aq = m / AQ_DENOM of the activity-derived step map
AQ_DENOM, AQ_M_MAX = 16, 32


def check_aq(aq):
    """The strength of adaptive quantisation of the API -> m, the integer with aq == m / 16 (None and 0 -> 0: off).  ValueError
    naming aq unless the value is exactly m / 16 with m in [1, 32]."""
    if aq is None:
        return 0
    try:
        m = float(aq) * AQ_DENOM
    except (TypeError, ValueError):
        raise ValueError("aq must be a number (got %r)" % (aq,)) from None
    if m == 0:
        return 0
    if not (m == m and 1 <= m <= AQ_M_MAX and m == int(m)):
        raise ValueError("aq must be m / %d with an integer m in [1, %d], i.e. a multiple of %g in [%g, %g], or 0 / None for off "
                         "(got %r)" % (AQ_DENOM, AQ_M_MAX, 1.0 / AQ_DENOM, 1.0 / AQ_DENOM, AQ_M_MAX / AQ_DENOM, aq))
    return int(m)


def _split_step(arith):
    """arithmetic string -> (n, the string without the step key); n = 16 when the key is absent.  ValueError naming step if
    the key occurs twice or its value is not a decimal integer in [4, 1024] other than 16 (the unit step is written by
    leaving the key out, so that there is one spelling of every arithmetic)."""
    parts = arith.split(",") if arith else []
    vals = [p[len("step="):] for p in parts if p.startswith("step=")]
    if not vals:
        return STEP_DENOM, arith
    ok = len(vals) == 1 and vals[0].isascii() and vals[0].isdigit() and vals[0] == str(int(vals[0])) \
        and STEP_N_MIN <= int(vals[0]) <= STEP_N_MAX and int(vals[0]) != STEP_DENOM
    if not ok:
        raise ValueError("step: bad quantisation step %r in the arithmetic string (an integer n in [%d, %d] other than %d, "
                         "once)" % (",".join(vals), STEP_N_MIN, STEP_N_MAX, STEP_DENOM))
    return int(vals[0]), ",".join(p for p in parts if not p.startswith("step="))


def _with_step(arith, n):
    """The arithmetic string (without a step key) with the key of step n / 16 merged in at its sorted place."""
    if n == STEP_DENOM:
        return arith
    return ",".join(sorted((arith.split(",") if arith else []) + ["step=%d" % n]))


def _split_qmap(arith):
    """arithmetic string -> (map CRC or None, the string without the qmap key).  ValueError naming the step map if the key occurs
    twice or its value is not 8 lowercase hex digits."""
    parts = arith.split(",") if arith else []
    vals = [p[len("qmap="):] for p in parts if p.startswith("qmap=")]
    if not vals:
        return None, arith
    if len(vals) != 1 or len(vals[0]) != 8 or any(c not in "0123456789abcdef" for c in vals[0]):
        raise ValueError("step map: bad qmap key %r in the arithmetic string (8 lowercase hex digits, once)" % ",".join(vals))
    return int(vals[0], 16), ",".join(p for p in parts if not p.startswith("qmap="))


def _with_qmap(arith, crc):
    """The arithmetic string (without a qmap key) with the key of the map CRC merged in at its sorted place; None: unchanged."""
    if crc is None:
        return arith
    return ",".join(sorted((arith.split(",") if arith else []) + ["qmap=%08x" % (crc & 0xFFFFFFFF)]))


# chroma formats: the API's names -> planes coded; the arithmetic string's "chroma" key holds the name and is
# absent for "444"
CHROMA_PLANES = {"444": 3, "420": 3, "400": 1}


def check_chroma(chroma):
    """The chroma argument of the API -> "444", "420" or "400" (None -> "444").  ValueError naming chroma otherwise."""
    if chroma is None:
        return "444"
    if not isinstance(chroma, str) or chroma not in CHROMA_PLANES:
        raise ValueError("chroma must be one of %s (got %r)" % (", ".join('"%s"' % c for c in sorted(CHROMA_PLANES, reverse=True)),
                                                                 chroma))
    return chroma


def _split_chroma(arith):
    """arithmetic string -> (chroma format, the string without the chroma key); "444" when the key is absent.  ValueError naming
    chroma if the key occurs twice or its value is not 420 or 400 (4:4:4 is written by leaving the key out)."""
    parts = arith.split(",") if arith else []
    vals = [p[len("chroma="):] for p in parts if p.startswith("chroma=")]
    if not vals:
        return "444", arith
    if len(vals) != 1 or vals[0] not in ("420", "400"):
        raise ValueError("chroma: unknown chroma format %r in the arithmetic string (this decoder reads 420 and 400, once; 4:4:4 "
                         "has no key)" % ",".join(vals))
    return vals[0], ",".join(p for p in parts if not p.startswith("chroma="))


def _with_chroma(arith, chroma):
    """The arithmetic string (without a chroma key) with the key of the format merged in at its sorted place; "444": unchanged."""
    if check_chroma(chroma) == "444":
        return arith
    return ",".join(sorted((arith.split(",") if arith else []) + ["chroma=%s" % chroma]))


def _no_chroma(bh, what):
    """Refuses a base header that carries a chroma key under a wrapper or lapped container (``what`` names it and the argument
    it stands for): those layers have no 4:2:0 / 4:0:0 form."""
    if "chroma" in bh:
        raise ValueError("chroma: the base container is coded with chroma=%s, which does not compose with %s" % (bh["chroma"], what))


# sample depth: 8 is the uint8 path and writes no key; the arithmetic string's "depth" key holds 9 .. 16
DEPTH_MIN, DEPTH_MAX = 9, 16


def check_depth(depth):
    """The depth argument of the API -> 8 (None or 8: uint8 samples) or the bit depth 9 .. 16 of uint16 samples.  ValueError
    naming depth otherwise."""
    if depth is None:
        return 8
    if isinstance(depth, bool) or not isinstance(depth, int) or not (depth == 8 or DEPTH_MIN <= depth <= DEPTH_MAX):
        raise ValueError("depth must be None or an integer in [8, %d] (got %r)" % (DEPTH_MAX, depth))
    return depth


def _split_depth(arith):
    """arithmetic string -> (depth, the string without the depth key); 8 when the key is absent.  ValueError naming depth if the
    key occurs twice or its value is not a canonical decimal integer in [9, 16] (8 bits are written by leaving the key out)."""
    parts = arith.split(",") if arith else []
    vals = [p[len("depth="):] for p in parts if p.startswith("depth=")]
    if not vals:
        return 8, arith
    ok = len(vals) == 1 and vals[0].isascii() and vals[0].isdigit() and vals[0] == str(int(vals[0])) \
        and DEPTH_MIN <= int(vals[0]) <= DEPTH_MAX
    if not ok:
        raise ValueError("depth: bad sample depth %r in the arithmetic string (an integer in [%d, %d], once; 8 bits have no key)"
                         % (",".join(vals), DEPTH_MIN, DEPTH_MAX))
    return int(vals[0]), ",".join(p for p in parts if not p.startswith("depth="))


def _with_depth(arith, depth):
    """The arithmetic string (without a depth key) with the key of the depth merged in at its sorted place; None and 8: unchanged."""
    d = check_depth(depth)
    if d == 8:
        return arith
    return ",".join(sorted((arith.split(",") if arith else []) + ["depth=%d" % d]))


def _no_depth(bh, what):
    """Refuses a base header that carries a depth key under a wrapper or lapped container (``what`` names it and the argument
    it stands for): those layers are built for 8-bit samples."""
    if bh.get("depth", 8) != 8:
        raise ValueError("depth: the base container is coded with depth=%d, which does not compose with %s" % (bh["depth"], what))


def _blocks(v, L):
    """ceil(v / 2^L): blocks of a step map along a side of v pixels."""
    return -(-int(v) >> L)


def check_step_map(step_map, H, W, L):
    """A step map of the API for an H x W image at L levels -> the (hb, wb) uint16 numpy array of n, step = n / 16.  step_map:
    (hb, wb) = (ceil(H / 2^L), ceil(W / 2^L)) steps (a tensor, an array or nested lists), each exactly n / 16 with n in [4, 1024].
    ValueError naming step_map for a wrong shape or value, or L < 2 (a step reaches the levels below the coarsest only)."""
    import numpy as np
    if L < 2:
        raise ValueError("step_map: a step map needs dwtlevels >= 2 (it applies to the levels below the coarsest; got %d)" % L)
    try:
        a = np.asarray(step_map.detach().cpu().numpy() if hasattr(step_map, "detach") else step_map, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("step_map must be a (hb, wb) array of steps") from None
    hb, wb = _blocks(H, L), _blocks(W, L)
    if a.shape != (hb, wb):
        raise ValueError("step_map: shape %s, a %d x %d image at %d levels has %d x %d blocks of %d pixels"
                         % (tuple(a.shape), H, W, L, hb, wb, 1 << L))
    if hb > 0xFFFF or wb > 0xFFFF:
        raise ValueError("step_map: hb, wb must fit 16 bits (got %d x %d)" % (hb, wb))
    n = a * STEP_DENOM
    if not (np.isfinite(n).all() and (n >= STEP_N_MIN).all() and (n <= STEP_N_MAX).all() and (n == np.rint(n)).all()):
        raise ValueError("step_map: every step must be n / %d with an integer n in [%d, %d], i.e. a multiple of %g in [%g, %g]"
                         % (STEP_DENOM, STEP_N_MIN, STEP_N_MAX, 1.0 / STEP_DENOM, STEP_N_MIN / STEP_DENOM, STEP_N_MAX / STEP_DENOM))
    return n.astype(np.uint16)


def step_map_from_regions(H, W, L, background, regions):
    """A step map painted from rectangles -> (hb, wb) float64 numpy array of steps for step_map=.  Every block starts at the step
    ``background``; regions is a list of (y0, x0, h, w, step) in pixels: every block that a rectangle intersects takes that
    rectangle's step, later rectangles override earlier ones.  ValueError naming step_map for an empty rectangle or one that is
    not inside the image, and for steps check_step_map refuses."""
    import numpy as np
    hb, wb = _blocks(H, L), _blocks(W, L)
    m = np.full((hb, wb), check_step(background) / STEP_DENOM, dtype=np.float64)
    for r in regions:
        try:
            y0, x0, h, w = (int(v) for v in r[:4])
            q = check_step(r[4]) / STEP_DENOM
            ok = len(r) == 5
        except (TypeError, ValueError, IndexError):
            ok = False
        if not ok:
            raise ValueError("step_map: a region must be (y0, x0, h, w, step) with a step n / 16 (got %r)" % (r,))
        if h < 1 or w < 1 or y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
            raise ValueError("step_map: region (%d, %d, %d, %d) is empty or not inside the %d x %d image" % (y0, x0, h, w, H, W))
        m[y0 >> L:((y0 + h - 1) >> L) + 1, x0 >> L:((x0 + w - 1) >> L) + 1] = q
    check_step_map(m, H, W, L)
    return m


def map_crc(map_n):
    """zlib.crc32 of a step map's values n as little-endian u16 in raster order (the LLDQ field and the qmap key)."""
    import numpy as np
    return zlib.crc32(np.ascontiguousarray(map_n, dtype="<u2").tobytes()) & 0xFFFFFFFF


def _base_header(hdr):
    """The header that carries the arithmetic string: the nested base header of an LLDR header, the header itself otherwise."""
    return hdr["base"] if "base" in hdr else hdr


def pack_mapped(map_n, inner):
    """map_n: (hb, wb) integer array of n = 16 * step; inner: a complete LLDW, LLDT, LLDO or LLDR container whose base carries
    ``qmap=<CRC of the map>`` -> LLDQ container.  The map is written as maximal runs in raster order.  ValueError naming the
    field when the map does not belong to the inner container; host only."""
    import numpy as np
    a = np.asarray(map_n)
    if a.ndim != 2 or a.dtype.kind not in "iu" or a.size == 0 or int(a.min()) < STEP_N_MIN or int(a.max()) > STEP_N_MAX:
        raise ValueError("step map: a (hb, wb) integer array of n in [%d, %d]" % (STEP_N_MIN, STEP_N_MAX))
    if _magic(inner) not in (MAGIC, TILED_MAGIC, LAPPED_MAGIC, REFINED_MAGIC):
        raise ValueError("inner container: a step map goes over an LLDW, LLDT, LLDO or LLDR container")
    bh = _base_header(read_header(inner))
    _no_chroma(bh, "a step map (step_map)")
    _no_depth(bh, "a step map (step_map)")
    L, hb, wb = bh["dwtlevels"], a.shape[0], a.shape[1]
    if (hb, wb) != (_blocks(bh["H"], L), _blocks(bh["W"], L)) or hb > 0xFFFF or wb > 0xFFFF:
        raise ValueError("hb, wb: a %d x %d map for an inner container of %d x %d pixels at %d levels" % (hb, wb, bh["H"], bh["W"], L))
    crc = map_crc(a)
    if _split_qmap(bh["arithmetic"])[0] != crc:
        raise ValueError("step map: the inner container's qmap key does not hold the CRC of this map (%08x)" % crc)
    flat = a.reshape(-1).astype(np.int64)
    cut = np.flatnonzero(np.diff(flat)) + 1
    starts = np.concatenate(([0], cut))
    lengths = np.diff(np.concatenate((starts, [flat.size])))
    body = bytearray(_QFIXED.pack(MAPPED_MAGIC, MAPPED_FORMAT_VERSION, L, hb, wb, crc))
    body += leb128_encode(len(starts))
    for st, ln in zip(starts.tolist(), lengths.tolist()):
        body += leb128_encode(ln) + struct.pack("<H", int(flat[st]))
    body += leb128_encode(len(inner)) + bytes(inner)
    return _seal(bytes(body))


def parse_mapped(blob):
    """LLDQ container -> (header dict, the (hb, wb) uint16 numpy array of n, the inner container's bytes).  The header carries
    version, block, hb, wb, map_crc, step_min, step_max (floats) and inner, the inner container's header.  Every check raises
    ValueError naming the field, on the host: magic, version, CRC, truncation; the runs (a length of 0, an n outside [4, 1024],
    adjacent runs of one value, a sum other than hb * wb); the map CRC; the inner container (parsed by its own parser); block
    log2, hb, wb against the inner header; and the inner base's qmap key against the map CRC."""
    import numpy as np
    blob, end = _open(blob, MAPPED_MAGIC, MAPPED_FORMAT_VERSION, _QFIXED.size + 1 + 3 + 1)
    _, _, block, hb, wb, crc = _QFIXED.unpack_from(blob, 0)
    try:
        nruns, pos = leb128_decode(blob, _QFIXED.size, end)
    except ValueError:
        raise ValueError("run count: container truncated or varint too long") from None
    if hb < 1 or wb < 1:
        raise ValueError("hb, wb: a step map of %d x %d blocks" % (hb, wb))
    if nruns < 1 or nruns > hb * wb:
        raise ValueError("run count: %d runs for a map of %d x %d blocks" % (nruns, hb, wb))
    vals, lens, prev, total = [], [], None, 0
    for r in range(nruns):
        try:
            ln, pos = leb128_decode(blob, pos, end)
        except ValueError:
            raise ValueError("runs: container truncated inside run %d" % r) from None
        if pos + 2 > end:
            raise ValueError("runs: container truncated inside run %d" % r)
        n = struct.unpack_from("<H", blob, pos)[0]
        pos += 2
        if ln < 1:
            raise ValueError("runs: run %d has length 0" % r)
        if not STEP_N_MIN <= n <= STEP_N_MAX:
            raise ValueError("runs: run %d holds n = %d, outside [%d, %d]" % (r, n, STEP_N_MIN, STEP_N_MAX))
        if n == prev:
            raise ValueError("runs: runs %d and %d hold the same n = %d (the runs are not maximal)" % (r - 1, r, n))
        total += ln
        if total > hb * wb:
            break
        vals.append(n)
        lens.append(ln)
        prev = n
    if total != hb * wb:
        raise ValueError("runs: the runs add up to %s%d blocks, the map has %d x %d = %d"
                         % ("more than " if total > hb * wb else "", min(total, hb * wb), hb, wb, hb * wb))
    m = np.repeat(np.asarray(vals, dtype=np.uint16), lens).reshape(hb, wb)
    if map_crc(m) != crc:
        raise ValueError("map CRC32: the runs give %08x, the container holds %08x" % (map_crc(m), crc))
    try:
        ilen, pos = leb128_decode(blob, pos, end)
    except ValueError:
        raise ValueError("inner length: container truncated or varint too long") from None
    if pos + ilen != end:
        raise ValueError("inner length: %d bytes announced, %d left" % (ilen, max(0, end - pos)))
    inner = blob[pos:end]
    if _magic(inner) not in (MAGIC, TILED_MAGIC, LAPPED_MAGIC, REFINED_MAGIC):
        raise ValueError("inner container: a step map goes over an LLDW, LLDT, LLDO or LLDR container (got magic %r)" % inner[:4])
    ih = parse_refined(inner, check_tables=False)[0] if _magic(inner) == REFINED_MAGIC else _parse_base(_magic(inner), inner)[0]
    bh = _base_header(ih)
    _no_chroma(bh, "a step map (step_map)")
    _no_depth(bh, "a step map (step_map)")
    if block != bh["dwtlevels"]:
        raise ValueError("block log2: the container holds %d, the inner container has dwtlevels %d" % (block, bh["dwtlevels"]))
    if block < 2:
        raise ValueError("block log2: a step map needs dwtlevels >= 2 (got %d)" % block)
    if (hb, wb) != (_blocks(bh["H"], block), _blocks(bh["W"], block)):
        raise ValueError("hb, wb: the container holds %d x %d, the inner container's %d x %d pixels at %d levels give %d x %d"
                         % (hb, wb, bh["H"], bh["W"], block, _blocks(bh["H"], block), _blocks(bh["W"], block)))
    key = _split_qmap(bh["arithmetic"])[0]
    if key != crc:
        raise ValueError("step map: the inner container's qmap key is %s, the map's CRC is %08x (the map was not the one the "
                         "streams were coded with)" % ("absent" if key is None else "%08x" % key, crc))
    hdr = dict(version=MAPPED_FORMAT_VERSION, block=block, hb=hb, wb=wb, map_crc=crc, step_min=int(m.min()) / STEP_DENOM,
               step_max=int(m.max()) / STEP_DENOM, inner=ih)
    return hdr, m, inner


def target_bpp_bytes(bpp, H, W):
    """A rate target in bits per pixel -> the byte target floor(bpp * H * W / 8) of an H x W image."""
    import math
    bpp = float(bpp)
    if not (bpp == bpp and 0 < bpp < float("inf")):
        raise ValueError("target_bpp must be a positive number (got %r)" % (bpp,))
    return int(math.floor(bpp * H * W / 8.0))


def leb128_encode(n):
    """Unsigned LEB128: 7 bits per byte, low groups first, high bit = more bytes follow."""
    if n < 0:
        raise ValueError("LEB128: negative value %d" % n)
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        if n:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def leb128_decode(buf, pos, end=None):
    """-> (value, next position); ValueError if the varint runs past ``end`` or beyond 9 bytes (63 bits)."""
    end = len(buf) if end is None else end
    n = shift = 0
    for i in range(9):
        if pos + i >= end:
            raise ValueError("container truncated inside the stream lengths")
        b = buf[pos + i]
        n |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            return n, pos + i + 1
    raise ValueError("stream lengths: varint longer than 9 bytes")


def _pack_identity(hdr):
    """The arithmetic string and weights digest fields (u8 length + ASCII, 16 bytes), shared by LLDW and LLDT."""
    arith = hdr["arithmetic"].encode("ascii")
    if len(arith) > 255:
        raise ValueError("arithmetic string longer than 255 bytes")
    if len(hdr["digest"]) != 16:
        raise ValueError("weights digest must be 16 bytes")
    return bytes([len(arith)]) + arith + hdr["digest"]


def _pack_streams(streams):
    """LEB128 stream lengths, then the payload."""
    body = bytearray()
    for s in streams:
        body += leb128_encode(len(s))
    for s in streams:
        body += s
    return bytes(body)


def _seal(body):
    return bytes(body) + struct.pack("<I", zlib.crc32(body) & 0xFFFFFFFF)


def _open(blob, magic, version, min_header):
    """The checks every container starts with: type, magic, version, minimum length, CRC32 -> (bytes, end of payload)."""
    if not isinstance(blob, (bytes, bytearray, memoryview)):
        raise ValueError("container must be bytes (got %s)" % type(blob).__name__)
    blob = bytes(blob)
    if len(blob) < 4 or blob[:4] != magic:
        raise ValueError("bad magic: not an %s container" % magic.decode())
    if len(blob) < 5:
        raise ValueError("container truncated before the format version")
    if blob[4] != version:
        raise ValueError("unsupported format version %d (this decoder reads %d)" % (blob[4], version))
    end = len(blob) - 4
    if end < min_header:
        raise ValueError("container truncated: %d bytes is shorter than the smallest header" % len(blob))
    if struct.unpack_from("<I", blob, end)[0] != zlib.crc32(blob[:end]) & 0xFFFFFFFF:
        raise ValueError("CRC32 mismatch: the container is corrupted or truncated")
    return blob, end


def _check_model_fields(layer, nettype, L, H, W):
    if layer not in _LAYER_NAMES:
        raise ValueError("unknown entropy layer code %d" % layer)
    if nettype not in _NETTYPE_NAMES:
        raise ValueError("unknown netType code %d" % nettype)
    if L < 1 or H < 1 or W < 1:
        raise ValueError("bad dwtlevels / H / W in the header (%d, %d, %d)" % (L, H, W))


def _parse_identity(blob, pos, end):
    """-> (arithmetic string, digest, count byte, position after the count byte)."""
    alen = blob[pos]
    pos += 1
    if pos + alen + 16 + 1 > end:
        raise ValueError("container truncated inside the arithmetic string / weights digest")
    try:
        arith = blob[pos:pos + alen].decode("ascii")
    except UnicodeDecodeError:
        raise ValueError("arithmetic string is not ASCII") from None
    pos += alen
    digest = blob[pos:pos + 16]
    pos += 16
    return arith, digest, blob[pos], pos + 1


def _split_coder(arith):
    """arithmetic string -> (coder name, the string without the coder key).  ValueError naming coder if its value is
    unknown."""
    parts = arith.split(",") if arith else []
    rest = [p for p in parts if not p.startswith("coder=")]
    vals = [p[len("coder="):] for p in parts if p.startswith("coder=")]
    if not vals:
        return "host", arith
    if len(vals) > 1 or vals[0] not in _CODER_NAMES:
        raise ValueError("coder: unknown entropy coder %r in the arithmetic string (this decoder reads: %s)"
                         % (",".join(vals), ", ".join(sorted(_CODER_NAMES))))
    return _CODER_NAMES[vals[0]], ",".join(rest)


def _parse_streams(blob, pos, end, count):
    """count LEB128 lengths, then the payload up to end -> (list of stream bytes, lengths)."""
    lengths = []
    for _ in range(count):
        n, pos = leb128_decode(blob, pos, end)
        lengths.append(n)
    if pos + sum(lengths) != end:
        raise ValueError("stream lengths: payload is %d bytes, the lengths add up to %d" % (end - pos, sum(lengths)))
    streams = []
    for n in lengths:
        streams.append(blob[pos:pos + n])
        pos += n
    return streams, lengths


def _check_overlap(L, th, tw, ov):
    """The overlap of a lapped grid against the level count and the tile size (ValueError naming overlap)."""
    if ov < 1 or ov & (ov - 1):
        raise ValueError("overlap: %d is not a power of two (the cross-fade weights must be exact in fp32)" % ov)
    if ov < 1 << L:
        raise ValueError("overlap: %d is below 2^dwtlevels = %d (the tile stride must stay a multiple of it)" % (ov, 1 << L))
    if 2 * ov > min(th, tw):
        raise ValueError("overlap: %d is more than half of a %d x %d tile (at most two tiles may cover a pixel along an axis)"
                         % (ov, th, tw))


def _check_grid(nettype, L, H, W, th, tw, ny, nx, ov=None, chroma="444"):
    """The grid fields of an LLDT (ov = None) or LLDO header against the image size and the transform (ValueError naming
    the field): the overlap rule of a lapped grid, then along each axis of n tiles of t at the stride s = t - ov (s = t for
    LLDT): (n - 1) s + t >= size, and for n >= 2 the last tile is needed, (n - 2) s + t < size.  chroma "420": the half of the
    tile, its chroma plane, must be a size the transform accepts (chroma_sizes)."""
    from .graphs.layers.lifting_dwt_nets import padded_dims
    if th < 1 or tw < 1 or ny < 1 or nx < 1:
        raise ValueError("tile grid: th, tw, ny, nx must be positive (got %d, %d, %d, %d)" % (th, tw, ny, nx))
    if chroma == "420":
        if th % 2 or tw % 2 or padded_dims(L, nettype == "CDF97", th // 2, tw // 2) != (th // 2, tw // 2):
            raise ValueError("tile size: the chroma plane of a %d x %d tile with chroma=420, %g x %g, is not a size the %s "
                             "transform at %d levels accepts" % (th, tw, th / 2, tw / 2, nettype, L))
    elif padded_dims(L, nettype == "CDF97", th, tw) != (th, tw):
        raise ValueError("tile size: %d x %d is not a size the %s transform at %d levels accepts" % (th, tw, nettype, L))
    if ov is not None:
        _check_overlap(L, th, tw, ov)
    sh, sw = th - (ov or 0), tw - (ov or 0)
    if (ny - 1) * sh + th < H or (ny >= 2 and (ny - 2) * sh + th >= H):
        raise ValueError("tile grid rows: %d tiles of %d rows%s do not fit an image of %d rows"
                         % (ny, th, "" if ov is None else " at a stride of %d" % sh, H))
    if (nx - 1) * sw + tw < W or (nx >= 2 and (nx - 2) * sw + tw >= W):
        raise ValueError("tile grid columns: %d tiles of %d columns%s do not fit an image of %d columns"
                         % (nx, tw, "" if ov is None else " at a stride of %d" % sw, W))


def _check_grid_lapped(nettype, L, H, W, th, tw, ny, nx, ov):
    """The grid fields of an LLDO header: _check_grid with the overlap rule (an overlap of 0 is refused)."""
    _check_grid(nettype, L, H, W, th, tw, ny, nx, int(ov))


def _pack_base(magic, hdr, units):
    """The pack routine of the three base containers.  hdr: dict with layer, netType, dwtlevels, H, W, numerics, arithmetic,
    digest, for LLDT / LLDO also th, tw, ny, nx and for LLDO overlap; units: the stream lists, one for LLDW (written as it is:
    the parser refuses a count other than 3 (L + 1)), ny * nx of 3 (L + 1) streams in raster order of (ty, tx) otherwise."""
    version, fixed = _BASE[magic]
    L, grid = hdr["dwtlevels"], ()
    chroma = _split_chroma(hdr["arithmetic"])[0]
    depth = _split_depth(hdr["arithmetic"])[0]
    if magic == LAPPED_MAGIC and depth != 8:
        raise ValueError("depth: depth=%d does not compose with lapped tiles (overlap)" % depth)
    if magic == MAGIC:
        count = len(units[0])
    else:
        count = CHROMA_PLANES[chroma] * (L + 1)
        grid = (hdr["th"], hdr["tw"], hdr["ny"], hdr["nx"]) + ((hdr["overlap"],) if magic == LAPPED_MAGIC else ())
        if magic == LAPPED_MAGIC and chroma != "444":
            raise ValueError("chroma: chroma=%s does not compose with lapped tiles (overlap)" % chroma)
        _check_grid(hdr["netType"], L, hdr["H"], hdr["W"], *grid, chroma=chroma)
        if hdr["ny"] > 0xFFFF or hdr["nx"] > 0xFFFF:
            raise ValueError("tile grid: ny, nx must fit 16 bits")
        if len(units) != hdr["ny"] * hdr["nx"] or any(len(u) != count for u in units):
            raise ValueError("stream count: expected %d tiles of %d streams" % (hdr["ny"] * hdr["nx"], count))
    ident = _pack_identity(hdr)
    if count > 255:
        raise ValueError("more than 255 streams")
    head = fixed.pack(magic, version, LAYER_CODES[hdr["layer"]], NETTYPE_CODES[hdr["netType"]], L, hdr["H"], hdr["W"], *grid,
                      hdr["numerics"])
    return _seal(head + ident + bytes([count]) + _pack_streams([s for u in units for s in u]))


def _parse_base(magic, blob):
    """The parse routine of the three base containers -> (header dict, list of per-unit lists of stream bytes: one unit for
    LLDW, ny * nx for LLDT / LLDO).  Every structural check (magic, version, CRC, truncation, the grid, stream count,
    lengths) raises ValueError naming the field; nothing here touches the GPU library.  A tiled header carries th, tw, ny,
    nx, overlap (0 for LLDT) and streams_per_tile; an LLDW header has none of them."""
    version, fixed = _BASE[magic]
    blob, end = _open(blob, magic, version, fixed.size + 1 + 16 + 1)
    _, _, layer, nettype, L, H, W, *grid, numerics = fixed.unpack_from(blob, 0)
    _check_model_fields(layer, nettype, L, H, W)
    arith, digest, count, pos = _parse_identity(blob, fixed.size, end)
    chroma, _ = _split_chroma(arith)
    depth, _ = _split_depth(arith)
    if magic == LAPPED_MAGIC and depth != 8:
        raise ValueError("depth: the container is coded with depth=%d, which does not compose with lapped tiles (overlap)" % depth)
    if magic == LAPPED_MAGIC and chroma != "444":
        raise ValueError("chroma: the container is coded with chroma=%s, which does not compose with lapped tiles (overlap)"
                         % chroma)
    if grid:
        _check_grid(_NETTYPE_NAMES[nettype], L, H, W, *grid, chroma=chroma)
    if count != CHROMA_PLANES[chroma] * (L + 1):
        raise ValueError("stream count %d%s does not match dwtlevels %d%s (expected %d)"
                         % (count, " per tile" if grid else "", L, "" if chroma == "444" else " with chroma=%s" % chroma,
                            CHROMA_PLANES[chroma] * (L + 1)))
    coder, _ = _split_coder(arith)
    step_n, _ = _split_step(arith)
    n = grid[2] * grid[3] if grid else 1
    streams, lengths = _parse_streams(blob, pos, end, n * count)
    hdr = dict(version=version, layer=_LAYER_NAMES[layer], netType=_NETTYPE_NAMES[nettype], dwtlevels=L, H=H, W=W,
               numerics=numerics, arithmetic=arith, coder=coder, step=step_n / STEP_DENOM, digest=digest,
               stream_lengths=lengths, header_bytes=end - sum(lengths))
    if depth != 8:                                    # only with the key, like chroma: a key-less header is what it was
        hdr["depth"] = depth
    if chroma != "444":                               # only with the key: a key-less header is what it was
        hdr["chroma"] = chroma
    if grid:
        hdr.update(th=grid[0], tw=grid[1], ny=grid[2], nx=grid[3], overlap=grid[4] if magic == LAPPED_MAGIC else 0,
                   streams_per_tile=count)
    return hdr, [streams[u * count:(u + 1) * count] for u in range(n)]


def pack_container(hdr, streams):
    """hdr: dict with layer, netType, dwtlevels, H, W, numerics, arithmetic, digest; streams: list of bytes -> container."""
    return _pack_base(MAGIC, hdr, [streams])


def parse_container(blob):
    """Container -> (header dict, list of stream bytes); ValueError as _parse_base, host only."""
    hdr, units = _parse_base(MAGIC, blob)
    return hdr, units[0]


def pack_tiled(hdr, tile_streams):
    """hdr: as pack_container plus th, tw, ny, nx; tile_streams: ny * nx lists of 3 (L + 1) streams in raster order of
    (ty, tx) -> LLDT container."""
    return _pack_base(TILED_MAGIC, hdr, tile_streams)


def parse_tiled(blob):
    """LLDT container -> (header dict, list of ny * nx lists of stream bytes).  The structural checks of parse_container plus
    the grid (ValueError naming the field); host only.  The dict carries overlap = 0 (LLDO: parse_lapped)."""
    return _parse_base(TILED_MAGIC, blob)


def pack_lapped(hdr, tile_streams):
    """hdr: as pack_tiled plus overlap (> 0); tile_streams as pack_tiled -> LLDO container."""
    return _pack_base(LAPPED_MAGIC, hdr, tile_streams)


def parse_lapped(blob):
    """LLDO container -> (header dict with overlap, list of ny * nx lists of stream bytes).  The structural checks of
    parse_tiled with the lapped grid rule (ValueError naming the field); host only."""
    return _parse_base(LAPPED_MAGIC, blob)


def pack_refined(near, table_crc, base, units):
    """near: the bound d; table_crc: residual.tables(d).crc; base: a complete LLDW or LLDT container; units: per unit, in
    tile order, dict(cs_xh, cs_x, scales (24 bytes), streams (3 bytes objects)) -> LLDR container."""
    from .residual import CLASSES, CONTEXTS, LADDER_ID, LADDER_SIZE, MAX_NEAR
    if not 0 <= int(near) <= MAX_NEAR:
        raise ValueError("near: %r is outside [0, %d]" % (near, MAX_NEAR))
    if _magic(base) not in (MAGIC, TILED_MAGIC):
        raise ValueError("base container: a residual layer goes over an LLDW or LLDT container")
    bh = read_header(base)
    _no_chroma(bh, "a residual layer (near)")
    _no_depth(bh, "a residual layer (near)")
    if len(units) != bh.get("ny", 1) * bh.get("nx", 1):
        raise ValueError("unit count: %d units for a base of %d" % (len(units), bh.get("ny", 1) * bh.get("nx", 1)))
    body = bytearray(_RFIXED.pack(REFINED_MAGIC, REFINED_FORMAT_VERSION, int(near), CLASSES, LADDER_ID,
                                  table_crc & 0xFFFFFFFF))
    body += leb128_encode(len(base)) + bytes(base) + struct.pack("<I", len(units))
    for u in units:
        sc = bytes(u["scales"])
        if len(sc) != CONTEXTS or max(sc) >= LADDER_SIZE:
            raise ValueError("scale index: a unit needs %d table indexes below %d" % (CONTEXTS, LADDER_SIZE))
        if len(u["streams"]) != _PLANES:
            raise ValueError("stream count: a unit has %d streams" % _PLANES)
        body += _RUNIT.pack(u["cs_xh"], u["cs_x"] if near == 0 else 0, sc)
    return _seal(bytes(body) + _pack_streams([s for u in units for s in u["streams"]]))


def parse_refined(blob, check_tables=True):
    """LLDR container -> (header dict, base container bytes, units), units being per unit dict(cs_xh, cs_x, scales, streams).
    The header carries near, classes, ladder, table_crc, base (the nested base header), units (the count), base_bytes,
    residual_bytes (everything but the base) and stream_lengths.  Every structural check raises ValueError naming the
    field, on the host: magic, version, CRC, truncation, near, classes, ladder id, the base (parsed by its own parser; a
    lapped base is refused), the unit count against the base grid, a table index >= 64, the stream lengths and -- with
    check_tables, which builds the ladder with the library's host code -- the table CRC32."""
    from .residual import CLASSES, LADDER_ID, LADDER_SIZE, MAX_NEAR
    blob, end = _open(blob, REFINED_MAGIC, REFINED_FORMAT_VERSION, _RFIXED.size + 1 + 4)
    _, _, near, classes, ladder, table_crc = _RFIXED.unpack_from(blob, 0)
    if near > MAX_NEAR:
        raise ValueError("near: the container holds %d, the largest bound is %d" % (near, MAX_NEAR))
    if classes != CLASSES:
        raise ValueError("classes: the container holds %d activity classes, this decoder has %d" % (classes, CLASSES))
    if ladder != LADDER_ID:
        raise ValueError("ladder id: the container holds %d, this decoder has %d" % (ladder, LADDER_ID))
    try:
        blen, pos = leb128_decode(blob, _RFIXED.size, end)
    except ValueError:
        raise ValueError("base length: container truncated or varint too long") from None
    if pos + blen + 4 > end:
        raise ValueError("base length: container truncated inside the base container (%d bytes announced, %d left)"
                         % (blen, max(0, end - pos)))
    base = blob[pos:pos + blen]
    if _magic(base) not in (MAGIC, TILED_MAGIC):
        raise ValueError("base container: a residual layer goes over an LLDW or LLDT container (got magic %r)" % base[:4])
    bh = read_header(base)
    _no_chroma(bh, "a residual layer (near)")
    _no_depth(bh, "a residual layer (near)")
    pos += blen
    count = struct.unpack_from("<I", blob, pos)[0]
    pos += 4
    if count != bh.get("ny", 1) * bh.get("nx", 1):
        raise ValueError("unit count: the container holds %d units, the base has %d" % (count, bh.get("ny", 1) * bh.get("nx", 1)))
    if pos + count * _RUNIT.size > end:
        raise ValueError("per-unit fields: container truncated inside them (%d units of %d bytes announced, %d bytes left)"
                         % (count, _RUNIT.size, max(0, end - pos)))
    units = []
    for u in range(count):
        cs_xh, cs_x, sc = _RUNIT.unpack_from(blob, pos)
        pos += _RUNIT.size
        if max(sc) >= LADDER_SIZE:
            raise ValueError("scale index: unit %d holds table index %d, the ladder has %d tables" % (u, max(sc), LADDER_SIZE))
        units.append(dict(cs_xh=cs_xh, cs_x=cs_x, scales=sc))
    streams, lengths = _parse_streams(blob, pos, end, _PLANES * count)
    for u in range(count):
        units[u]["streams"] = streams[_PLANES * u:_PLANES * (u + 1)]
    if check_tables:
        from .residual import tables
        if tables(near).crc != table_crc:
            raise ValueError("table CRC32: the container's ladder for near=%d has CRC %08x, this platform builds %08x; the "
                             "streams cannot be decoded here" % (near, table_crc, tables(near).crc))
    hdr = dict(version=REFINED_FORMAT_VERSION, near=near, classes=classes, ladder=ladder, table_crc=table_crc, base=bh,
               units=count, base_bytes=blen, residual_bytes=len(blob) - blen, stream_lengths=lengths)
    return hdr, base, units


def _check_layered_base(bh, m):
    """The base header of an LLDP container against its layer count m (ValueError naming the field): a level below the coarsest
    must exist, the base carries one step (no step map), and the finest step n / (16 * 3^m) stays at or above 1 / 16."""
    from .quality_layers import MAX_LAYERS
    if not 1 <= m <= MAX_LAYERS:
        raise ValueError("m: a layered container holds 1 .. %d quality layers (got %d)" % (MAX_LAYERS, m))
    if bh["dwtlevels"] < 2:
        raise ValueError("base container: quality layers refine the levels below the coarsest, which needs dwtlevels >= 2 (the "
                         "base has %d)" % bh["dwtlevels"])
    if _split_qmap(bh["arithmetic"])[0] is not None:
        raise ValueError("base container: quality layers go over a base coded with one step, not a step map")
    n = int(round(bh["step"] * STEP_DENOM))
    if n < 3 ** m:
        raise ValueError("m: %d layers need a base step n / 16 with n / 3^m >= 1 (the base has n = %d)" % (m, n))
    return n


def pack_layered(table_crc, base, layers):
    """table_crc: quality_layers.tables().crc; base: a complete LLDW or LLDT container; layers[j - 1][u]: the 3 (L - 1) streams
    of layer j and unit u (plane-major, inside a plane the levels 0 .. L-2) -> LLDP container."""
    from .quality_layers import K
    if _magic(base) not in (MAGIC, TILED_MAGIC):
        raise ValueError("base container: quality layers go over an LLDW or LLDT container")
    bh = read_header(base)
    _no_chroma(bh, "quality layers (layers)")
    _no_depth(bh, "quality layers (layers)")
    m = len(layers)
    _check_layered_base(bh, m)
    units, per = bh.get("ny", 1) * bh.get("nx", 1), _PLANES * (bh["dwtlevels"] - 1)
    if any(len(lay) != units or any(len(u) != per for u in lay) for lay in layers):
        raise ValueError("stream count: every layer holds %d units of %d streams" % (units, per))
    body = _PFIXED.pack(LAYERED_MAGIC, LAYERED_FORMAT_VERSION, m, K, table_crc & 0xFFFFFFFF)
    body += leb128_encode(len(base)) + bytes(base) + struct.pack("<I", units)
    return _seal(body + _pack_streams([bytes(s) for lay in layers for u in lay for s in u]))


def parse_layered(blob, check_tables=True):
    """LLDP container -> (header dict, base container bytes, layers), layers[j - 1][u] being the 3 (L - 1) streams of layer j and
    unit u.  The header carries layers (m), K, table_crc, base (the nested base header), units, base_bytes, stream_lengths and
    layer_bytes (``layer_bytes``).  Every check raises ValueError naming the field, on the host: magic, version, CRC,
    truncation, m in 1..4, K, the base (parsed by its own parser; LLDW or LLDT with dwtlevels >= 2 and one step), n / 3^m >= 1,
    the unit count, the stream lengths and -- with check_tables -- the table CRC32 against this process's tables."""
    from . import quality_layers
    blob, end = _open(blob, LAYERED_MAGIC, LAYERED_FORMAT_VERSION, _PFIXED.size + 1 + 4)
    _, _, m, K, table_crc = _PFIXED.unpack_from(blob, 0)
    if not 1 <= m <= quality_layers.MAX_LAYERS:
        raise ValueError("m: the container holds %d quality layers, a layered container has 1 .. %d" % (m, quality_layers.MAX_LAYERS))
    if K != quality_layers.K:
        raise ValueError("K: the container's tables have bell positions 0 .. %d, this decoder's 0 .. %d" % (K, quality_layers.K))
    try:
        blen, pos = leb128_decode(blob, _PFIXED.size, end)
    except ValueError:
        raise ValueError("base length: container truncated or varint too long") from None
    if pos + blen + 4 > end:
        raise ValueError("base length: container truncated inside the base container (%d bytes announced, %d left)"
                         % (blen, max(0, end - pos)))
    base = blob[pos:pos + blen]
    if _magic(base) not in (MAGIC, TILED_MAGIC):
        raise ValueError("base container: quality layers go over an LLDW or LLDT container (got magic %r)" % base[:4])
    bh = read_header(base)
    _no_chroma(bh, "quality layers (layers)")
    _no_depth(bh, "quality layers (layers)")
    _check_layered_base(bh, m)
    pos += blen
    base_end = pos
    count = struct.unpack_from("<I", blob, pos)[0]
    pos += 4
    units, per = bh.get("ny", 1) * bh.get("nx", 1), _PLANES * (bh["dwtlevels"] - 1)
    if count != units:
        raise ValueError("unit count: the container holds %d units, the base has %d" % (count, units))
    streams, lengths = _parse_streams(blob, pos, end, m * units * per)
    if check_tables and quality_layers.tables().crc != table_crc:
        raise ValueError("table CRC32: the container's layer tables have CRC %08x, this platform builds %08x; the streams "
                         "cannot be decoded here" % (table_crc, quality_layers.tables().crc))
    layers = [[streams[(j * units + u) * per:(j * units + u + 1) * per] for u in range(units)] for j in range(m)]
    payload = end - sum(lengths)
    sizes = [base_end] + [payload + sum(lengths[:(j + 1) * units * per]) for j in range(m)]
    hdr = dict(version=LAYERED_FORMAT_VERSION, layers=m, K=K, table_crc=table_crc, base=bh, units=units, base_bytes=blen,
               stream_lengths=lengths, layer_bytes=sizes)
    return hdr, base, layers


def layer_bytes(blob):
    """LLDP container -> list of m + 1 ints: entry j is the number of container bytes a decode of the base plus the first j
    layers reads.  Entry 0 ends with the embedded base container; entry j >= 1 is every byte before the payload (the fields
    around the base and all stream lengths) plus the streams of the layers 1 .. j.  The 4-byte CRC32 trailer is not counted.
    CPU only."""
    return list(parse_layered(blob, check_tables=False)[0]["layer_bytes"])


def truncate_layers(blob, j):
    """LLDP container -> a valid container holding its first j layers (0 <= j <= m): for j = 0 the base container itself, else
    an LLDP container with m = j whose streams are the first j layers' bytes.  CPU only."""
    hdr, base, layers = parse_layered(blob, check_tables=False)
    if isinstance(j, bool) or not isinstance(j, int) or not 0 <= j <= hdr["layers"]:
        raise ValueError("layers: the container holds %d layers, asked to keep %r" % (hdr["layers"], j))
    return bytes(base) if j == 0 else pack_layered(hdr["table_crc"], base, layers[:j])


def _magic(blob):
    return bytes(blob[:4]) if isinstance(blob, (bytes, bytearray, memoryview)) else None


def read_header(blob):
    """The header of a container (LLDW, LLDT, LLDO, LLDR or LLDQ) as a dict (CPU only; the library is never loaded).  An LLDQ
    header carries version, block, hb, wb, map_crc, step_min, step_max and the inner container's header under ``inner``
    (parse_mapped).  A tiled
    header carries ``overlap``: 0 for LLDT.  An LLDR header carries ``near``, ``residual_bytes`` and the nested base header
    under ``base`` (parse_refined; the table CRC is compared by the decoders).  Raises ValueError as parse_container /
    parse_tiled / parse_lapped / parse_refined.  An LLDP header carries ``layers`` (the number of quality layers m),
    ``layer_bytes`` and the nested base header under ``base`` (parse_layered; the table CRC is compared by the decoders)."""
    if _magic(blob) == LAYERED_MAGIC:
        return parse_layered(blob, check_tables=False)[0]
    if _magic(blob) == MAPPED_MAGIC:
        return parse_mapped(blob)[0]
    if _magic(blob) == REFINED_MAGIC:
        return parse_refined(blob, check_tables=False)[0]
    return _parse_base(_magic(blob) if _magic(blob) in _BASE else MAGIC, blob)[0]


def reduce_bytes(hdr):
    """-> list of L + 1 ints: entry k is the number of container bytes a decode at reduce=k reads, the header (every byte
    before the payload) plus the xe streams and the xo streams of levels k .. L-1 of every plane (for LLDT / LLDO, of every
    tile).  The 4-byte CRC32 trailer is not counted.  hdr: read_header's dict (LLDW, LLDT or LLDO; for LLDR the base alone is
    counted, as a reduced decode never reads the residual layer); CPU only."""
    if "inner" in hdr:
        hdr = hdr["inner"]
    if "base" in hdr:
        hdr = hdr["base"]
    L, lengths = hdr["dwtlevels"], hdr["stream_lengths"]
    per = L + 1                                       # streams per plane: xe, xo finest -> coarsest
    if len(lengths) % per:
        raise ValueError("stream lengths: %d streams are not a whole number of planes of %d" % (len(lengths), per))
    out = []
    for k in range(L + 1):
        need = sum(n for i, n in enumerate(lengths) if i % per == 0 or i % per - 1 >= k)
        out.append(hdr["header_bytes"] + need)
    return out


# ------------------------------------------------------------------------------------------------ model identity
def arithmetic_string(coder="host", step=None, qmap=None, chroma=None, depth=None):
    """Canonical "key=value,..." of every process switch that selects the arithmetic of the coding context path, plus the
    entropy coder: ``coder=irans32`` for coder="gpu", no key for the host coder (so the host string is unchanged), plus the
    quantisation step: ``step=<n>`` for step = n / 16 other than 1, no key for None or 1; or, for a step map,
    ``qmap=<8 hex digits>`` of its CRC (qmap: the CRC as an int), which excludes a step; plus the chroma format:
    ``chroma=420`` or ``chroma=400``, no key for None or "444" (DESIGN.md 7.1.11); plus the sample depth: ``depth=<d>`` for
    d in 9 .. 16, no key for None or 8.
    Which reach which layer (the others are carried along, harmlessly):
      plc_mode, plc_fuse, plc_algo, plc_shape, storage -- the tree-context pair: conditioned2ZTsepSubbands, onlyEZWT;
      precision -- the split-fp16 pair and cgp chain (conditioned2ZTsepSubbands, onlyEZWT) and the lifting steps (all);
      cgp -- the training path only: the coding wavefront step always runs the split-fp16 register chain.
    DWTConditioned2EntropyLayerZTBlock's phase kernel and the crop-stack conv engine have no switch."""
    from . import ops
    if coder not in CODER_KEYS:
        raise ValueError("coder must be one of %s (got %r)" % (", ".join(sorted(CODER_KEYS)), coder))
    kv = [("cgp", ops.cgp_mode()), ("plc_algo", ops.plc_algo()), ("plc_fuse", int(ops.plc_fuse())),
          ("plc_mode", ops.plc_mode()), ("plc_shape", ops.plc_shape()), ("precision", ops.get_precision()),
          ("storage", ops.storage_dtype())]
    if CODER_KEYS[coder] is not None:
        kv.append(("coder", CODER_KEYS[coder]))
    if qmap is not None and check_step(step) != STEP_DENOM:
        raise ValueError("step and step_map: give one of them (the map holds every step)")
    return _with_depth(_with_chroma(_with_qmap(_with_step(",".join("%s=%s" % p for p in sorted(kv)), check_step(step)), qmap),
                                    chroma), depth)


def _batch_invariant(arith):
    """True when the coding path is per image in this arithmetic, so images can be coded together.  Not so when the
    non-fused split-fp16 pair takes its operand scale from an absmax over the whole batch (plc_fuse=0), or with fp16
    storage (a bound over the batch's parents); the one-product precisions are not verified.  Otherwise: one image per call."""
    # neither the coder nor the step(s) nor the chroma format nor the sample depth change what a batch shares
    arith = _split_depth(_split_chroma(_split_qmap(_split_step(_split_coder(arith)[1])[1])[1])[1])[1]
    d = dict(p.split("=") for p in arith.split(","))
    if d["precision"] != "f16x3" or d["storage"] != "fp32":
        return False
    return d["plc_mode"] == "f32" or d["plc_fuse"] == "1"


def weights_digest(net):
    """First 16 bytes of sha256 over net.named_parameters() sorted by name: name, dtype, shape, contiguous CPU bytes of each.
    Parameters only: the buffers (quantized_cdf, offset, cdf_length, scale_table) are derived from them and rewritten by
    update() during coding."""
    import torch
    from .graphs.layers.masked_conv2d import MaskedConv2d
    h = hashlib.sha256()
    # a MaskedConv2d weight is hashed masked (exact: x * 1 and x * 0), as every forward leaves it; so the digest is the same
    # before and after coding, and is taken on the host before any GPU work of the decoder
    masks = {name + ".weight": m.mask for name, m in net.named_modules() if isinstance(m, MaskedConv2d)}

    def put(b):
        h.update(struct.pack("<Q", len(b)))
        h.update(b)
    for name, p in sorted(net.named_parameters(), key=lambda kv: kv[0]):
        t = p.detach().to("cpu")
        if name in masks:
            t = t * masks[name].to("cpu")
        t = t.contiguous()
        put(name.encode())
        put(str(t.dtype).encode())
        put(struct.pack("<%dq" % t.dim(), *t.shape))
        put(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.digest()[:16]


def _prepare(net):
    """Bring the net to the state coding leaves it in: MaskedConv2d zeroes its masked taps on every forward (apply_mask_, as
    the reference does), and EntropyBottleneck.update() keeps the CDF tables it finds in its buffers (a checkpoint may carry
    stale ones), so rebuild them from the parameters.  Then what the weights digest pins is what the coder uses."""
    import torch
    from .entropy_models import EntropyBottleneck
    from .graphs.layers.masked_conv2d import MaskedConv2d
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, MaskedConv2d):
                m.apply_mask_()
            elif isinstance(m, EntropyBottleneck):
                m.update(force=True)


def describe(net):
    """-> (layer name, netType name, dwtlevels) of a LiftingBasedDWTNetWrapper; refuses what cannot be coded."""
    from .graphs.models.LiftingBasedDWT_net import LiftingBasedDWTNetWrapper
    from .graphs.layers.lifting_dwt_nets import DWTPytorchWaveletsLayer
    if not isinstance(net, LiftingBasedDWTNetWrapper):
        raise TypeError("the codec takes a LiftingBasedDWTNetWrapper (got %s)" % type(net).__name__)
    if net.clrch == 3:
        raise NotImplementedError("the codec codes clrch == 1 only: with clrch == 3 the coded layers define no coding "
                                  "(DWTConditioned2EntropyLayerZTBlock rates 3 of the 9 subband channels)")
    if net.training:
        raise NotImplementedError("the codec needs the net in eval mode: training mode adds quantisation noise")
    n0 = net.nets()[0]
    if n0.entropy_layer not in LAYER_CODES:
        from .graphs.models.LiftingBasedDWT_net import _NOT_CODED
        raise NotImplementedError(_NOT_CODED)
    ae = n0.autoencoder
    if isinstance(ae, DWTPytorchWaveletsLayer):
        return n0.entropy_layer, "CDF97", ae.dwtlevels
    return n0.entropy_layer, "LiftingBasedNeuralWaveletv4", ae.waveletLevel


# ------------------------------------------------------------------------------------------------ public API
def _check_images(images_u8, chroma="444", depth=8):
    """The image batch of an encode or of ``quality`` -> (B, H, W).  depth: 8 takes uint8, 9 .. 16 take uint16;
    a tensor of the other type is a ValueError naming depth."""
    import torch
    ch = 1 if chroma == "400" else 3
    if isinstance(images_u8, torch.Tensor) and images_u8.dtype == torch.uint16 and depth == 8:
        raise ValueError("depth: a uint16 tensor needs depth=<bits per sample> in [%d, %d]" % (DEPTH_MIN, DEPTH_MAX))
    if isinstance(images_u8, torch.Tensor) and images_u8.dtype == torch.uint8 and depth != 8:
        raise ValueError("depth: depth=%d takes a uint16 tensor (got uint8; 8-bit samples need no depth)" % depth)
    dt = torch.uint8 if depth == 8 else torch.uint16
    if not (isinstance(images_u8, torch.Tensor) and images_u8.dtype == dt and images_u8.dim() == 4
            and images_u8.shape[3] == ch):
        raise ValueError("images must be a (B,H,W,%d) %s tensor%s%s" % (ch, "uint8" if depth == 8 else "uint16",
                                                                        "" if chroma == "444" else " with chroma=%s" % chroma,
                                                                        "" if depth == 8 else " with depth=%d" % depth))
    B, H, W, _ = images_u8.shape
    if B < 1 or H < 1 or W < 1 or H >= 1 << 32 or W >= 1 << 32:
        raise ValueError("bad image batch shape %s" % (tuple(images_u8.shape),))
    return B, H, W


def msssim_db(m):
    """MS-SSIM in decibels, -10 log10(1 - m); inf for m >= 1, None for None."""
    import math
    if m is None:
        return None
    return float("inf") if m >= 1.0 else -10.0 * math.log10(1.0 - m)


def _check_range(flag, depth):
    """Reads the range flag of the uint16 input kernels (a synchronisation): ValueError naming depth when one of them met a
    sample above 2^depth - 1 (an error, not a clamp)."""
    if int(flag.item()):
        raise ValueError("depth: the images hold a sample above %d = 2^%d - 1, the largest of depth=%d"
                         % ((1 << depth) - 1, depth, depth))


def quality(a_u8, b_u8, depth=None):
    """PSNR and MS-SSIM of image pairs: (B,H,W,3) or (H,W,3) uint8 RGB tensors of one shape, on the host or the device.
    -> {"psnr": ..., "msssim": ...} with one Python float per image (lists for a batch, plain values for a single (H,W,3)
    pair).  PSNR is 10 log10(1 / mse) on values in [0,1] over the three channels, inf for identical images; MS-SSIM is the
    mean over the channels (ops.ms_ssim, five scales), None when a side is below its minimum of 161.
    depth = d in 9..16: uint16 tensors of d-bit samples, v / (2^d - 1) in [0,1], so the PSNR is
    10 log10(M^2 3 H W / SSE) of the samples; a sample above 2^d - 1 is a ValueError naming depth."""
    import math
    import torch
    from . import ops
    single = isinstance(a_u8, torch.Tensor) and a_u8.dim() == 3
    if single:
        a_u8, b_u8 = a_u8[None], (b_u8[None] if isinstance(b_u8, torch.Tensor) and b_u8.dim() == 3 else b_u8)
    d = check_depth(depth)
    B, H, W = _check_images(a_u8, depth=d)
    _check_images(b_u8, depth=d)
    if tuple(a_u8.shape) != tuple(b_u8.shape):
        raise ValueError("quality: the images differ in shape: %s and %s" % (tuple(a_u8.shape), tuple(b_u8.shape)))
    dev = a_u8.device if a_u8.is_cuda else (b_u8.device if b_u8.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    if d == 8:
        a = ops.u8hwc_to_f32chw(a_u8.to(dev).contiguous())                            # (B,3,H,W) in [0,1]
        b = ops.u8hwc_to_f32chw(b_u8.to(dev).contiguous())
    else:
        flag = ops.depth_flag(dev)
        a = ops.u16hwc_to_f32chw(a_u8.to(dev).contiguous(), d, flag)
        b = ops.u16hwc_to_f32chw(b_u8.to(dev).contiguous(), d, flag)
        _check_range(flag, d)
    sq = torch.zeros(B, dtype=torch.float64, device=dev)
    for i in range(B):
        ops.sq_err_sum(a[i], b[i], sq[i:i + 1])
    ms = None
    if min(H, W) >= ops.ms_ssim_min_side(5):
        ms = ops.ms_ssim(a, b, offset=0.0).mean(1).tolist()
    psnr = [float("inf") if e == 0.0 else 10.0 * math.log10(3.0 * H * W / e) for e in sq.tolist()]
    msssim = ms if ms is not None else [None] * B
    if single:
        return {"psnr": psnr[0], "msssim": msssim[0]}
    return {"psnr": psnr, "msssim": msssim}


def _refine(base_blobs, img, xh, grid, near, coder):
    """The residual layer of a batch: base_blobs: the B base containers; img, xh: (B,H,W,3) uint8 device tensors (originals,
    base reconstructions); grid = (H, W, th, tw, ny, nx) -> B LLDR containers."""
    from . import residual
    per = grid[4] * grid[5]
    units = residual.encode_units(img, xh, grid, list(range(len(base_blobs) * per)), near, coder)
    crc = residual.tables(near).crc
    return [pack_refined(near, crc, base_blobs[b], units[b * per:(b + 1) * per]) for b in range(len(base_blobs))]


def _rdo_arg(rdo, L):
    """The rdo argument of encode_images / encode_tiled, checked on the host -> rho as a float, or None for off."""
    m = check_rdo(rdo)
    if m and L < 2:
        raise ValueError("rdo: rate-distortion optimised quantisation needs dwtlevels >= 2 (it applies to the levels below the "
                         "coarsest; the net has %d)" % L)
    return m / RDO_DENOM if m else None


def _layer_args(layers, step, L, near=None, step_map=None, overlap=0, target_bytes=None, target_psnr=None, target_msssim=None):
    """The layers argument of encode_images / encode_tiled, checked on the host before the other arguments -> m (0: none).
    ValueError naming the pair for everything the layers do not compose with: near (the residual layer sits on the base's
    pixels, which the layers change), step_map (a layer's step is one number per level), overlap > 0, and the three targets
    (they choose a step for a single-rate container); also without a level that carries a step (dwtlevels < 2) and for a step
    below 3^m / 16."""
    from .quality_layers import check_layers, check_step_divides
    m = check_layers(layers)
    if m == 0:
        return 0
    for name, val in (("near", near), ("step_map", step_map), ("target_bytes", target_bytes), ("target_psnr", target_psnr),
                      ("target_msssim", target_msssim)):
        if val is not None:
            raise ValueError("layers and %s: quality layers do not compose with %s" % (name, name))
    if overlap:
        raise ValueError("layers and overlap: quality layers over lapped tiles (overlap > 0) are not defined; use overlap=0")
    if L < 2:
        raise ValueError("layers: quality layers refine the levels below the coarsest, which needs dwtlevels >= 2 (the net has "
                         "%d)" % L)
    check_step_divides(check_step(step), m)
    return m


def _chroma_args(chroma, near=None, layers=None, step_map=None, overlap=0, target_psnr=None, target_msssim=None):
    """The chroma argument of encode_images / encode_tiled, checked on the host before everything else -> "444", "420" or "400".
    ValueError naming chroma and the other argument for what a chroma format does not compose with: each of
    near, layers, step_map, overlap > 0, target_psnr and target_msssim needs a 4:2:0 form of its own kernel."""
    ch = check_chroma(chroma)
    if ch == "444":
        return ch
    for name, val in (("near", near), ("layers", layers), ("step_map", step_map), ("target_psnr", target_psnr),
                      ("target_msssim", target_msssim)):
        if val is not None and not (name == "layers" and not isinstance(val, bool) and val == 0):
            raise ValueError("chroma and %s: chroma=%s does not compose with %s; use chroma=\"444\"" % (name, ch, name))
    if overlap:
        raise ValueError("chroma and overlap: chroma=%s over lapped tiles (overlap > 0) is not defined; use overlap=0" % ch)
    return ch


def _depth_args(depth, near=None, layers=None, step_map=None, overlap=0, target_psnr=None, target_msssim=None):
    """The depth argument of encode_images / encode_tiled, checked on the host before any GPU work -> 8, or d in 9 .. 16.
    ValueError naming depth and the other argument for what more than 8 bits do not compose with: near (the
    residual ladder and its histogram are built for 511 bins), layers, step_map, overlap > 0, target_psnr and target_msssim
    (their kernels measure and blend bytes)."""
    d = check_depth(depth)
    if d == 8:
        return d
    for name, val in (("near", near), ("layers", layers), ("step_map", step_map), ("target_psnr", target_psnr),
                      ("target_msssim", target_msssim)):
        if val is not None and not (name == "layers" and not isinstance(val, bool) and val == 0):
            raise ValueError("depth and %s: depth=%d does not compose with %s; it is defined for 8-bit samples" % (name, d, name))
    if overlap:
        raise ValueError("depth and overlap: depth=%d over lapped tiles (overlap > 0) is not defined; use overlap=0" % d)
    return d


def _rate_args(step, target_bytes, near, L):
    """The rate arguments of encode_images / encode_tiled, checked on the host -> (n of the step, target or None)."""
    if step is not None and target_bytes is not None:
        raise ValueError("step and target_bytes: give one of them (a byte target chooses the step)")
    n = check_step(step)
    if n != STEP_DENOM and L < 2:
        raise ValueError("step: a step other than 1 needs dwtlevels >= 2 (it applies to the levels below the coarsest; the "
                         "net has %d)" % L)
    if target_bytes is None:
        return n, None
    if L < 2:
        raise ValueError("target_bytes: the search varies the step, which needs dwtlevels >= 2 (the net has %d)" % L)
    if near is not None:
        raise ValueError("target_bytes: not with near (the residual layer grows as the base shrinks, so the step does not "
                         "control the size)")
    try:
        T = int(target_bytes)
    except (TypeError, ValueError):
        raise ValueError("target_bytes must be a positive integer (got %r)" % (target_bytes,)) from None
    if T != target_bytes or T < 1:
        raise ValueError("target_bytes must be a positive integer (got %r)" % (target_bytes,))
    return n, T


def _map_arg(step_map, step, target_bytes, B, H, W, L):
    """The step_map argument of encode_images / encode_tiled, checked on the host -> None or the (B, hb, wb) uint16 array of n:
    one (hb, wb) map for the whole batch or (B, hb, wb).  Not with step or target_bytes."""
    import numpy as np
    if step_map is None:
        return None
    if step is not None:
        raise ValueError("step_map and step: give one of them (the map holds every step)")
    if target_bytes is not None:
        raise ValueError("step_map and target_bytes: a byte target over a step map is not defined (it needs a rule for moving a "
                         "whole map along the step grid)")
    dims = step_map.dim() if hasattr(step_map, "dim") else np.ndim(step_map)
    if dims == 3:
        if len(step_map) != B:
            raise ValueError("step_map: %d maps for a batch of %d images" % (len(step_map), B))
        return np.stack([check_step_map(m, H, W, L) for m in step_map])
    m = check_step_map(step_map, H, W, L)
    return np.broadcast_to(m, (B,) + m.shape)


def _unit_maps(maps, units, grid, L, dev):
    """The step maps of a group of units as the coded layers take them: maps[b] is image b's (hb, wb) array of n; units: the
    unit numbers b * ny * nx + ty * nx + tx; grid = (th, tw, ny, nx, ov) -> (len(units), th >> L, tw >> L) int32 tensor on dev.
    A unit's map is the slice of its image's map at the tile's origin (a multiple of 2^L), one entry per coefficient of the
    tile's coarsest level, clamped to the last block where the tile (or the padding) runs past the image."""
    import numpy as np
    import torch
    th, tw, ny, nx, ov = grid
    out = []
    for u in units:
        m = maps[u // (ny * nx)]
        ty, tx = divmod(u % (ny * nx), nx)
        ys = np.minimum(((ty * (th - ov)) >> L) + np.arange(_blocks(th, L)), m.shape[0] - 1)
        xs = np.minimum(((tx * (tw - ov)) >> L) + np.arange(_blocks(tw, L)), m.shape[1] - 1)
        out.append(np.asarray(m)[ys][:, xs])
    return torch.from_numpy(np.stack(out).astype(np.int32)).to(dev)


def _aq_args(aq, L, step_map=None, layers=None, chroma="444", depth=None):
    """The aq argument of encode_images / encode_tiled, checked on the host before any GPU work -> m (0: off).  ValueError naming
    aq and the other argument for what adaptive quantisation does not compose with: step_map (two sources of
    a map), layers (a layer's step is one number per level), a chroma format other than "444" and depth > 8 (the analysis reads
    uint8 RGB); also without a level that carries a step (dwtlevels < 2)."""
    m = check_aq(aq)
    if m == 0:
        return 0
    if step_map is not None:
        raise ValueError("aq and step_map: give one of them (each is a source of the step map)")
    if layers is not None and not (not isinstance(layers, bool) and layers == 0):
        raise ValueError("aq and layers: quality layers do not compose with a step map, so not with aq")
    if check_chroma(chroma) != "444":
        raise ValueError("aq and chroma: aq analyses uint8 RGB, it does not compose with chroma=%s; use chroma=\"444\"" % chroma)
    if check_depth(depth) != 8:
        raise ValueError("aq and depth: aq analyses uint8 RGB, it does not compose with depth=%d" % check_depth(depth))
    if L < 2:
        raise ValueError("aq: a step map needs dwtlevels >= 2 (it applies to the levels below the coarsest; the net has %d)" % L)
    if L > 8:
        raise ValueError("aq: the analysis is defined for blocks of up to 256 pixels, dwtlevels <= 8 (the net has %d)" % L)
    return m


class _Activity:
    """The activity of a batch, computed ONCE on the device (ops.aq_activity); maps(n_q) -> the (B, hb, wb)
    uint16 array of n at the base step n_q / 16, maps(n_q, b) -> that of image b alone as (1, hb, wb): only ops.aq_steps runs."""

    def __init__(self, images_u8, L, m, dev):
        from . import ops
        self.m = m
        self.a, self.A = ops.aq_activity(images_u8.to(dev).contiguous(), L)

    def maps(self, n_q, b=None):
        import numpy as np
        from . import ops
        a, A = (self.a, self.A) if b is None else (self.a[b:b + 1], self.A[b:b + 1])
        return ops.aq_steps(a, A, self.m / AQ_DENOM, n_q).cpu().numpy().astype(np.uint16)


def activity_step_map(images_u8, L, aq, step=1.0):
    """The step map of adaptive quantisation -> (B, hb, wb) float64 numpy array of steps, which step_map=
    accepts: encode_*(..., aq=aq, step=step) writes the bytes of encode_*(..., step_map=activity_step_map(images, L, aq, step)).
    images_u8: (B,H,W,3) uint8 (CPU or device; analysed on the current device); L: the net's dwtlevels (2 .. 8); aq: the strength
    m / 16, m in 1..32; step: the base step n / 16.  Flat blocks get finer and busy blocks coarser steps around the base, a
    quarter octave per octave of (luma variance + 4)^(aq / 4), centred on the image's own mean."""
    import numpy as np
    import torch
    m = _aq_args(aq, L)
    if m == 0:
        raise ValueError("aq: activity_step_map needs a strength m / 16 with m in [1, 32] (got %r)" % (aq,))
    _check_images(images_u8)
    dev = images_u8.device if images_u8.is_cuda else torch.device("cuda", torch.cuda.current_device())
    return _Activity(images_u8, L, m, dev).maps(check_step(step)).astype(np.float64) / STEP_DENOM


def psnr_sse_bound(psnr, H, W):
    """The largest sum of squared byte errors over the 3 H W samples of an H x W uint8 RGB image at which its PSNR,
    10 log10(255^2 * 3 H W / SSE) as ``quality`` reports it, is still at least ``psnr`` dB: floor(3 H W * 65025 / 10^(psnr / 10))
    in float64.  The encoder of target_psnr and its tests call this one function, so that "meets the target" is the integer
    comparison SSE <= bound.  ValueError naming target_psnr unless psnr is a finite number > 0."""
    import math
    try:
        p = float(psnr)
    except (TypeError, ValueError):
        raise ValueError("target_psnr must be a finite number of dB > 0 (got %r)" % (psnr,)) from None
    if not (p == p and 0 < p < float("inf")) or int(H) < 1 or int(W) < 1:
        raise ValueError("target_psnr must be a finite number of dB > 0, for an image of positive size (got %r, %r x %r)"
                         % (psnr, H, W))
    return int(math.floor(3.0 * int(H) * int(W) * 65025.0 / 10.0 ** (p / 10.0)))


def sse_psnr(sse, H, W):
    """The PSNR in dB of an H x W uint8 RGB image whose squared byte errors sum to ``sse``; inf at 0 (as ``quality``)."""
    import math
    return float("inf") if sse == 0 else 10.0 * math.log10(65025.0 * 3.0 * H * W / sse)


def _meets_psnr(sse, psnr, H, W):
    """The predicate of target_psnr: the integer SSE of a decoded image is within psnr_sse_bound."""
    return int(sse) <= psnr_sse_bound(psnr, H, W)


def _quality_args(target_psnr, target_msssim, target_bytes, step, step_map, near, L, H=None, W=None):
    """The quality arguments of encode_images / encode_tiled, checked on the host (ValueError naming the argument) -> None (no
    target), ("psnr", P) or ("msssim", M).  One of target_psnr, target_msssim, target_bytes, step, step_map at most; no target
    with near (the residual layer sets the quality); L >= 2 (the step reaches no level otherwise); P a finite number > 0,
    0 < M < 1; target_msssim needs min(H, W) >= ops.ms_ssim_min_side(5) when the size is given."""
    if target_psnr is None and target_msssim is None:
        return None
    name = "target_psnr" if target_psnr is not None else "target_msssim"
    if target_psnr is not None and target_msssim is not None:
        raise ValueError("target_psnr and target_msssim: give one of them (each chooses the step)")
    for other, val in (("target_bytes", target_bytes), ("step", step), ("step_map", step_map)):
        if val is not None:
            raise ValueError("%s and %s: give one of them (a quality target chooses the step%s)"
                             % (name, other, "; a target over a step map is not defined" if other == "step_map" else ""))
    if near is not None:
        raise ValueError("%s: not with near (the residual layer, not the step, sets the quality of the decoded image)" % name)
    if L < 2:
        raise ValueError("%s: the search varies the step, which needs dwtlevels >= 2 (the net has %d)" % (name, L))
    try:
        v = float(target_psnr if target_psnr is not None else target_msssim)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number (got %r)" % (name, target_psnr if target_psnr is not None else target_msssim)) from None
    if target_psnr is not None:
        if not (v == v and 0 < v < float("inf")):
            raise ValueError("target_psnr must be a finite number of dB > 0 (got %r)" % (target_psnr,))
        return "psnr", v
    if not (v == v and 0 < v < 1):
        raise ValueError("target_msssim must be a number in (0, 1) (got %r)" % (target_msssim,))
    if H is not None and W is not None:
        from .ops import ms_ssim_min_side
        if min(H, W) < ms_ssim_min_side(5):
            raise ValueError("target_msssim: MS-SSIM over five scales needs sides of at least %d pixels (the image is %d x %d)"
                             % (ms_ssim_min_side(5), H, W))
    return "msssim", v


def _search_quality(meets, fail=None):
    """The quality target of DESIGN.md 7.1.9 over the indexes k of STEP_GRID.  meets(k) -> whether the image decoded at step
    STEP_GRID[k] / 16 meets the target; it is called at most once per k (the probes are memoised) and at most
    1 + ceil(log2 33) = 7 times.  Index 0 is probed first: if the finest step misses, ``fail()`` gives the exception to raise
    (a ValueError by default).  Then a bisection with the invariant "meets(lo), and hi == 33 or not meets(hi)" from lo = 0,
    hi = 33 until hi == lo + 1 -> (lo, number of probes): index lo meets the target and the next coarser one does not (or lo is
    the coarsest), whether or not the quality is monotone along the grid; where it falls monotonically, lo is the coarsest
    step that meets the target."""
    memo = {}

    def probe(k):
        if k not in memo:
            memo[k] = bool(meets(k))
        return memo[k]
    if not probe(0):
        raise (fail() if fail is not None else ValueError("the quality target cannot be met at the finest step"))
    lo, hi = 0, len(STEP_GRID)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if probe(mid):
            lo = mid
        else:
            hi = mid
    return lo, len(memo)


# diagnostics: the last search's probes (estimates), real encodes, chosen step and container size; after a quality target also
# the chosen step's "sse" or "msssim" and, under "images", one such dict per image of the batch
SEARCH_STATS = {}


def _search_step(estimate, encode, T):
    """The byte target of DESIGN.md 7.1.6 over STEP_GRID.  estimate(n) -> estimated container bytes at step n / 16 (no range
    coder runs); encode(n) -> the real container.  Bisection on the estimates for the finest grid step that fits T, then
    the walk on REAL containers that alone decides: while the container exceeds T one grid step coarser, otherwise one
    grid step finer as long as that still fits.  -> the container of the finest grid step that is <= T bytes; should the
    sizes not fall monotonically along the grid, the one this walk finds.  ValueError naming target_bytes and the smallest
    achievable size if the coarsest step does not fit."""
    lo, hi = 0, len(STEP_GRID) - 1
    probes = encodes = 0
    while lo < hi:
        mid = (lo + hi) // 2
        probes += 1
        if estimate(STEP_GRID[mid]) <= T:
            hi = mid
        else:
            lo = mid + 1
    k = lo
    blob = encode(STEP_GRID[k])
    encodes += 1
    if len(blob) > T:
        while len(blob) > T:
            if k == len(STEP_GRID) - 1:
                raise ValueError("target_bytes: %d bytes cannot be met; at the coarsest step %g the smallest achievable is %d"
                                 % (T, STEP_GRID[k] / STEP_DENOM, len(blob)))
            k += 1
            blob = encode(STEP_GRID[k])
            encodes += 1
    else:
        while k > 0:
            finer = encode(STEP_GRID[k - 1])
            encodes += 1
            if len(finer) > T:
                break
            blob, k = finer, k - 1
    SEARCH_STATS.update(probes=probes, encodes=encodes, step=STEP_GRID[k] / STEP_DENOM, bytes=len(blob))
    return blob


def _estimated_size(empty, estimates):
    """The size of a container from the estimated stream lengths: ``empty`` is the container packed with empty streams, to
    which the streams and the bytes of their LEB128 lengths beyond the first are added."""
    return len(empty) + sum(e + len(leb128_encode(e)) - 1 for e in estimates)


def encode_images(net, images_u8, coder="host", near=None, step=None, target_bytes=None, rdo=None, step_map=None,
                  layers=None, chroma="444", depth=None, aq=None, target_psnr=None, target_msssim=None):
    """(B,H,W,3) uint8 RGB tensor (CPU or device, one size per call) -> list of B containers (bytes).  coder: "host" (the
    default; rans64 on the host) or "gpu" (irans32 on the device, recorded in the arithmetic string).
    near: None -> LLDW as ever; 0 -> lossless, d in 1..32 -> every decoded sample within d of the original: LLDR containers
    holding the same LLDW bytes plus the residual layer.
    step: the quantisation step q = n / 16 of the levels 0 .. L-2, recorded in the arithmetic string; None
    and 1 write the same bytes as ever.  target_bytes = T instead: per image, the finest step of STEP_GRID whose container is
    at most T bytes (_search_step: estimates first, real containers decide; if the sizes are not monotone along the grid,
    the step that walk finds); ValueError naming the smallest achievable size if even the coarsest step does not fit.  Not
    both, and no target with near.
    rdo: the Lagrangian rho = m / 64 of rate-distortion optimised quantisation on the same levels; None and 0
    write the same bytes as ever.  The encoder's choice only: no header key, and the containers decode as any other.
    step_map: a step per block of 2^L x 2^L pixels: (hb, wb) steps for the whole batch or (B, hb, wb)
    (check_step_map, step_map_from_regions) -> LLDQ containers around what the other arguments select.  Not with step or
    target_bytes.
    target_psnr = P (dB) or target_msssim = M (0 < M < 1) instead of any of step, target_bytes, step_map, and not with near
    (DESIGN.md 7.1.9): per image, a step of STEP_GRID whose decoded image -- the one decode_images returns -- meets the target
    while the next coarser grid step does not (or which is the coarsest); where the quality falls monotonically along the
    grid that is the coarsest step that meets it.  PSNR is met iff the integer SSE of the decoded bytes is at most
    psnr_sse_bound(P, H, W); MS-SSIM (the channel mean ``quality`` reports, sides >= 161) iff the value is >= M -- its sums
    are double atomics, so a target within rounding of a probe's value may resolve either way.  At most 7 probes without a
    range coder, then ONE real encode: the container is byte for byte that of step=<chosen>, nothing is recorded.
    ValueError naming the target and the best achievable value if the finest step misses it.
    layers = m in 1..4: LLDP containers holding the container of the other arguments byte for byte plus m
    quality layers, layer j refining the levels 0 .. L-2 to the step q / 3^j; decode_images(..., layers=j) decodes any prefix.
    With coder, step (n / 3^m >= 1) and rdo; not with near, step_map or a target.  None and 0 write the bytes above.
    chroma: "444" (the default) codes three full-size planes and writes the bytes above; "420" codes Y at full
    and Cb, Cr at half size (the chroma is averaged over 2 x 2 pixels and interpolated back on decoding); "400" takes a
    (B,H,W,1) greyscale tensor and codes one plane.  The format is one more key of the arithmetic string and the decoders read
    it from the header.  With coder, step, target_bytes and rdo; not with near, layers, step_map or a quality target.
    depth: None and 8 take uint8 and write the bytes above; d in 9..16 takes a uint16 tensor of d-bit samples
    (a sample above 2^d - 1 is a ValueError naming depth), recorded as one more key of the arithmetic string; the decoders then
    return uint16.  With coder, step, target_bytes, rdo and chroma; not with near, layers, step_map or a quality target.
    aq = m / 16, m in 1..32: adaptive quantisation, a step map derived from the image on the device -- flat
    blocks of 2^L x 2^L pixels get finer steps, busy ones coarser, around a base step, with the image's mean log-step held.
    With step = q (or none) the bytes are those of step_map=activity_step_map(images, L, aq, q): an LLDQ container, nothing new
    to a decoder.  With target_bytes, target_psnr or target_msssim the searches above move the BASE step along STEP_GRID (the map
    is the rule's at every base) and SEARCH_STATS reports the base.  With coder, rdo and near (no target then); not with
    step_map, layers, chroma other than "444", depth > 8 or dwtlevels < 2.  None and 0 write the bytes above."""
    from .graphs.layers.lifting_dwt_nets import padded_size
    ch = _chroma_args(chroma, near, layers, step_map, 0, target_psnr, target_msssim)
    d = _depth_args(depth, near, layers, step_map, 0, target_psnr, target_msssim)
    layer, nettype, L = describe(net)
    aq = _aq_args(aq, L, step_map, layers, chroma, depth)
    B, H, W = _check_images(images_u8, ch, d)
    m = _layer_args(layers, step, L, near, step_map, 0, target_bytes, target_psnr, target_msssim)
    target = _quality_args(target_psnr, target_msssim, target_bytes, step, step_map, near, L, H, W)
    if near is not None:
        from .residual import check_near
        near = check_near(near)
    maps = _map_arg(step_map, step, target_bytes, B, H, W, L)
    n, T = _rate_args(step, target_bytes, near, L)
    rdo = _rdo_arg(rdo, L)
    if ch == "444":
        Hp, Wp = padded_size([m.autoencoder for m in net.nets()], H, W)
    else:
        Hp, Wp, _, _ = chroma_sizes(L, nettype == "CDF97", H, W, ch)
    return _encode_at_rate(net, images_u8, (MAGIC, (Hp, Wp, 1, 1, 0), B, coder), near, n, T, rdo, maps, target, m, ch, d, aq)


def _encode_at_rate(net, images_u8, walk, near, step_n, T, rdo=None, maps=None, target=None, layers=0, chroma="444", depth=8, aq=0):
    """_encode at the step step_n / 16, or with a byte target T the search of _search_step, or with a quality target (the
    pair of _quality_args) that of _encode_at_quality, one image at a time.  walk: the (magic, grid, group, coder) of _encode.
    rdo: probes and real encodes alike.  layers: the number of quality layers (_layer_args: no target then).  chroma: the
    format of _chroma_args (not "444": no near, maps, quality target or layers).  depth: that of _depth_args (not 8: the same).
    aq: the m of _aq_args ("444", 8 bits, no maps or layers): the batch's activity is taken once, step_n / 16
    is the BASE step of the activity's map, which is coded as any step map (the unit step in the arithmetic string), and a
    target moves that base along STEP_GRID -- per probe only the map is formed again."""
    act = None
    if aq:
        act = _Activity(images_u8, describe(net)[2], aq, next(net.parameters()).device)
    if target is not None:
        return _encode_at_quality(net, images_u8, walk, rdo, target, act)
    kw = dict(rdo=rdo, chroma=chroma, depth=depth)
    if T is None:
        if act is not None:
            step_n, maps = STEP_DENOM, act.maps(step_n)
        return _encode(net, images_u8, *walk, near, step_n, maps=maps, layers=layers, **kw)

    def coded(b, estimate):
        """n -> image b's container (or its estimated size) at the step n / 16, with aq at the BASE step n / 16."""
        img = images_u8[b:b + 1]
        if act is None:
            return lambda n: _encode(net, img, *walk, None, n, estimate=estimate, **kw)[0]
        return lambda n: _encode(net, img, *walk, None, STEP_DENOM, estimate=estimate, maps=act.maps(n, b), **kw)[0]
    return [_search_step(coded(b, True), coded(b, False), T) for b in range(images_u8.shape[0])]


def _probe_quality(net, image_u8, magic, grid, group, step_n, rdo, kind, maps=None):
    """One probe of a quality target: ONE image (1,H,W,3) goes through the encode walk of _encode at the step
    step_n / 16 with the estimating sink (no range coder runs) and the encoder's own reconstruction, which is the decoder's
    (encode_strings_planes(..., recon=True)), and the image decode_images / decode_tiled would return for that container is
    measured on the device: kind "psnr" -> its exact integer SSE against the original (lldwt_ycc_tiles_sq_err; no image is
    written), kind "msssim" -> the channel mean of ops.ms_ssim on the u8 pair, as ``quality`` computes it.  Plain tiles are
    measured on their in-image rectangles; lapped tiles are blended in ascending tile index into an fp32 frame
    (ops.ycc_tiles_blend), which is then taken as the tile of a 1 x 1 grid, as decode_tiled finishes such a frame.
    maps: the image's (1, hb, wb) array of n instead of the one step (step_n is then 16): every tile is quantised with its slice
    (_unit_maps), as _encode codes it and the decoders read it from an LLDQ container."""
    import torch
    from . import ops
    from .graphs.models.LiftingBasedDWT_net import encode_strings_planes
    from .graphs.models.entropy_coding import ESTIMATE
    _, H, W = _check_images(image_u8)
    th, tw, ny, nx, ov = grid
    nets = net.nets()
    step = step_n / STEP_DENOM
    _prepare(net)
    dev = next(net.parameters()).device
    img = image_u8.to(dev).contiguous()
    per = ny * nx
    g = group if _batch_invariant(arithmetic_string("host", step)) else 1
    with torch.no_grad():
        sse = torch.zeros(1, dtype=torch.int64, device=dev)
        acc = torch.zeros(3, 1, 1, H, W, device=dev, dtype=torch.float32) if ov else None
        rec = torch.empty_like(img) if kind == "msssim" and not ov else None
        for first in range(0, per, g):
            n = min(g, per - first)
            if ov:
                x = ops.u8hwc_to_ycc_tiles_lapped(img, th, tw, ov, ny, nx, first, n)
            else:
                x = ops.u8hwc_to_ycc_tiles(img, th, tw, ny, nx, first, n)
            st = step if maps is None else _unit_maps(maps, range(first, first + n), grid, describe(net)[2], dev)
            xhat = encode_strings_planes(nets, x, coder=ESTIMATE, recon=True, step=st, rdo=rdo)[2].contiguous()
            if ov:
                ops.ycc_tiles_blend(xhat, (H, W, th, tw, ov, ny, nx), (0, 0, H, W), list(range(first, first + n)), acc)
            elif kind == "psnr":
                ops.ycc_tiles_sq_err(xhat, (H, W, th, tw, ny, nx), img, first=first, out=sse)
            else:
                ops.ycc_tiles_to_u8hwc(xhat, (H, W, th, tw, ny, nx), (0, 0, H, W), first=first, out=rec)
        if kind == "psnr":
            if ov:
                ops.ycc_tiles_sq_err(acc, (H, W, H, W, 1, 1), img, out=sse)
            return int(sse.item())
        if ov:
            rec = ops.ycc_tiles_to_u8hwc(acc, (H, W, H, W, 1, 1), (0, 0, H, W))
        return float(ops.ms_ssim(ops.u8hwc_to_f32chw(img), ops.u8hwc_to_f32chw(rec), offset=0.0).mean(1).item())


def _encode_at_quality(net, images_u8, walk, rdo, target, act=None):
    """The quality target of DESIGN.md 7.1.9, one image (or one tiled frame) at a time: _search_quality over probes of
    _probe_quality, then ONE real encode at the chosen step -- the container of encode_*(..., step=<chosen>) byte for byte.
    walk: the (magic, grid, group, coder) of _encode; target: the pair of _quality_args; rdo: probes and the encode alike.
    act: the batch's _Activity (adaptive quantisation): the search moves the BASE step of the activity's map,
    and the container is that of encode_*(..., step_map=<the map at the chosen base>)."""
    magic, grid, group, coder = walk
    kind, want = target
    B, H, W = _check_images(images_u8)
    bound = psnr_sse_bound(want, H, W) if kind == "psnr" else None
    blobs, stats = [], []
    for b in range(B):
        img, vals = images_u8[b:b + 1], {}

        def at(k):
            """Grid index k -> (step_n, maps) of _probe_quality and _encode: the step alone, or with aq the unit step and the
            activity's map at the base STEP_GRID[k] / 16."""
            return (STEP_GRID[k], None) if act is None else (STEP_DENOM, act.maps(STEP_GRID[k], b))

        def meets(k):
            step_n, maps = at(k)
            vals[k] = _probe_quality(net, img, magic, grid, group, step_n, rdo, kind, maps=maps)
            return vals[k] <= bound if kind == "psnr" else vals[k] >= want

        def fail():
            q0 = STEP_GRID[0] / STEP_DENOM
            if kind == "psnr":
                return ValueError("target_psnr: %g dB cannot be met; at the finest step %g the best is %.2f dB"
                                  % (want, q0, sse_psnr(vals[0], H, W)))
            return ValueError("target_msssim: %g cannot be met; at the finest step %g the best is %.6f" % (want, q0, vals[0]))
        k, probes = _search_quality(meets, fail)
        step_n, maps = at(k)
        blob = _encode(net, img, magic, grid, group, coder, None, step_n, rdo=rdo, maps=maps)[0]
        blobs.append(blob)
        stats.append({"probes": probes, "encodes": 1, "step": STEP_GRID[k] / STEP_DENOM, "bytes": len(blob),
                      "sse" if kind == "psnr" else "msssim": vals[k]})
    for key in ("sse", "msssim"):
        SEARCH_STATS.pop(key, None)
    SEARCH_STATS.update(stats[-1], images=stats)
    return blobs


def _unit_layers(lay, j, L):
    """The layer streams of unit j of an encode_strings_planes(..., layers=...) result, lay[jj][i][p][b] -> per layer the
    3 (L - 1) streams in the LLDP order: plane-major, inside a plane the levels 0 .. L-2."""
    return [[lay[jj][i][p][j] for p in range(_PLANES) for i in range(L - 1)] for jj in range(len(lay))]


def _gather_layers(units, k, L):
    """The layer streams of a group of units (each as _unit_layers gives them) -> lay[jj][i][p][b] as decode_strings_planes
    takes them at first_level = k: the entries of the levels below k are None, their streams are never touched."""
    return [[None if i < k else [[u[jj][p * (L - 1) + i] for u in units] for p in range(_PLANES)] for i in range(L - 1)]
            for jj in range(len(units[0]))]


def _cut_tiles(img, chroma, grid, first, n, depth=8, flag=None):
    """The input step of every encode: the tiles first .. first+n-1 of the grid cut out of the image batch as the nets' fp32
    planes -- (3,n,1,th,tw) for "444", (luma, chroma planes) for "420", (1,n,1,th,tw) for "400" -- by the uint8 kernels, or at
    depth 9 .. 16 by their uint16 siblings with the encode's range flag."""
    from . import ops
    th, tw, ny, nx, ov = grid
    deep = () if depth == 8 else (depth, flag)
    if ov:
        return ops.u8hwc_to_ycc_tiles_lapped(img, th, tw, ov, ny, nx, first, n)      # _depth_args: 8 bits only
    if chroma == "400":
        return (ops.u16hw_to_y_tiles if deep else ops.u8hw_to_y_tiles)(img, th, tw, ny, nx, first, n, *deep)
    if chroma == "420":
        return (ops.u16hwc_to_ycc420_tiles if deep else ops.u8hwc_to_ycc420_tiles)(img, th, tw, ny, nx, first, n, *deep)
    return (ops.u16hwc_to_ycc_tiles if deep else ops.u8hwc_to_ycc_tiles)(img, th, tw, ny, nx, first, n, *deep)


def _encode_chroma_planes(nets, planes, chroma, **kw):
    """One group of tiles of a 4:2:0 or 4:0:0 encode -> (s_xe, s_xo) with one entry per coded plane, as
    encode_strings_planes gives them for three planes.  Luma goes through nets[0:1] at (th, tw); Cb and Cr share one two-plane
    call through nets[1:3] at (th / 2, tw / 2).  The coding path is per plane, so a plane's streams are those of coding it
    alone, encode_strings_planes([nets[p]], x_p, ...) (tests/test_gpu_codec_chroma.py holds them to that).  planes: the
    group's tiles as _cut_tiles gives them for the format.  kw: coder, step, rdo."""
    from .graphs.models.LiftingBasedDWT_net import encode_strings_planes
    if chroma == "400":
        return encode_strings_planes(nets[0:1], planes, **kw)[:2]
    luma, chr2 = planes
    y_xe, y_xo = encode_strings_planes(nets[0:1], luma, **kw)[:2]
    c_xe, c_xo = encode_strings_planes(nets[1:3], chr2, **kw)[:2]
    return list(y_xe) + list(c_xe), [list(a) + list(b) for a, b in zip(y_xo, c_xo)]


def _encode(net, images_u8, magic, grid, group, coder, near, step_n, estimate=False, rdo=None, maps=None, layers=0,
            chroma="444", depth=8):
    """The encode walk behind encode_images and encode_tiled (arguments checked there): the batch is cut into the tiles of
    grid = (th, tw, ny, nx, ov) -- the untiled codec is the 1 x 1 grid of one padded_size tile, which the untiled input and
    output kernels serve -- and coded ``group`` tiles at a time (over all images of the batch; one per call in the
    arithmetics that are not batch invariant) at the step step_n / 16 -> the B containers of ``magic``, with near the LLDR
    containers over them.  estimate: -> the estimated container sizes (ints) from the code-length kernel instead; no range
    coder runs (with maps the estimate counts the qmap key and the LLDQ wrapper too).  rdo: the Lagrangian of DESIGN.md 7.1.7
    (None: off), which only the encoder's symbols see.
    maps: the (B, hb, wb) array of _map_arg (None: the step alone): every unit is coded with its slice of its image's map
    (_unit_maps), every base carries the qmap key of its image's map, and the result is wrapped into LLDQ (pack_mapped).
    layers: m > 0 quality layers (without near or maps, and not estimated): every group's layer streams are coded right
    after its base, from the group's own tensors, and the containers are wrapped into LLDP (pack_layered).
    chroma: "420" / "400" (without near, maps, layers or overlap): the same walk, each group cut and coded
    plane by plane (_encode_chroma_planes), the streams interleaved into the LLDW order, the header carrying the chroma key.
    depth: 9 .. 16 (without near, maps, layers or overlap): the same walk on uint16 samples, cut by the uint16
    input kernels (_cut_tiles), whose range flag is read after every cut, before the group is coded."""
    import torch
    from . import ops
    from .graphs.models.LiftingBasedDWT_net import encode_strings_planes
    from .graphs.models.entropy_coding import ESTIMATE
    layer, nettype, L = describe(net)
    B, H, W = _check_images(images_u8, chroma, depth)
    th, tw, ny, nx, ov = grid
    nets = net.nets()
    step = step_n / STEP_DENOM
    arith = arithmetic_string(coder, step, chroma=chroma, depth=depth)
    planes = CHROMA_PLANES[chroma]
    _prepare(net)
    hdr = dict(layer=layer, netType=nettype, dwtlevels=L, H=H, W=W, th=th, tw=tw, ny=ny, nx=nx, overlap=ov,
               numerics=CODING_NUMERICS_VERSION, arithmetic=arith, digest=weights_digest(net))
    # with a map every image has its own header: the arithmetic string names the image's map
    hdrs = [hdr if maps is None else dict(hdr, arithmetic=_with_qmap(arith, map_crc(maps[b]))) for b in range(B)]
    dev = next(net.parameters()).device
    img = images_u8.to(dev).contiguous()
    per, count = ny * nx, planes * (L + 1)
    g = group if _batch_invariant(arith) else 1
    tiles, unit_layers = [], []
    xh = torch.empty_like(img) if near is not None else None
    flag = None if depth == 8 else ops.depth_flag(dev)
    with torch.no_grad():
        for first in range(0, B * per, g):
            n = min(g, B * per - first)
            x = _cut_tiles(img, chroma, grid, first, n, depth, flag)                  # "444": (3,n,1,th,tw)
            if flag is not None:                      # before the nets see the group: a sample past the range is an error
                _check_range(flag, depth)
            if chroma != "444":
                s_xe, s_xo = _encode_chroma_planes(nets, x, chroma, coder=ESTIMATE if estimate else coder, step=step, rdo=rdo)
                tiles += [_tile_streams(s_xe, s_xo, j, planes) for j in range(n)]
                continue
            st = step if maps is None else _unit_maps(maps, range(first, first + n), grid, L, dev)
            if layers:
                s_xe, s_xo, lay = encode_strings_planes(nets, x, coder=coder, step=st, rdo=rdo, layers=(step_n, layers))
                unit_layers += [_unit_layers(lay, j, L) for j in range(n)]
            elif near is None:
                s_xe, s_xo = encode_strings_planes(nets, x, coder=ESTIMATE if estimate else coder, step=st, rdo=rdo)
            else:
                s_xe, s_xo, xhat = encode_strings_planes(nets, x, coder=coder, recon=True, step=st, rdo=rdo)
                # the decoder's call on the same values
                ops.ycc_tiles_to_u8hwc(xhat.contiguous(), (H, W, th, tw, ny, nx), (0, 0, H, W), first=first, B=B, out=xh)
            tiles += [_tile_streams(s_xe, s_xo, j) for j in range(n)]
        if estimate:
            sizes = []
            for b in range(B):
                empty = _pack_base(magic, hdrs[b], [[b""] * count] * per)
                size = _estimated_size(empty, [e for t in tiles[b * per:(b + 1) * per] for e in t])
                if maps is not None:         # the LLDQ wrapper, whose inner length field grows with the inner container
                    size += len(pack_mapped(maps[b], empty)) - len(empty) + len(leb128_encode(size)) - len(leb128_encode(len(empty)))
                sizes.append(size)
            return sizes
        blobs = [_pack_base(magic, hdrs[b], tiles[b * per:(b + 1) * per]) for b in range(B)]
        if near is not None:
            blobs = _refine(blobs, img, xh, (H, W, th, tw, ny, nx), near, coder)
        if layers:
            from . import quality_layers
            crc = quality_layers.tables().crc
            blobs = [pack_layered(crc, blobs[b], [[u[jj] for u in unit_layers[b * per:(b + 1) * per]] for jj in range(layers)])
                     for b in range(B)]
        if maps is not None:
            blobs = [pack_mapped(maps[b], blobs[b]) for b in range(B)]
    return blobs


def check_header(hdr, layer, nettype, L, digest, arith, qmap=None):
    """The identity checks of a parsed header against the decoding net and process (ValueError naming the field).  arith:
    the process's arithmetic string without a coder key; the header's coder and step keys are checked and set aside first.
    qmap: the CRC of the step map that came with the container (its LLDQ wrapper), None without one.  The header's qmap key is
    set aside only when it equals that CRC: a base coded with a step map cannot be decoded without the map."""
    _, hdr_arith = _split_coder(hdr["arithmetic"])
    _, hdr_arith = _split_step(hdr_arith)
    _, hdr_arith = _split_chroma(hdr_arith)             # the chroma format selects planes and sizes, not arithmetic
    _, hdr_arith = _split_depth(hdr_arith)              # the sample depth selects the boundary kernels, not arithmetic
    key, hdr_arith = _split_qmap(hdr_arith)
    if key != qmap:
        if qmap is None:
            raise ValueError("step map: the container was coded with a step map (qmap=%08x) and cannot be decoded without its LLDQ "
                             "wrapper, which holds the map" % key)
        raise ValueError("step map: the container's qmap key is %s, the step map given has CRC %08x"
                         % ("absent" if key is None else "%08x" % key, qmap))
    if hdr["layer"] != layer:
        raise ValueError("entropy layer: the container holds %s, the net is %s" % (hdr["layer"], layer))
    if hdr["netType"] != nettype:
        raise ValueError("netType: the container holds %s, the net is %s" % (hdr["netType"], nettype))
    if hdr["dwtlevels"] != L:
        raise ValueError("dwtlevels: the container holds %d, the net has %d" % (hdr["dwtlevels"], L))
    if hdr["digest"] != digest:
        raise ValueError("weights digest: the container was encoded with other weights (%s != %s)"
                         % (hdr["digest"].hex(), digest.hex()))
    if hdr["numerics"] != CODING_NUMERICS_VERSION:
        raise ValueError("numerics version: the container was written with coding numerics version %d, this decoder has %d"
                         % (hdr["numerics"], CODING_NUMERICS_VERSION))
    if hdr_arith != arith:
        got = dict(p.split("=", 1) for p in hdr_arith.split(",") if "=" in p)
        have = dict(p.split("=", 1) for p in arith.split(","))
        diff = sorted(k for k in set(got) | set(have) if got.get(k) != have.get(k))
        raise ValueError("arithmetic: the container was coded with %s, this process has %s (differs in: %s)"
                         % (hdr_arith, arith, ", ".join(diff)))


def _reduce(reduce, L):
    """The reduce factor of a decode, checked on the host (ValueError naming reduce)."""
    try:
        k = int(reduce)
    except (TypeError, ValueError):
        raise ValueError("reduce must be an integer in [0, %d] (got %r)" % (L, reduce)) from None
    if k != reduce or not 0 <= k <= L:
        raise ValueError("reduce must be an integer in [0, %d], the net's dwtlevels (got %r)" % (L, reduce))
    return k


def _reduced(v, k):
    """ceil(v / 2^k): a side of the image at reduce=k."""
    return -(-v >> k)


def ll_norm(net, k):
    """-> (inv_a, b), 3 floats each, rounded to fp32: the per-plane map (LL_k - b) * inv_a of a reduce=k decode, with
    (a, b) = lifting_dwt_nets.ll_affine of the net's transforms and inv_a = fp32(1 / a) computed here on the host."""
    import torch
    from .graphs.layers.lifting_dwt_nets import ll_affine
    a, b = ll_affine([n.autoencoder for n in net.nets()], k)
    inv = [1.0 / v if v != 0 else float("inf") for v in a]
    return torch.tensor(inv, dtype=torch.float32).tolist(), torch.tensor(b, dtype=torch.float32).tolist()


def decode_images(net, blobs, reduce=0, refine=True, layers=None, recon=None):
    """List of containers -> list of (H,W,3) uint8 CPU tensors, in input order.  Every container is checked on the host
    first; then containers of equal (H, W), coder and quantisation step are decoded together (both come from each header).
    reduce = k in [0, L]: the image at 1/2^k of each side, (ceil(H / 2^k), ceil(W / 2^k), 3), decoded from the xe streams
    and the levels k .. L-1 only (the module docstring); reduce=0 is the full decode.
    An LLDR container over LLDW is decoded through its base and then refined on the device (lossless or within its bound,
    DESIGN.md 7.1.5); refine=False, or reduce > 0 (the residual lives at full resolution), gives exactly the base decode.
    An LLDQ container is decoded as its inner container, with its step map on the levels 0 .. L-2 that the
    decode reaches; images with different maps are decoded together, the map being per image.
    An LLDP container over LLDW is decoded through its base plus its first ``layers`` quality layers (None:
    all it holds; 0: exactly the base decode); with reduce = k the levels k .. L-2 are refined and the streams of finer levels
    are never touched.  ``layers`` above a container's count, or other than None / 0 for a container without layers, is a
    ValueError.
    A container coded with chroma="420" decodes to (H,W,3), one coded with chroma="400" to (H,W,1); the
    format comes from the header, containers are grouped by it as well, and a mix comes back in input order.
    A container coded with depth=d decodes to a uint16 tensor of d-bit samples; the depth comes from the
    header, and containers of different depths in one call are a ValueError naming depth (a list of one dtype comes back).
    recon="centroid" (DESIGN.md 7.1.13): every coefficient of the levels 0 .. L-2 that the decode reaches is put at the mean of
    its quantisation bin under the entropy model's Gaussian instead of the bin's centre -- after the quality layers, with the
    step of the last layer decoded, and with the step map of an LLDQ container.  A decoder's choice: no container records it, and
    None or "centre" is the decode as ever.  Over an LLDR container whose residual would be applied (refine=True, reduce=0) it is
    a ValueError naming recon and near: the residual was taken against the centre reconstruction."""
    import torch
    from . import ops
    from .graphs.layers.lifting_dwt_nets import padded_size
    rc = _recon_arg(recon)
    layer, nettype, L = describe(net)
    k = _reduce(reduce, L)
    refined, maps, layered = {}, {}, {}
    blobs = list(blobs)
    for i, b in enumerate(blobs):
        if _magic(b) == LAYERED_MAGIC:
            phdr, b, lay = parse_layered(b)
            if _magic(b) != MAGIC:
                raise ValueError("base container: decode_images takes an LLDP over LLDW; this one is over %s (decode_tiled)"
                                 % bytes(b[:4]).decode("ascii", "replace"))
            blobs[i] = b
            j = _layers_arg(layers, phdr["layers"])
            if j:
                layered[i] = [lay[jj][0] for jj in range(j)]
        else:
            _layers_arg(layers, 0)
        if _magic(b) == MAPPED_MAGIC:
            _, maps[i], b = parse_mapped(b)
            blobs[i] = b
        if _magic(b) == REFINED_MAGIC:
            if refine and k == 0:
                _recon_refined(rc)
            rhdr, base, units = parse_refined(b)
            if _magic(base) != MAGIC:
                raise ValueError("base container: decode_images takes an LLDR over LLDW; this one is over %s (decode_tiled)"
                                 % bytes(base[:4]).decode("ascii", "replace"))
            blobs[i] = base
            if refine and k == 0:
                refined[i] = (rhdr["near"], units)
    parsed = [parse_container(b) for b in blobs]
    depths = sorted({hdr.get("depth", 8) for hdr, _ in parsed})
    if len(depths) > 1:
        raise ValueError("depth: the containers hold samples of %s bits; decode one depth per call"
                         % " and ".join(str(d) for d in depths))
    depth = depths[0] if depths else 8
    digest, arith = weights_digest(net), arithmetic_string()
    for i, (hdr, _) in enumerate(parsed):
        check_header(hdr, layer, nettype, L, digest, arith, qmap=map_crc(maps[i]) if i in maps else None)
    _prepare(net)
    nets = net.nets()
    dev = next(net.parameters()).device
    by_size = {}
    for i, (hdr, _) in enumerate(parsed):
        by_size.setdefault((hdr["H"], hdr["W"], hdr["coder"], hdr["step"], i in maps, len(layered.get(i, ())),
                            hdr.get("chroma", "444")), []).append(i)
    out = [None] * len(parsed)
    with torch.no_grad():
        if k:
            inv_a, b = ll_norm(net, k)
        for (H, W, coder, step, mapped, nlay, chroma), idx in by_size.items():
            units = [parsed[i][1] for i in idx]
            if chroma != "444":                       # the 1 x 1 grid of the format's padded size
                Hp, Wp, _, _ = chroma_sizes(L, nettype == "CDF97", H, W, chroma)
            else:
                Hp, Wp = padded_size([n.autoencoder for n in nets], H, W)
            if chroma != "444" or depth != 8:         # no step map, layers or residual here (_chroma_args, _depth_args)
                Hr, Wr = _reduced(H, k), _reduced(W, k)
                for a, n, res in _decode_groups(nets, units, Hp, Wp, len(idx), parsed[idx[0]][0], k, recon=rc):
                    img = _write_tiles(chroma, depth, res, (Hr, Wr, Hp >> k, Wp >> k, 1, 1), (0, 0, Hr, Wr),
                                       (inv_a, b) if k else None, B=n).cpu()
                    for j, i in enumerate(idx[a:a + n]):
                        out[i] = img[j]
                continue
            um = _unit_maps([maps[i] for i in idx], range(len(idx)), (Hp, Wp, 1, 1, 0), L, dev) if mapped else None
            ul = [layered[i] for i in idx] if nlay else None
            for a, n, xhat in _decode_groups(nets, units, Hp, Wp, len(idx), parsed[idx[0]][0], k, um, ul, rc):
                g = idx[a:a + n]
                if k == 0:
                    img = ops.ycc_to_u8hwc_crop(xhat.contiguous(), H, W)
                    for d in sorted({refined[i][0] for i in g if i in refined}):
                        from . import residual
                        js = [j for j, i in enumerate(g) if i in refined and refined[i][0] == d]
                        residual.decode_units(img, (H, W, Hp, Wp, 1, 1), (0, 0, H, W), js,
                                              [refined[g[j]][1][0] for j in js], d, coder)
                    img = img.cpu()
                else:
                    Hr, Wr = _reduced(H, k), _reduced(W, k)
                    img = ops.ll_tiles_to_u8hwc(xhat.contiguous(), (Hr, Wr, Hp >> k, Wp >> k, 1, 1), (0, 0, Hr, Wr), inv_a,
                                                b, B=len(g)).cpu()
                for j, i in enumerate(g):
                    out[i] = img[j]
    return out


# ------------------------------------------------------------------------------------------------ tiled coding
def tile_grid(nets, H, W, tile=512):
    """The tile grid of an H x W image for a target tile side -> (th, tw, ny, nx).  nets: the per-plane transform modules
    (padded_size).  Every tile has the size padded_size gives for ceil(H / ny) x ceil(W / nx), and the grid is recounted
    with it (rounding up to 2^L, or to CDF 9/7's 5 * 2^L, can otherwise leave whole tile rows or columns outside)."""
    from .graphs.layers.lifting_dwt_nets import padded_size
    if int(tile) < 1 or H < 1 or W < 1:
        raise ValueError("tile grid: tile, H and W must be positive (got %d, %d, %d)" % (tile, H, W))
    nx, ny = -(-W // tile), -(-H // tile)
    th, tw = padded_size(nets, -(-H // ny), -(-W // nx))
    return th, tw, -(-H // th), -(-W // tw)


def chroma_sizes(L, cdf97, H, W, chroma="444", tile=None):
    """The coded sizes of an H x W image in a chroma format -> (th, tw, ny, nx): the luma (or only) plane of
    a tile and the grid; tile=None is the untiled codec, the 1 x 1 grid of one padded image.  L, cdf97: the level count and the
    transform kind (padded_dims).  With share = (ceil(H / ny0), ceil(W / nx0)) for the counts ny0 = ceil(H / tile), nx0 =
    ceil(W / tile) of the target tile side (the image itself when untiled): "444" and "400" code planes of padded_dims(share),
    as tile_grid; "420" codes chroma planes of (Hc, Wc) = padded_dims(ceil(share / 2)) and a luma plane of (2 Hc, 2 Wc), so both
    are sizes the transform accepts.  The grid is recounted with the tile size, as tile_grid does."""
    from .graphs.layers.lifting_dwt_nets import padded_dims
    ch = check_chroma(chroma)
    if H < 1 or W < 1 or (tile is not None and int(tile) < 1):
        raise ValueError("tile grid: tile, H and W must be positive (got %r, %d, %d)" % (tile, H, W))
    sh, sw = (H, W) if tile is None else (-(-H // -(-H // int(tile))), -(-W // -(-W // int(tile))))
    if ch == "420":
        hc, wc = padded_dims(L, cdf97, -(-sh // 2), -(-sw // 2))
        th, tw = 2 * hc, 2 * wc
    else:
        th, tw = padded_dims(L, cdf97, sh, sw)
    if tile is None:
        return th, tw, 1, 1
    return th, tw, -(-H // th), -(-W // tw)


def lap_weights(t, ov, q, n):
    """The 1-D cross-fade weights of tile number q of n along an axis: a float32 tensor of t values.  (i + 0.5) / ov on the
    first ov samples of a tile that has a predecessor (q > 0), (t - i - 0.5) / ov on the last ov of one that has a successor
    (q < n - 1), 1 elsewhere; ov = 0: all ones.  ov is a power of two, so every weight is exact in fp32 and the falling ramp
    of a tile and the rising ramp of the next sum to exactly 1.  A pixel's weight is wy * wx (lldwt_ycc_tiles_blend)."""
    import torch
    t, ov, q, n = int(t), int(ov), int(q), int(n)
    if t < 1 or n < 1 or not 0 <= q < n or ov < 0 or ov & (ov - 1) or 2 * ov > t:
        raise ValueError("lap_weights: need t >= 1, 0 <= q < n and overlap a power of two with 2 * overlap <= t "
                         "(got t=%d, overlap=%d, q=%d, n=%d)" % (t, ov, q, n))
    w = torch.ones(t, dtype=torch.float32)
    if ov:
        i = torch.arange(ov, dtype=torch.float32)
        if q > 0:
            w[:ov] = (i + 0.5) / ov
        if q < n - 1:
            w[t - ov:] = (ov - i - 0.5) / ov          # local index t - ov + i: (t - (t - ov + i) - 0.5) / ov
    return w


def tile_grid_lapped(nets, H, W, tile=512, overlap=0):
    """tile_grid for tiles that share ``overlap`` pixels with each neighbour -> (th, tw, ny, nx).  Along an axis of size S
    the count n0 = ceil(S / tile) of the plain grid gives the tile side padded_size(ceil((S + (n0 - 1) overlap) / n0)) -- n0
    tiles at the stride side - overlap then cover S -- and the count is redone with it: 1 if one tile covers the axis, else
    ceil((S - side) / stride) + 1, the smallest that covers, so the last tile is needed.  ValueError naming overlap unless
    it is a power of two with 2^L <= overlap <= min(th, tw) / 2; overlap = 0 is tile_grid."""
    from .graphs.layers.lifting_dwt_nets import _levels, padded_size
    ov = int(overlap)
    if ov != overlap or ov < 0:
        raise ValueError("overlap must be a non-negative integer (got %r)" % (overlap,))
    if ov == 0:
        return tile_grid(nets, H, W, tile)
    if int(tile) < 1 or H < 1 or W < 1:
        raise ValueError("tile grid: tile, H and W must be positive (got %d, %d, %d)" % (tile, H, W))
    ny, nx = -(-H // tile), -(-W // tile)
    th, tw = padded_size(nets, -(-(H + (ny - 1) * ov) // ny), -(-(W + (nx - 1) * ov) // nx))
    _check_overlap(_levels(nets[0]), th, tw, ov)
    count = lambda size, t: 1 if t >= size else -(-(size - t) // (t - ov)) + 1
    return th, tw, count(H, th), count(W, tw)


def _tile_streams(s_xe, s_xo, j, planes=_PLANES):
    """The planes * (L + 1) streams of image j of an encode_strings_planes result, in the LLDW order."""
    return [s for p in range(planes) for s in [s_xe[p][j]] + [lev[p][j] for lev in s_xo]]


def encode_tiled(net, images_u8, tile=512, tiles_per_call=32, coder="host", overlap=0, near=None, step=None, target_bytes=None,
                 rdo=None, step_map=None, layers=None, chroma="444", depth=None, aq=None, target_psnr=None, target_msssim=None):
    """(B,H,W,3) uint8 RGB tensor -> list of B LLDT containers, or with overlap > 0 LLDO containers of lapped tiles
    (tile_grid_lapped; the tiles are cut by lldwt_u8hwc_to_ycc_tiles_lapped and coded exactly as below).
    Every tile is coded as an independent image: its streams
    are those of encode_images(net, padded_tile).  The images are uploaded once; groups of tiles_per_call tiles (over all
    images of the batch) are cut out on the device (lldwt_u8hwc_to_ycc_tiles) and coded together, which bounds the device
    memory; one tile per call in the arithmetics that are not batch invariant.  The bytes do not depend on tiles_per_call.
    coder: as encode_images.  near: as encode_images, every tile's in-image rectangle being a unit of the residual layer
    (LLDR over LLDT; the bytes do not depend on tiles_per_call either); not with overlap > 0, where the decoded pixels are
    a blend of two units.
    step, target_bytes: as encode_images, with ONE step for all tiles of a frame; a target is met by each frame's container
    (the images of a batch are searched one at a time).  rdo: as encode_images, for every tile.
    step_map: as encode_images, the map of the whole image; a tile is coded with the slice at its origin (tile origins are
    multiples of 2^L for plain and lapped grids alike), clamped at the image's last block -> LLDQ over LLDT / LLDO / LLDR.
    target_psnr, target_msssim: as encode_images, with ONE step for all tiles of a frame, met by the image decode_tiled returns
    for the frame: the tiles' in-image rectangles, or with overlap > 0 the blended frame.  The result does
    not depend on tiles_per_call.
    layers: as encode_images, every tile being a unit with its own layer streams (LLDP over LLDT; not with overlap > 0), so a
    region decodes the refinement of the tiles it touches only.
    chroma: as encode_images; with "420" the tile grid is that of chroma_sizes (the half of a tile is a size the transform
    accepts) and every tile's streams are those of encode_images(net, tile, chroma="420"); not with overlap > 0.
    depth: as encode_images (uint16 samples of 9..16 bits); not with overlap > 0.
    aq: as encode_images; the map is that of the whole frame and a tile takes its slice as with step_map, for plain and lapped
    tiles alike; a target moves the one base step of the frame."""
    ch = _chroma_args(chroma, near, layers, step_map, overlap, target_psnr, target_msssim)
    d = _depth_args(depth, near, layers, step_map, overlap, target_psnr, target_msssim)
    layer, nettype, L = describe(net)
    aq = _aq_args(aq, L, step_map, layers, chroma, depth)
    B, H, W = _check_images(images_u8, ch, d)
    m = _layer_args(layers, step, L, near, step_map, overlap, target_bytes, target_psnr, target_msssim)
    target = _quality_args(target_psnr, target_msssim, target_bytes, step, step_map, near, L, H, W)
    if near is not None:
        from .residual import check_near
        near = check_near(near)
        if overlap:
            raise ValueError("near: a residual layer over lapped tiles (overlap > 0) is not defined; use overlap=0")
    maps = _map_arg(step_map, step, target_bytes, B, H, W, L)
    n, T = _rate_args(step, target_bytes, near, L)
    rdo = _rdo_arg(rdo, L)
    group = _tiles_per_call(tiles_per_call)
    ov = int(overlap)
    if ov != overlap or ov < 0 or ov > 0xFFFF:
        raise ValueError("overlap must be an integer in [0, 65535] (got %r)" % (overlap,))
    if ch == "444":
        th, tw, ny, nx = tile_grid_lapped([m.autoencoder for m in net.nets()], H, W, int(tile), ov)
    else:
        th, tw, ny, nx = chroma_sizes(L, nettype == "CDF97", H, W, ch, int(tile))
    if ny > 0xFFFF or nx > 0xFFFF:
        raise ValueError("tile grid %d x %d: ny, nx must fit 16 bits" % (ny, nx))
    walk = (LAPPED_MAGIC if ov else TILED_MAGIC, (th, tw, ny, nx, ov), group, coder)
    return _encode_at_rate(net, images_u8, walk, near, n, T, rdo, maps, target, m, ch, d, aq)


def _tiles_per_call(tiles_per_call):
    """The group size of a tiled walk, checked on the host (ValueError naming tiles_per_call)."""
    if int(tiles_per_call) < 1 or int(tiles_per_call) > 65535:
        raise ValueError("tiles_per_call must be in [1, 65535] (got %d)" % tiles_per_call)
    return int(tiles_per_call)


def _decode_tiles(nets, s_xe, s_xo, th, tw, n, coder="host", first_level=0, step=1.0, layers=None, recon=None):
    """One group of n tiles -> xhat (3,n,1,th,tw), or at first_level = k the LL band (3,n,1,th>>k,tw>>k)
    (decode_strings_planes; a module-level hook so the number of tiles a decode touches can be counted).  layers: the
    (streams, n of the base step, layer count) of decode_strings_planes, given only for a decode with quality layers; recon:
    given only for a centroid decode."""
    from .graphs.models.LiftingBasedDWT_net import decode_strings_planes
    kw = {} if layers is None else {"layers": layers}
    if recon is not None:
        kw["recon"] = recon
    return decode_strings_planes(nets, s_xe, s_xo, th, tw, n, coder=coder, first_level=first_level, step=step, **kw)


def _gather(units, k, L, planes=_PLANES):
    """The stream lists of a group of units (images or tiles, each in the LLDW order) -> (s_xe, s_xo) as
    decode_strings_planes takes them at first_level = k: the xe streams and the xo streams of the levels k .. L-1."""
    per = L + 1                                       # streams per plane: xe, xo finest -> coarsest
    s_xe = [[u[p * per] for u in units] for p in range(planes)]
    s_xo = [[[u[p * per + 1 + lev] for u in units] for p in range(planes)] for lev in range(k, L)]
    return s_xe, s_xo


def _write_tiles(chroma, depth, res, grid, region, affine=None, **kw):
    """The output step of a 4:2:0 / 4:0:0 decode and of every decode at more than 8 bits:
    res, what _decode_groups yields for the format -- the three planes, (luma, chroma planes) or the single plane -- -> the
    uint8 pixels of ops.ycc420_tiles_to_u8hwc / ops.y_tiles_to_u8hw, or at depth 9 .. 16 the uint16 samples of their siblings
    and of ops.ycc_tiles_to_u16hwc.  affine: None, or the (inv_a, b) of ll_norm at reduce > 0 (three values each; 4:0:0 takes
    plane 0's).  The 8-bit 4:4:4 decode keeps its own calls (decode_images, decode_tiled)."""
    from . import ops
    deep = () if depth == 8 else (depth,)
    if chroma == "420":
        return (ops.ycc420_tiles_to_u16hwc if deep else ops.ycc420_tiles_to_u8hwc)(res[0], res[1], grid, region, *deep,
                                                                                  affine=affine, **kw)
    if chroma == "400":
        return (ops.y_tiles_to_u16hw if deep else ops.y_tiles_to_u8hw)(
            res, grid, region, *deep, affine=None if affine is None else (affine[0][:1], affine[1][:1]), **kw)
    return ops.ycc_tiles_to_u16hwc(res.contiguous(), grid, region, depth, affine=affine, **kw)


def _recon_arg(recon):
    """The recon argument of the decoders -> "centroid" or None (None and "centre": the decode as ever).
    ValueError naming recon; host only."""
    from .ops import check_recon
    return "centroid" if check_recon(recon) == "centroid" else None


def _recon_refined(rc):
    """A centroid decode under a residual layer that is about to be applied: ValueError naming recon and near."""
    if rc is not None:
        raise ValueError("recon and near: the residual layer of an LLDR container was taken against the centre reconstruction "
                         "and its checksum would refuse any other; decode with refine=False (or reduce > 0) for recon=%r" % rc)


def _layers_arg(layers, m):
    """The layers argument of a decode against a container of m quality layers (0: none) -> the count to decode (None: all).
    ValueError naming layers."""
    if layers is None:
        return m
    if isinstance(layers, bool) or not isinstance(layers, int) or not 0 <= layers <= m:
        raise ValueError("layers must be an integer in [0, %d], the quality layers the container holds (got %r)" % (m, layers))
    return layers


def _decode_groups(nets, units, th, tw, group, hdr, k, maps=None, layers=None, recon=None):
    """The decode walk behind decode_images and decode_tiled: the units (stream lists of images or tiles of th x tw, all of
    the coder and step of hdr) are decoded ``group`` at a time, one per call in the arithmetics that are not batch invariant,
    through the _decode_tiles hook -> yields (index of the group's first unit, its size n, the hook's result).
    maps: the units' step maps (_unit_maps, one per unit) when the units were coded with one; each group then decodes with its
    slice in place of the header's step.
    layers: (per unit its layer streams in the LLDP order, truncated to the count j > 0 to decode) of a layered decode (DESIGN.md
    7.1.10): each group's levels k .. L-2 are refined with its own streams before the inverse transform.
    recon: "centroid" for a centroid decode, else None; it goes to every call of the hook, chroma planes too."""
    g = group if _batch_invariant(hdr["arithmetic"]) else 1
    rk = {} if recon is None else {"recon": recon}
    L = hdr["dwtlevels"]
    chroma = hdr.get("chroma", "444")
    for a in range(0, len(units), g):
        grp = units[a:a + g]
        if chroma != "444":
            # luma through nets[0:1] at the tile size (th, tw), Cb and Cr in one call through nets[1:3] at half
            # of it, as the encoder coded them.  4:2:0 -> (luma (1,n,1,th>>k,tw>>k), chroma (2,n,1,th>>(k+1),tw>>(k+1))); 4:0:0 ->
            # the plane.
            s_xe, s_xo = _gather(grp, k, L, CHROMA_PLANES[chroma])
            kw = dict(coder=hdr["coder"], first_level=k, step=hdr["step"], **rk)
            res = _decode_tiles(nets[0:1], s_xe[0:1], [lev[0:1] for lev in s_xo], th, tw, len(grp), **kw).contiguous()
            if chroma == "420":
                res = (res, _decode_tiles(nets[1:3], s_xe[1:3], [lev[1:3] for lev in s_xo], th // 2, tw // 2, len(grp),
                                          **kw).contiguous())
            yield a, len(grp), res
            continue
        s_xe, s_xo = _gather(grp, k, L)
        kw = dict(rk)
        if layers is not None:
            lay = _gather_layers(layers[a:a + g], k, L)
            kw["layers"] = (lay, int(round(hdr["step"] * STEP_DENOM)), len(lay))
        yield a, len(grp), _decode_tiles(nets, s_xe, s_xo, th, tw, len(grp), coder=hdr["coder"], first_level=k,
                                         step=hdr["step"] if maps is None else maps[a:a + g], **kw)


def _region(region, H, W):
    if region is None:
        return 0, 0, H, W
    try:
        y0, x0, h, w = (int(v) for v in region)
    except (TypeError, ValueError):
        raise ValueError("region must be (y0, x0, h, w) (got %r)" % (region,)) from None
    if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > H or x0 + w > W:
        raise ValueError("region (%d, %d, %d, %d) is not inside the %d x %d image" % (y0, x0, h, w, H, W))
    return y0, x0, h, w


def decode_tiled(net, blob, region=None, tiles_per_call=32, reduce=0, refine=True, layers=None, recon=None):
    """LLDT or LLDO container (or an LLDQ over one, DESIGN.md 7.1.8: each tile decodes with its slice of the step map) ->
    (h, w, 3) uint8 CPU tensor: the whole image, or region = (y0, x0, h, w).  Only the tiles that
    intersect the region are decoded, tiles_per_call at a time, and written into the region by lldwt_ycc_tiles_to_u8hwc.
    LLDO (lapped tiles): the tiles covering any pixel of the region, overlap included, are decoded in
    ascending index, each group is blended into a region-sized fp32 buffer (lldwt_ycc_tiles_blend) and the buffer is
    written once, as the single tile of a 1 x 1 grid, by the same output kernels.
    reduce = k in [0, L]: the image at 1/2^k of each side (decode_images); region is then in the coordinates of the reduced
    image, each tile covers th>>k x tw>>k of its pixels and is written by lldwt_ll_tiles_to_u8hwc.
    LLDR over LLDT: the base and residual streams of the touched tiles are decoded and the region is cut from their refined
    rectangles; refine=False, or reduce > 0, gives exactly the base decode.
    LLDP over LLDT: the touched tiles are decoded with their first ``layers`` quality layers (None: all, 0: the
    base decode), as decode_images; only those tiles' layer streams are read.
    A container coded with chroma="420" / "400"  decodes to (h, w, 3) / (h, w, 1); the chroma of a tile is
    upsampled from that tile alone, so a region still touches only the tiles it intersects.
    A container coded with depth=d decodes to uint16 samples of d bits.
    recon="centroid" (DESIGN.md 7.1.13): the touched tiles are decoded to their bins' centroids, as decode_images does; lapped
    tiles are blended afterwards as ever.  Refused over an LLDR container whose residual would be applied.
    Every check (container, region, identity) runs on the host before any GPU work."""
    import torch
    from . import ops
    rc = _recon_arg(recon)
    layer, nettype, L = describe(net)
    k = _reduce(reduce, L)
    units = smap = lay = None
    if _magic(blob) == LAYERED_MAGIC:
        phdr, blob, lay = parse_layered(blob)
        if _magic(blob) != TILED_MAGIC:
            raise ValueError("base container: decode_tiled takes an LLDP over LLDT; this one is over %s (decode_images)"
                             % bytes(blob[:4]).decode("ascii", "replace"))
        lay = lay[:_layers_arg(layers, phdr["layers"])] or None
    else:
        _layers_arg(layers, 0)
    if _magic(blob) == MAPPED_MAGIC:           # the inner container with its step map
        _, smap, blob = parse_mapped(blob)
    if _magic(blob) == REFINED_MAGIC:
        if refine and not k:
            _recon_refined(rc)
        rhdr, blob, units = parse_refined(blob)
        if _magic(blob) != TILED_MAGIC:
            raise ValueError("base container: decode_tiled takes an LLDR over LLDT; this one is over %s (decode_images)"
                             % bytes(blob[:4]).decode("ascii", "replace"))
        if not refine or k:
            units = None
    hdr, tiles = _parse_base(LAPPED_MAGIC if _magic(blob) == LAPPED_MAGIC else TILED_MAGIC, blob)
    ny, nx, chroma, depth = hdr["ny"], hdr["nx"], hdr.get("chroma", "444"), hdr.get("depth", 8)
    # at reduce = k the tile side, the stride and the overlap are all shifted by k (they are multiples of 2^L)
    H, W, th, tw, ov = _reduced(hdr["H"], k), _reduced(hdr["W"], k), hdr["th"] >> k, hdr["tw"] >> k, hdr["overlap"] >> k
    y0, x0, h, w = _region(region, H, W)
    # tile q of an axis covers [q s, q s + t) at the stride s = t - ov: the tiles with q s + t > first and q s <= last
    span = lambda first, last, t, n: range(max(0, (first - t) // (t - ov) + 1), min(n - 1, last // (t - ov)) + 1)
    rows, cols = span(y0, y0 + h - 1, th, ny), span(x0, x0 + w - 1, tw, nx)
    want = [ty * nx + tx for ty in rows for tx in cols]                        # ascending tile index: the blend's order
    if units is not None:
        # the residual's contexts reach every pixel of a unit: decode the rectangles of the touched tiles whole, refine
        # them, and cut the region out on the device
        asked = (y0, x0, h, w)
        y0, x0 = rows[0] * th, cols[0] * tw
        h, w = min(H, (rows[-1] + 1) * th) - y0, min(W, (cols[-1] + 1) * tw) - x0
    group = _tiles_per_call(tiles_per_call)
    check_header(hdr, layer, nettype, L, weights_digest(net), arithmetic_string(), qmap=None if smap is None else map_crc(smap))
    _prepare(net)
    nets = net.nets()
    dev = next(net.parameters()).device
    um = None if smap is None else _unit_maps([smap], want, (hdr["th"], hdr["tw"], ny, nx, hdr["overlap"]), L, dev)
    with torch.no_grad():
        if k:
            inv_a, b = ll_norm(net, k)

        def write(y, grid, reg, **kw):
            if k == 0:
                return ops.ycc_tiles_to_u8hwc(y, grid, reg, **kw)
            return ops.ll_tiles_to_u8hwc(y, grid, reg, inv_a, b, **kw)
        if ov:
            acc = torch.zeros(3, 1, 1, h, w, device=dev, dtype=torch.float32)
        else:
            out = torch.empty(1, h, w, 1 if chroma == "400" else 3, device=dev,
                              dtype=torch.uint8 if depth == 8 else torch.uint16)
        ul = None if lay is None else [[lay[jj][t] for jj in range(len(lay))] for t in want]
        for a, n, xhat in _decode_groups(nets, [tiles[t] for t in want], hdr["th"], hdr["tw"], group, hdr, k, um, ul, rc):
            if chroma != "444" or depth != 8:
                # the chroma is upsampled inside the tile, so no neighbour tile is needed
                _write_tiles(chroma, depth, xhat, (H, W, th, tw, ny, nx), (y0, x0, h, w), (inv_a, b) if k else None,
                             tiles=want[a:a + n], out=out)
            elif ov:                 # lapped: the raw samples are blended, then written once as the tile of a 1 x 1 grid
                ops.ycc_tiles_blend(xhat.contiguous(), (H, W, th, tw, ov, ny, nx), (y0, x0, h, w), want[a:a + n], acc)
            else:
                write(xhat.contiguous(), (H, W, th, tw, ny, nx), (y0, x0, h, w), tiles=want[a:a + n], out=out)
        if ov:
            out = write(acc, (h, w, h, w, 1, 1), (0, 0, h, w))
        if units is not None:
            from . import residual
            residual.decode_units(out, (H, W, th, tw, ny, nx), (y0, x0, h, w), want, [units[t] for t in want], rhdr["near"],
                                  hdr["coder"])
            ay, ax, ah, aw = asked
            out = out[:, ay - y0:ay - y0 + ah, ax - x0:ax - x0 + aw]
    return out[0].cpu()
