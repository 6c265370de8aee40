"""Host (CPU) tests of reduced-resolution decoding (codec.py): reduce_bytes from known stream lengths for LLDW and LLDT
containers, and the host refusals of a bad reduce factor or a region outside the reduced image, before the library is
loaded."""
import os
import subprocess
import sys

import pytest

from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import codec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ID = dict(layer="onlyEZWT", netType="LiftingBasedNeuralWaveletv4", numerics=7, arithmetic="plc_mode=f16x3,storage=fp32",
           digest=bytes(range(16)))


def _streams(L, seed):
    """3 (L + 1) streams of distinct non-zero lengths, plane-major: xe, then xo finest -> coarsest."""
    return [bytes((seed + i) & 0xFF for _ in range(1 + (seed * 7 + i * 13) % 50)) for i in range(3 * (L + 1))]


def _want(hdr, per_image, L):
    out = []
    for k in range(L + 1):
        n = hdr["header_bytes"]
        for streams in per_image:
            for p in range(3):
                n += len(streams[p * (L + 1)]) + sum(len(streams[p * (L + 1) + 1 + lev]) for lev in range(k, L))
        out.append(n)
    return out


@pytest.mark.parametrize("L", [1, 3, 4])
def test_reduce_bytes_lldw(L):
    streams = _streams(L, L)
    blob = codec.pack_container(dict(_ID, dwtlevels=L, H=37, W=53), streams)
    hdr = codec.read_header(blob)
    got = codec.reduce_bytes(hdr)
    assert got == _want(hdr, [streams], L)
    assert len(got) == L + 1
    assert got[0] == len(blob) - 4                                            # everything but the CRC32 trailer
    assert got[L] == hdr["header_bytes"] + sum(len(streams[p * (L + 1)]) for p in range(3))
    assert all(a > b for a, b in zip(got, got[1:]))


@pytest.mark.parametrize("L", [2, 3])
def test_reduce_bytes_lldt(L):
    th = tw = 8 << L
    ny, nx = 2, 3
    tiles = [_streams(L, 5 * t + 1) for t in range(ny * nx)]
    blob = codec.pack_tiled(dict(_ID, dwtlevels=L, H=2 * th - 3, W=3 * tw - 1, th=th, tw=tw, ny=ny, nx=nx), tiles)
    hdr = codec.read_header(blob)
    got = codec.reduce_bytes(hdr)
    assert got == _want(hdr, tiles, L)
    assert got[0] == len(blob) - 4
    assert all(a > b for a, b in zip(got, got[1:]))


def test_bad_reduce_and_region_are_refused_on_the_host():
    """A CPU net: describe, the container and the reduce / region checks need no library, and run before any of it."""
    code = "import sys; sys.path.insert(0, %r)\n" % REPO + r'''
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import codec, _lib
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import LiftingBasedDWTNetWrapper
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
net = LiftingBasedDWTNetWrapper(make_config(dwtlevels=3, entropy_layer="onlyEZWT")).eval()
L = 3
per = [bytes([i + 1]) * (i + 2) for i in range(3 * (L + 1))]
ident = dict(layer="onlyEZWT", netType="LiftingBasedNeuralWaveletv4", numerics=codec.CODING_NUMERICS_VERSION,
             arithmetic="precision=f16x3", digest=bytes(16), dwtlevels=L)
blob = codec.pack_container(dict(ident, H=37, W=53), per)
tiled = codec.pack_tiled(dict(ident, H=100, W=70, th=64, tw=40, ny=2, nx=2), [per] * 4)
for bad in (-1, L + 1, 0.5, None):
    try:
        codec.decode_images(net, [blob], reduce=bad)
    except ValueError as e:
        assert "reduce" in str(e), e
    else:
        raise AssertionError("reduce=%r accepted" % (bad,))
    try:
        codec.decode_tiled(net, tiled, reduce=bad)
    except ValueError as e:
        assert "reduce" in str(e), e
    else:
        raise AssertionError("tiled reduce=%r accepted" % (bad,))
# at reduce=2 the image is 25 x 18: regions are in those coordinates
for region in ((0, 0, 26, 1), (0, 17, 1, 2), (25, 0, 1, 1), (-1, 0, 2, 2)):
    try:
        codec.decode_tiled(net, tiled, region=region, reduce=2)
    except ValueError as e:
        assert "region" in str(e), e
    else:
        raise AssertionError("region %r accepted" % (region,))
assert _lib._lib is None, "library loaded"
print("ok")
'''
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]
