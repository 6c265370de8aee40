"""Host (CPU) tests of the chroma formats 4:2:0 and 4:0:0: the chroma key of the arithmetic string, the LLDW /
LLDT containers that carry it, chroma_sizes and the 4:2:0 tile grid, the phase of the reference resampling (tests/chroma_ref.py)
and the argument pairs the encoders refuse.  Nothing here touches the GPU."""
import struct
import zlib

import pytest
import torch

import chroma_ref
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import codec
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.layers.lifting_dwt_nets import padded_dims

BASE = "cgp=f16,plc_algo=direct,plc_fuse=1,plc_mode=f16x3,plc_shape=16,precision=f16x3,storage=fp32"
DIGEST = bytes(range(16))


def _hdr(arith, L=3, H=64, W=96, nettype="LiftingBasedNeuralWaveletv4"):
    return dict(layer="onlyEZWT", netType=nettype, dwtlevels=L, H=H, W=W, numerics=codec.CODING_NUMERICS_VERSION,
                arithmetic=arith, digest=DIGEST)


def _streams(count, seed=0):
    return [bytes((seed + 7 * i + j) & 0xFF for j in range(3 + i)) for i in range(count)]


def _reseal(body):
    return bytes(body) + struct.pack("<I", zlib.crc32(bytes(body)) & 0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ the arithmetic string
def test_the_chroma_key_round_trips_and_444_has_none():
    assert codec._with_chroma(BASE, None) == BASE and codec._with_chroma(BASE, "444") == BASE
    assert codec._split_chroma(BASE) == ("444", BASE)
    for ch in ("420", "400"):
        a = codec._with_chroma(BASE, ch)
        assert a.split(",")[0] == "cgp=f16" and "chroma=%s" % ch in a.split(",") and a.split(",") == sorted(a.split(","))
        assert codec._split_chroma(a) == (ch, BASE)
        # beside the other keys, in any order of merging
        full = codec._with_chroma(codec._with_step(BASE + ",coder=irans32", 40), ch)
        assert codec._split_chroma(full) == (ch, codec._with_step(BASE + ",coder=irans32", 40))
        assert codec._split_step(codec._split_chroma(full)[1])[0] == 40
        assert codec._batch_invariant(full) == codec._batch_invariant(BASE)
    for bad in ("422", 420, "4:2:0", True):
        with pytest.raises(ValueError, match="chroma"):
            codec.check_chroma(bad)
    for bad in (BASE + ",chroma=422", BASE + ",chroma=444", BASE + ",chroma=420,chroma=420", BASE + ",chroma="):
        with pytest.raises(ValueError, match="chroma"):
            codec._split_chroma(bad)


def test_an_unknown_chroma_value_is_refused_in_read_header():
    blob = codec.pack_container(_hdr(BASE), _streams(12))
    at = blob.index(BASE.encode())
    arith = (BASE + ",chroma=422").encode()
    bad = _reseal(blob[:at - 1] + bytes([len(arith)]) + arith + blob[at + len(BASE):-4])
    with pytest.raises(ValueError, match="chroma"):
        codec.read_header(bad)


# ------------------------------------------------------------------------------------------------ the containers
@pytest.mark.parametrize("ch,planes", [("420", 3), ("400", 1)])
def test_lldw_and_lldt_round_trip_with_the_key(ch, planes):
    L = 3
    arith = codec._with_chroma(BASE, ch)
    streams = _streams(planes * (L + 1))
    blob = codec.pack_container(_hdr(arith), streams)
    hdr, got = codec.parse_container(blob)
    assert got == streams and hdr["chroma"] == ch and hdr["arithmetic"] == arith and len(hdr["stream_lengths"]) == planes * (L + 1)
    assert codec.read_header(blob) == hdr and blob[:4] == b"LLDW" and blob[4] == codec.FORMAT_VERSION
    # reduce_bytes: per plane of L + 1 streams, the xe stream and the levels k .. L-1
    rb = codec.reduce_bytes(hdr)
    lens = [len(s) for s in streams]
    for k in range(L + 1):
        assert rb[k] == hdr["header_bytes"] + sum(lens[p * (L + 1)] + sum(lens[p * (L + 1) + 1 + k:(p + 1) * (L + 1)])
                                                  for p in range(planes))
    assert rb[0] == len(blob) - 4
    # a wrong stream count is refused, in both directions
    for count in (3 * (L + 1) if planes == 1 else L + 1, planes * (L + 1) + 1):
        with pytest.raises(ValueError, match="stream count"):
            codec.parse_container(codec.pack_container(_hdr(arith), _streams(count)))
    # tiled: 2 x 1 tiles of 64 x 96 (the half, 32 x 48, is a padded size at L = 3)
    th = dict(_hdr(arith, H=100, W=96), th=64, tw=96, ny=2, nx=1)
    tiles = [_streams(planes * (L + 1), seed=1), _streams(planes * (L + 1), seed=2)]
    tb = codec.pack_tiled(th, tiles)
    thdr, tgot = codec.parse_tiled(tb)
    assert tgot == tiles and thdr["chroma"] == ch and thdr["streams_per_tile"] == planes * (L + 1) and tb[:4] == b"LLDT"
    assert codec.reduce_bytes(thdr)[0] == len(tb) - 4 and codec.reduce_bytes(thdr)[L] < codec.reduce_bytes(thdr)[0]
    with pytest.raises(ValueError, match="stream count"):
        codec.pack_tiled(th, [t[:-1] for t in tiles])


def test_a_key_less_container_has_no_chroma_entry():
    hdr, _ = codec.parse_container(codec.pack_container(_hdr(BASE), _streams(12)))
    assert "chroma" not in hdr and hdr.get("chroma", "444") == "444"
    thdr, _ = codec.parse_tiled(codec.pack_tiled(dict(_hdr(BASE, H=100, W=64), th=64, tw=64, ny=2, nx=1),
                                                 [_streams(12, 1), _streams(12, 2)]))
    assert "chroma" not in thdr


def test_a_420_tile_must_halve_to_a_padded_size():
    arith = codec._with_chroma(BASE, "420")
    L = 3
    # 8 = 2^L is a tile of the transform, but its half is not; 16 = 2^(L+1) is
    bad = dict(_hdr(arith, H=8, W=8), th=8, tw=8, ny=1, nx=1)
    with pytest.raises(ValueError, match="tile size"):
        codec.pack_tiled(bad, [_streams(12)])
    ok = codec.pack_tiled(dict(bad, th=16, tw=16), [_streams(12)])
    assert codec.parse_tiled(ok)[0]["th"] == 16
    # the parser refuses it too: a 4:4:4 container of tile 8 whose arithmetic string is given the key afterwards
    blob = codec.pack_tiled(dict(_hdr(BASE, H=8, W=8), th=8, tw=8, ny=1, nx=1), [_streams(12)])
    at = blob.index(BASE.encode())
    keyed = _reseal(blob[:at - 1] + bytes([len(arith)]) + arith.encode() + blob[at + len(BASE):-4])
    with pytest.raises(ValueError, match="tile size"):
        codec.read_header(keyed)
    # "400" keeps the rule of 4:4:4
    codec.pack_tiled(dict(_hdr(codec._with_chroma(BASE, "400"), H=8, W=8), th=8, tw=8, ny=1, nx=1), [_streams(4)])
    # CDF 9/7: the half must reach 5 * 2^L
    with pytest.raises(ValueError, match="tile size"):
        codec.pack_tiled(dict(_hdr(arith, H=40, W=40, nettype="CDF97"), th=40, tw=40, ny=1, nx=1), [_streams(12)])
    codec.pack_tiled(dict(_hdr(arith, H=40, W=40, nettype="CDF97"), th=80, tw=80, ny=1, nx=1), [_streams(12)])


def test_wrappers_and_lapped_tiles_refuse_a_base_with_the_key():
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import quality_layers as ql
    L = 3
    for ch, planes in (("420", 3), ("400", 1)):
        arith = codec._with_chroma(codec._with_step(BASE, 48), ch)
        base = codec.pack_container(_hdr(arith), _streams(planes * (L + 1)))
        with pytest.raises(ValueError, match="chroma.*layers"):
            codec.pack_layered(ql.tables().crc, base, [[[b"x"] * (3 * (L - 1))]])
        with pytest.raises(ValueError, match="chroma.*near"):
            codec.pack_refined(0, 0, base, [dict(cs_xh=0, cs_x=0, scales=bytes(24), streams=[b""] * 3)])
        import numpy as np
        with pytest.raises(ValueError, match="chroma.*step_map"):
            codec.pack_mapped(np.full((8, 12), 16, dtype=np.int64), base)
        lapped = dict(_hdr(arith, H=100, W=64), th=64, tw=64, ny=2, nx=1, overlap=16)
        with pytest.raises(ValueError, match="chroma.*overlap"):
            codec.pack_lapped(lapped, [_streams(planes * (L + 1))] * 2)
        # and the parsers: an LLDO container whose arithmetic string is given the key afterwards
        plain = codec._with_step(BASE, 48)
        lo = codec.pack_lapped(dict(lapped, arithmetic=plain), [_streams(12, 1), _streams(12, 2)])
        at = lo.index(plain.encode())
        keyed = _reseal(lo[:at - 1] + bytes([len(arith)]) + arith.encode() + lo[at + len(plain):-4])
        with pytest.raises(ValueError, match="chroma.*overlap"):
            codec.read_header(keyed)


# ------------------------------------------------------------------------------------------------ sizes and the grid
@pytest.mark.parametrize("cdf97", [False, True])
@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_chroma_sizes_and_the_420_grid(L, cdf97):
    nettype = "CDF97" if cdf97 else "LiftingBasedNeuralWaveletv4"
    for H in range(1, 131):
        for W in range(1, 131):
            th, tw, ny, nx = codec.chroma_sizes(L, cdf97, H, W, "420")
            assert (ny, nx) == (1, 1) and th % 2 == 0 and tw % 2 == 0
            assert padded_dims(L, cdf97, th // 2, tw // 2) == (th // 2, tw // 2)            # the halves are padded sizes
            assert (th // 2, tw // 2) == padded_dims(L, cdf97, -(-H // 2), -(-W // 2)) and th >= H and tw >= W
            assert codec.chroma_sizes(L, cdf97, H, W, "400") == padded_dims(L, cdf97, H, W) + (1, 1)
            assert codec.chroma_sizes(L, cdf97, H, W, "444") == padded_dims(L, cdf97, H, W) + (1, 1)
    for H in range(1, 131, 3):
        for W in range(1, 131):
            for tile in (16, 48, 100):
                th, tw, ny, nx = codec.chroma_sizes(L, cdf97, H, W, "420", tile)
                assert padded_dims(L, cdf97, th // 2, tw // 2) == (th // 2, tw // 2) and th % 2 == 0 and tw % 2 == 0
                assert ny * th >= H and nx * tw >= W                                        # the image is covered
                assert (ny - 1) * th < H and (nx - 1) * tw < W                              # the last row and column are needed
                codec._check_grid(nettype, L, H, W, th, tw, ny, nx, chroma="420")          # what the parser will check
                p = padded_dims(L, cdf97, -(-H // -(-H // tile)), -(-W // -(-W // tile)))
                assert codec.chroma_sizes(L, cdf97, H, W, "400", tile) == p + (-(-H // p[0]), -(-W // p[1]))


def test_chroma_sizes_of_444_is_tile_grid():
    class _N:                                    # what tile_grid reads of a transform module
        waveletLevel = 3
    for H, W, tile in ((100, 150, 48), (37, 53, 16), (1, 1, 512), (130, 7, 64)):
        assert codec.chroma_sizes(3, False, H, W, "444", tile) == codec.tile_grid([_N()], H, W, tile)


# ------------------------------------------------------------------------------------------------ the reference resampling
def test_a_linear_plane_survives_down_then_up():
    """The centred phase: a chroma sample stands for the middle of its 2 x 2 pixels, and the 3/4, 1/4 weights interpolate back to
    the pixel centres, so a plane linear in x and y returns within rounding away from the one-sample border (where the clamp
    replicates).  A co-sited phase would be off by a quarter pixel of slope."""
    y, x = torch.meshgrid(torch.arange(40, dtype=torch.float32), torch.arange(56, dtype=torch.float32), indexing="ij")
    for a, b, c in ((0.004, -0.003, 0.1), (0.0, 0.007, -0.2), (-0.005, 0.0, 0.3)):
        plane = a * y + b * x + c
        back = chroma_ref.upsample(chroma_ref.downsample(plane))
        assert back.shape == plane.shape and back.dtype == torch.float32
        assert float((back - plane)[2:-2, 2:-2].abs().max()) <= 1e-6
    # the clamp: a constant plane is exact everywhere, and the border rows hold the border sample
    assert torch.equal(chroma_ref.upsample(torch.full((3, 5), 0.25)), torch.full((6, 10), 0.25))
    ramp = torch.arange(4, dtype=torch.float32)[None, :].repeat(2, 1)
    up = chroma_ref.upsample(ramp)
    assert up[0].tolist() == [0.0, 0.25, 0.75, 1.25, 1.75, 2.25, 2.75, 3.0]
    g = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(chroma_ref.grey_out(chroma_ref.grey_in(g)), g)


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_argument_pairs_raise_on_the_host():
    args = codec._chroma_args
    assert args(None) == "444" and args("444", near=0, layers=2, overlap=16, target_psnr=30.0) == "444"
    assert args("420") == "420" and args("400", layers=0) == "400" and args("420", layers=None, overlap=0) == "420"
    for ch in ("420", "400"):
        for name, kw in (("near", dict(near=0)), ("near", dict(near=2)), ("layers", dict(layers=1)),
                         ("step_map", dict(step_map=[[1.0]])), ("overlap", dict(overlap=16)),
                         ("target_psnr", dict(target_psnr=30.0)), ("target_msssim", dict(target_msssim=0.9))):
            with pytest.raises(ValueError, match="chroma and %s" % name):
                args(ch, **kw)
    with pytest.raises(ValueError, match="chroma"):
        args("422")


def test_the_encoders_refuse_on_the_host_before_any_gpu_work(monkeypatch):
    """Through the public entry points, with the library unreachable: every refusal of the list, and the input shape rule."""
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import _lib
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
        LiftingBasedDWTNetWrapper
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
    net = LiftingBasedDWTNetWrapper(make_config(dwtlevels=3, mode="validate")).eval()

    def no_library():
        raise AssertionError("the GPU library was loaded")
    monkeypatch.setattr(_lib, "load", no_library)
    rgb, grey = torch.zeros(1, 24, 40, 3, dtype=torch.uint8), torch.zeros(1, 24, 40, 1, dtype=torch.uint8)
    for enc in (codec.encode_images, codec.encode_tiled):
        for ch, img in (("420", rgb), ("400", grey)):
            for name, kw in (("near", dict(near=0)), ("layers", dict(layers=1, step=3.0)), ("step_map", dict(step_map=[[1.0] * 5] * 3)),
                             ("target_psnr", dict(target_psnr=30.0)), ("target_msssim", dict(target_msssim=0.9))):
                with pytest.raises(ValueError, match="chroma and %s" % name):
                    enc(net, img, chroma=ch, **kw)
        with pytest.raises(ValueError, match="chroma"):
            enc(net, rgb, chroma="422")
        with pytest.raises(ValueError, match=r"\(B,H,W,1\)"):
            enc(net, rgb, chroma="400")
        with pytest.raises(ValueError, match=r"\(B,H,W,3\)"):
            enc(net, grey, chroma="420")
        with pytest.raises(ValueError, match=r"\(B,H,W,3\)"):
            enc(net, grey)
    with pytest.raises(ValueError, match="chroma and overlap"):
        codec.encode_tiled(net, rgb, chroma="420", overlap=16)
