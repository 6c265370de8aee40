"""GPU: 9- to 16-bit samples in the codec -- the seven kernels of csrc/depth.hip bit for bit against
tests/depth_ref.py and, at depth 8, against their uint8 siblings; the range flag; the v8 * 257 identity of the streams; the
container round trip against the encoder's own reconstruction, batch invariance, tiles and regions, reduced decoding, the rate
options, codec.quality and the command-line tool.  The weights are seeded, not trained: no test asserts a byte saving or a PSNR.

uint16 tensors are compared on the host (or as int16 views): this torch implements few ops for the type on the device."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import depth_ref
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import codec, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = ("conditioned2ZTsepSubbands", "onlyEZWT", "DWTConditioned2EntropyLayerZTBlock")
FORMATS = ("444", "420", "400")
SENTINEL = 0xABCD
_NETS = {}


def _net(layer="conditioned2ZTsepSubbands", L=3):
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
        LiftingBasedDWTNetWrapper
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
    if (layer, L) not in _NETS:
        cfg = make_config(dwtlevels=L, mode="validate", entropy_layer=layer)
        torch.manual_seed(0)
        _NETS[layer, L] = LiftingBasedDWTNetWrapper(cfg).to(DEV).eval()
    return _NETS[layer, L]


def _gain_net(L=3, gain=100.0):
    """The net of the rate tests, as tests/test_gpu_codec_step.py builds it: filled weights with the last layer of the subband
    auto-encoders of the levels 0 .. L-2 scaled, so that a step, a Lagrangian or a byte target changes the symbols."""
    from helpers import filled
    from oracle import weights
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
        LiftingBasedDWTNetWrapper
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
    if ("gain", L) not in _NETS:
        cfg = make_config(dwtlevels=L, mode="validate", entropy_layer="conditioned2ZTsepSubbands")
        net = LiftingBasedDWTNetWrapper(cfg)
        net.load_state_dict(filled(weights.wrapper_template(dict(cfg))), strict=False)
        net = net.to(DEV).eval()
        with torch.no_grad():
            for n in net.nets():
                for lev in range(L - 1):
                    last = n.autoencoder.Yh_ae[lev].ae_down[6]
                    last.weight.mul_(gain)
                    last.bias.mul_(gain)
        _NETS["gain", L] = net
    return _NETS["gain", L]


def _images8(B, H, W, seed, chroma="444"):
    """Smooth fields plus noise as int32 values in [0, 255], (B,H,W,3) on the host, or (B,H,W,1) for "400"."""
    ch = 1 if chroma == "400" else 3
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(B, ch, max(2, H // 16), max(2, W // 16), generator=g)
    x = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
    x = x * 200 + torch.rand(B, ch, H, W, generator=g) * 40
    return x.clamp(0, 255).round().to(torch.int32).permute(0, 2, 3, 1).contiguous()


def _images(B, H, W, seed, d, chroma="444"):
    """The same fields at depth d, every low bit in use: uint16 (B,H,W,C) on the host with values in [0, 2^d - 1]."""
    M = (1 << d) - 1
    g = torch.Generator().manual_seed(seed + 1000 * d)
    x = _images8(B, H, W, seed, chroma).to(torch.float32) / 255.0 * M + torch.rand(B, H, W, 1 if chroma == "400" else 3, generator=g)
    return x.floor().clamp(0, M).to(torch.int32).to(torch.uint16)


def _u16(x_i32):
    return x_i32.to(torch.uint16)


def _tile_gather(plane, th, tw, ny, nx, first, n):
    """plane (B,H,W) on the host -> (n,th,tw): the tiles first .. first+n-1 of the grid, replicate-edge padded."""
    B, H, W = plane.shape
    out = []
    for t in range(first, first + n):
        b, r = divmod(t, ny * nx)
        ty, tx = divmod(r, nx)
        ri = (ty * th + torch.arange(th)).clamp(max=H - 1)
        ci = (tx * tw + torch.arange(tw)).clamp(max=W - 1)
        out.append(plane[b][ri][:, ci])
    return torch.stack(out)


def _tile_scatter(tiles_px, tiles, grid, region, B, fill=0):
    """tiles_px (n,th,tw,C) uint16 on the host, their tile indexes -> (B,h,w,C): the pixels inside the image and the region, the
    others holding ``fill``."""
    H, W, th, tw, ny, nx = grid
    y0, x0, h, w = region
    out = torch.full((B, h, w, tiles_px.shape[3]), fill, dtype=torch.int32)
    px = tiles_px.to(torch.int32)
    for j, t in enumerate(tiles):
        b, r = divmod(t, ny * nx)
        ty, tx = divmod(r, nx)
        ylo, yhi = max(y0, ty * th), min(y0 + h, H, (ty + 1) * th)
        xlo, xhi = max(x0, tx * tw), min(x0 + w, W, (tx + 1) * tw)
        if yhi > ylo and xhi > xlo:
            out[b, ylo - y0:yhi - y0, xlo - x0:xhi - x0] = px[j, ylo - ty * th:yhi - ty * th, xlo - tx * tw:xhi - tx * tw]
    return out.to(torch.uint16)


def _ref_in(img, chroma, d, th, tw, ny, nx, first, n):
    """What the input kernel of the format must give for the tiles first .. first+n-1: the reference on the whole image, the
    tiles gathered with the clamp, and for 4:2:0 the reference downsampling of each tile's chroma."""
    if chroma == "400":
        return _tile_gather(depth_ref.grey_in(img[..., 0], d), th, tw, ny, nx, first, n)[None, :, None]
    planes = [_tile_gather(p, th, tw, ny, nx, first, n) for p in depth_ref.rgb_in(img, d)]
    if chroma == "444":
        return torch.stack(planes)[:, :, None]
    return planes[0][None, :, None], depth_ref.downsample(torch.stack(planes[1:]))[:, :, None]


def _ref_out(chroma, res, d, affine=None):
    """What the output kernel of the format must write for every pixel of the decoded tiles res (as _decode_groups yields them,
    on the host): (n,th,tw,C) uint16.  affine: the (inv_a, b) of a reduced decode, applied per plane before the upsampling."""
    af = (lambda s, p: s) if affine is None else (lambda s, p: depth_ref.affine(s, affine[0][p], affine[1][p]))
    if chroma == "400":
        return depth_ref.grey_out(af(res[0, :, 0], 0), d)[..., None]
    if chroma == "444":
        return depth_ref.rgb_out([af(res[p, :, 0], p) for p in range(3)], d)
    luma, c = res
    return depth_ref.rgb_out([af(luma[0, :, 0], 0)] + [depth_ref.upsample(af(c[p, :, 0], p + 1)) for p in range(2)], d)


def _fp32(vals):
    return torch.tensor(vals, dtype=torch.float32).tolist()


def _cut(img_dev, chroma, grid, first, n, d, flag=None):
    return codec._cut_tiles(img_dev, chroma, grid + (0,), first, n, d, ops.depth_flag(DEV) if flag is None else flag)


def _cpu(res):
    return tuple(r.cpu() for r in res) if isinstance(res, tuple) else res.cpu()


def _spy(monkeypatch):
    """Wraps the codec._decode_tiles hook -> list of (th, tw, n, streams handed to the coder, result) per call."""
    seen, real = [], codec._decode_tiles

    def wrapped(nets, s_xe, s_xo, th_, tw_, n, **kw):
        out = real(nets, s_xe, s_xo, th_, tw_, n, **kw)
        seen.append((th_, tw_, n, [s for p in s_xe for s in p] + [s for lev in s_xo for p in lev for s in p], out))
        return out
    monkeypatch.setattr(codec, "_decode_tiles", wrapped)
    return seen


def _seen_res(chroma, seen):
    """The results of the hook's calls of ONE group, on the host, as _ref_out takes them."""
    planes = [s[4].contiguous().cpu() for s in seen]
    assert [p.shape[0] for p in planes] == {"444": [3], "420": [1, 2], "400": [1]}[chroma]
    return (planes[0], planes[1]) if chroma == "420" else planes[0]


# ------------------------------------------------------------------------------------------------ 1. input kernels
@pytest.mark.parametrize("B,H,W", [(1, 37, 53), (3, 200, 120)])
@pytest.mark.parametrize("L", [3, 4])
@pytest.mark.parametrize("d", [10, 12, 16])
def test_input_kernels_bit_exact(B, H, W, L, d):
    """The padded 1 x 1 grid of each format.  W = 53 is odd: every second row of the uint16 image starts at an address that is
    2 mod 4."""
    M = (1 << d) - 1
    img = torch.randint(0, M + 1, (B, H, W, 3), dtype=torch.int32, generator=torch.Generator().manual_seed(B * H + L + d))
    img[0, 0, 0] = torch.tensor([M, 0, M])
    img[0, H - 1, W - 1] = torch.tensor([0, M, 0])
    img = _u16(img)
    dev = img.to(DEV)
    flag = ops.depth_flag(DEV)
    for chroma in FORMATS:
        src, dsrc = (img[..., 1:2].contiguous(), dev[..., 1:2].contiguous()) if chroma == "400" else (img, dev)
        th, tw, _, _ = codec.chroma_sizes(L, False, H, W, chroma)
        got = _cpu(_cut(dsrc, chroma, (th, tw, 1, 1), 0, B, d, flag))
        want = _ref_in(src, chroma, d, th, tw, 1, 1, 0, B)
        if chroma == "420":
            assert got[0].shape == (1, B, 1, th, tw) and got[1].shape == (2, B, 1, th // 2, tw // 2)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (chroma, d)
        else:
            assert got.shape == (1 if chroma == "400" else 3, B, 1, th, tw) and torch.equal(got, want), (chroma, d)
    assert int(flag.item()) == 0                                      # M itself is inside the range


@pytest.mark.parametrize("W", [110, 111])
@pytest.mark.parametrize("d", [10, 12, 16])
def test_input_kernels_on_a_tile_grid(d, W):
    """(2,75,110) on 40 x 48 tiles (2 x 3), whole and with first / n in the middle of the grid; and the same at W = 111, where
    every second row of the image starts at an address that is 2 mod 4."""
    B, H, th, tw, ny, nx = 2, 75, 40, 48, 2, 3
    M = (1 << d) - 1
    img = _u16(torch.randint(0, M + 1, (B, H, W, 3), dtype=torch.int32, generator=torch.Generator().manual_seed(d)))
    dev = img.to(DEV)
    for chroma in FORMATS:
        src, dsrc = (img[..., 1:2].contiguous(), dev[..., 1:2].contiguous()) if chroma == "400" else (img, dev)
        for first, n in ((0, B * ny * nx), (4, 5)):
            got = _cpu(_cut(dsrc, chroma, (th, tw, ny, nx), first, n, d))
            want = _ref_in(src, chroma, d, th, tw, ny, nx, first, n)
            if chroma == "420":
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (chroma, first)
            else:
                assert torch.equal(got, want), (chroma, first)
    # the refusals of the uint8 forms, and the new ones
    with pytest.raises(RuntimeError):
        ops.u16hwc_to_ycc420_tiles(dev, th + 1, tw, ny, nx, 0, 1, d)                  # an odd tile side
    with pytest.raises(RuntimeError):
        ops.u16hw_to_y_tiles(dev, th, tw, ny, nx, 0, 1, d)                            # three channels
    with pytest.raises(RuntimeError):
        ops.u16hwc_to_ycc_tiles(dev, th, tw, ny, nx, 10, 3, d)                        # a tile range past the grid
    with pytest.raises(RuntimeError):
        ops.u16hwc_to_ycc_tiles(dev, th, tw, 1, nx, 0, 1, d)                          # a grid that does not cover the image
    with pytest.raises(RuntimeError):
        ops.u16hwc_to_ycc_tiles(dev, th, tw, ny, nx, 0, 1, 17)
    with pytest.raises(RuntimeError):
        ops.u16hwc_to_ycc_tiles(dev.view(torch.int16), th, tw, ny, nx, 0, 1, d)       # not uint16


def test_depth_8_on_uint16_data_is_the_uint8_kernels():
    B, H, W, th, tw, ny, nx = 2, 75, 111, 40, 48, 2, 3
    g = torch.Generator().manual_seed(8)
    v8 = torch.randint(0, 256, (B, H, W, 3), dtype=torch.int32, generator=g)
    a8, a16 = v8.to(torch.uint8).to(DEV), _u16(v8).to(DEV)
    n = B * ny * nx
    assert torch.equal(ops.u16hwc_to_ycc_tiles(a16, th, tw, ny, nx, 0, n, 8), ops.u8hwc_to_ycc_tiles(a8, th, tw, ny, nx, 0, n))
    assert torch.equal(ops.u16hwc_to_ycc_tiles(a16, 80, 112, 1, 1, 0, B, 8), ops.u8hwc_to_ycc_tiles(a8, 80, 112, 1, 1, 0, B))
    for x, y in zip(ops.u16hwc_to_ycc420_tiles(a16, th, tw, ny, nx, 1, n - 2, 8), ops.u8hwc_to_ycc420_tiles(a8, th, tw, ny, nx, 1, n - 2)):
        assert torch.equal(x, y)
    assert torch.equal(ops.u16hw_to_y_tiles(a16[..., :1].contiguous(), th, tw, ny, nx, 0, n, 8),
                       ops.u8hw_to_y_tiles(a8[..., :1].contiguous(), th, tw, ny, nx, 0, n))
    assert torch.equal(ops.u16hwc_to_f32chw(a16, 8), ops.u8hwc_to_f32chw(a8))
    # and the output kernels: the same values, wider storage
    luma = (torch.rand(1, n, 1, th, tw, generator=g) * 1.4 - 0.7).to(DEV)
    chroma = (torch.rand(2, n, 1, th // 2, tw // 2, generator=g) * 1.4 - 0.7).to(DEV)
    ycc = (torch.rand(3, n, 1, th, tw, generator=g) * 1.4 - 0.7).to(DEV)
    grid, region = (H, W, th, tw, ny, nx), (3, 5, H - 10, W - 12)
    inv_a, b = _fp32([0.3517, 0.127, 0.509]), _fp32([0.0123, -0.0456, 0.0789])
    same = lambda u16, u8: torch.equal(u16.cpu().to(torch.int32), u8.cpu().to(torch.int32))
    assert same(ops.ycc_tiles_to_u16hwc(ycc, grid, region, 8, B=B), ops.ycc_tiles_to_u8hwc(ycc, grid, region, B=B))
    assert same(ops.ycc_tiles_to_u16hwc(ycc, grid, region, 8, affine=(inv_a, b), B=B), ops.ll_tiles_to_u8hwc(ycc, grid, region, inv_a, b, B=B))
    for af in (None, (inv_a, b)):
        assert same(ops.ycc420_tiles_to_u16hwc(luma, chroma, grid, region, 8, affine=af, B=B),
                    ops.ycc420_tiles_to_u8hwc(luma, chroma, grid, region, affine=af, B=B))
        af1 = None if af is None else (inv_a[:1], b[:1])
        assert same(ops.y_tiles_to_u16hw(luma, grid, region, 8, affine=af1, B=B), ops.y_tiles_to_u8hw(luma, grid, region, affine=af1, B=B))


# ------------------------------------------------------------------------------------------------ 2. output kernels
def _planes(shape, d, g):
    """Random planes for the output rule: values beyond [-0.5, 0.5] (the clamp), +-0.5 exactly, and the half-integers of the
    rounding rule, s = (k + 0.5) / M - 0.5, where floor(. + 0.5) steps."""
    M = float((1 << d) - 1)
    x = torch.rand(shape, generator=g) * 1.4 - 0.7
    flat = x.view(-1)
    k = torch.randint(0, int(M), (flat.numel() // 4,), generator=g).to(torch.float32)
    flat[0::4][:k.numel()] = (k + 0.5) / M - 0.5
    flat[1] = 0.5
    flat[2] = -0.5
    flat[5] = 0.5 - 0.25 / M
    return x


@pytest.mark.parametrize("d", [10, 12, 16])
@pytest.mark.parametrize("B,H,W,th,tw,ny,nx", [(2, 37, 53, 48, 64, 1, 1), (2, 75, 110, 40, 48, 2, 3), (2, 75, 111, 40, 48, 2, 3)])
def test_output_kernels_bit_exact(B, H, W, th, tw, ny, nx, d):
    g = torch.Generator().manual_seed(H + d)
    per = ny * nx
    tile_lists = [None] if per == 1 else [None, [7, 2, 11, 5, 0]]
    regions = [(0, 0, H, W), (3, 5, H - 10, W - 12), (H - 1, W - 1, 1, 1), (th - 1 if per > 1 else 11, tw - 1 if per > 1 else 9, 7, 5)]
    inv_a, b = _fp32([0.3517, 0.127, 0.509]), _fp32([0.0123, -0.0456, 0.0789])
    grid = (H, W, th, tw, ny, nx)
    for tiles in tile_lists:
        n = B * per if tiles is None else len(tiles)
        ident = list(range(n)) if tiles is None else tiles
        res = {"444": _planes((3, n, 1, th, tw), d, g), "400": _planes((1, n, 1, th, tw), d, g),
               "420": (_planes((1, n, 1, th, tw), d, g), _planes((2, n, 1, th // 2, tw // 2), d, g))}
        for chroma in FORMATS:
            for af in (None, (inv_a, b)):
                px = _ref_out(chroma, res[chroma], d, af)
                for region in regions:
                    h, w = region[2:]
                    out = torch.full((B, h, w, px.shape[3]), SENTINEL, dtype=torch.uint16).to(DEV)
                    dev = tuple(r.to(DEV) for r in res[chroma]) if chroma == "420" else res[chroma].to(DEV)
                    got = codec._write_tiles(chroma, d, dev, grid, region, af, tiles=tiles, B=B, out=out)
                    assert got is out and got.dtype == torch.uint16
                    # every pixel no tile covers keeps the sentinel
                    want = _tile_scatter(px, ident, grid, region, B, fill=SENTINEL)
                    assert torch.equal(got.cpu(), want), (chroma, tiles, region, af is not None)
    ycc = res["444"].to(DEV)
    assert ops.ycc_tiles_to_u16hwc(ycc, grid, regions[0], d, tiles=tiles, B=B).shape == (B, H, W, 3)
    with pytest.raises(RuntimeError):
        ops.ycc_tiles_to_u16hwc(ycc, grid, (0, 0, H + 1, W), d, tiles=tiles, B=B)     # a region outside the image
    with pytest.raises(RuntimeError):
        ops.ycc_tiles_to_u16hwc(ycc, grid, regions[0], 7, tiles=tiles, B=B)
    with pytest.raises(RuntimeError):
        ops.ycc_tiles_to_u16hwc(ycc, grid, regions[0], d, tiles=tiles, B=B, out=torch.zeros(B, H, W, 3, dtype=torch.int16, device=DEV))
    with pytest.raises(RuntimeError):
        ops.ycc420_tiles_to_u16hwc(res["420"][0].to(DEV), res["420"][1][:, :, :, :-1].contiguous().to(DEV), grid, regions[0], d,
                                   tiles=tiles, B=B)


# ------------------------------------------------------------------------------------------------ 3. the range flag
def test_a_sample_above_the_range_is_an_error_not_a_clamp():
    net = _net()
    d, M = 10, 1023
    x = _images(2, 37, 53, 1, d).to(torch.int32)
    x[1, 36, 52, 2] = M
    ok = _u16(x)
    assert len(codec.encode_images(net, ok, depth=d)) == 2 and len(codec.encode_tiled(net, ok, tile=32, depth=d)) == 2
    x[1, 36, 52, 2] = M + 1
    bad = _u16(x)
    for chroma, img in (("444", bad), ("420", bad), ("400", bad[..., 2:3].contiguous())):
        with pytest.raises(ValueError, match="depth"):
            codec.encode_images(net, img, depth=d, chroma=chroma)
        with pytest.raises(ValueError, match="depth"):
            codec.encode_tiled(net, img, tile=32, depth=d, chroma=chroma)
    with pytest.raises(ValueError, match="depth"):
        codec.quality(ok, bad, depth=d)
    # the flag is only ever set: a clean call leaves a raised flag raised
    flag = ops.depth_flag(DEV)
    ops.u16hwc_to_ycc_tiles(bad.to(DEV), 40, 56, 1, 1, 0, 2, d, flag)
    ops.u16hwc_to_ycc_tiles(ok.to(DEV), 40, 56, 1, 1, 0, 2, d, flag)
    assert int(flag.item()) == 1


# ------------------------------------------------------------------------------------------------ 4. the 257 identity
@pytest.mark.parametrize("layer", LAYERS)
def test_depth_16_of_v8_times_257_has_the_streams_of_the_8_bit_encode(layer):
    """65535 = 255 * 257: the nets see bitwise the same tensors, so only the header key differs."""
    net = _net(layer)
    v8 = _images8(1, 37, 53, 2)
    x8, x16 = v8.to(torch.uint8), _u16(v8 * 257)
    for kw in (dict(), dict(coder="gpu"), dict(chroma="420")):
        h8, s8 = codec.parse_container(codec.encode_images(net, x8, **kw)[0])
        h16, s16 = codec.parse_container(codec.encode_images(net, x16, depth=16, **kw)[0])
        assert s16 == s8, kw
        assert h16["depth"] == 16 and "depth" not in h8 and h16["arithmetic"] == codec._with_depth(h8["arithmetic"], 16)
        skip = ("arithmetic", "depth", "header_bytes")
        assert {k: v for k, v in h16.items() if k not in skip} == {k: v for k, v in h8.items() if k not in skip}
        assert h16["header_bytes"] == h8["header_bytes"] + len(",depth=16")
    t8, u8 = codec.parse_tiled(codec.encode_tiled(net, x8, tile=32)[0])
    t16, u16 = codec.parse_tiled(codec.encode_tiled(net, x16, tile=32, depth=16)[0])
    assert u16 == u8 and len(u8) == 4 and t16["arithmetic"] == codec._with_depth(t8["arithmetic"], 16)
    assert (t16["th"], t16["tw"], t16["ny"], t16["nx"]) == (t8["th"], t8["tw"], t8["ny"], t8["nx"])


# ------------------------------------------------------------------------------------------------ 5. round trip
@pytest.mark.parametrize("d", [10, 16])
@pytest.mark.parametrize("chroma", FORMATS)
def test_round_trip_is_the_encoders_reconstruction_alone_and_in_a_batch(chroma, d):
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import encode_strings_planes
    net = _net()
    nets = net.nets()
    B, H, W, L = 3, 37, 53, 3
    x = _images(B, H, W, 3, d, chroma)
    blobs = codec.encode_images(net, x, depth=d, chroma=chroma)
    got = codec.decode_images(net, blobs)
    th, tw, _, _ = codec.chroma_sizes(L, False, H, W, chroma)
    planes = _cut(x.to(DEV), chroma, (th, tw, 1, 1), 0, B, d)
    with torch.no_grad():
        if chroma == "420":
            y = encode_strings_planes(nets[0:1], planes[0], recon=True)
            c = encode_strings_planes(nets[1:3], planes[1], recon=True)
            streams = [[s for r, np_ in ((y, 1), (c, 2)) for p in range(np_) for s in [r[0][p][b]] + [lev[p][b] for lev in r[1]]]
                       for b in range(B)]
            xhat = (y[2].contiguous(), c[2].contiguous())
        else:
            r = encode_strings_planes(nets[0:1] if chroma == "400" else nets, planes, recon=True)
            streams = [[s for p in range(len(r[0])) for s in [r[0][p][b]] + [lev[p][b] for lev in r[1]]] for b in range(B)]
            xhat = r[2].contiguous()
    want = codec._write_tiles(chroma, d, xhat, (H, W, th, tw, 1, 1), (0, 0, H, W), B=B).cpu()
    assert torch.equal(want, _tile_scatter(_ref_out(chroma, _cpu(xhat), d), list(range(B)), (H, W, th, tw, 1, 1), (0, 0, H, W), B))
    for b in range(B):
        hdr, s = codec.parse_container(blobs[b])
        assert s == streams[b] and hdr["depth"] == d and hdr.get("chroma", "444") == chroma and blobs[b][:4] == b"LLDW"
        assert got[b].dtype == torch.uint16 and got[b].shape == x.shape[1:] and torch.equal(got[b], want[b]), b
        # batch invariance: the image alone gives the same container and the same pixels
        alone = codec.encode_images(net, x[b:b + 1], depth=d, chroma=chroma)
        assert alone == [blobs[b]] and torch.equal(codec.decode_images(net, alone)[0], got[b])
    with pytest.raises(ValueError, match="depth"):                      # one depth per decode call
        codec.decode_images(net, [blobs[0], codec.encode_images(net, _images8(1, H, W, 3, chroma).to(torch.uint8), chroma=chroma)[0]])


def test_none_and_8_are_todays_bytes():
    net = _net()
    x = _images8(2, 40, 56, 3).to(torch.uint8)
    plain = codec.encode_images(net, x)
    assert plain == codec.encode_images(net, x, depth=None) == codec.encode_images(net, x, depth=8)
    hdr = codec.read_header(plain[0])
    assert "depth" not in hdr and "depth" not in hdr["arithmetic"]
    tiled = codec.encode_tiled(net, x, tile=32)
    assert tiled == codec.encode_tiled(net, x, tile=32, depth=None) == codec.encode_tiled(net, x, tile=32, depth=8)
    dec = codec.decode_images(net, plain)
    assert dec[0].dtype == torch.uint8 and codec.decode_tiled(net, tiled[0]).dtype == torch.uint8
    grey = x[..., :1].contiguous()
    assert codec.encode_images(net, grey, chroma="400") == codec.encode_images(net, grey, chroma="400", depth=8)


# ------------------------------------------------------------------------------------------------ 6. tiles
@pytest.mark.parametrize("chroma", FORMATS)
def test_tiled_streams_regions_and_touched_tiles(chroma, monkeypatch):
    net = _net()
    H, W, L, d = 100, 150, 3, 12
    x = _images(1, H, W, 6, d, chroma)
    blob = codec.encode_tiled(net, x, tile=48, depth=d, chroma=chroma)[0]
    assert blob == codec.encode_tiled(net, x, tile=48, tiles_per_call=5, depth=d, chroma=chroma)[0]
    hdr, tiles = codec.parse_tiled(blob)
    th, tw, ny, nx = hdr["th"], hdr["tw"], hdr["ny"], hdr["nx"]
    assert (th, tw, ny, nx) == codec.chroma_sizes(L, False, H, W, chroma, 48) and blob[:4] == b"LLDT" and hdr["depth"] == d
    # every tile is an independent image: its streams are those of encode_images of the tile's (replicate-padded) crop
    crops = torch.stack([_tile_gather(x[..., c].to(torch.int32), th, tw, ny, nx, 0, ny * nx) for c in range(x.shape[3])], -1)
    for t, single in enumerate(codec.encode_images(net, _u16(crops), depth=d, chroma=chroma)):
        assert codec.parse_container(single)[1] == tiles[t], t
    full = codec.decode_tiled(net, blob)
    assert full.shape == (H, W, x.shape[3]) and full.dtype == torch.uint16
    assert torch.equal(full, codec.decode_tiled(net, blob, tiles_per_call=5))
    seen = _spy(monkeypatch)
    for region in [(11, 21, 59, 71), (th - 1, tw - 1, 3, 3), (99, 149, 1, 1), (31, 0, 5, 150)]:
        y0, x0, h, w = region
        seen.clear()
        got = codec.decode_tiled(net, blob, region=region, tiles_per_call=2)
        assert torch.equal(got, full[y0:y0 + h, x0:x0 + w]), region
        touched = ((y0 + h - 1) // th - y0 // th + 1) * ((x0 + w - 1) // tw - x0 // tw + 1)
        assert sum(n for th_, tw_, n, _, _ in seen if (th_, tw_) == (th, tw)) == touched, region


# ------------------------------------------------------------------------------------------------ 7. reduce
@pytest.mark.parametrize("chroma", FORMATS)
def test_reduced_decoding_untiled_and_tiled(chroma, monkeypatch):
    """reduce = 1, 2: the reference applied to the LL band the decoder reached, with the ll_affine map."""
    net = _net()
    d = 12
    B, H, W = 2, 72, 90
    x = _images(B, H, W, 7, d, chroma)
    blobs = codec.encode_images(net, x, depth=d, chroma=chroma)
    th, tw, _, _ = codec.chroma_sizes(3, False, H, W, chroma)
    big = _images(1, 100, 150, 8, d, chroma)
    tiled = codec.encode_tiled(net, big, tile=48, depth=d, chroma=chroma)[0]
    thdr = codec.read_header(tiled)
    seen = _spy(monkeypatch)
    for k in (1, 2):
        af = codec.ll_norm(net, k)
        Hr, Wr = -(-H >> k), -(-W >> k)
        seen.clear()
        got = codec.decode_images(net, blobs, reduce=k)
        px = _ref_out(chroma, _seen_res(chroma, seen), d, af)
        want = _tile_scatter(px, list(range(B)), (Hr, Wr, th >> k, tw >> k, 1, 1), (0, 0, Hr, Wr), B)
        for b in range(B):
            assert got[b].dtype == torch.uint16 and torch.equal(got[b], want[b]), (k, b)
        Hr, Wr = -(-100 >> k), -(-150 >> k)
        grid = (Hr, Wr, thdr["th"] >> k, thdr["tw"] >> k, thdr["ny"], thdr["nx"])
        seen.clear()
        got = codec.decode_tiled(net, tiled, reduce=k, tiles_per_call=64)
        px = _ref_out(chroma, _seen_res(chroma, seen), d, af)
        assert torch.equal(got, _tile_scatter(px, list(range(thdr["ny"] * thdr["nx"])), grid, (0, 0, Hr, Wr), 1)[0]), k
        if k == 1:                                                    # a region in the reduced image's coordinates, odd origin
            assert torch.equal(codec.decode_tiled(net, tiled, reduce=1, region=(7, 19, 30, 41)), got[7:37, 19:60])


# ------------------------------------------------------------------------------------------------ 8. rate options
@pytest.mark.parametrize("kw", [dict(coder="gpu"), dict(step=2.5), dict(step=2.0, rdo=13 / 64)], ids=["gpu", "step", "rdo"])
def test_rate_options_round_trip_at_depth_12(kw):
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import encode_strings_planes
    net = _gain_net()
    H, W, d = 72, 90, 12
    x = _images(1, H, W, 9, d)
    blob = codec.encode_images(net, x, depth=d, **kw)[0]
    hdr, s = codec.parse_container(blob)
    assert hdr["depth"] == d and hdr["coder"] == kw.get("coder", "host") and hdr["step"] == kw.get("step", 1.0)
    planes = ops.u16hwc_to_ycc_tiles(x.to(DEV), 72, 96, 1, 1, 0, 1, d)
    with torch.no_grad():
        s_xe, s_xo, xhat = encode_strings_planes(net.nets(), planes, recon=True, **kw)
    assert s == [t for p in range(3) for t in [s_xe[p][0]] + [lev[p][0] for lev in s_xo]]
    want = ops.ycc_tiles_to_u16hwc(xhat.contiguous(), (H, W, 72, 96, 1, 1), (0, 0, H, W), d).cpu()[0]
    assert torch.equal(codec.decode_images(net, [blob])[0], want)
    # the option reached the streams: the finest level's stream of each plane differs from the call without it
    other = dict(kw, rdo=None) if "rdo" in kw else {}
    plain = codec.parse_container(codec.encode_images(net, x, depth=d, **other)[0])[1]
    assert all(s[p * 4 + 1] != plain[p * 4 + 1] for p in range(3))


def test_target_bytes_at_depth_12():
    net = _gain_net()
    H, W, d = 72, 90, 12
    x = _images(1, H, W, 10, d)
    size = len(codec.encode_images(net, x, depth=d)[0])
    T = int(0.7 * size)
    blob = codec.encode_images(net, x, depth=d, target_bytes=T)[0]
    hdr = codec.read_header(blob)
    assert len(blob) <= T and hdr["depth"] == d and hdr["step"] > 1.0
    assert blob == codec.encode_images(net, x, depth=d, step=hdr["step"])[0]
    out = codec.decode_images(net, [blob])[0]
    assert out.dtype == torch.uint16 and out.shape == (H, W, 3)


# ------------------------------------------------------------------------------------------------ 9. quality
def test_quality_at_depth_12():
    d, M = 12, 4095
    B, H, W = 2, 61, 83
    a = _images(B, H, W, 11, d)
    g = torch.Generator().manual_seed(12)
    b = _u16((a.to(torch.int32) + torch.randint(-200, 201, a.shape, generator=g, dtype=torch.int32)).clamp(0, M))
    q = codec.quality(a, b, depth=d)
    sse = ((a.numpy().astype(np.float64) - b.numpy().astype(np.float64)) ** 2).reshape(B, -1).sum(1)
    want = 10.0 * np.log10(float(M) ** 2 * 3 * H * W / sse)
    for i in range(B):
        print("quality depth 12: psnr %.9f dB, float64 %.9f dB" % (q["psnr"][i], want[i]))
        assert abs(q["psnr"][i] - want[i]) <= 1e-6 * want[i]
    assert q["msssim"] == [None, None]
    same = codec.quality(a[0], a[0].to(DEV), depth=d)
    assert same["psnr"] == math.inf and same["msssim"] is None
    big = _images(1, 161, 170, 13, d)
    q = codec.quality(big, big.clone(), depth=d)
    assert q["psnr"] == [math.inf] and abs(q["msssim"][0] - 1.0) <= 1e-6


# ------------------------------------------------------------------------------------------------ 10. the tool
@pytest.mark.parametrize("ext", ["npy", "ppm"])
def test_command_line_tool(ext, tmp_path):
    import importlib.util
    d = 10
    cfg = {"dwtlevels": 3, "entropy_layer": "conditioned2ZTsepSubbands", "seed": 7}
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    tool = os.path.join(REPO, "tools", "codec.py")
    spec = importlib.util.spec_from_file_location("codec_cli", tool)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    x = _images(1, 77, 101, 11, d)
    src, dst = str(tmp_path / ("in." + ext)), str(tmp_path / ("out." + ext))
    if ext == "npy":
        np.save(src, x[0].numpy())
    else:
        cli.write_pnm(src, x[0].numpy(), (1 << d) - 1)
    run = lambda *a: subprocess.run([sys.executable, tool] + list(a), capture_output=True, text=True, timeout=600)
    r = run("encode", "--config", str(tmp_path / "cfg.json"), "--depth", str(d), src, str(tmp_path / "out.lld"))
    assert r.returncode == 0, r.stderr[-3000:]
    r = run("info", str(tmp_path / "out.lld"))
    assert r.returncode == 0 and "sample depth    10 bits" in r.stdout, r.stdout + r.stderr
    r = run("decode", "--config", str(tmp_path / "cfg.json"), str(tmp_path / "out.lld"), dst)
    assert r.returncode == 0, r.stderr[-3000:]
    r = run("compare", "--depth", str(d), src, dst)
    assert r.returncode == 0 and r.stdout.startswith("psnr "), r.stdout + r.stderr
    net = cli.build_net(str(tmp_path / "cfg.json"))
    blob = codec.encode_images(net, x, depth=d)[0]
    assert blob == (tmp_path / "out.lld").read_bytes()
    want = codec.decode_images(net, [blob])[0]
    got = cli.load_deep(dst, d)
    assert torch.equal(got, want)
    assert float(r.stdout.split()[1]) == pytest.approx(codec.quality(x[0], want, depth=d)["psnr"], abs=1e-4)
