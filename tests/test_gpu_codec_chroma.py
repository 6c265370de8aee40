"""GPU: the chroma formats 4:2:0 and 4:0:0 of the codec -- the four kernels of csrc/chroma.hip bit for bit
against tests/chroma_ref.py and their 4:4:4 siblings, the container round trip against single-plane coding, batch invariance,
tiles and regions, reduced decoding, the rate options and the command-line tool.  The weights are seeded, not trained: no test
asserts a byte saving or a PSNR."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest
import torch

import chroma_ref
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import codec, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = ("conditioned2ZTsepSubbands", "onlyEZWT", "DWTConditioned2EntropyLayerZTBlock")
MODELS = [(l, "LiftingBasedNeuralWaveletv4") for l in LAYERS] + [("onlyEZWT", "CDF97")]
FORMATS = ("420", "400")
_NETS = {}


def _net(layer="conditioned2ZTsepSubbands", L=3, **over):
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
        LiftingBasedDWTNetWrapper
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
    key = (layer, L, tuple(sorted(over.items())))
    if key not in _NETS:
        cfg = make_config(dwtlevels=L, mode="validate", entropy_layer=layer, **over)
        torch.manual_seed(0)
        _NETS[key] = LiftingBasedDWTNetWrapper(cfg).to(DEV).eval()
    return _NETS[key]


def _gain_net(layer="conditioned2ZTsepSubbands", L=3, gain=100.0):
    """The net of the rate tests, as tests/test_gpu_codec_step.py builds it: the deterministic filled weights with the last
    (linear) layer of the subband auto-encoders of the levels 0 .. L-2 scaled by ``gain``.  With seeded or filled weights alone
    every symbol of those levels is 0 from step 1 on, so no step, Lagrangian or byte target could be told from another."""
    from helpers import filled
    from oracle import weights
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
        LiftingBasedDWTNetWrapper
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
    key = ("gain", layer, L)
    if key not in _NETS:
        cfg = make_config(dwtlevels=L, mode="validate", entropy_layer=layer)
        net = LiftingBasedDWTNetWrapper(cfg)
        net.load_state_dict(filled(weights.wrapper_template(dict(cfg))), strict=False)
        net = net.to(DEV).eval()
        with torch.no_grad():
            for n in net.nets():
                for lev in range(L - 1):
                    last = n.autoencoder.Yh_ae[lev].ae_down[6]
                    last.weight.mul_(gain)
                    last.bias.mul_(gain)
        _NETS[key] = net
    return _NETS[key]


def _images(B, H, W, seed, chroma="420"):
    """Smooth fields plus noise, as uint8 (B,H,W,3) on the host, or (B,H,W,1) for "400"."""
    ch = 1 if chroma == "400" else 3
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(B, ch, max(2, H // 16), max(2, W // 16), generator=g)
    x = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
    x = x * 200 + torch.rand(B, ch, H, W, generator=g) * 40
    return x.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _fp32(vals):
    return torch.tensor(vals, dtype=torch.float32).tolist()


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
    """tiles_px (n,th,tw) uint8 on the host, their tile indexes -> (B,h,w): the pixels inside the image and the region."""
    H, W, th, tw, ny, nx = grid
    y0, x0, h, w = region
    out = torch.full((B, h, w), fill, dtype=torch.uint8)
    for j, t in enumerate(tiles):
        b, r = divmod(t, ny * nx)
        ty, tx = divmod(r, nx)
        for y in range(max(y0, ty * th), min(y0 + h, H, (ty + 1) * th)):
            lo, hi = max(x0, tx * tw), min(x0 + w, W, (tx + 1) * tw)
            if hi > lo:
                out[b, y - y0, lo - x0:hi - x0] = tiles_px[j, y - ty * th, lo - tx * tw:hi - tx * tw]
    return out


def _full_planes(luma, chroma, affine=None):
    """luma (1,n,1,h,w), chroma (2,n,1,h/2,w/2) on the device -> (3,n,1,h,w): the chroma upsampled by the reference (after the
    per-plane affine map of a reduced decode, when given)."""
    c = chroma.cpu()
    if affine is not None:
        c = torch.stack([chroma_ref.affine(c[i], affine[0][i + 1], affine[1][i + 1]) for i in range(2)])
    return torch.cat([luma, chroma_ref.upsample(c).to(DEV)], 0).contiguous()


def _compose(chroma, res, H, W, affine=None):
    """What a decode must return for the decoded planes res -- (luma, chroma planes) or the single plane, n images each the one
    tile of a 1 x 1 grid: the reference upsampling and the byte rule -> (n,H,W,C) uint8 on the host."""
    if chroma == "400":
        s = res.cpu()[0, :, 0, :H, :W]
        if affine is not None:
            s = chroma_ref.affine(s, affine[0][0], affine[1][0])
        return chroma_ref.grey_out(s)[..., None]
    full = _full_planes(res[0], res[1], affine)
    n, h, w = full.shape[1], full.shape[3], full.shape[4]
    if affine is None:
        return ops.ycc_tiles_to_u8hwc(full, (H, W, h, w, 1, 1), (0, 0, H, W), B=n).cpu()
    return ops.ll_tiles_to_u8hwc(full, (H, W, h, w, 1, 1), (0, 0, H, W), [affine[0][0], 1.0, 1.0], [affine[1][0], 0.0, 0.0],
                                 B=n).cpu()


def _input_planes(x_dev, chroma, th, tw):
    """The planes an untiled encode codes, one (1,B,1,h,w) tensor per plane."""
    B = x_dev.shape[0]
    if chroma == "400":
        return [ops.u8hw_to_y_tiles(x_dev, th, tw, 1, 1, 0, B)]
    luma, c = ops.u8hwc_to_ycc420_tiles(x_dev, th, tw, 1, 1, 0, B)
    return [luma, c[0:1], c[1:2]]


def _single_plane_coding(net, planes, **kw):
    """Every plane coded alone by its own net, encode_strings_planes([nets[p]], x_p, ...), and decoded alone from those strings,
    decode_strings_planes([nets[p]], ...) -> (the streams per image in the LLDW order, the decoded planes as _compose takes
    them).  kw: coder, step, rdo (the decoder takes the first two)."""
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
        decode_strings_planes, encode_strings_planes
    nets = net.nets()
    B = planes[0].shape[1]
    dkw = {k: v for k, v in kw.items() if k in ("coder", "step")}
    with torch.no_grad():
        parts = [encode_strings_planes([nets[p]], x, **kw) for p, x in enumerate(planes)]
        xh = [decode_strings_planes([nets[p]], r[0], r[1], x.shape[3], x.shape[4], B, **dkw).contiguous()
              for p, (r, x) in enumerate(zip(parts, planes))]
    streams = [[s for r in parts for s in [r[0][0][b]] + [lev[0][b] for lev in r[1]]] for b in range(B)]
    return streams, (xh[0] if len(xh) == 1 else (xh[0], torch.cat(xh[1:], 0)))


def _spy(monkeypatch):
    """Wraps the codec._decode_tiles hook -> list of (th, tw, n, streams handed to the coder, result) per call."""
    seen, real = [], codec._decode_tiles

    def wrapped(nets, s_xe, s_xo, th_, tw_, n, **kw):
        out = real(nets, s_xe, s_xo, th_, tw_, n, **kw)
        seen.append((th_, tw_, n, [s for p in s_xe for s in p] + [s for lev in s_xo for p in lev for s in p], out))
        return out
    monkeypatch.setattr(codec, "_decode_tiles", wrapped)
    return seen


# ------------------------------------------------------------------------------------------------ 1. input kernels
@pytest.mark.parametrize("B,H,W", [(1, 37, 53), (3, 200, 120)])
@pytest.mark.parametrize("L", [3, 4])
def test_input_kernels_bit_exact(B, H, W, L):
    img = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(B * H + L)).to(DEV)
    grey = img[..., 1:2].contiguous()
    th, tw, _, _ = codec.chroma_sizes(L, False, H, W, "420")
    # untiled, then a 2 x 3 grid (even tiles that cover the image) with a first / n sub-range
    for (gh, gw, ny, nx, first, n) in ((th, tw, 1, 1, 0, B), (2 * -(-H // 4), 2 * -(-W // 6), 2, 3, 1, 6 * B - 2)):
        luma, chroma = ops.u8hwc_to_ycc420_tiles(img, gh, gw, ny, nx, first, n)
        full = ops.u8hwc_to_ycc_tiles(img, gh, gw, ny, nx, first, n)
        assert luma.shape == (1, n, 1, gh, gw) and chroma.shape == (2, n, 1, gh // 2, gw // 2)
        assert torch.equal(luma, full[0:1])
        # odd H and W: the clamp falls inside a 2 x 2 block, which the padded 4:4:4 planes already hold
        assert torch.equal(chroma.cpu(), chroma_ref.downsample(full[1:3].cpu()))
        y = ops.u8hw_to_y_tiles(grey, gh, gw, ny, nx, first, n)
        assert y.shape == (1, n, 1, gh, gw)
        assert torch.equal(y.cpu()[0, :, 0], _tile_gather(chroma_ref.grey_in(grey.cpu()[..., 0]), gh, gw, ny, nx, first, n))
    with pytest.raises(RuntimeError):
        ops.u8hwc_to_ycc420_tiles(img, th + 1, tw, 1, 1, 0, B)                        # an odd tile side
    with pytest.raises(RuntimeError):
        ops.u8hw_to_y_tiles(img, th, tw, 1, 1, 0, B)                                  # three channels


# ------------------------------------------------------------------------------------------------ 2. output kernels
@pytest.mark.parametrize("B,H,W,th,tw,ny,nx", [(2, 37, 53, 48, 64, 1, 1), (2, 75, 110, 40, 48, 2, 3)])
def test_output_kernels_bit_exact(B, H, W, th, tw, ny, nx):
    g = torch.Generator().manual_seed(H)
    per = ny * nx
    tile_lists = [None] if per == 1 else [None, [7, 2, 11, 5, 0]]
    regions = [(0, 0, H, W), (3, 5, H - 10, W - 12), (H - 1, W - 1, 1, 1), (th - 1 if per > 1 else 11, tw - 1 if per > 1 else 9, 7, 5)]
    inv_a, b = _fp32([0.3517, 0.127, 0.509]), _fp32([0.0123, -0.0456, 0.0789])
    for tiles in tile_lists:
        n = B * per if tiles is None else len(tiles)
        luma = (torch.rand(1, n, 1, th, tw, generator=g) * 1.4 - 0.7).to(DEV)          # beyond [-0.5, 0.5]: the clamp
        chroma = (torch.rand(2, n, 1, th // 2, tw // 2, generator=g) * 1.4 - 0.7).to(DEV)
        ident = list(range(n)) if tiles is None else tiles
        for region in regions:
            kw = dict(tiles=tiles, B=B)
            grid = (H, W, th, tw, ny, nx)
            h, w = region[2:]
            # 4:2:0, plain and affine: the 4:4:4 kernels on the reference-upsampled planes
            want = ops.ycc_tiles_to_u8hwc(_full_planes(luma, chroma), grid, region, out=torch.zeros(B, h, w, 3, dtype=torch.uint8,
                                                                                                  device=DEV), **kw)
            got = ops.ycc420_tiles_to_u8hwc(luma, chroma, grid, region, out=torch.zeros(B, h, w, 3, dtype=torch.uint8, device=DEV),
                                            **kw)
            assert torch.equal(got, want), (tiles, region)
            want = ops.ll_tiles_to_u8hwc(_full_planes(luma, chroma, (inv_a, b)), grid, region, [inv_a[0], 1.0, 1.0],
                                         [b[0], 0.0, 0.0], out=torch.zeros(B, h, w, 3, dtype=torch.uint8, device=DEV), **kw)
            got = ops.ycc420_tiles_to_u8hwc(luma, chroma, grid, region, affine=(inv_a, b),
                                            out=torch.zeros(B, h, w, 3, dtype=torch.uint8, device=DEV), **kw)
            assert torch.equal(got, want), (tiles, region, "affine")
            # 4:0:0, plain and affine: the torch expression
            for af in (None, (inv_a[:1], b[:1])):
                s = luma.cpu()[0, :, 0]
                if af is not None:
                    s = chroma_ref.affine(s, af[0][0], af[1][0])
                want = _tile_scatter(chroma_ref.grey_out(s), ident, grid, region, B)[..., None]
                got = ops.y_tiles_to_u8hw(luma, grid, region, affine=af, out=torch.zeros(B, h, w, 1, dtype=torch.uint8, device=DEV),
                                          **kw)
                assert torch.equal(got.cpu(), want), (tiles, region, af)
    assert ops.ycc420_tiles_to_u8hwc(luma, chroma, grid, regions[0], **kw).shape == (B, H, W, 3)
    with pytest.raises(RuntimeError):
        ops.ycc420_tiles_to_u8hwc(luma, chroma[:, :, :, :-1].contiguous(), grid, regions[0], **kw)
    with pytest.raises(RuntimeError):
        ops.ycc420_tiles_to_u8hwc(luma, chroma, grid, (0, 0, H + 1, W), **kw)          # a region outside the image


# ------------------------------------------------------------------------------------------------ 3. round trip
@pytest.mark.parametrize("chroma", FORMATS)
@pytest.mark.parametrize("layer,netType", MODELS)
def test_round_trip_equals_single_plane_coding(layer, netType, chroma):
    net = _net(layer, netType=netType)
    B, H, W, L = 2, 72, 90, 3
    x = _images(B, H, W, 1, chroma)
    blobs = codec.encode_images(net, x, chroma=chroma)
    got = codec.decode_images(net, blobs)
    th, tw, _, _ = codec.chroma_sizes(L, netType == "CDF97", H, W, chroma)
    assert (th, tw) == ((80, 96) if chroma == "420" else (72, 96))
    planes = _input_planes(x.to(DEV), chroma, th, tw)
    streams, xhat = _single_plane_coding(net, planes)
    ref = _compose(chroma, xhat, H, W)
    for b in range(B):
        hdr, s = codec.parse_container(blobs[b])
        assert s == streams[b] and len(s) == len(planes) * (L + 1)
        assert hdr["chroma"] == chroma and "chroma=%s" % chroma in hdr["arithmetic"].split(",") and blobs[b][:4] == b"LLDW"
        assert (hdr["H"], hdr["W"], hdr["dwtlevels"], hdr["layer"], hdr["netType"]) == (H, W, L, layer, netType)
        assert len(blobs[b]) == hdr["header_bytes"] + sum(len(t) for t in s) + 4
        assert got[b].shape == (H, W, len(planes)) and got[b].dtype == torch.uint8
        assert torch.equal(got[b], ref[b]), b
    print("%s / %s chroma=%s 72x90: %d bytes (seeded weights)" % (layer, netType, chroma, len(blobs[0])))


def test_444_is_the_default_and_writes_no_key():
    net = _net()
    x = _images(2, 40, 56, 3)
    plain = codec.encode_images(net, x)
    assert plain == codec.encode_images(net, x, chroma="444") == codec.encode_images(net, x, chroma=None)
    hdr = codec.read_header(plain[0])
    assert "chroma" not in hdr and "chroma" not in hdr["arithmetic"]
    assert codec.encode_tiled(net, x, tile=32) == codec.encode_tiled(net, x, tile=32, chroma="444")


# ------------------------------------------------------------------------------------------------ 4. batch invariance
def test_batch_invariance_and_a_mixed_decode():
    net = _net()
    H, W = 56, 72
    x = _images(4, H, W, 2)
    grey = _images(4, H, W, 4, "400")
    out = {}
    for chroma, imgs in (("420", x), ("400", grey)):
        batch = codec.encode_images(net, imgs, chroma=chroma)
        alone = [codec.encode_images(net, imgs[b:b + 1], chroma=chroma)[0] for b in range(4)]
        assert batch == alone, chroma
        out[chroma] = (batch, codec.decode_images(net, batch))
        assert torch.equal(codec.decode_images(net, [batch[2]])[0], out[chroma][1][2])
    full = codec.encode_images(net, x[:2])
    dec_full = codec.decode_images(net, full)
    # one call on a 444 / 420 / 400 mix of one size: grouped by format, returned in input order
    mixed = codec.decode_images(net, [out["420"][0][1], full[0], out["400"][0][3], out["420"][0][0], full[1], out["400"][0][0]])
    want = [out["420"][1][1], dec_full[0], out["400"][1][3], out["420"][1][0], dec_full[1], out["400"][1][0]]
    assert [tuple(m.shape) for m in mixed] == [(H, W, 3), (H, W, 3), (H, W, 1), (H, W, 3), (H, W, 3), (H, W, 1)]
    for m, w_ in zip(mixed, want):
        assert torch.equal(m, w_)


# ------------------------------------------------------------------------------------------------ 5. tiles
@pytest.mark.parametrize("chroma", FORMATS)
def test_tiled_streams_regions_and_touched_tiles(chroma, monkeypatch):
    net = _net()
    H, W, L = 100, 150, 3
    x = _images(1, H, W, 6, chroma)
    blob = codec.encode_tiled(net, x, tile=48, chroma=chroma)[0]
    assert blob == codec.encode_tiled(net, x, tile=48, tiles_per_call=5, chroma=chroma)[0]
    hdr, tiles = codec.parse_tiled(blob)
    th, tw, ny, nx = hdr["th"], hdr["tw"], hdr["ny"], hdr["nx"]
    assert (th, tw, ny, nx) == codec.chroma_sizes(L, False, H, W, chroma, 48) == ((48, 48, 3, 4) if chroma == "420" else (40, 40, 3, 4))
    assert hdr["chroma"] == chroma and hdr["streams_per_tile"] == codec.CHROMA_PLANES[chroma] * (L + 1) and blob[:4] == b"LLDT"
    # every tile is an independent image: its streams are those of encode_images of the tile's (replicate-padded) crop
    crops = torch.stack([_tile_gather(x[..., c], th, tw, ny, nx, 0, ny * nx) for c in range(x.shape[3])], -1)
    for t, single in enumerate(codec.encode_images(net, crops, chroma=chroma)):
        assert codec.parse_container(single)[1] == tiles[t], t
    full = codec.decode_tiled(net, blob)
    assert full.shape == (H, W, x.shape[3])
    assert torch.equal(full, codec.decode_tiled(net, blob, tiles_per_call=5))
    seen = _spy(monkeypatch)
    for region in [(11, 21, 59, 71), (th - 1, tw - 1, 3, 3), (99, 149, 1, 1), (31, 0, 5, 150)]:
        y0, x0, h, w = region
        seen.clear()
        got = codec.decode_tiled(net, blob, region=region, tiles_per_call=2)
        assert torch.equal(got, full[y0:y0 + h, x0:x0 + w]), region
        touched = ((y0 + h - 1) // th - y0 // th + 1) * ((x0 + w - 1) // tw - x0 // tw + 1)
        assert sum(n for th_, tw_, n, _, _ in seen if (th_, tw_) == (th, tw)) == touched, region
        if chroma == "420":                                           # and the same tiles' chroma plane pairs, no neighbour
            assert sum(n for th_, tw_, n, _, _ in seen if (th_, tw_) == (th // 2, tw // 2)) == touched, region
            assert all(tuple(out.shape[:2]) == ((1, n) if th_ == th else (2, n)) for th_, _, n, _, out in seen)


# ------------------------------------------------------------------------------------------------ 6. reduce
@pytest.mark.parametrize("chroma", FORMATS)
def test_reduced_decoding_untiled(chroma, monkeypatch):
    net = _net()
    B, H, W, L = 2, 72, 90, 3
    x = _images(B, H, W, 7, chroma)
    blobs = codec.encode_images(net, x, chroma=chroma)
    hdrs = [codec.read_header(b) for b in blobs]
    seen = _spy(monkeypatch)
    for k in range(L + 1):
        seen.clear()
        got = codec.decode_images(net, blobs, reduce=k)
        Hr, Wr = -(-H >> k), -(-W >> k)
        planes = [s[4].contiguous() for s in seen]                    # luma, then for 4:2:0 the (Cb, Cr) pair: one call each
        assert [p.shape[0] for p in planes] == ([1] if chroma == "400" else [1, 2])
        res = planes[0] if chroma == "400" else (planes[0], planes[1])
        want = _compose(chroma, res, Hr, Wr, codec.ll_norm(net, k) if k else None)
        for b in range(B):
            assert got[b].shape == (Hr, Wr, x.shape[3]) and torch.equal(got[b], want[b]), (k, b)
        # the bytes a reduced decode reads are the streams actually handed to the coder, plus the headers
        handed = sum(len(s) for call in seen for s in call[3])
        assert sum(codec.reduce_bytes(h)[k] - h["header_bytes"] for h in hdrs) == handed, k
    assert torch.equal(codec.decode_images(net, blobs, reduce=0)[0], codec.decode_images(net, blobs)[0])


@pytest.mark.parametrize("chroma", FORMATS)
def test_reduced_decoding_tiled(chroma, monkeypatch):
    net = _net()
    H, W, L = 100, 150, 3
    x = _images(1, H, W, 8, chroma)
    blob = codec.encode_tiled(net, x, tile=48, chroma=chroma)[0]
    hdr, tiles = codec.parse_tiled(blob)
    th, tw, ny, nx = hdr["th"], hdr["tw"], hdr["ny"], hdr["nx"]
    # every tile as a container of its own: a th x tw image with the tile's streams
    own = [codec.pack_container(dict(hdr, H=th, W=tw), t) for t in tiles]
    seen = _spy(monkeypatch)
    for k in range(L + 1):
        Hr, Wr = -(-H >> k), -(-W >> k)
        seen.clear()
        got = codec.decode_tiled(net, blob, reduce=k)
        assert got.shape == (Hr, Wr, x.shape[3])
        handed = sum(len(s) for call in seen for s in call[3])
        assert codec.reduce_bytes(hdr)[k] - hdr["header_bytes"] == handed, k
        # the composition: each tile decoded alone at reduce = k, cropped to the reduced image
        alone = codec.decode_images(net, own, reduce=k)
        for c in range(x.shape[3]):
            want = _tile_scatter(torch.stack([a[..., c] for a in alone]), list(range(ny * nx)), (Hr, Wr, th >> k, tw >> k, ny, nx),
                                 (0, 0, Hr, Wr), 1)[0]
            assert torch.equal(got[..., c], want), (k, c)
        if k == 1:                                                    # a region in the reduced image's coordinates, odd origin
            assert torch.equal(codec.decode_tiled(net, blob, reduce=1, region=(7, 19, 30, 41)), got[7:37, 19:60])


# ------------------------------------------------------------------------------------------------ 7. rate options
@pytest.mark.parametrize("kw", [dict(coder="gpu"), dict(step=2.5), dict(step=2.0, rdo=13 / 64)], ids=["gpu", "step", "rdo"])
def test_rate_options_on_420(kw):
    net = _gain_net()
    H, W = 72, 90
    x = _images(1, H, W, 9)
    blob = codec.encode_images(net, x, chroma="420", **kw)[0]
    hdr, s = codec.parse_container(blob)
    assert hdr["chroma"] == "420" and hdr["coder"] == kw.get("coder", "host") and hdr["step"] == kw.get("step", 1.0)
    streams, xhat = _single_plane_coding(net, _input_planes(x.to(DEV), "420", 80, 96), **kw)
    assert s == streams[0]
    assert torch.equal(codec.decode_images(net, [blob])[0], _compose("420", xhat, H, W)[0])
    # the option reached all three planes: the finest level's stream of each differs from the call without it
    other = dict(kw, rdo=None) if "rdo" in kw else {}
    plain = codec.parse_container(codec.encode_images(net, x, chroma="420", **other)[0])[1]
    assert all(s[p * 4 + 1] != plain[p * 4 + 1] for p in range(3))


def test_target_bytes_on_420():
    net = _gain_net()
    H, W = 72, 90
    x = _images(1, H, W, 10)
    size = len(codec.encode_images(net, x, chroma="420")[0])
    chosen = []
    for T in (int(0.8 * size), int(0.55 * size)):
        blob = codec.encode_images(net, x, chroma="420", target_bytes=T)[0]
        hdr = codec.read_header(blob)
        assert len(blob) <= T and hdr["chroma"] == "420"
        assert blob == codec.encode_images(net, x, chroma="420", step=hdr["step"])[0]
        chosen.append(hdr["step"])
    assert chosen[1] >= chosen[0] > 1.0                               # a coarser target gives a coarser step
    _, xhat = _single_plane_coding(net, _input_planes(x.to(DEV), "420", 80, 96), step=chosen[1])
    assert torch.equal(codec.decode_images(net, [blob])[0], _compose("420", xhat, H, W)[0])


# ------------------------------------------------------------------------------------------------ 8. the tool
@pytest.mark.parametrize("chroma", FORMATS)
def test_command_line_tool(chroma, tmp_path):
    import numpy as np
    from PIL import Image
    cfg = {"dwtlevels": 3, "entropy_layer": "conditioned2ZTsepSubbands", "seed": 7}
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    x = _images(1, 77, 101, 11, chroma)
    Image.fromarray(x[0, ..., 0].numpy() if chroma == "400" else x[0].numpy()).save(tmp_path / "in.png")
    tool = os.path.join(REPO, "tools", "codec.py")
    run = lambda *a: subprocess.run([sys.executable, tool] + list(a), capture_output=True, text=True, timeout=600)
    r = run("encode", "--config", str(tmp_path / "cfg.json"), "--chroma", chroma, str(tmp_path / "in.png"), str(tmp_path / "out.lld"))
    assert r.returncode == 0, r.stderr[-3000:]
    r = run("decode", "--config", str(tmp_path / "cfg.json"), str(tmp_path / "out.lld"), str(tmp_path / "out.png"))
    assert r.returncode == 0, r.stderr[-3000:]
    r = run("info", str(tmp_path / "out.lld"))
    assert r.returncode == 0 and "chroma format   %s" % chroma in r.stdout, r.stdout + r.stderr
    spec = importlib.util.spec_from_file_location("codec_cli", tool)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    net = cli.build_net(str(tmp_path / "cfg.json"))
    blob = codec.encode_images(net, x, chroma=chroma)[0]
    assert blob == (tmp_path / "out.lld").read_bytes()
    want = codec.decode_images(net, [blob])[0]
    out = Image.open(tmp_path / "out.png")
    assert out.mode == ("L" if chroma == "400" else "RGB")
    got = torch.from_numpy(np.asarray(out, dtype=np.uint8).copy())
    assert torch.equal(got if chroma == "420" else got[..., None], want)
