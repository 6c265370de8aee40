"""GPU: the codec's residual layer (codec.encode_images / encode_tiled(..., near=d), LLDR, csrc/residual.hip, DESIGN.md
7.1.5) -- the three kernels against an integer torch-CPU reference written here (exact equality), lossless and bounded round
trips for the three coded layers, batch and tiles_per_call independence of the bytes, regions, reduced decoding, the device
coder, the code length against the ideal length under the chosen tables, the refusals and guards, and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import codec, irans, ops, residual
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.ans import decode_streams
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models import entropy_coding as ec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = ("conditioned2ZTsepSubbands", "onlyEZWT", "DWTConditioned2EntropyLayerZTBlock")
H, W, TILE, L = 100, 150, 64, 3                 # -> 2 x 3 tiles of 56 x 56, last row 44 high, last column 38 wide
_NETS = {}
_CACHE = {}
_M64 = (1 << 64) - 1


def _net(layer):
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
        LiftingBasedDWTNetWrapper
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
    if layer not in _NETS:
        cfg = make_config(dwtlevels=L, mode="validate", entropy_layer=layer)
        torch.manual_seed(0)
        _NETS[layer] = LiftingBasedDWTNetWrapper(cfg).to(DEV).eval()
    return _NETS[layer]


def _images(B, H, W, seed):
    """Smooth colour fields plus noise, as uint8 (B,H,W,3) on the host."""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(B, 3, max(2, H // 16), max(2, W // 16), generator=g)
    x = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
    x = x * 200 + torch.rand(B, 3, H, W, generator=g) * 40
    return x.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ reference (integers, CPU)
def _cs(u8):
    """sum_i (byte_i + 1) * (1 + i mod 65521) mod 2^64 in Python integers."""
    return sum((v + 1) * (1 + i % 65521) for i, v in enumerate(u8.reshape(-1).tolist())) & _M64


def _ref_unit(x, xh, d):
    """x, xh: (uh,uw,3) uint8 CPU -> sym (3,n), ctx (3,n), hist (3,8,2Q+1), cs(xh), cs(x), out (uh,uw,3) uint8."""
    uh, uw, _ = x.shape
    Q = (255 + d) // (2 * d + 1)
    xi, hi = x.long(), xh.long()
    r = xi - hi
    q = torch.sign(r) * ((r.abs() + d) // (2 * d + 1))
    ys, xs = torch.arange(uh), torch.arange(uw)
    g = (hi[:, (xs + 1).clamp(max=uw - 1)] - hi[:, (xs - 1).clamp(min=0)]).abs() \
        + (hi[(ys + 1).clamp(max=uh - 1)] - hi[(ys - 1).clamp(min=0)]).abs()
    a = sum((g >= (1 << k)).long() for k in range(7))             # 0 for g == 0, else min(7, 1 + floor(log2 g))
    ctx = a + 8 * torch.arange(3)
    hist = torch.zeros(24 * (2 * Q + 1), dtype=torch.long)
    hist.index_add_(0, (ctx * (2 * Q + 1) + q + Q).reshape(-1), torch.ones(uh * uw * 3, dtype=torch.long))
    out = (hi + q * (2 * d + 1)).clamp(0, 255).to(torch.uint8)
    flat = lambda t: t.permute(2, 0, 1).reshape(3, -1).int()
    return flat(q), flat(ctx), hist.reshape(3, 8, 2 * Q + 1).int(), _cs(xh), _cs(x), out


def _rect(grid, t):
    Hi, Wi, th, tw, ny, nx = grid
    b, r = divmod(t, ny * nx)
    ty, tx = divmod(r, nx)
    return b, ty * th, tx * tw, min(th, Hi - ty * th), min(tw, Wi - tx * tw)


def _pair(B, Hi, Wi, seed):
    """Originals and a reconstruction that differs by smooth error plus noise."""
    g = torch.Generator().manual_seed(seed)
    x = _images(B, Hi, Wi, seed)
    xh = (x.long() + torch.randint(-9, 10, x.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    return x, xh


def _special(Hi, Wi):
    """Image 0: constant xh (class 0 only); image 1: a 0/255 checkerboard xh with the inverse as original (g up to 510
    along the border, residuals +-255)."""
    x = _images(2, Hi, Wi, 5)
    xh = torch.empty_like(x)
    xh[0] = 77
    yy, xx = torch.meshgrid(torch.arange(Hi), torch.arange(Wi), indexing="ij")
    xh[1] = (((yy + xx) % 2) * 255).to(torch.uint8)[..., None]
    x[1] = 255 - xh[1]
    return x, xh


# (name, B, H, W, th, tw, ny, nx, calls): every call lists tiles of one rectangle size
_KCASES = [
    ("1x1", 1, 1, 1, 8, 8, 1, 1, [[0]]),
    ("3x5", 1, 3, 5, 8, 8, 1, 1, [[0]]),
    ("37x130", 1, 37, 130, 40, 136, 1, 1, [[0]]),
    ("9x257-B2", 2, 9, 257, 16, 264, 1, 1, [[0, 1], [1]]),        # crosses a 256-pixel block; B = 2
    ("special", 2, 37, 130, 40, 136, 1, 1, [[0, 1]]),
    ("grid", 2, H, W, 56, 56, 2, 3, [[1, 7], [6], [2], [10, 3], [11], [5]]),   # ragged 2 x 3 grid, tiles skipped
]


@pytest.mark.parametrize("d", [0, 1, 3])
@pytest.mark.parametrize("case", _KCASES, ids=[c[0] for c in _KCASES])
def test_kernels_equal_the_integer_reference(case, d):
    name, B, Hi, Wi, th, tw, ny, nx, calls = case
    grid, region = (Hi, Wi, th, tw, ny, nx), (0, 0, Hi, Wi)
    x, xh = _special(Hi, Wi) if name == "special" else _pair(B, Hi, Wi, 11)
    xd, hd = x.to(DEV), xh.to(DEV)
    Q = (255 + d) // (2 * d + 1)
    for tiles in calls:
        sym, ctx, hist, cs_h, cs_x = ops.resid_analyse(xd, hd, grid, region, tiles, d)
        scales = torch.randint(0, 64, (len(tiles), 24), generator=torch.Generator().manual_seed(d), dtype=torch.uint8)
        idx, cs_h2 = ops.resid_contexts(hd, grid, region, tiles, scales.to(DEV))
        out = torch.full_like(hd, 9)
        _, cs_o = ops.resid_apply(hd, grid, region, tiles, d, sym, out=out)
        sym, ctx, hist, idx, out = (t.cpu() for t in (sym, ctx, hist, idx, out))
        touched = torch.zeros(B, Hi, Wi, dtype=torch.bool)
        for j, t in enumerate(tiles):
            b, y0, x0, uh, uw = _rect(grid, t)
            rs, rc, rh, rcs_h, rcs_x, rout = _ref_unit(x[b, y0:y0 + uh, x0:x0 + uw], xh[b, y0:y0 + uh, x0:x0 + uw], d)
            assert torch.equal(sym[3 * j:3 * j + 3], rs), (tiles, t)
            assert torch.equal(ctx[3 * j:3 * j + 3], rc), (tiles, t)
            assert torch.equal(hist[j], rh) and int(hist[j].sum()) == 3 * uh * uw
            assert torch.equal(idx[3 * j:3 * j + 3], scales[j].int()[rc.long()]), (tiles, t)
            assert int(cs_h[j]) & _M64 == rcs_h and int(cs_h2[j]) & _M64 == rcs_h and int(cs_x[j]) & _M64 == rcs_x
            assert torch.equal(out[b, y0:y0 + uh, x0:x0 + uw], rout)
            assert int(cs_o[j]) & _M64 == _cs(rout)
            err = (rout.long() - x[b, y0:y0 + uh, x0:x0 + uw].long()).abs().max()
            assert int(err) <= d and int(rs.abs().max()) <= Q
            touched[b, y0:y0 + uh, x0:x0 + uw] = True
        assert torch.all(out[~touched] == 9)                      # nothing outside the listed units is written
        if name == "special":
            assert set(ctx[0:3].reshape(-1).tolist()) == {0, 8, 16}                      # constant xh: class 0 only
            # checkerboard: the two neighbours along an axis are equal, so g = 0 inside; the clamped border gives 255 and
            # the corners 510, the largest g there is
            assert set(ctx[3:6].reshape(-1).tolist()) == {0, 7, 8, 15, 16, 23}
            assert set(sym[3:6].reshape(-1).tolist()) == {-Q, Q}


def test_kernels_on_a_region_buffer_and_in_place():
    """The decoder's shape: buffers that hold the rectangle of the touched tiles only, refined in place."""
    grid = (H, W, 56, 56, 2, 3)
    x, xh = _pair(1, H, W, 12)
    region, tiles = (56, 56, 44, 94), [4, 5]                      # the last tile row, columns 1 and 2
    full = (0, 0, H, W)
    crop = lambda t: t[:, 56:100, 56:150].contiguous()
    for grp in ([4], [5]):
        sym, ctx, hist, cs_h, cs_x = ops.resid_analyse(x.to(DEV), xh.to(DEV), grid, full, grp, 1)
        sym_r, ctx_r, hist_r, cs_hr, cs_xr = ops.resid_analyse(crop(x).to(DEV), crop(xh).to(DEV), grid, region, grp, 1)
        assert torch.equal(sym, sym_r) and torch.equal(ctx, ctx_r) and torch.equal(hist, hist_r)
        assert torch.equal(cs_h, cs_hr) and torch.equal(cs_x, cs_xr)
        buf = crop(xh).to(DEV)
        want, _ = ops.resid_apply(xh.to(DEV), grid, full, grp, 1, sym, out=xh.to(DEV))
        got, _ = ops.resid_apply(buf, grid, region, grp, 1, sym)
        assert got is buf and torch.equal(crop(want.cpu()), got.cpu())


def test_kernel_wrappers_refuse_bad_arguments():
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd._lib import LLDWTError
    grid = (H, W, 56, 56, 2, 3)
    x, xh = (t.to(DEV) for t in _pair(1, H, W, 13))
    with pytest.raises(LLDWTError, match="one rectangle size"):
        ops.resid_analyse(x, xh, grid, (0, 0, H, W), [0, 2], 0)
    with pytest.raises(LLDWTError, match="tile index"):
        ops.resid_analyse(x, xh, grid, (0, 0, H, W), [6], 0)
    with pytest.raises(LLDWTError, match="bound"):
        ops.resid_analyse(x, xh, grid, (0, 0, H, W), [0], 33)
    with pytest.raises(LLDWTError, match="inside the region"):
        ops.resid_contexts(xh[:, :56, :56].contiguous(), grid, (0, 0, 56, 56), [1], torch.zeros(1, 24, dtype=torch.uint8).to(DEV))
    with pytest.raises(LLDWTError, match="image buffers"):
        ops.resid_analyse(x, xh[:, :50].contiguous(), grid, (0, 0, H, W), [0], 0)
    with pytest.raises(LLDWTError, match="sym"):
        ops.resid_apply(xh, grid, (0, 0, H, W), [0], 0, torch.zeros(3, 10, dtype=torch.int32, device=DEV))


# ------------------------------------------------------------------------------------------------ end to end, untiled
def _untiled(layer):
    """(net, x (4,72,90,3), the four lossless containers of one B = 4 call, the plain containers), once per layer."""
    key = ("u", layer)
    if key not in _CACHE:
        net = _net(layer)
        x = _images(4, 72, 90, 41)
        _CACHE[key] = (net, x, codec.encode_images(net, x, near=0), codec.encode_images(net, x))
    return _CACHE[key]


@pytest.mark.parametrize("layer", LAYERS)
def test_lossless_and_near_lossless_images(layer):
    net, x, blobs, plain = _untiled(layer)
    for i in range(4):
        hdr, base, units = codec.parse_refined(blobs[i])
        assert blobs[i][:4] == b"LLDR" and hdr["near"] == 0 and base == plain[i]        # the base is the plain container
        assert codec.encode_images(net, x[i:i + 1], near=0)[0] == blobs[i]               # the batch changes no byte
        assert torch.equal(codec.decode_images(net, [blobs[i]])[0], x[i])               # bit for bit, decoded alone
    together = codec.decode_images(net, blobs)
    assert all(torch.equal(a, b) for a, b in zip(together, x))
    base_dec = codec.decode_images(net, plain)
    assert all(torch.equal(a, b) for a, b in zip(codec.decode_images(net, blobs, refine=False), base_dec))
    assert torch.equal(codec.decode_images(net, [blobs[1]], reduce=1)[0], codec.decode_images(net, [plain[1]], reduce=1)[0])
    near2 = codec.encode_images(net, x[:2], near=2)
    assert codec.parse_refined(near2[0])[1] == plain[0] and codec.read_header(near2[1])["near"] == 2
    mixed = codec.decode_images(net, [near2[0], blobs[2], plain[3], near2[1]])         # bounds and plain containers mixed
    for got, want, d in zip(mixed, (x[0], x[2], base_dec[3], x[1]), (2, 0, 0, 2)):
        assert int((got.int() - want.int()).abs().max()) <= d
    assert len(near2[0]) < len(blobs[0])


# ------------------------------------------------------------------------------------------------ end to end, tiled
def _tiled(layer):
    key = ("t", layer)
    if key not in _CACHE:
        net = _net(layer)
        x = _images(1, H, W, 42)
        blob = codec.encode_tiled(net, x, tile=TILE, near=0)[0]
        _CACHE[key] = (net, x, blob, codec.encode_tiled(net, x, tile=TILE)[0])
    return _CACHE[key]


@pytest.mark.parametrize("layer", LAYERS)
def test_lossless_tiled(layer, monkeypatch):
    net, x, blob, plain = _tiled(layer)
    hdr, base, units = codec.parse_refined(blob)
    assert base == plain and hdr["units"] == 6 and (hdr["base"]["th"], hdr["base"]["tw"]) == (56, 56)
    for g in (1, 3):
        assert codec.encode_tiled(net, x, tile=TILE, tiles_per_call=g, near=0)[0] == blob, g
    assert torch.equal(codec.decode_tiled(net, blob), x[0])
    assert torch.equal(codec.decode_tiled(net, blob, tiles_per_call=1), x[0])
    assert torch.equal(codec.decode_tiled(net, blob, refine=False), codec.decode_tiled(net, plain))
    assert torch.equal(codec.decode_tiled(net, blob, reduce=1), codec.decode_tiled(net, plain, reduce=1))
    near2 = codec.encode_tiled(net, x, tile=TILE, near=2)[0]
    assert codec.parse_refined(near2)[1] == plain
    assert int((codec.decode_tiled(net, near2).int() - x[0].int()).abs().max()) <= 2
    seen = []
    real = codec._decode_tiles

    def counting(nets, s_xe, s_xo, th_, tw_, n, **kw):
        seen.append(n)
        return real(nets, s_xe, s_xo, th_, tw_, n, **kw)
    monkeypatch.setattr(codec, "_decode_tiles", counting)
    for region, touched in [((50, 40, 20, 30), 4), ((60, 60, 30, 40), 1), ((99, 149, 1, 1), 1), ((55, 0, 2, 150), 6)]:
        y0, x0, h, w = region
        seen.clear()
        got = codec.decode_tiled(net, blob, region=region, tiles_per_call=2)
        assert torch.equal(got, x[0, y0:y0 + h, x0:x0 + w]), region                     # the crop of the original
        assert sum(seen) == touched, (region, seen)
    with pytest.raises(ValueError, match="base container"):
        codec.decode_images(net, [blob])


@pytest.mark.parametrize("layer", LAYERS)
def test_device_coder_round_trips_with_the_host_coder_s_symbols(layer):
    """With the device coder the encoder's xh comes from the dequantised tensors of compress_planes' device-coder path; that
    it equals, bit for bit, what the decoder rebuilds is a property of each layer, so every layer is checked: lossless, a
    region, the host coder's checksums and table choice, and the same symbols out of both coders' streams."""
    net, x, blob, plain = _tiled(layer)
    gblob = codec.encode_tiled(net, x, tile=TILE, near=0, coder="gpu")[0]
    gh, gbase, gunits = codec.parse_refined(gblob)
    hh, hbase, hunits = codec.parse_refined(blob)
    assert gh["base"]["coder"] == "gpu" and gbase == codec.encode_tiled(net, x, tile=TILE, coder="gpu")[0]
    assert torch.equal(codec.decode_tiled(net, gblob), x[0])
    assert torch.equal(codec.decode_tiled(net, gblob, region=(50, 40, 20, 30)), x[0, 50:70, 40:70])
    # the same reconstruction, so the same checksums and table choice; other bytes; and the same symbols from both streams
    for gu, hu in zip(gunits, hunits):
        assert (gu["cs_xh"], gu["cs_x"], gu["scales"]) == (hu["cs_xh"], hu["cs_x"], hu["scales"])
    assert any(gu["streams"] != hu["streams"] for gu, hu in zip(gunits, hunits))
    xh = codec.decode_tiled(net, plain)[None].to(DEV)
    grid, tab = (H, W, 56, 56, 2, 3), residual.tables(0)
    for grp in ([0, 1], [5]):
        sc = torch.from_numpy(np.frombuffer(b"".join(hunits[t]["scales"] for t in grp), dtype=np.uint8).reshape(-1, 24).copy())
        idx, _ = ops.resid_contexts(xh, grid, (0, 0, H, W), grp, sc.to(DEV))
        host = decode_streams([s for t in grp for s in hunits[t]["streams"]], idx.cpu().numpy(), tab.cdf, tab.sizes, tab.offsets)
        dec = irans.Decoder([s for t in grp for s in gunits[t]["streams"]], idx.shape[1], irans.device_tables(tab, xh.device),
                            xh.device)
        dev = dec.pop(idx)
        dec.finish()
        sym = ops.resid_analyse(x.to(DEV), xh, grid, (0, 0, H, W), grp, 0)[0]
        assert torch.equal(dev.cpu(), torch.from_numpy(host)) and torch.equal(dev, sym)


# ------------------------------------------------------------------------------------------------ code length
@pytest.mark.parametrize("coder", ["host", "gpu"])
def test_code_length_and_scale_choice(coder):
    """Every stream is at most its ideal length under the chosen tables plus the coder's allowance: for the host coder the
    1 % slack and 64 bits per stream of tests/test_gpu_coding.py; for the device coder that bound times the 1 % of
    tests/test_gpu_irans.py plus its 4 K + 16 bytes of lane states (K = irans.lanes(n)).  The layer has no escapes.  The
    chosen table of every non-empty context is an argmin of the ideal length recomputed here from the kernel's histogram."""
    net = _net("onlyEZWT")
    x = _images(2, 72, 90, 43)
    blobs = codec.encode_images(net, x, near=0, coder=coder)
    xh = torch.stack(codec.decode_images(net, blobs, refine=False)).to(DEV)
    grid, region, tab = (72, 90, 72, 96, 1, 1), (0, 0, 72, 90), residual.tables(0)
    units = [codec.parse_refined(b)[2][0] for b in blobs]
    sym, ctx, hist, _, _ = ops.resid_analyse(x.to(DEV), xh, grid, region, [0, 1], 0)
    scales = np.stack([np.frombuffer(u["scales"], dtype=np.uint8) for u in units])
    idx, _ = ops.resid_contexts(xh, grid, region, [0, 1], torch.from_numpy(scales.copy()).to(DEV))
    sym, idx, hist = sym.cpu().numpy(), idx.cpu().numpy(), hist.cpu().numpy().reshape(2, 24, -1).astype(np.float64)
    K = irans.lanes(sym.shape[1])
    total = 0.0
    for j in range(2):
        for c in range(3):
            ideal, escapes = ec.ideal_bits(sym[3 * j + c], idx[3 * j + c], tab)
            bits = 8 * len(units[j]["streams"][c])
            bound = ideal * 1.01 + 64
            if coder == "gpu":
                bound = bound * 1.01 + 8 * (4 * K + 16)
            print("[residual %s] unit %d channel %d: %.0f bits ideal, %d written" % (coder, j, c, ideal, bits))
            assert escapes == 0 and ideal <= bits <= bound, (j, c, ideal, bits)
            total += bits
    print("[residual %s] lossless layer: %.3f bpp over the base (seeded, untrained weights)" % (coder, total / (2 * 72 * 90)))
    freq = np.diff(tab.cdf.astype(np.int64), axis=1)[:, :511].astype(np.float64)
    cost = hist @ (-np.log2(freq / 65536.0)).T                                          # (2, 24, 64)
    for j in range(2):
        for k in range(24):
            if hist[j, k].sum() == 0:
                assert scales[j, k] == 0
            else:
                assert cost[j, k, scales[j, k]] <= cost[j, k].min() * (1 + 1e-12), (j, k)


# ------------------------------------------------------------------------------------------------ refusals and guards
def test_refusals_and_reconstruction_guards():
    net, x, blobs, plain = _untiled("onlyEZWT")
    with pytest.raises(ValueError, match="near"):
        codec.encode_tiled(net, x[:1], tile=TILE, overlap=8, near=0)
    for bad in (33, -1, 1.5, "0", True):
        with pytest.raises(ValueError, match="near"):
            codec.encode_images(net, x[:1], near=bad)
        with pytest.raises(ValueError, match="near"):
            codec.encode_tiled(net, x[:1], tile=TILE, near=bad)
    hdr, base, units = codec.parse_refined(blobs[0])
    crc = hdr["table_crc"]

    def with_unit(**over):
        u = dict(units[0])
        u.update(over)
        return codec.pack_refined(0, crc, base, [u])              # resealed: only the named field differs
    assert torch.equal(codec.decode_images(net, [with_unit()])[0], x[0])
    with pytest.raises(ValueError, match="reconstruction check"):
        codec.decode_images(net, [with_unit(cs_xh=units[0]["cs_xh"] ^ 1)])
    with pytest.raises(ValueError, match="reconstruction check"):
        codec.decode_images(net, [with_unit(cs_x=units[0]["cs_x"] ^ 1)])
    body = bytearray(blobs[0][:-4])
    pos = 12 + len(codec.leb128_encode(len(base))) + len(base) + 4 + 16
    assert bytes(body[pos:pos + 24]) == units[0]["scales"]
    body[pos + 5] = 64
    with pytest.raises(ValueError, match="scale index"):
        codec.decode_images(net, [codec._seal(bytes(body))])
    with pytest.raises(ValueError, match="table CRC32"):
        codec.decode_images(net, [codec.pack_refined(0, crc ^ 1, base, units)])
    # a base decoded with other weights never reaches the residual layer: the base's identity check comes first
    with pytest.raises(ValueError, match="entropy layer"):
        codec.decode_images(_net("conditioned2ZTsepSubbands"), [blobs[0]])


# ------------------------------------------------------------------------------------------------ command line
def test_command_line_lossless(tmp_path):
    from PIL import Image
    cfg = {"dwtlevels": 3, "entropy_layer": "onlyEZWT", "seed": 7}
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    x = _images(1, 97, 131, 44)
    Image.fromarray(x[0].numpy()).save(tmp_path / "in.png")
    tool = os.path.join(REPO, "tools", "codec.py")
    run = lambda *a: subprocess.run([sys.executable, tool] + list(a), capture_output=True, text=True, timeout=600)
    c = str(tmp_path / "cfg.json")
    r = run("encode", "--config", c, "--tile", "64", "--lossless", str(tmp_path / "in.png"), str(tmp_path / "o.lld"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "near 0: base" in r.stdout and "tiles: 2 x 3" in r.stdout
    blob = (tmp_path / "o.lld").read_bytes()
    hdr = codec.read_header(blob)
    assert blob[:4] == b"LLDR" and hdr["near"] == 0
    r = run("info", str(tmp_path / "o.lld"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "lossless" in r.stdout and "base_bytes      %d" % hdr["base_bytes"] in r.stdout
    assert "residual_bytes  %d" % hdr["residual_bytes"] in r.stdout and "2 x 3 tiles" in r.stdout
    r = run("decode", "--config", c, str(tmp_path / "o.lld"), str(tmp_path / "out.png"))          # a fresh child process
    assert r.returncode == 0, r.stderr[-3000:]
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out.png").convert("RGB")), x[0].numpy())
