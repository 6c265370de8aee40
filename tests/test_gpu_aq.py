"""GPU: adaptive quantisation -- the two kernels of csrc/aq.hip against the integer restatement of
tests/aq_ref.py (torch.equal; odd sizes, images smaller than a block, one-pixel last blocks, every lane layout from one cell per
block to a block per wave, a batch, the extreme images, 16 384 blocks) and the entry points' refusals; then the codec's aq=
argument: with a step it writes the bytes of the step_map= form, and under a byte or quality target the search moves the base
step of the map and the container is again that of the step_map= form.  Every comparison is exact equality.
(Helpers of test_gpu_codec_map.py are copied, not imported.)"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import aq_ref

from helpers import filled
from oracle import weights

from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import _lib, codec, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYERS = ("conditioned2ZTsepSubbands", "onlyEZWT", "DWTConditioned2EntropyLayerZTBlock")
GRID = codec.STEP_GRID
EINVAL = -1                                    # LLDWT_EINVAL
AE_GAIN = 100.0
L = 3
_CACHE = {}
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ images
def _images(B, H, W, seed):
    """test_gpu_codec_map._images: smooth colour fields plus noise, uint8 (B,H,W,3) on the host."""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(B, 3, max(2, H // 16), max(2, W // 16), generator=g)
    x = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
    x = x * 200 + torch.rand(B, 3, H, W, generator=g) * 40
    return x.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _quadrants(B, H, W, seed):
    """(B,H,W,3) uint8: constant 128 top left, a 0 / 255 checkerboard top right (the largest S a block can have), seeded uniform
    noise bottom left, the smooth pattern of _images bottom right."""
    g = torch.Generator().manual_seed(1000 + seed)
    x = _images(B, H, W, seed)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    h2, w2 = H // 2, W // 2
    x[:, :h2, :w2] = 128
    x[:, :h2, w2:] = (((yy + xx) & 1) * 255).to(torch.uint8)[None, :h2, w2:, None]
    x[:, h2:, :w2] = torch.randint(0, 256, (B, H - h2, w2, 3), generator=g, dtype=torch.uint8)
    return x.contiguous()


def _check_kernels(img, Lv, ms=(1, 16, 32), nqs=(4, 16, 40, 1024)):
    """Both kernels on a (B,H,W,3) uint8 host batch against the reference, whose activity is computed once -> the device (a, A)."""
    ref = [aq_ref.activity(im.numpy(), Lv) for im in img]
    a, A = ops.aq_activity(img.to(DEV), Lv)
    assert a.dtype == torch.int32 and A.dtype == torch.int64 and tuple(A.shape) == (img.shape[0],)
    assert torch.equal(a.cpu(), torch.from_numpy(np.stack([r[0] for r in ref])).int())
    assert A.cpu().tolist() == [r[1] for r in ref]
    for m in ms:
        for n_q in nqs:
            n = ops.aq_steps(a, A, m / 16, n_q)
            want = np.stack([aq_ref.steps(ra, rA, m, n_q) for ra, rA in ref])
            assert n.dtype == torch.int32 and torch.equal(n.cpu(), torch.from_numpy(want).int()), (m, n_q)
    return a, A


# ------------------------------------------------------------------------------------------------ 1. the kernels
# (65, 130, 5): a block is the 64 lanes of a wave; (70, 140, 6) and (130, 70, 7): a wave walks its block's cells 64 at a time
SHAPES = [(33, 17, 2), (70, 85, 3), (72, 88, 3), (64, 64, 4), (3, 5, 3), (129, 257, 4), (65, 130, 5), (70, 140, 6), (130, 70, 7)]


@pytest.mark.parametrize("H,W,Lv", SHAPES)
def test_kernels_equal_the_integer_reference(H, W, Lv):
    img = _quadrants(1, H, W, H + W + Lv)
    _check_kernels(img, Lv)
    if (H, W, Lv) == (72, 88, 3):
        n = ops.aq_steps(*ops.aq_activity(img.to(DEV), Lv), 1.0, 16)
        assert len(torch.unique(n)) >= 4                                            # the map is a map


def test_kernels_on_a_batch_of_different_images():
    """The sums are per image: three different images, at a width that takes the word reads and one that takes the byte reads."""
    for H, W in ((40, 48), (37, 53)):
        img = torch.cat([_quadrants(1, H, W, 5), _images(1, H, W, 6), torch.full((1, H, W, 3), 128, dtype=torch.uint8)])
        a, A = _check_kernels(img, 3, ms=(16,), nqs=(16, 40))
        assert len(set(A.cpu().tolist())) == 3
        one, A1 = ops.aq_activity(img[1:2].to(DEV), 3)                               # an image alone is the image in the batch
        assert torch.equal(one[0], a[1]) and A1.item() == A[1].item()
        assert (ops.aq_steps(a, A, 1.0, 40)[2] == 40).all()                          # a constant image: the base step


def test_kernels_on_the_extreme_images():
    for value in (0, 255):
        img = torch.full((1, 33, 49, 3), value, dtype=torch.uint8)
        a, A = _check_kernels(img, 2, ms=(32,), nqs=(4, 1024))
        assert (a == 8 * 10).all() and A.item() == 80 * a.numel()                    # S = 0: x = 2^10
    # a checkerboard everywhere: the largest x, still a constant map
    yy, xx = torch.meshgrid(torch.arange(64), torch.arange(64), indexing="ij")
    img = (((yy + xx) & 1) * 255).to(torch.uint8)[None, :, :, None].expand(1, 64, 64, 3).contiguous()
    a, A = _check_kernels(img, 4, ms=(32,), nqs=(16,))
    assert (a == aq_ref.lg(16 * 256 * 255 * 255 // 4 + (1 << 14))).all()


def test_kernels_on_16384_blocks():
    img = _quadrants(1, 512, 512, 3)
    a, A = _check_kernels(img, 2, ms=(16,), nqs=(16,))
    assert tuple(a.shape) == (1, 128, 128)


def test_entry_points_refuse_bad_arguments():
    lib = _lib.load()
    img = torch.zeros(1, 16, 16, 3, dtype=torch.uint8, device=DEV)
    a = torch.full((1, 4, 4), -7, dtype=torch.int32, device=DEV)
    A = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    n = torch.full((1, 4, 4), -7, dtype=torch.int32, device=DEV)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    null = C.c_void_p(0)
    ok = [p(img), p(a), p(A), 1, 16, 16, 2, null]
    for pos, bad in ((0, null), (1, null), (2, null), (1, p(a, 2)), (2, p(A, 4)), (3, 0), (3, 70000), (4, 0), (5, 0), (4, -1),
                     (6, 1), (6, 9), (6, 0)):
        args = list(ok)
        args[pos] = bad
        assert lib.lldwt_aq_activity(*args) == EINVAL, (pos, bad)
    ok = [p(a), p(A), p(n), 1, 16, 16, 16, null]
    for pos, bad in ((0, null), (1, null), (2, null), (0, p(a, 1)), (1, p(A, 4)), (2, p(n, 2)), (3, 0), (4, 0), (5, 0), (5, 33),
                     (6, 3), (6, 1025)):
        args = list(ok)
        args[pos] = bad
        assert lib.lldwt_aq_steps(*args) == EINVAL, (pos, bad)
    torch.cuda.synchronize()
    assert (a == -7).all() and (A == -7).all() and (n == -7).all()                   # a refused call writes nothing
    E = _lib.LLDWTError
    with pytest.raises(E):
        ops.aq_activity(img.cpu(), 2)
    with pytest.raises(E):
        ops.aq_activity(img, 1)
    with pytest.raises(E):
        ops.aq_steps(a, A, 1.0, 16)                                                  # one sum per image
    with pytest.raises(E):
        ops.aq_steps(a, A[:1].contiguous(), 0.03, 16)
    with pytest.raises(E):
        ops.aq_steps(a, A[:1].contiguous(), 1.0, 2000)


# ------------------------------------------------------------------------------------------------ 2. the codec
def _layer_net(layer, Lv):
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
        LiftingBasedDWTNetWrapper
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
    cfg = make_config(dwtlevels=Lv, mode="validate", entropy_layer=layer)
    net = LiftingBasedDWTNetWrapper(cfg)
    net.load_state_dict(filled(weights.wrapper_template(dict(cfg))), strict=False)
    return net.to(DEV).eval()


def _net(layer):
    """test_gpu_codec_map._net: the layer's net with the filled weights, L = 3, the subband auto-encoders of the levels a step
    reaches scaled by AE_GAIN so that their symbols are not all zero."""
    if ("net", layer) not in _CACHE:
        net = _layer_net(layer, L)
        with torch.no_grad():
            for n in net.nets():
                for lev in range(2):
                    last = n.autoencoder.Yh_ae[lev].ae_down[6]
                    last.weight.mul_(AE_GAIN)
                    last.bias.mul_(AE_GAIN)
        _CACHE[("net", layer)] = net
    return _CACHE[("net", layer)]


def _sse(dec, img):
    return int(((dec.to(torch.int64) - img.to(torch.int64)) ** 2).sum())


@pytest.mark.parametrize("H,W", [(64, 64), (72, 88)])
@pytest.mark.parametrize("layer", LAYERS)
def test_aq_with_a_step_writes_the_bytes_of_its_step_map(layer, H, W):
    net = _net(layer)
    img = _quadrants(2, H, W, H + W)
    for aq, q in ((1.0, 2.5), (0.5, None)):
        steps = codec.activity_step_map(img, L, aq, 1.0 if q is None else q)
        assert steps.dtype == np.float64 and steps.shape == (2, -(-H >> L), -(-W >> L))
        n_q = 16 if q is None else int(q * 16)
        want = np.stack([aq_ref.step_map(im.numpy(), L, int(aq * 16), n_q) for im in img])
        assert np.array_equal(steps * 16, want)                                      # the public view is the rule's map
        for coder in ("host", "gpu"):
            got = codec.encode_images(net, img, coder=coder, aq=aq, step=q)
            assert got == codec.encode_images(net, img, coder=coder, step_map=steps)
            assert all(b[:4] == b"LLDQ" for b in got)
        dec = codec.decode_images(net, got)
        assert all(torch.equal(x, y) for x, y in zip(dec, codec.decode_images(net, codec.encode_images(net, img, coder="gpu",
                                                                                                      step_map=steps))))
    assert len(np.unique(steps[0])) >= 4
    # rdo composes, and the lossless layer over it returns the input bit for bit
    assert codec.encode_images(net, img, aq=1.0, step=2.5, rdo=13 / 64) == \
        codec.encode_images(net, img, step_map=codec.activity_step_map(img, L, 1.0, 2.5), rdo=13 / 64)
    ll = codec.encode_images(net, img, near=0, aq=1.0)
    assert codec.read_header(ll[0])["inner"]["near"] == 0
    assert torch.equal(torch.stack(codec.decode_images(net, ll)), img)


def test_a_batch_whose_images_get_different_maps():
    net = _net(LAYERS[1])
    img = torch.cat([_quadrants(1, 64, 64, 1), _images(1, 64, 64, 2), torch.full((1, 64, 64, 3), 77, dtype=torch.uint8)])
    blobs = codec.encode_images(net, img, aq=1.0, step=2.0)
    maps = [codec.parse_mapped(b)[1] for b in blobs]
    assert not np.array_equal(maps[0], maps[1]) and (maps[2] == 32).all()
    for b in range(3):                                                               # an image's map is its own: alone or in a batch
        assert np.array_equal(maps[b], aq_ref.step_map(img[b].numpy(), L, 16, 32))
        assert codec.encode_images(net, img[b:b + 1], aq=1.0, step=2.0)[0] == blobs[b]


@pytest.mark.parametrize("layer", LAYERS)
def test_aq_over_tiles(layer):
    net = _net(layer)
    img = _quadrants(1, 128, 128, 9)
    steps = codec.activity_step_map(img, L, 1.0, 2.0)
    assert steps.shape == (1, 16, 16)
    for ov in (0, 16):
        blob = codec.encode_tiled(net, img, tile=64, overlap=ov, aq=1.0, step=2.0)[0]
        assert blob == codec.encode_tiled(net, img, tile=64, overlap=ov, step_map=steps)[0]
        hdr = codec.read_header(blob)
        assert blob[:4] == b"LLDQ" and hdr["inner"]["ny"] * hdr["inner"]["nx"] > 1 and hdr["inner"]["overlap"] == ov
        assert tuple(codec.decode_tiled(net, blob).shape) == (128, 128, 3)


@pytest.mark.parametrize("H,W", [(64, 64), (72, 88)])
@pytest.mark.parametrize("layer", LAYERS[1:])
def test_target_bytes_with_aq(layer, H, W):
    net = _net(layer)
    img = _quadrants(1, H, W, H + W + 1)
    form = lambda k: codec.encode_images(net, img, step_map=codec.activity_step_map(img, L, 1.0, GRID[k] / 16))[0]
    T = len(form(14)) + 3
    blob = codec.encode_images(net, img, aq=1.0, target_bytes=T)[0]
    stats = dict(codec.SEARCH_STATS)
    print("%s %dx%d: target %d -> %s" % (layer, H, W, T, stats))
    n = int(round(stats["step"] * 16))
    assert n in GRID and stats["bytes"] == len(blob) <= T
    k = GRID.index(n)
    assert blob == form(k)
    assert k == 0 or len(form(k - 1)) > T
    assert codec.read_header(blob)["inner"]["step"] == 1.0                           # the map holds every step
    with pytest.raises(ValueError, match="target_bytes.*cannot be met"):
        codec.encode_images(net, img, aq=1.0, target_bytes=40)


def test_target_bytes_with_aq_over_tiles():
    net = _net(LAYERS[2])
    img = _quadrants(1, 128, 128, 4)
    form = lambda k: codec.encode_tiled(net, img, tile=64, step_map=codec.activity_step_map(img, L, 0.5, GRID[k] / 16))[0]
    T = len(form(10)) + 3
    blob = codec.encode_tiled(net, img, tile=64, aq=0.5, target_bytes=T)[0]
    k = GRID.index(int(round(codec.SEARCH_STATS["step"] * 16)))
    assert blob == form(k) and len(blob) <= T and (k == 0 or len(form(k - 1)) > T)


@pytest.mark.parametrize("H,W", [(64, 64), (72, 88)])
@pytest.mark.parametrize("layer", LAYERS)
def test_target_psnr_with_aq(layer, H, W):
    net = _net(layer)
    img = _quadrants(1, H, W, H + W + 2)

    def form(k):
        blob = codec.encode_images(net, img, step_map=codec.activity_step_map(img, L, 1.0, GRID[k] / 16))[0]
        return blob, _sse(codec.decode_images(net, [blob])[0], img[0])
    s0, s_mid = form(0)[1], form(12)[1]
    P = codec.sse_psnr(s_mid * 1.02 + 1, H, W)
    bound = codec.psnr_sse_bound(P, H, W)
    print("%s %dx%d: SSE at the bases 0.25 / 2 = %d / %d, target %.3f dB (bound %d)" % (layer, H, W, s0, s_mid, P, bound))
    assert s0 <= bound, "precondition: the finest base meets the target"
    blob = codec.encode_images(net, img, aq=1.0, target_psnr=P)[0]
    stats = dict(codec.SEARCH_STATS)
    n = int(round(stats["step"] * 16))
    assert n in GRID and stats["probes"] <= 7 and stats["encodes"] == 1 and stats["bytes"] == len(blob)
    k = GRID.index(n)
    same, sse = form(k)
    assert blob == same
    assert sse <= bound and sse == stats["sse"]                                      # the probe measured the decoder's bytes
    if k + 1 < len(GRID):
        assert form(k + 1)[1] > bound


def test_target_psnr_with_aq_where_the_quality_follows_the_step():
    """The filled nets above reconstruct far from the image, so their SSE hardly moves with the base and the search ends at the
    coarsest.  On the near-identity net of test_gpu_codec_quality (through_ae, gain 16) the SSE follows the base step: a target
    between two neighbouring bases must choose the finer one."""
    from test_gpu_codec_oracle import through_ae
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
        LiftingBasedDWTNetWrapper
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
    torch.manual_seed(0)
    net = LiftingBasedDWTNetWrapper(make_config(dwtlevels=L, mode="validate", entropy_layer=LAYERS[1]))
    net.load_state_dict(through_ae(net.state_dict(), 16.0))
    net = net.to(DEV).eval()
    img = _quadrants(1, 64, 64, 31)
    K2 = GRID.index(32)

    def form(k):
        blob = codec.encode_images(net, img, step_map=codec.activity_step_map(img, L, 1.0, GRID[k] / 16))[0]
        return blob, _sse(codec.decode_images(net, [blob])[0], img[0])
    s0, s_lo, s_hi = form(0)[1], form(K2)[1], form(K2 + 1)[1]
    print("SSE at the bases 0.25 / 2 / 2.38 = %d / %d / %d" % (s0, s_lo, s_hi))
    assert s_hi > s_lo > 0, "precondition: the SSE grows from the finer to the coarser base"
    P = codec.sse_psnr((s_lo + s_hi) / 2.0, 64, 64)
    bound = codec.psnr_sse_bound(P, 64, 64)
    assert s_lo <= bound < s_hi and s0 <= bound, "precondition: the bound separates the two bases, the finest meets it"
    blob = codec.encode_images(net, img, aq=1.0, target_psnr=P)[0]
    stats = dict(codec.SEARCH_STATS)
    k = GRID.index(int(round(stats["step"] * 16)))
    same, sse = form(k)
    assert blob == same and sse <= bound and sse == stats["sse"] and stats["probes"] <= 7 and stats["encodes"] == 1
    assert k + 1 < len(GRID) and form(k + 1)[1] > bound
    print("target %.3f dB -> base %g, %d probes" % (P, stats["step"], stats["probes"]))


def test_target_psnr_with_aq_over_lapped_tiles():
    net = _net(LAYERS[1])
    img = _quadrants(1, 128, 128, 6)

    def form(k):
        blob = codec.encode_tiled(net, img, tile=64, overlap=16, step_map=codec.activity_step_map(img, L, 1.0, GRID[k] / 16))[0]
        return blob, _sse(codec.decode_tiled(net, blob), img[0])
    s0, s_mid = form(0)[1], form(12)[1]
    P = codec.sse_psnr(s_mid * 1.02 + 1, 128, 128)
    bound = codec.psnr_sse_bound(P, 128, 128)
    assert s0 <= bound, "precondition: the finest base meets the target"
    blob = codec.encode_tiled(net, img, tile=64, overlap=16, aq=1.0, target_psnr=P)[0]
    stats = dict(codec.SEARCH_STATS)
    k = GRID.index(int(round(stats["step"] * 16)))
    same, sse = form(k)
    assert blob == same and sse <= bound and sse == stats["sse"] and stats["probes"] <= 7 and stats["encodes"] == 1
    if k + 1 < len(GRID):
        assert form(k + 1)[1] > bound


def test_target_msssim_with_aq():
    side = -(-ops.ms_ssim_min_side(5) // 8) * 8
    net = _net(LAYERS[1])
    img = _quadrants(1, side, side, 11)

    def form(k):
        blob = codec.encode_images(net, img, step_map=codec.activity_step_map(img, L, 1.0, GRID[k] / 16))[0]
        return blob, codec.quality(img[0], codec.decode_images(net, [blob])[0])["msssim"]
    m0, m_mid = form(0)[1], form(12)[1]
    M = m_mid - 1e-6
    print("%d x %d: MS-SSIM at the bases 0.25 / 2 = %.6f / %.6f" % (side, side, m0, m_mid))
    assert 0 < M < 1 and m0 > M + 1e-6, "precondition: the finest base meets the target by more than the atomics' last bits"
    blob = codec.encode_images(net, img, aq=1.0, target_msssim=M)[0]
    stats = dict(codec.SEARCH_STATS)
    n = int(round(stats["step"] * 16))
    assert n in GRID and "sse" not in stats and stats["probes"] <= 7 and stats["encodes"] == 1
    same, got = form(GRID.index(n))
    assert blob == same and got >= M and abs(got - stats["msssim"]) < 1e-9


def test_calls_without_aq_write_the_bytes_they_wrote_before():
    net = _net(LAYERS[2])
    img = _quadrants(1, 64, 64, 21)
    T = len(codec.encode_images(net, img, step=4.0)[0]) + 3
    calls = lambda: (codec.encode_images(net, img), codec.encode_images(net, img, step=2.0),
                     codec.encode_images(net, img, step_map=np.full((8, 8), 2.0)), codec.encode_images(net, img, target_bytes=T),
                     codec.encode_images(net, img, aq=None), codec.encode_images(net, img, aq=0, step=2.0))
    before = calls()
    assert before[4] == before[0] and before[5] == before[1]                         # None and 0 are off
    blob = codec.encode_images(net, img, aq=1.0, target_bytes=T + 64)[0]
    assert blob[:4] == b"LLDQ" and "aq" not in codec.read_header(blob)["inner"]["arithmetic"]      # nothing new is recorded
    assert calls() == before
    for kw in (dict(step_map=np.full((8, 8), 2.0)), dict(layers=1, step=3.0)):
        with pytest.raises(ValueError, match="aq and"):
            codec.encode_images(net, img, aq=1.0, **kw)
    for kw in (dict(step=2.0), dict(target_bytes=T)):                             # the refusals of a user's map stay
        with pytest.raises(ValueError, match="step_map and"):
            codec.encode_images(net, img, step_map=np.full((8, 8), 2.0), **kw)


def test_command_line_aq(tmp_path):
    """tools/codec.py in fresh child processes: encode --aq over tiles with --lossless, whose map is the rule's and whose decode
    is the input; --aq with a byte target; --aq with --roi is refused."""
    from PIL import Image
    cfg = {"dwtlevels": 3, "entropy_layer": "onlyEZWT", "seed": 7}
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    x = _quadrants(1, 97, 131, 44)
    Image.fromarray(x[0].numpy()).save(tmp_path / "in.png")
    tool = os.path.join(REPO, "tools", "codec.py")
    run = lambda *a: subprocess.run([sys.executable, tool] + list(a), capture_output=True, text=True, timeout=600)
    c, src, dst = str(tmp_path / "cfg.json"), str(tmp_path / "in.png"), str(tmp_path / "o.lld")
    r = run("encode", "--config", c, "--tile", "64", "--lossless", "--aq", "1", "--step", "2", src, dst)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "step map: 13 x 17 blocks" in r.stdout and "near 0: base" in r.stdout
    m = codec.parse_mapped((tmp_path / "o.lld").read_bytes())[1]
    assert np.array_equal(m, aq_ref.step_map(x[0].numpy(), 3, 16, 32))
    r = run("decode", "--config", c, dst, str(tmp_path / "out.png"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out.png").convert("RGB")), x[0].numpy())
    r = run("encode", "--config", c, "--aq", "0.5", "--target-bpp", "8", src, dst)
    assert r.returncode == 0 and "aq 0.5: base step" in r.stdout, r.stderr[-3000:]
    assert (tmp_path / "o.lld").read_bytes()[:4] == b"LLDQ" and len((tmp_path / "o.lld").read_bytes()) <= 97 * 131
    r = run("encode", "--config", c, "--aq", "1", "--roi", "10,20,40,50:0.5", src, dst)
    assert r.returncode == 2 and "--aq" in r.stderr
