"""GPU: quality-targeted coding.  1. lldwt_ycc_tiles_sq_err against the int64 SSE of the bytes the store
kernel writes; 2. target_psnr on the untiled codec; 3. on tiled and lapped frames; 4. target_msssim; 5. nothing else moved.

The nets are L = 3 wrappers with seeded weights whose subband auto-encoders are the near-identity map of
test_gpu_codec_oracle.through_ae (gain 16), so that the reconstruction follows the image and responds to the step.  Every test
that derives a target from a pair of neighbouring grid steps first asserts, on real encode + decode, what it needs of that
pair; the assertions that follow are in integers (the SSE of decoded bytes against codec.psnr_sse_bound)."""
import numpy as np
import pytest
import torch

from test_gpu_codec_oracle import through_ae

from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import _lib, codec, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYERS = ("conditioned2ZTsepSubbands", "onlyEZWT", "DWTConditioned2EntropyLayerZTBlock")
GAIN = 16.0
GRID = codec.STEP_GRID
K2 = GRID.index(32)                      # the grid index of step 2
_CACHE = {}


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _ycc(n, th, tw, seed, scale=0.45):
    """Random plane-major YCbCr that overshoots [-0.5, 0.5] after the colour transform, so the clamp is exercised."""
    g = torch.Generator().manual_seed(seed)
    y = (torch.rand(3, n, 1, th, tw, generator=g) - 0.5) * 2 * scale
    y[1:] += 0.5                                                     # Cb, Cr are centred on 0.5
    return y.to(DEV)


def _src(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to(DEV)


def _np_sse(a, b):
    """int64 SSE per image of two (B,H,W,3) uint8 tensors."""
    d = a.cpu().numpy().astype(np.int64) - b.cpu().numpy().astype(np.int64)
    return (d * d).reshape(d.shape[0], -1).sum(1)


@pytest.mark.parametrize("B,H,W,Hp,Wp", [(1, 1, 1, 8, 8), (1, 5, 257, 8, 264), (3, 70, 85, 72, 88), (2, 19, 600, 24, 600)])
def test_sq_err_equals_the_store_kernels_bytes_untiled(B, H, W, Hp, Wp):
    y, src = _ycc(B, Hp, Wp, H + W), _src(B, H, W, H * W)
    stored = ops.ycc_to_u8hwc_crop(y, H, W)
    assert torch.equal(stored, ops.ycc_tiles_to_u8hwc(y, (H, W, Hp, Wp, 1, 1), (0, 0, H, W), B=B))
    want = _np_sse(stored, src)
    if H * W >= 64:
        assert int(stored.min()) == 0 and int(stored.max()) == 255       # the clamp is hit at both ends
    got = ops.ycc_tiles_sq_err(y, (H, W, Hp, Wp, 1, 1), src, B=B)
    assert got.dtype == torch.int64 and tuple(got.shape) == (B,) and got.is_cuda
    assert got.cpu().numpy().tolist() == want.tolist()
    assert len(set(want.tolist())) == B                                  # the images have distinct sums
    # reproducible: integer atomics do not depend on the order of arrival
    assert torch.equal(got, ops.ycc_tiles_sq_err(y, (H, W, Hp, Wp, 1, 1), src, B=B))


def test_sq_err_on_a_tile_grid_in_two_calls_and_with_a_tile_list():
    B, H, W, th, tw, ny, nx = 2, 100, 150, 64, 64, 2, 3
    grid, per = (H, W, th, tw, ny, nx), ny * nx
    y, src = _ycc(B * per, th, tw, 7), _src(B, H, W, 8)
    stored = ops.ycc_tiles_to_u8hwc(y, grid, (0, 0, H, W), B=B)
    want = _np_sse(stored, src).tolist()
    sse = torch.zeros(B, dtype=torch.int64, device=DEV)
    assert ops.ycc_tiles_sq_err(y[:, :7].contiguous(), grid, src, first=0, B=B, out=sse) is sse
    assert sse[1].item() > 0 and sse.tolist() != want                   # tile 6 is image 1's first: both are fed, neither whole
    ops.ycc_tiles_sq_err(y[:, 7:].contiguous(), grid, src, first=7, B=B, out=sse)
    assert sse.tolist() == want
    # an explicit shuffled list with two indexes outside the grid, whose slots add nothing
    order = torch.randperm(B * per, generator=torch.Generator().manual_seed(3)).tolist()
    tiles = order[:5] + [-1] + order[5:] + [B * per]
    slots = torch.empty(3, len(tiles), 1, th, tw, device=DEV)
    for j, t in enumerate(tiles):
        slots[:, j] = y[:, t] if 0 <= t < B * per else _ycc(1, th, tw, 100 + j)[:, 0]
    assert ops.ycc_tiles_sq_err(slots, grid, src, tiles=tiles, B=B).tolist() == want


@pytest.mark.parametrize("B,ny,nx,th,tw,H,W", [(5, 5, 5, 520, 8, 2590, 37), (1, 23, 20, 1030, 8, 23673, 157)])
def test_sq_err_with_several_strips_per_workgroup(B, ny, nx, th, tw, H, W):
    """Narrow tall tiles in numbers at which the launcher gives a workgroup 2 and 8 strips of 8 rows (at least 4096 workgroups
    must remain): the last workgroup of a tile ends inside a strip, the last tile row ends inside the image."""
    grid = (H, W, th, tw, ny, nx)
    y, src = _ycc(B * ny * nx, th, tw, th + B), _src(B, H, W, th)
    want = _np_sse(ops.ycc_tiles_to_u8hwc(y, grid, (0, 0, H, W), B=B), src).tolist()
    assert ops.ycc_tiles_sq_err(y, grid, src, B=B).tolist() == want


def test_sq_err_extreme_and_accumulation():
    B, H, W, Hp, Wp = 2, 37, 300, 40, 304
    y = torch.zeros(3, B, 1, Hp, Wp, device=DEV)
    y[0], y[1], y[2] = -0.5, 0.5, 0.5                                    # Y = 0 with neutral chroma: black
    src = torch.full((B, H, W, 3), 255, dtype=torch.uint8, device=DEV)
    assert int(ops.ycc_to_u8hwc_crop(y, H, W).max()) == 0
    assert ops.ycc_tiles_sq_err(y, (H, W, Hp, Wp, 1, 1), src, B=B).tolist() == [3 * H * W * 65025] * B
    out = torch.tensor([5, 1 << 40], dtype=torch.int64, device=DEV)
    ops.ycc_tiles_sq_err(y, (H, W, Hp, Wp, 1, 1), src, B=B, out=out)
    assert out.tolist() == [5 + 3 * H * W * 65025, (1 << 40) + 3 * H * W * 65025]


def test_sq_err_refuses_bad_arguments():
    y, src = _ycc(1, 8, 8, 1), _src(1, 8, 8, 2)
    grid = (8, 8, 8, 8, 1, 1)
    E = _lib.LLDWTError
    with pytest.raises(E):
        ops.ycc_tiles_sq_err(y, (8, 8, 16, 8, 1, 1), src)                # tiles are not the grid's size
    with pytest.raises(E):
        ops.ycc_tiles_sq_err(y, grid, src.float())
    with pytest.raises(E):
        ops.ycc_tiles_sq_err(y, grid, _src(1, 8, 9, 2))                  # src is not the image of the grid
    with pytest.raises(E):
        ops.ycc_tiles_sq_err(y, grid, src, out=torch.zeros(1, dtype=torch.int32, device=DEV))
    with pytest.raises(E):
        ops.ycc_tiles_sq_err(y, grid, src, out=torch.zeros(2, dtype=torch.int64, device=DEV))
    with pytest.raises(E):
        ops.ycc_tiles_sq_err(y, grid, src, tiles=[0, 0])                 # one index per slot
    with pytest.raises(E):
        ops.ycc_tiles_sq_err(y, grid, src, first=1)                      # the range leaves the grid
    with pytest.raises(E):
        ops.ycc_tiles_sq_err(y, (16, 8, 8, 8, 1, 1), _src(1, 16, 8, 2))  # the grid does not cover the image
    # the entry point itself: null pointers, non-positive sizes, th < 1
    import ctypes as C
    lib, out = _lib.load(), torch.zeros(1, dtype=torch.int64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    ok = [p(y), C.c_void_p(0), 0, 1, 1, 8, 8, 8, 8, 1, 1, p(src), p(out), C.c_void_p(0)]
    for pos, bad in ((0, C.c_void_p(0)), (11, C.c_void_p(0)), (12, C.c_void_p(0)), (3, 0), (4, 0), (5, 0), (6, -1), (7, 0), (8, 0),
                     (9, 0), (10, 0), (3, 70000)):
        args = list(ok)
        args[pos] = bad
        assert lib.lldwt_ycc_tiles_sq_err(*args) != 0, pos
    torch.cuda.synchronize()
    assert out.item() == 0


# ------------------------------------------------------------------------------------------------ the nets and images
def _net(layer):
    """The layer's L = 3 wrapper with seeded weights and near-identity subband auto-encoders (through_ae, gain 16)."""
    if layer not in _CACHE:
        from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
            LiftingBasedDWTNetWrapper
        from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
        cfg = make_config(dwtlevels=3, mode="validate", entropy_layer=layer)
        torch.manual_seed(0)
        net = LiftingBasedDWTNetWrapper(cfg)
        net.load_state_dict(through_ae(net.state_dict(), GAIN))
        _CACHE[layer] = net.to(DEV).eval()
    return _CACHE[layer]


def _images(B, H, W, seed):
    """Smooth colour fields plus noise, as uint8 (B,H,W,3) on the host (test_gpu_codec_step._images)."""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(B, 3, max(2, H // 16), max(2, W // 16), generator=g)
    x = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
    x = x * 200 + torch.rand(B, 3, H, W, generator=g) * 40
    return x.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _sse(dec, img):
    """int SSE of one decoded (H,W,3) uint8 image against its original."""
    return int(_np_sse(dec[None], img[None])[0])


def _untiled(net, img, k, **kw):
    """The real container of one image (1,H,W,3) at grid index k and the SSE of its decode."""
    blob = codec.encode_images(net, img, step=GRID[k] / 16, **kw)[0]
    return blob, _sse(codec.decode_images(net, [blob])[0], img[0])


def _between(s_lo, s_hi, H, W):
    """A PSNR target between those of two SSEs s_lo < s_hi, with the precondition that its bound separates them."""
    assert s_hi > s_lo > 0, "precondition: the SSE grows from the finer to the coarser step (%d, %d)" % (s_lo, s_hi)
    P = codec.sse_psnr((s_lo + s_hi) / 2.0, H, W)
    assert s_lo <= codec.psnr_sse_bound(P, H, W) < s_hi, "precondition: the bound separates the two steps"
    return P


def _check_untiled(net, img, blob, P, stats, **kw):
    """The contract of target_psnr on one untiled image, in integers, on real decodes."""
    _, H, W, _ = img.shape
    hdr = codec.read_header(blob)
    n = int(round(hdr["step"] * 16))
    assert n in GRID and hdr["step"] == stats["step"]
    k = GRID.index(n)
    same, sse = _untiled(net, img, k, **kw)
    assert blob == same                                                  # the container of step=<chosen>, byte for byte
    bound = codec.psnr_sse_bound(P, H, W)
    assert sse <= bound and sse == stats["sse"]                          # met, and the probe measured the decoder's bytes
    if k + 1 < len(GRID):
        assert _untiled(net, img, k + 1, **kw)[1] > bound                # the next coarser grid step misses
    assert stats["probes"] <= 7 and stats["encodes"] == 1 and stats["bytes"] == len(blob)
    return k


@pytest.mark.parametrize("H,W", [(64, 64), (72, 88)])
@pytest.mark.parametrize("layer", LAYERS)
def test_target_psnr_untiled(layer, H, W):
    _target_psnr_untiled(layer, H, W, {})


def test_target_psnr_untiled_with_the_device_coder_and_rdo():
    _target_psnr_untiled(LAYERS[0], 64, 64, {"coder": "gpu", "rdo": 0.5})


def _target_psnr_untiled(layer, H, W, kw):
    net, img = _net(layer), _images(1, H, W, H + W)
    s0 = _untiled(net, img, 0, **kw)[1]
    s_lo, s_hi = _untiled(net, img, K2, **kw)[1], _untiled(net, img, K2 + 1, **kw)[1]
    print("%s %dx%d %s: SSE at steps 0.25 / 2 / 2.38 = %d / %d / %d" % (layer, H, W, kw, s0, s_lo, s_hi))
    P = _between(s_lo, s_hi, H, W)
    assert s0 <= codec.psnr_sse_bound(P, H, W), "precondition: the finest step meets the target"
    blobs = codec.encode_images(net, img, target_psnr=P, **kw)
    assert len(blobs) == 1
    stats = dict(codec.SEARCH_STATS)
    print("target %.3f dB -> %s" % (P, {k: v for k, v in stats.items() if k != "images"}))
    _check_untiled(net, img, blobs[0], P, stats, **kw)


def test_target_psnr_searches_a_batch_image_by_image():
    net, img = _net(LAYERS[1]), _images(2, 64, 64, 77)
    pairs = [(_untiled(net, img[b:b + 1], K2)[1], _untiled(net, img[b:b + 1], K2 + 1)[1]) for b in range(2)]
    # one target for both: between the finer steps' largest and the coarser steps' smallest SSE
    P = _between(max(p[0] for p in pairs), min(p[1] for p in pairs), 64, 64)
    blobs = codec.encode_images(net, img, target_psnr=P)
    assert len(blobs) == 2 and len(codec.SEARCH_STATS["images"]) == 2
    assert {k: v for k, v in codec.SEARCH_STATS.items() if k != "images"} == codec.SEARCH_STATS["images"][1]
    for b in range(2):
        _check_untiled(net, img[b:b + 1], blobs[b], P, codec.SEARCH_STATS["images"][b])


def test_target_psnr_out_of_reach_and_below_the_coarsest_step():
    net, img = _net(LAYERS[1]), _images(1, 64, 64, 5)
    with pytest.raises(ValueError, match="target_psnr.*cannot be met.*best is"):
        codec.encode_images(net, img, target_psnr=200.0)
    coarsest, s = _untiled(net, img, len(GRID) - 1)
    assert s > 0
    blob = codec.encode_images(net, img, target_psnr=codec.sse_psnr(s, 64, 64) - 1.0)[0]
    assert blob == coarsest and codec.read_header(blob)["step"] == 64.0
    assert codec.SEARCH_STATS["sse"] == s and codec.SEARCH_STATS["probes"] <= 7 and codec.SEARCH_STATS["encodes"] == 1


# ------------------------------------------------------------------------------------------------ 3. tiled and lapped
def _tiled(net, img, k, ov, **kw):
    blob = codec.encode_tiled(net, img, tile=64, overlap=ov, step=GRID[k] / 16, **kw)[0]
    return blob, _sse(codec.decode_tiled(net, blob), img[0])


@pytest.mark.parametrize("ov", [0, 16])
def test_target_psnr_tiled(ov):
    net, img = _net(LAYERS[1]), _images(1, 128, 192, 9)
    H, W = 128, 192
    s0, s_lo, s_hi = _tiled(net, img, 0, ov)[1], _tiled(net, img, K2, ov)[1], _tiled(net, img, K2 + 1, ov)[1]
    print("overlap %d: SSE at steps 0.25 / 2 / 2.38 = %d / %d / %d" % (ov, s0, s_lo, s_hi))
    P = _between(s_lo, s_hi, H, W)
    bound = codec.psnr_sse_bound(P, H, W)
    assert s0 <= bound, "precondition: the finest step meets the target"
    blob = codec.encode_tiled(net, img, tile=64, overlap=ov, target_psnr=P)[0]
    stats = dict(codec.SEARCH_STATS)
    hdr = codec.read_header(blob)
    assert blob[:4] == (b"LLDO" if ov else b"LLDT") and hdr["ny"] * hdr["nx"] > 1
    n = int(round(hdr["step"] * 16))
    assert n in GRID
    k = GRID.index(n)
    same, sse = _tiled(net, img, k, ov)
    assert blob == same
    assert sse <= bound and sse == stats["sse"]      # lapped: the encoder-side blend is the decoder's, to the byte sum
    if k + 1 < len(GRID):
        assert _tiled(net, img, k + 1, ov)[1] > bound
    assert stats["probes"] <= 7 and stats["encodes"] == 1
    # the result does not depend on tiles_per_call
    assert codec.encode_tiled(net, img, tile=64, overlap=ov, target_psnr=P, tiles_per_call=1)[0] == blob
    assert codec.SEARCH_STATS["sse"] == sse


# ------------------------------------------------------------------------------------------------ 4. MS-SSIM
def test_target_msssim():
    net, img = _net(LAYERS[1]), _images(1, 176, 176, 11)
    ms = {}
    for k in (0, K2, K2 + 1):
        blob = codec.encode_images(net, img, step=GRID[k] / 16)[0]
        ms[k] = codec.quality(img[0], codec.decode_images(net, [blob])[0])["msssim"]
    print("MS-SSIM at steps 0.25 / 2 / 2.38 = %.6f / %.6f / %.6f" % (ms[0], ms[K2], ms[K2 + 1]))
    assert ms[K2] - ms[K2 + 1] > 1e-4, "precondition: the two steps differ by far more than the atomics' last bits"
    M = (ms[K2] + ms[K2 + 1]) / 2
    assert ms[0] > M + 1e-4, "precondition: the finest step meets the target"
    blob = codec.encode_images(net, img, target_msssim=M)[0]
    stats = dict(codec.SEARCH_STATS)
    n = int(round(codec.read_header(blob)["step"] * 16))
    assert n in GRID and "sse" not in stats and stats["probes"] <= 7 and stats["encodes"] == 1
    k = GRID.index(n)
    assert blob == codec.encode_images(net, img, step=n / 16)[0]
    got = codec.quality(img[0], codec.decode_images(net, [blob])[0])["msssim"]
    assert got >= M and abs(got - stats["msssim"]) < 1e-9
    if k + 1 < len(GRID):
        coarser = codec.encode_images(net, img, step=GRID[k + 1] / 16)[0]
        assert codec.quality(img[0], codec.decode_images(net, [coarser])[0])["msssim"] < M
    with pytest.raises(ValueError, match="target_msssim"):
        codec.encode_images(net, _images(1, 64, 64, 1), target_msssim=0.9)
    with pytest.raises(ValueError, match="target_msssim.*cannot be met.*best is"):
        codec.encode_images(net, img, target_msssim=0.9999999)


@pytest.mark.parametrize("ov", [0, 16])
def test_target_msssim_tiled(ov):
    """The MS-SSIM target on a tiled and a lapped frame: the bytes of the tiles' rectangles, or of the blended frame, as
    decode_tiled writes them."""
    net, img = _net(LAYERS[1]), _images(1, 176, 208, 13)
    ms = {}
    for k in (0, K2, K2 + 1):
        blob = codec.encode_tiled(net, img, tile=128, overlap=ov, step=GRID[k] / 16)[0]
        ms[k] = codec.quality(img[0], codec.decode_tiled(net, blob))["msssim"]
    print("overlap %d: MS-SSIM at steps 0.25 / 2 / 2.38 = %.6f / %.6f / %.6f" % (ov, ms[0], ms[K2], ms[K2 + 1]))
    assert ms[K2] - ms[K2 + 1] > 1e-4, "precondition: the two steps differ by far more than the atomics' last bits"
    M = (ms[K2] + ms[K2 + 1]) / 2
    assert ms[0] > M + 1e-4, "precondition: the finest step meets the target"
    blob = codec.encode_tiled(net, img, tile=128, overlap=ov, target_msssim=M)[0]
    stats = dict(codec.SEARCH_STATS)
    hdr = codec.read_header(blob)
    assert blob[:4] == (b"LLDO" if ov else b"LLDT") and hdr["ny"] * hdr["nx"] > 1
    n = int(round(hdr["step"] * 16))
    assert n in GRID and stats["probes"] <= 7 and stats["encodes"] == 1
    k = GRID.index(n)
    assert blob == codec.encode_tiled(net, img, tile=128, overlap=ov, step=n / 16)[0]
    got = codec.quality(img[0], codec.decode_tiled(net, blob))["msssim"]
    assert got >= M and abs(got - stats["msssim"]) < 1e-9
    if k + 1 < len(GRID):
        coarser = codec.encode_tiled(net, img, tile=128, overlap=ov, step=GRID[k + 1] / 16)[0]
        assert codec.quality(img[0], codec.decode_tiled(net, coarser))["msssim"] < M


# ------------------------------------------------------------------------------------------------ 5. nothing else moved
def test_a_targeted_call_leaves_the_other_calls_as_they_were():
    net, img = _net(LAYERS[2]), _images(1, 64, 64, 21)
    before = (codec.encode_images(net, img), codec.encode_images(net, img, step=2.0))
    s_lo, s_hi = _untiled(net, img, K2)[1], _untiled(net, img, K2 + 1)[1]
    blob = codec.encode_images(net, img, target_psnr=_between(s_lo, s_hi, 64, 64))[0]
    assert (codec.encode_images(net, img), codec.encode_images(net, img, step=2.0)) == before
    assert "target" not in codec.read_header(blob)["arithmetic"]        # nothing is recorded
    dec = codec.decode_images(net, [blob])[0]                            # no argument tells the decoder of the target
    assert tuple(dec.shape) == (64, 64, 3) and dec.dtype == torch.uint8
    for bad in (dict(step=2.0), dict(target_bytes=4000), dict(near=0), dict(target_msssim=0.9)):
        with pytest.raises(ValueError, match="target_psnr"):
            codec.encode_images(net, img, target_psnr=30.0, **bad)
