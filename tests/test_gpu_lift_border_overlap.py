"""Border tiles of the fused lifting step (k_lift_fused_f16, eval path), second part: the correction sums of a border tile run
in the barrier interval of the composite loop (each wave turns to them after its own composite tiles, the passes dealt by a
counter) instead of behind the barrier that follows it, and a tile at the top / bottom of the image computes no conv1 / conv2
MFMA tile whose 16 pixels all lie above / below the image (their pixels are zero-filled).  Neither changes a bit of the output:
diagnostics flag 128 (ops.set_diagnostics kind 0) keeps the earlier order and the full first and last tiles, and the default
form must be torch.equal to it and to flags 64 | 128 (the earlier strip correction too), in all three precision modes.  The
f16x3 outputs are also held against float64 with the bars of tests/lift_ref.py (those of tests/test_gpu_lift_domain.py).

Step arrays (h x w as the kernel sees them; tiles are 16 x 32; P = 3 planes with distinct weights, B = 2):
  the row-pass (H/2 x W) and column-pass (H/2 x W/2) arrays of the shapes of tests/test_gpu_lift_border.py -- every tile a border
      tile, runs of one tile: a top tile skips 16 conv1 / 10 conv2 tiles, a bottom tile what lies under the image
  16 x 96 and 13 x 70: one tile row, so every tile is top and bottom at once (13 rows: the image ends inside the tile)
  64 x 64 with B = 16: 48 x 2 x 4 = 384 tiles exceed the CU count, the dispatch's cost rule takes runs of two (asserted from
      the rule and the device's CU count): a top first tile, continuing tiles, a continuing bottom tile, the hand-down between
      them, and first tiles that are not at the top"""
import pytest
import torch

import lift_ref as R
from helpers import filled, maxdiff
from oracle import model, weights

pytestmark = pytest.mark.gpu

SHAPES = [(32, 64), (64, 96), (96, 160), (80, 144)]           # those of tests/test_gpu_lift_border.py
P, B, C = 3, 2, 16
ORDER, LEGACY = 128, 64
PRECISIONS = ("f16x3", "fp16", "bf16")
STEP_OF = {1: (1, "U_blocks.0.", (0, 1)), 0: (2, "P_blocks.1.", (1, 0))}          # by `vertical`: tap index, block, pack index


def _ops():
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    import gpu_util
    return ops, gpu_util


_cache = {}


def _weights():
    if "w" not in _cache:
        _, gu = _ops()
        cfg = dict(model.DEFAULT_CFG, filtersize=5, dwtlevels=1)
        sds = [filled(weights.autoencoder_template(cfg), "ovl%d." % p) for p in range(P)]
        taps, packed = gu.lifting_params(sds)
        _cache["w"] = (cfg, sds, taps, packed)
    return _cache["w"]


def _three_forms(fn, precisions=PRECISIONS):
    """{precision: [fn() with no flag, with flag 128, with flags 64 | 128]}"""
    ops, _ = _ops()
    before = ops.get_precision()
    outs = {}
    try:
        for prec in precisions:
            ops.set_precision(prec)
            outs[prec] = []
            for flags in (0, ORDER, ORDER | LEGACY):
                ops.set_diagnostics(0, None, flags)
                outs[prec].append(fn())
                torch.cuda.synchronize()
    finally:
        ops.set_diagnostics(0, None, 0)
        ops.set_precision(before)
    return outs


def _flat(o):
    if torch.is_tensor(o):
        return [o]
    return [t for e in o for t in _flat(e)]


def _assert_bits(tag, outs):
    for prec, (new, old, older) in outs.items():
        for i, (a, b, c) in enumerate(zip(_flat(new), _flat(old), _flat(older))):
            assert torch.equal(a, b), (tag, prec, "flag 128", i, maxdiff(a, b))
            assert torch.equal(a, c), (tag, prec, "flags 64 | 128", i, maxdiff(a, c))


def _step(h, w, vertical, sign, batch=B):
    """The step on (P, batch, 1, h, w) in the three forms and precisions: bits, then the f16x3 default form against float64."""
    ops, gu = _ops()
    _, sds, taps, packed = _weights()
    j, prefix, (blk, u) = STEP_OF[vertical]
    g = torch.Generator().manual_seed(5000 + 131 * h + w + 7 * vertical)
    src = torch.rand(P, batch, 1, h, w, generator=g) - 0.5
    dst = torch.rand(P, batch, 1, h, w, generator=g) - 0.5
    src_d, dst_d = gu.dev(src), gu.dev(dst)
    Z = P * batch
    v = lambda t: ops.view_of(t, Z, h, w)
    tp, pk = taps[j].contiguous(), packed[:, blk, u].contiguous()

    def run():
        out_d = torch.empty_like(dst_d)
        ops.lift_step(v(src_d), v(dst_d), v(out_d), Z, batch, h, w, tp, pk, C, 5, vertical, sign, 0.1)
        return out_d.cpu()
    outs = _three_forms(run)
    tag = "step %dx%d v=%d s=%+.0f" % (h, w, vertical, sign)
    _assert_bits(tag, outs)

    def fn(p, dtype, tanh):
        sd = R.cast_sd(sds[p], dtype)
        f = R.step(src[p].to(dtype), dst[p].to(dtype), R.tap_of(sd, j), R.block_of(sd, prefix), sign, bool(vertical), False, tanh=tanh)
        return {"out": f["out"]}
    ref, f32s = R.evaluate(fn, P)
    got = outs["f16x3"][0]
    bad = R.check(tag, "out", [got[p] for p in range(P)], ref, f32s)
    assert not bad, bad


@pytest.mark.parametrize("sign", [1.0, -1.0])          # forward / inverse direction of a step
@pytest.mark.parametrize("vertical", [1, 0])           # row step on H/2 x W, column step on H/2 x W/2
@pytest.mark.parametrize("hw", SHAPES)
def test_step_bits_and_float64(hw, vertical, sign):
    h, w = (hw[0] // 2, hw[1]) if vertical else (hw[0] // 2, hw[1] // 2)
    _step(h, w, vertical, sign)


@pytest.mark.parametrize("vertical,sign", [(1, 1.0), (0, -1.0)])
@pytest.mark.parametrize("hw", [(16, 96), (13, 70)])
def test_tile_at_top_and_bottom_at_once(hw, vertical, sign):
    _step(hw[0], hw[1], vertical, sign)


def _dispatch_run_length(Z, h, w, ncu):
    """The cost rule of lift_f16_launch (composed path): the longest run that still fills whole rounds."""
    cdiv = lambda a, b: -(-a // b)
    tiles_x, tiles_y = cdiv(w, 32), cdiv(h, 16)
    best, best_rl = 1e30, 1
    for rl in range(1, tiles_y + 1):
        cost = cdiv(Z * tiles_x * cdiv(tiles_y, rl), ncu) * (1.0 + 0.8 * (rl - 1))
        if cost < best - 1e-9:
            best, best_rl = cost, rl
    return best_rl


@pytest.mark.parametrize("vertical,sign", [(1, 1.0), (0, -1.0)])
def test_runs_of_two_tiles(vertical, sign):
    batch, h, w = 16, 64, 64
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    rl = _dispatch_run_length(P * batch, h, w, ncu)
    assert 2 <= rl < 4, "on %d CUs the launch takes runs of %d tiles: this case needs runs of 2 or 3 in a column of 4" % (ncu, rl)
    _step(h, w, vertical, sign, batch=batch)


@pytest.mark.parametrize("hw", SHAPES)
def test_level_forward_inverse_bits(hw):
    """One level forward (row pass, then the paired L/H column pass) and its inverse from the forward's own outputs."""
    ops, gu = _ops()
    _, _, taps, packed = _weights()
    g = torch.Generator().manual_seed(77 + hw[0])
    x_d = gu.dev(torch.rand(P, B, 1, *hw, generator=g) - 0.5)

    def run():
        ll, yh = ops.lifting_forward(x_d, taps, packed, 1, C, 5, 0.1)
        xr = ops.lifting_inverse(ll, yh, taps, packed, C, 5, 0.1)
        return [t.cpu() for t in _flat([ll, yh, xr])]
    _assert_bits("level %s" % (hw,), _three_forms(run))
