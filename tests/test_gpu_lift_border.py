"""Border tiles of the fused lifting step (k_lift_fused_f16, eval path): the strip correction of the composed 9x9 kernel issues
only the k-steps of the strip convolutions whose taps can read non-zero T2 values, and sums the out-of-image conv4 terms of a
pixel on a quarter of a wave.  Neither changes a bit of the output: diagnostics flag 64 (ops.set_diagnostics kind 0) keeps the
earlier form -- every k-step, half a wave per pixel -- and both forms must be torch.equal, in all three precision modes.  The same
outputs are held against the oracle.

Shapes are per plane, one lifting level, P = 3 planes, B = 2 (tiles are 16 x 32; the row pass works on H/2 x W, the paired L/H
column pass on H/2 x W/2):
  32 x 64    one tile row in the row pass: every tile is top and bottom edge at once
  64 x 96    every tile is a border tile, corners and edges distinct
  96 x 160   exactly one tile row of the row pass holds interior tiles
  80 x 144   neither dimension is a multiple of the tile
At every one of these shapes Z * tiles stays below the CU count, so the launch takes runs of ONE tile: nothing here exercises the
hand-down of T1 / T2 rows between the tiles of a run (tests/test_gpu_lift_domain.py does).

Tolerances: a single step against the oracle step uses the 2e-5 of test_gpu_lifting.test_lift_step_vs_oracle; a whole level
(four chained steps per pass, paired column launches) uses that file's TOL = 1e-4 for subband coefficients."""
import pytest
import torch

from helpers import filled, maxdiff
from oracle import lifting, model, weights

pytestmark = pytest.mark.gpu

SHAPES = [(32, 64), (64, 96), (96, 160), (80, 144)]
P, B = 3, 2
LEGACY = 64
STEP_TOL = 2e-5
LEVEL_TOL = 1e-4


def _ops():
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    import gpu_util
    return ops, gpu_util


_cache = {}


def _setup():
    """Weights, device parameters, inputs and oracle results: built once, shared by every test, never modified."""
    if _cache:
        return _cache
    ops, gu = _ops()
    cfg = dict(model.DEFAULT_CFG, filtersize=5, dwtlevels=1)
    sds = [filled(weights.autoencoder_template(cfg), "b%d." % p) for p in range(P)]
    taps, packed = gu.lifting_params(sds)
    g = torch.Generator().manual_seed(77)
    x, olevel = {}, {}
    for hw in SHAPES:
        x[hw] = torch.rand(P, B, 1, *hw, generator=g) - 0.5
        per_plane = []
        for p in range(P):
            oLL, oYh = lifting.lifting_forward(x[hw][p], sds[p], cfg)
            per_plane.append((oLL, oYh, lifting.lifting_inverse(oLL, oYh, sds[p], cfg)))
        olevel[hw] = per_plane
    _cache.update(cfg=cfg, sds=sds, taps=taps, packed=packed, x=x, olevel=olevel)
    return _cache


def _both_forms(fn):
    """fn() with the current border path, then with the earlier one (flag 64)."""
    ops, _ = _ops()
    outs = []
    try:
        for flags in (0, LEGACY):
            ops.set_diagnostics(0, None, flags)
            outs.append(fn())
            torch.cuda.synchronize()
    finally:
        ops.set_diagnostics(0, None, 0)
    return outs


def _flat(o):
    if torch.is_tensor(o):
        return [o]
    return [t for e in o for t in _flat(e)]


@pytest.mark.parametrize("sign", [1.0, -1.0])          # forward / inverse direction of a step
@pytest.mark.parametrize("vertical", [1, 0])           # row step on H/2 x W, column step on H/2 x W/2
@pytest.mark.parametrize("hw", SHAPES)
def test_step_bits_and_oracle(hw, vertical, sign):
    ops, gu = _ops()
    s = _setup()
    h, w = (hw[0] // 2, hw[1]) if vertical else (hw[0] // 2, hw[1] // 2)
    g = torch.Generator().manual_seed(1000 + 7 * h + w)
    src = torch.rand(P, B, 1, h, w, generator=g) - 0.5
    dst = torch.rand(P, B, 1, h, w, generator=g) - 0.5
    src_d, dst_d = gu.dev(src), gu.dev(dst)
    Z = P * B
    v = lambda t: ops.view_of(t, Z, h, w)
    tp, pk = s["taps"][1].contiguous(), s["packed"][:, 0, 1].contiguous()          # U0 with taps[1]

    def run():
        out_d = torch.empty_like(dst_d)
        ops.lift_step(v(src_d), v(dst_d), v(out_d), Z, B, h, w, tp, pk, 16, 5, vertical, sign, 0.1)
        return out_d.cpu()
    new, old = _both_forms(run)
    assert torch.equal(new, old), (hw, vertical, sign, maxdiff(new, old))
    worst = 0.0
    for p in range(P):
        a, d = src[p], dst[p]
        if not vertical:
            a, d = a.transpose(2, 3), d.transpose(2, 3)
        skip = lifting.skip_filter(a, s["sds"][p]["preProcessingList.1.weight"])
        ref = d + sign * (skip + 0.1 * lifting.p_block(skip, s["sds"][p], "U_blocks.0."))
        if not vertical:
            ref = ref.transpose(2, 3)
        worst = max(worst, maxdiff(new[p], ref))
    print("\n[lift border] step %s vertical=%d sign=%+.0f: max |kernel - oracle| = %.3g" % (hw, vertical, sign, worst))
    assert worst < STEP_TOL, (hw, vertical, sign, worst)


def _level(hw):
    """One level forward (row pass, then the paired L/H column pass) and its inverse from the forward's own outputs."""
    ops, gu = _ops()
    s = _setup()
    ll, yh = ops.lifting_forward(gu.dev(s["x"][hw]), s["taps"], s["packed"], 1, 16, 5, 0.1)
    xr = ops.lifting_inverse(ll, yh, s["taps"], s["packed"], 16, 5, 0.1)
    return [t.cpu() for t in _flat([ll, yh, xr])]


@pytest.mark.parametrize("hw", SHAPES)
def test_level_forward_inverse_bits_and_oracle(hw):
    s = _setup()
    new, old = _both_forms(lambda: _level(hw))
    assert len(new) == len(old)
    for i, (a, b) in enumerate(zip(new, old)):
        assert torch.equal(a, b), (hw, i, maxdiff(a, b))
    ops, gu = _ops()
    ll, yh = ops.lifting_forward(gu.dev(s["x"][hw]), s["taps"], s["packed"], 1, 16, 5, 0.1)
    xr = ops.lifting_inverse(ll, yh, s["taps"], s["packed"], 16, 5, 0.1)
    worst = 0.0
    for p in range(P):
        oLL, oYh, oxr = s["olevel"][hw][p]
        worst = max(worst, maxdiff(ll[p].cpu(), oLL), maxdiff(yh[0][p].cpu(), oYh[0][:, 0]), maxdiff(xr[p].cpu(), oxr))
    print("\n[lift border] level %s: max |kernel - oracle| over LL, LH/HL/HH and the reconstruction = %.3g" % (hw, worst))
    assert worst < LEVEL_TOL, (hw, worst)


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_one_product_modes_bits(prec):
    ops, _ = _ops()
    before = ops.get_precision()
    try:
        ops.set_precision(prec)
        new, old = _both_forms(lambda: _level((64, 96)))
    finally:
        ops.set_precision(before)
    for i, (a, b) in enumerate(zip(new, old)):
        assert torch.equal(a, b), (prec, i, maxdiff(a, b))
