"""P2 of the fused lifting step (k_lift_fused_f16, eval path): conv2's 26 weight fragments are requested in six chunks between the
pieces of P1's first two iterations (written out for that) instead of at the head of P2.  The fragments and every accumulator's
sequence of MFMAs -- the same k order, the same product order lo.hi, hi.lo, hi.hi -- stay what they were, so no output bit may
change: diagnostics flag 256 (ops.set_diagnostics kind 0) runs the earlier form, and the default form must be torch.equal to it
in all three precision modes.  The training forward and the backward-data mode keep the earlier form (their kernels are not
rebuilt), so there is nothing to compare for them.

Step arrays (h x w as the kernel sees them; tiles are 16 x 32; P = 2 planes with distinct weights), chosen for the conv2 tile
counts of a tile (tile_range / nit2 / single / rem2 of the kernel's P2) and the conv1 iteration counts of P1 (nit1: one for the
continuing bottom tile of 41 rows, where the second written-out iteration repeats the last tile and stores the same bytes; two
for a whole continuing bottom tile; three for an interior continuing tile; four and five for first-of-run tiles):
  height 16: one tile row, every tile top and bottom at once
  height 32: a first tile at the top, then a bottom tile
  height 48: first, interior, bottom
  widths 32 and 64 (one and two tile columns), and 41 x 70: the image ends inside the last tile row and column
Each shape runs twice.  With B = 2 images per plane the launch has fewer tiles than the device has CUs, the dispatch's cost rule
takes runs of one tile, and every tile is a first-of-run tile (four pairs of conv2 tiles per wave where the tile is whole).  A
tile only CONTINUES a run (two pairs and a single conv2 tile per wave) when the rule takes longer runs, which it does once the
tiles outnumber the CUs: the second run uses the smallest B for which the rule, evaluated here from the device's CU count as
lift_f16_launch does, takes the whole column as one run (asserted), and runs it with and without flag 32 (no hand-down: runs of
one tile again, at that batch).  Inputs lie in [-1, 1], one case is a constant image; weights are the seeded random fills
of the test suite at the scale of the default initialisers."""
import pytest
import torch

from helpers import filled, maxdiff
from oracle import model, weights

pytestmark = pytest.mark.gpu

P, C = 2, 16
OLD_P2, NO_REUSE = 256, 32
PRECISIONS = ("f16x3", "fp16", "bf16")
STEP_OF = {1: (1, (0, 1)), 0: (2, (1, 0))}          # by `vertical`: tap index, (block, pack index)
SHAPES = [(16, 32), (16, 64), (32, 32), (32, 64), (48, 32), (48, 64), (41, 70)]


def _ops():
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    import gpu_util
    return ops, gpu_util


_cache = {}


def _weights():
    if "w" not in _cache:
        _, gu = _ops()
        cfg = dict(model.DEFAULT_CFG, filtersize=5, dwtlevels=1)
        sds = [filled(weights.autoencoder_template(cfg), "c2s%d." % p) for p in range(P)]
        _cache["w"] = gu.lifting_params(sds)
    return _cache["w"]


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


def _batch_for_whole_column_runs(h, w, ncu):
    tiles_y = -(-h // 16)
    for batch in range(2, 1025):
        if _dispatch_run_length(P * batch, h, w, ncu) == tiles_y:
            return batch
    raise AssertionError("no batch up to 1024 makes the dispatch take runs of %d tiles at %dx%d on %d CUs" % (tiles_y, h, w, ncu))


def _both_schedules(h, w, vertical, batch, extra_flags, constant=False):
    ops, gu = _ops()
    taps, packed = _weights()
    j, (blk, u) = STEP_OF[vertical]
    if constant:
        src = torch.full((P, batch, 1, h, w), 1.0)
        dst = torch.full((P, batch, 1, h, w), -1.0)
    else:
        g = torch.Generator().manual_seed(9000 + 131 * h + w + 7 * vertical + batch)
        src = 2.0 * torch.rand(P, batch, 1, h, w, generator=g) - 1.0
        dst = 2.0 * torch.rand(P, batch, 1, h, w, generator=g) - 1.0
    src_d, dst_d = gu.dev(src), gu.dev(dst)
    Z = P * batch
    v = lambda t: ops.view_of(t, Z, h, w)
    tp, pk = taps[j].contiguous(), packed[:, blk, u].contiguous()
    before = ops.get_precision()
    try:
        for prec in PRECISIONS:
            ops.set_precision(prec)
            outs = []
            for flags in (extra_flags, extra_flags | OLD_P2):
                ops.set_diagnostics(0, None, flags)
                out_d = torch.empty_like(dst_d)
                ops.lift_step(v(src_d), v(dst_d), v(out_d), Z, batch, h, w, tp, pk, C, 5, vertical, 1.0, 0.1)
                torch.cuda.synchronize()
                outs.append(out_d.cpu())
            tag = (h, w, vertical, batch, extra_flags, prec)
            assert bool(torch.isfinite(outs[0]).all()), tag
            assert not torch.equal(outs[0], dst), tag                          # the step did run
            assert torch.equal(outs[0], outs[1]), (tag, "flag 256", maxdiff(outs[0], outs[1]))
    finally:
        ops.set_diagnostics(0, None, 0)
        ops.set_precision(before)


@pytest.mark.parametrize("vertical", [1, 0])
@pytest.mark.parametrize("hw", SHAPES)
def test_first_of_run_tiles_bits(hw, vertical):
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    assert _dispatch_run_length(P * 2, hw[0], hw[1], ncu) == 1
    _both_schedules(hw[0], hw[1], vertical, 2, 0)


@pytest.mark.parametrize("vertical", [1, 0])
@pytest.mark.parametrize("hw", [s for s in SHAPES if s[0] > 16])
def test_continuing_tiles_bits(hw, vertical):
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    batch = _batch_for_whole_column_runs(hw[0], hw[1], ncu)
    assert _dispatch_run_length(P * batch, hw[0], hw[1], ncu) == -(-hw[0] // 16)
    _both_schedules(hw[0], hw[1], vertical, batch, 0)
    _both_schedules(hw[0], hw[1], vertical, batch, NO_REUSE)


@pytest.mark.parametrize("vertical", [1, 0])
def test_constant_image_bits(vertical):
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    _both_schedules(48, 64, vertical, 2, 0, constant=True)
    _both_schedules(48, 64, vertical, _batch_for_whole_column_runs(48, 64, ncu), 0, constant=True)
