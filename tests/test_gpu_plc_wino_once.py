"""GPU: the Winograd tree pair (k_plc_wino) computes every first-conv pixel once.  Its current form runs the first conv on the pixel
sets 0 and 1 of a pair only; a lane takes the sets 2 and 3 from its neighbour in the 16-lane row, and lane 15 from an extra
16-column tile that holds pair 16 of the wave's rows.  The barrier of a chunk sits behind unit 10, and unit 11 loads the next
chunk's first fragments.  The earlier form (lldwt_set_diagnostics(1, ..., flags bit 0)) computes all four shifted sets in every
lane: both forms do the same arithmetic per value in the same order, so the outputs are equal bit for bit.

The shapes are the smallest at which the new paths can go wrong (see SHAPES).  Per shape: bit equality with the earlier form with
and without a bias, the float64 evaluation within the bars of test_gpu_plc_winograd.py (2e-6 of the output scale, 2e-5 with tanh),
and bit equality once more on a column-sensitive input (a parent that grows with x and y, first-conv weights on one off-centre
tap, a bias that keeps the LeakyReLU in its identity half), which a shifted or swapped lane cannot pass by symmetry."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (P, B, cmid, cout, hp, wp, act); the output is 2hp x 2wp
SHAPES = [
    (1, 1, 17, 5, 4, 32, 0),        # two chunks, two full 8 x 32 tiles side by side: tile 0's pair 16 lies inside the image (the extra
                                    # tile's values are live), tile 1's outside (masked to zero)
    (1, 1, 17, 5, 4, 17, 0),        # output width 34: the second tile holds pair 0 only, its first-conv patch ends inside the tile
    (1, 2, 40, 129, 5, 32, 2),      # three chunks (the buffers alternate on an odd count), a partial second tile row (10 output rows),
                                    # a second channel block with one live channel; LeakyReLU through the partial-tile epilogue
    (1, 1, 243, 243, 4, 32, 1),     # the hot path: 16 chunks, two full tiles; tanh epilogue
    (1, 1, 5, 5, 1, 1, 0),          # one chunk: the staged chunk is the chunk itself, the last unit 11 has no successor
    (1, 1, 16, 5, 4, 16, 0),        # exactly one full chunk, nothing to stage behind it
]
IDS = ["x".join(str(v) for v in s) for s in SHAPES]


def _ops():
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    return ops


def _case(i, column_sensitive=False):
    P, B, cmid, cout, hp, wp, act = SHAPES[i]
    g = torch.Generator().manual_seed(190 + i)
    parent = (torch.rand(P, B, 3, hp, wp, generator=g) - 0.5) * 4.0
    w1 = (torch.rand(P, cmid, 3, 3, 3, generator=g) - 0.5) * 0.6
    b1 = torch.rand(P, cmid, generator=g) - 0.5
    w2 = (torch.rand(P, cout, cmid, 3, 3, generator=g) - 0.5) * (2.0 / (cmid * 9) ** 0.5)
    b2 = torch.rand(P, cout, generator=g) - 0.5
    if column_sensitive:
        # every parent pixel has a value of its own, growing with x and y; the first conv reads ONE off-centre tap of channel 0, and
        # all its pre-activations are positive: the conv's output at a pixel names the pixel it was computed from
        yy, xx = torch.meshgrid(torch.arange(hp, dtype=torch.float32), torch.arange(wp, dtype=torch.float32), indexing="ij")
        parent = (xx + 100.0 * yy).expand(P, B, 3, hp, wp) + torch.rand(P, B, 3, hp, wp, generator=g) * 0.25
        w1 = torch.zeros(P, cmid, 3, 3, 3)
        w1[:, :, 0, 1, 2] = 0.25 + 0.5 * torch.rand(P, cmid, generator=g)
        b1 = 0.5 + torch.rand(P, cmid, generator=g)
    return parent, w1, b1, w2, b2, cmid, cout, act


_dev_cache = {}


def _run(ops, i, bias=True, earlier=False, column_sensitive=False):
    """The pair on case i; the operands are packed once per case and shared by every test."""
    key = (i, column_sensitive)
    if key not in _dev_cache:
        parent, w1, b1, w2, b2, cmid, cout, act = _case(i, column_sensitive)
        _dev_cache[key] = (parent.to(DEV), ops.plc_fused_pack1(w1.to(DEV), b1.to(DEV)), ops.conv_f16x3_pack(w2.to(DEV)), b2.to(DEV))
    parent, pk1, pk2, b2 = _dev_cache[key]
    _, _, cmid, cout, _, _, act = SHAPES[i]
    if not earlier:
        return ops.plc_fused(parent, pk1, pk2, b2 if bias else None, cmid, cout, act=act)
    ops.set_diagnostics(1, None, flags=1)
    try:
        return ops.plc_fused(parent, pk1, pk2, b2 if bias else None, cmid, cout, act=act)
    finally:
        ops.set_diagnostics(1, None, flags=0)


_ref_cache = {}


def _reference(i, bias=True):
    """float64 evaluation of the same maths (nearest 2x upsample, LeakyReLU 0.01 between the convs), computed once per case."""
    if (i, bias) not in _ref_cache:
        parent, w1, b1, w2, b2, cmid, cout, act = _case(i)
        out = []
        for p in range(parent.shape[0]):
            up = F.interpolate(parent[p].double(), scale_factor=2, mode="nearest")
            t = F.leaky_relu(F.conv2d(up, w1[p].double(), b1[p].double(), padding=1), 0.01)
            r = F.conv2d(t, w2[p].double(), b2[p].double() if bias else None, padding=1)
            r = F.leaky_relu(r, 0.01) if act == 2 else (F.relu(r) if act == 3 else r)
            out.append(torch.tanh(r) if act == 1 else r)
        _ref_cache[(i, bias)] = torch.stack(out)
    return _ref_cache[(i, bias)]


def _check_float64(i, y, bias=True):
    r = _reference(i, bias)
    act = SHAPES[i][6]
    for p in range(r.shape[0]):
        e = float((y[p].cpu().double() - r[p]).abs().max()) / max(float(r[p].abs().max()), 1e-6)
        print("\n[plc wino once] %s bias=%d plane %d: %.3g of the output scale" % (IDS[i], bias, p, e))
        assert e < (2e-6 if act != 1 else 2e-5), (SHAPES[i], p, e)


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_equals_earlier_form_bit_for_bit(i, bias):
    ops = _ops()
    y = _run(ops, i, bias=bias)
    y_earlier = _run(ops, i, bias=bias, earlier=True)
    P, B, _, cout, hp, wp, _ = SHAPES[i]
    assert y.shape == y_earlier.shape == (P, B, cout, 2 * hp, 2 * wp)
    assert torch.equal(y, y_earlier), (SHAPES[i], float((y - y_earlier).abs().max()))


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_against_float64(i, bias):
    _check_float64(i, _run(_ops(), i, bias=bias), bias=bias)


def test_repeats_are_bit_identical():
    ops = _ops()
    a = _run(ops, 2)
    for _ in range(3):
        assert torch.equal(_run(ops, 2), a)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_column_sensitive_input_equals_earlier_form(i):
    """Every first-conv value names its pixel: a lane that took its neighbour's value from the wrong side, or pair 16 from the wrong
    column of the extra tile, changes the output.  The input must tell columns apart, or the test proves nothing: checked first."""
    ops = _ops()
    parent = _case(i, column_sensitive=True)[0]
    if parent.shape[-1] > 1:
        assert float((parent[..., 1:] - parent[..., :-1]).min()) > 0.5
    y = _run(ops, i, column_sensitive=True)
    y_earlier = _run(ops, i, earlier=True, column_sensitive=True)
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
    assert torch.equal(y, y_earlier), (SHAPES[i], float((y - y_earlier).abs().max()))
