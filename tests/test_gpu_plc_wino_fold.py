"""GPU: the Winograd tree pair (k_plc_wino) with the channel blocks of a pixel tile folded into one workgroup.  The folded form
(lldwt_set_diagnostics(1, ..., flags=4) forces it at any size) runs the parent patch, its |max|, the split im2col and the chunk-0
rows of the first conv once per tile and loops over the tile's blocks of 128 output channels; the last chunk of a pass stages
chunk 0 again for the next one, the buffer parity, the weight ring and the first conv's operands run on across the passes, and
the bias goes through two LDS images that alternate by pass.  The unfolded form (flags=2) is one workgroup per (tile, channel
block), the earlier form (flags=1) the kernel of tests/test_gpu_plc_wino_once.py's reference leg; the default (flags=0) is whatever
the host's rule picks.  Same arithmetic per value and same MFMA order per accumulator everywhere: all four are equal bit for bit.

Per shape, with and without a bias: the folded form against the three others bit for bit, and against the float64 evaluation within
the bars of test_gpu_plc_wino_once.py (2e-6 of the output scale, 2e-5 with tanh).  The two-pass shapes once more on that test's
column-sensitive input, which a pass that read the wrong buffer or a stale chunk-0 image cannot pass by symmetry."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (P, B, cmid, cout, hp, wp, act); the output is 2hp x 2wp
SHAPES = [
    (1, 1, 17, 129, 4, 32, 0),      # two passes, two chunks (even: both passes start on buffer 0), second block with one live channel
    (1, 2, 40, 129, 5, 32, 2),      # three chunks: the second pass starts on buffer 1; a partial tile row; LeakyReLU through the
                                    # partial-tile epilogue
    (1, 1, 5, 129, 1, 1, 0),        # one chunk: the chunk stages itself into the other buffer for the next pass
    (1, 1, 16, 300, 4, 16, 0),      # three passes: both bias images written twice, the weight ring wraps twice
    (1, 1, 17, 5, 4, 17, 0),        # one channel block: the fold is the unfolded kernel; output width 34
    (2, 1, 243, 243, 4, 32, 1),     # the hot path: 16 chunks, two planes, tanh
]
IDS = ["x".join(str(v) for v in s) for s in SHAPES]
TWO_PASS = [i for i, s in enumerate(SHAPES) if 128 < s[3] <= 256]
FOLDED, UNFOLDED, EARLIER, DEFAULT = 4, 2, 1, 0


def _ops():
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    return ops


def _case(i, column_sensitive=False):
    P, B, cmid, cout, hp, wp, act = SHAPES[i]
    g = torch.Generator().manual_seed(1100 + i)
    parent = (torch.rand(P, B, 3, hp, wp, generator=g) - 0.5) * 4.0
    w1 = (torch.rand(P, cmid, 3, 3, 3, generator=g) - 0.5) * 0.6
    b1 = torch.rand(P, cmid, generator=g) - 0.5
    w2 = (torch.rand(P, cout, cmid, 3, 3, generator=g) - 0.5) * (2.0 / (cmid * 9) ** 0.5)
    b2 = torch.rand(P, cout, generator=g) - 0.5
    if column_sensitive:
        # as in test_gpu_plc_wino_once.py: every parent pixel has a value of its own, growing with x and y; the first conv reads one
        # off-centre tap of channel 0 and all its pre-activations are positive
        yy, xx = torch.meshgrid(torch.arange(hp, dtype=torch.float32), torch.arange(wp, dtype=torch.float32), indexing="ij")
        parent = (xx + 100.0 * yy).expand(P, B, 3, hp, wp) + torch.rand(P, B, 3, hp, wp, generator=g) * 0.25
        w1 = torch.zeros(P, cmid, 3, 3, 3)
        w1[:, :, 0, 1, 2] = 0.25 + 0.5 * torch.rand(P, cmid, generator=g)
        b1 = 0.5 + torch.rand(P, cmid, generator=g)
    return parent, w1, b1, w2, b2, cmid, cout, act


_dev_cache = {}


def _run(ops, i, flags, bias=True, column_sensitive=False):
    """The pair on case i under the diagnostics flags; the operands are packed once per case and shared by every test."""
    key = (i, column_sensitive)
    if key not in _dev_cache:
        parent, w1, b1, w2, b2, cmid, cout, act = _case(i, column_sensitive)
        _dev_cache[key] = (parent.to(DEV), ops.plc_fused_pack1(w1.to(DEV), b1.to(DEV)), ops.conv_f16x3_pack(w2.to(DEV)), b2.to(DEV))
    parent, pk1, pk2, b2 = _dev_cache[key]
    _, _, cmid, cout, _, _, act = SHAPES[i]
    ops.set_diagnostics(1, None, flags=flags)
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


def _assert_bias_differs_between_blocks(i):
    """A stale bias image passes when two channel blocks carry the same bias: the test's bias must tell them apart."""
    b2 = _case(i)[4]
    cout = SHAPES[i][3]
    for blk in range(1, (cout + 127) // 128):
        n = min(128, cout - 128 * blk)
        assert not torch.equal(b2[:, 128 * blk:128 * blk + n], b2[:, 128 * (blk - 1):128 * (blk - 1) + n]), (SHAPES[i], blk)
        assert float((b2[:, 128 * blk:128 * blk + n] - b2[:, 128 * (blk - 1):128 * (blk - 1) + n]).abs().max()) > 1e-3


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_folded_equals_the_other_forms_bit_for_bit(i, bias):
    ops = _ops()
    _assert_bias_differs_between_blocks(i)
    P, B, _, cout, hp, wp, _ = SHAPES[i]
    y = _run(ops, i, FOLDED, bias=bias)
    assert y.shape == (P, B, cout, 2 * hp, 2 * wp)
    for name, flags in (("unfolded", UNFOLDED), ("earlier", EARLIER), ("default", DEFAULT)):
        o = _run(ops, i, flags, bias=bias)
        assert o.shape == y.shape
        assert torch.equal(y, o), (SHAPES[i], name, float((y - o).abs().max()))


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_folded_against_float64(i, bias):
    y = _run(_ops(), i, FOLDED, bias=bias)
    r = _reference(i, bias)
    act = SHAPES[i][6]
    for p in range(r.shape[0]):
        e = float((y[p].cpu().double() - r[p]).abs().max()) / max(float(r[p].abs().max()), 1e-6)
        print("\n[plc wino fold] %s bias=%d plane %d: %.3g of the output scale" % (IDS[i], bias, p, e))
        assert e < (2e-6 if act != 1 else 2e-5), (SHAPES[i], p, e)


def test_repeats_are_bit_identical():
    ops = _ops()
    a = _run(ops, 1, FOLDED)
    for _ in range(3):
        assert torch.equal(_run(ops, 1, FOLDED), a)


@pytest.mark.parametrize("i", TWO_PASS, ids=[IDS[i] for i in TWO_PASS])
def test_column_sensitive_input_on_two_pass_shapes(i):
    """Every first-conv value names its pixel, so the second pass cannot pass on a wrong buffer or a stale chunk-0 image by symmetry.
    The input must tell columns apart, or the test proves nothing: checked first."""
    ops = _ops()
    parent = _case(i, column_sensitive=True)[0]
    if parent.shape[-1] > 1:
        assert float((parent[..., 1:] - parent[..., :-1]).min()) > 0.5
    y = _run(ops, i, FOLDED, column_sensitive=True)
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
    for name, flags in (("unfolded", UNFOLDED), ("earlier", EARLIER)):
        o = _run(ops, i, flags, column_sensitive=True)
        assert torch.equal(y, o), (SHAPES[i], name, float((y - o).abs().max()))
