"""GPU: the Winograd tree pair (k_plc_wino) in its current form against its earlier form, which stays selectable through
lldwt_set_diagnostics(1, ..., flags bit 0): both forms do the same arithmetic per value and the same MFMA sequence per
accumulator, so their outputs are equal bit for bit.  The current form is also held to the float64 evaluation and the bars of
test_gpu_plc_winograd.py (2e-6 of the output scale, 2e-5 with tanh), with and without a bias, and repeats bit for bit.
What these tests cannot tell: whether flag 1 selects the other instantiation at all -- no output shows which form ran, by
design, so a library that ignored the flag would pass the equality tests trivially.  That the two legs are different code is
shown by tools/plc_stamps.py, whose legs differ in the epilogue's and the chunks' cycles."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (P, B, cmid, cout, hp, wp, act)
SHAPES = [
    (1, 1, 5, 5, 1, 1, 0),          # one chunk: the staged chunk is the chunk itself; a 2 x 2 output
    (1, 1, 17, 5, 1, 1, 0),         # two chunks, one live channel in the second
    (2, 1, 40, 129, 7, 35, 2),      # three chunks (the buffers alternate on an odd count); a second channel block with one live
                                    # channel; tiles overhang both ways
    (1, 2, 243, 243, 4, 16, 0),     # 16 chunks, exactly one full 8 x 32 tile: the hot path, with every activation
    (1, 2, 243, 243, 4, 16, 2),
    (1, 2, 243, 243, 4, 16, 3),
    (1, 2, 243, 243, 4, 16, 1),
    (1, 3, 243, 243, 9, 16, 1),     # partial rows
]
IDS = ["x".join(str(v) for v in s) for s in SHAPES]
NO_BIAS = [2, 4]                    # a partial-tile and a full-tile case run once more without a bias


def _ops():
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    return ops


def _case(i):
    P, B, cmid, cout, hp, wp, act = SHAPES[i]
    g = torch.Generator().manual_seed(90 + i)
    parent = (torch.rand(P, B, 3, hp, wp, generator=g) - 0.5) * 4.0
    w1 = (torch.rand(P, cmid, 3, 3, 3, generator=g) - 0.5) * 0.6
    b1 = torch.rand(P, cmid, generator=g) - 0.5
    w2 = (torch.rand(P, cout, cmid, 3, 3, generator=g) - 0.5) * (2.0 / (cmid * 9) ** 0.5)
    b2 = torch.rand(P, cout, generator=g) - 0.5
    return parent, w1, b1, w2, b2, cmid, cout, act


_dev_cache = {}


def _run(ops, i, bias=True, earlier=False):
    """The pair on case i; the operands are packed once per case and shared by every test."""
    if i not in _dev_cache:
        parent, w1, b1, w2, b2, cmid, cout, act = _case(i)
        _dev_cache[i] = (parent.to(DEV), ops.plc_fused_pack1(w1.to(DEV), b1.to(DEV)), ops.conv_f16x3_pack(w2.to(DEV)), b2.to(DEV))
    parent, pk1, pk2, b2 = _dev_cache[i]
    _, _, _, _, _, cmid, cout, act = _case(i)
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
        print("\n[plc wino sched] %s bias=%d plane %d: %.3g of the output scale" % (IDS[i], bias, p, e))
        assert e < (2e-6 if act != 1 else 2e-5), (SHAPES[i], p, e)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_current_form_equals_earlier_form_bit_for_bit(i):
    ops = _ops()
    y = _run(ops, i)
    y_earlier = _run(ops, i, earlier=True)
    assert y.shape == y_earlier.shape
    assert torch.equal(y, y_earlier), (SHAPES[i], float((y - y_earlier).abs().max()))


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_current_form_against_float64(i):
    _check_float64(i, _run(_ops(), i))


@pytest.mark.parametrize("i", NO_BIAS, ids=[IDS[i] for i in NO_BIAS])
def test_without_bias(i):
    """No bias pointer: both forms agree bit for bit, and the current one holds the float64 bar."""
    ops = _ops()
    y = _run(ops, i, bias=False)
    assert torch.equal(y, _run(ops, i, bias=False, earlier=True))
    _check_float64(i, y, bias=False)


def test_repeats_are_bit_identical():
    ops = _ops()
    a = _run(ops, 2)
    for _ in range(2):
        assert torch.equal(_run(ops, 2), a)

