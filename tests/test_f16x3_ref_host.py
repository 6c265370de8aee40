"""CPU: proves the float64 reference, the split evaluation and the inputs of tests/test_gpu_f16x3_domain.py (tests/f16x3_ref.py).

  * the reference equals F.conv2d / F.interpolate / torch autograd in float64 to 1e-12 of the output scale;
  * pow2_scale is csrc/split_f16.h's, the case of a power-of-two amax included;
  * the split evaluation on small integers equals the float64 result exactly, in every form;
  * every case's own inputs reject every applicable planted fault under that case's own bar (per plane, per output tile for the
    region inputs, per image row for the row ramps) and the clean split evaluation passes it; every fault applies somewhere;
  * the region exponents: the probe prints what a step of 2^20 and of 2^24 between neighbouring regions leaves of each misplaced
    scale, and asserts that the chosen step rejects all three.
Every test prints its yardsticks (pytest -s)."""
import pytest
import torch
import torch.nn.functional as F

import f16x3_ref as X
import lift_ref as R

F64 = torch.float64


def _close(a, b):
    return float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


# ------------------------------------------------------------------------------------------------ the reference is torch's
def _torch_act(v, act):
    return torch.tanh(v) if act == 1 else F.leaky_relu(v, 0.01) if act == 2 else F.relu(v) if act == 3 else v


@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", list(X.PARENTS))
def test_pair_reference_equals_torch(shape, act):
    d = X.pair_inputs(shape)
    for p in range(X.P):
        par, w1, b1, w2, b2 = (t[p].double() for t in (d.parent, d.w1, d.b1, d.w2, d.b2))
        t = F.leaky_relu(F.conv2d(F.interpolate(par, scale_factor=2, mode="nearest"), w1, b1, padding=1), 0.01)
        want = _torch_act(F.conv2d(t, w2, b2, padding=1), act)
        assert _close(X.epilogue(X.pair_lin(par, w1, b1, w2), b2, act), want)
        assert _close(X.epilogue(X.pair_lin_torch(par, w1, b1, w2), b2, act), want)
        assert _close(X.epilogue(X.pair_lin_chain(par, w1, b1, w2, 16), b2, act), want)


def test_conv_adjoint_and_wgrad_reference_equal_torch_autograd():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 6, 9, generator=g, dtype=F64, requires_grad=True)
    w = torch.randn(7, 5, 3, 3, generator=g, dtype=F64, requires_grad=True)
    b = torch.randn(7, generator=g, dtype=F64, requires_grad=True)
    dy = torch.randn(2, 7, 6, 9, generator=g, dtype=F64)
    y = F.conv2d(x, w, b, padding=1)
    dx, dw, db = torch.autograd.grad((y * dy).sum(), [x, w, b])
    assert _close(X.conv3(x.detach(), w.detach()) + b.detach().view(1, -1, 1, 1), y.detach())
    assert _close(X.conv3_chain(x.detach(), w.detach(), 4), F.conv2d(x.detach(), w.detach(), None, padding=1))
    assert _close(X.conv3(dy, X.adjoint_weight(w.detach())), dx)
    rw, rb = X.wgrad(x.detach(), dy, alpha=-0.5)
    assert _close(rw, -0.5 * dw) and _close(rb, -0.5 * db)
    cw, cb = X.wgrad_chain(x.detach(), dy, -0.5, 3)
    assert _close(cw, -0.5 * dw) and _close(cb, -0.5 * db)


def test_pow2_scale_is_the_kernels():
    for n in (-130, -24, -1, 0, 1, 14, 15, 30, 100):
        a = torch.tensor(2.0 ** n if n > -127 else 2.0 ** -126 * 2.0 ** (n + 126))
        s = float(X.pow2_scale(a))
        assert s == 2.0 ** min(120, 14 - n), (n, s)                       # amax = 2^n: m = 0.5, e = n + 1
        assert float(X.pow2_scale(a * 1.5)) == s and float(X.pow2_scale(a * 0.75)) == 2 * s or n <= -126
    for amax, top in ((3.0, 15), (1e-3, 14), (65504.0, 15), (7e22, 14)):
        s = float(X.pow2_scale(torch.tensor(amax), top))
        assert 2.0 ** (top - 1) <= amax * s < 2.0 ** top
    assert float(X.pow2_scale(torch.tensor(0.0))) == 1.0 and float(X.pow2_scale(torch.tensor(float("inf")))) == 1.0
    assert float(X.pow2_scale(torch.tensor(float("nan")))) == 1.0
    v = torch.tensor([1.0 + 2.0 ** -12, 3.0001, -0.126, 40000.0 / 3, -32767.9])      # the 18 binades in which lo stays a normal number
    hi, lo = X.split(v)
    assert bool(((v - hi - lo).abs() <= 2.0 ** -22 * v.abs()).all())


# ------------------------------------------------------------------------------------------------ integers are exact
def test_split_evaluation_is_exact_on_integers():
    g = torch.Generator().manual_seed(11)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    parent, w1, b1 = ri(0, 3, 2, 2, 3, 7, 19), ri(0, 2, 2, 21, 3, 3, 3), ri(0, 3, 2, 21)            # the first conv is non-negative
    w2 = ri(-2, 2, 2, 9, 21, 3, 3)
    want = torch.stack([X.pair_lin(parent[p].double(), w1[p].double(), b1[p].double(), w2[p].double()) for p in range(2)])
    for form in ("direct", "wino"):
        assert torch.equal(X.pair_split(parent, w1, b1, w2, form).double(), want), form
    x, w = ri(-4, 4, 2, 37, 5, 9), ri(-3, 3, 6, 37, 3, 3)
    assert torch.equal(X.conv_split(x, w, x.abs().max()).double(), X.conv3(x.double(), w.double()))
    assert torch.equal(X.conv_split(x * 8, w, None, in16_scale=8.0).double(), X.conv3(x.double(), w.double()))
    dy = ri(-3, 3, 2, 6, 5, 9)
    dw, db = X.wgrad_split(x, dy, x.abs().max(), dy.abs().max())
    rw, rb = X.wgrad(x.double(), dy.double())
    assert torch.equal(dw.double(), rw) and torch.equal(db.double(), rb)


# ------------------------------------------------------------------------------------------------ planted faults
applied = set()


def _pair_check(c, got, ref, f32s):
    if c.tiles:
        tr, tf = X.tiled_eval(ref, f32s)
        return X.exceeds([X.tiled(t) for t in got], tr, tf, "y", R.VALUE_FLOOR, X.TILE_DIMS)
    return X.exceeds(got, ref, f32s, "y", R.VALUE_FLOOR)


@pytest.mark.parametrize("c", X.PAIR_CASES, ids=lambda c: c.name)
def test_pair_inputs_reject_every_applicable_fault(c):
    ref, f32s = X.pair_evaluate(c)
    yard = R.yardstick(ref, f32s, "y")
    print("\n%-44s yardstick %s  max|f64| %s" % (c.name, ["%.2e" % float(y) for y in yard], ["%.2e" % float(t.abs().max()) for t in ref["y"]]))
    for leg in (4, 5):                                                   # the clean split evaluations, direct and Winograd
        bad, _ = _pair_check(c, f32s[leg]["y"], ref, f32s)
        assert not bad, (c.name, leg)
    for fault in X.FAULTS:
        if not X.applies(c, fault):
            continue
        applied.add(fault)
        bad, ratio = _pair_check(c, X.pair_faulty(c, fault), ref, f32s)
        print("    %-14s rejected at %.3g x bar" % (fault, ratio) if bad else "    %-14s NOT REJECTED" % fault)
        assert bad, (c.name, fault)


@pytest.mark.parametrize("c", X.CONV_CASES + X.IN16_CASES + X.BWD_CASES + X.WGRAD_CASES, ids=lambda c: c.name)
def test_conv_inputs_reject_every_applicable_fault(c):
    d = X.conv_inputs(c)
    ref, f32s = X.conv_evaluate(c, d)
    floor = R.VALUE_FLOOR if c.kind in ("conv", "in16") else R.GRAD_FLOOR
    keys = ("dw", "db") if c.kind == "wgrad" else ("y",)
    rd = X.ROW_DIMS if c.rows else None
    for k in keys:
        print("\n%-28s %-3s yardstick %s" % (c.name, k, ["%.2e" % float(torch.as_tensor(y).max()) for y in R.yardstick(ref, f32s, k)]))
        bad, _ = X.exceeds(f32s[-1][k], ref, f32s, k, floor, rd)
        assert not bad
    for fault in X.FAULTS:
        if not X.applies(c, fault):
            continue
        applied.add(fault)
        got = X.conv_faulty(c, d, fault)
        res = [X.exceeds(got[k], ref, f32s, k, floor, rd) for k in keys]
        bad, ratio = any(r[0] for r in res), max(r[1] for r in res)
        print("    %-14s rejected at %.3g x bar" % (fault, ratio) if bad else "    %-14s NOT REJECTED" % fault)
        assert bad, (c.name, fault)


def test_every_fault_applies_somewhere():
    cases = X.PAIR_CASES + X.CONV_CASES + X.IN16_CASES + X.BWD_CASES + X.WGRAD_CASES
    for fault in X.FAULTS:
        assert any(X.applies(c, fault) for c in cases), fault
    for c in X.PAIR_REGIONS:
        assert all(X.applies(c, f) for f in X.SCALE_FAULTS)
    for shape in ("4x144", "36x16"):
        assert len(X.middle_tiles(*X.PARENTS[shape])) == 3
    assert not X.middle_tiles(*X.PARENTS["7x19"])


# ------------------------------------------------------------------------------------------------ the region exponents
def test_region_exponents_are_needed_and_enough():
    """What a scale that is ONE region step too small leaves of the per-tile bar: plane 0's region 0 (exponent 0) is handed the scale of
    exponent +step by the launch-wide scale and by the neighbouring plane's.  Printed for steps of 2^16, 2^20 and the chosen one
    (f16x3_ref.REGION_EXP) as error / bar of that region's middle tile; the chosen step must leave the bar there, and all three
    misplaced scales must be rejected on the chosen input as a whole."""
    chosen = max(abs(k) for ex in X.REGION_EXP for k in ex)
    assert chosen == 24
    hp, wp = X.PARENTS["4x144"]
    (_, y0, x0), = [m for m in X.middle_tiles(hp, wp) if m[0] == 0]
    for step in (16, 20, chosen):
        c = X.pair_case("4x144", "regions%d" % step, 0, False)
        ref, f32s = X.pair_evaluate(c)
        tr, tf = X.tiled_eval(ref, f32s)
        yard = R.yardstick(tr, tf, "y", X.TILE_DIMS)[0][y0 // X.TH, x0 // X.TW]
        bar = 4.0 * float(yard) + R.VALUE_FLOOR * float(tr["y"][0][:, :, y0 // X.TH, :, x0 // X.TW].abs().max())
        for fault in ("scale_launch", "scale_plane"):
            got = X.tiled(X.pair_faulty(c, fault)[0])[:, :, y0 // X.TH, :, x0 // X.TW]
            e = float((got.double() - tr["y"][0][:, :, y0 // X.TH, :, x0 // X.TW]).abs().max())
            print("\nregion step 2^%d  %-13s one step off: error %.3g  yardstick %.3g  bar %.3g  (%.2f x bar)" % (step, fault, e, float(yard), bar, e / bar))
            if step == chosen:
                assert e > bar, (fault, e, bar)
        if step == chosen:
            for fault in X.SCALE_FAULTS:
                assert _pair_check(c, X.pair_faulty(c, fault), ref, f32s)[0], fault
