"""GPU: the split-fp16 3x3 conv family (csrc/conv_f16x3.hip, csrc/conv_wgrad_f16x3.hip) against the float64 reference of
tests/f16x3_ref.py, scales included.  Bars are the project's rule, 4 x yardstick + floor x max|f64| (tests/lift_ref.py), per plane,
per 8 x 32 output tile for the region inputs and per image row for the row ramps; tests/test_f16x3_ref_host.py shows that every input
used here rejects every applicable planted fault under the same bars.  Every comparison prints its error beside its bar (pytest -s).

Forms of the pair: k_plc_wino as the host's fold rule picks it, its earlier form (diagnostics flags 1), one workgroup per (tile,
channel block) (2) and per tile (4) in this process; the direct kernel (LLDWT_PLC_ALGO=direct) and the 16x16x32 shape
(LLDWT_PLC_SHAPE=16) in one child process each, which runs groups 1 and 2 and hands its outputs back.

  1. scale covariance, bit for bit: with b1 = 0 and no b2 every scale is a power of two and the pair is homogeneous, so
     y(2^k parent) == 2^k y(parent) for k = -24, +24, and on the region inputs (parent x 2^k_r on three regions, f16x3_ref.REGION_EXP)
     the middle tile of each region, whose whole 6 x 18 patch lies inside it, equals 2^k_r times the unscaled run's tile.  The dense
     conv with planes x 2^0, 2^-30, 2^30 and the fp16-storage form with xscale multiplied get the same test;
  2. the pair against float64: activations 0 .. 3 with and without b2 at the three parents, the numeric domain at 7x19 and 4x144,
     the region inputs per tile;
  3. the dense conv (slots handed in and computed) and the fp16-storage form (against float64 on the dequantised stored values);
  4. the one-product class (set_precision fp16 / bf16) under 4 x the one-product evaluation + floor;
  5. backward through the split kernels: dx of autograd.conv against the float64 adjoint conv, lldwt_conv3x3_wgrad_f16x3 with x and
     dy planes at distinct magnitudes, under the gradient rule."""
import os
import subprocess
import sys
import tempfile
import types

import pytest
import torch

import f16x3_ref as X
import lift_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = [("default", 0), ("earlier", 1), ("unfolded", 2), ("folded", 4)]
COV_ACTS = (X.ACT_NONE, X.ACT_LRELU, X.ACT_RELU)
CHILDREN = {"direct": {"LLDWT_PLC_ALGO": "direct"}, "shape16": {"LLDWT_PLC_SHAPE": "16"}}


def _ops():
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    return ops


def _in_process_forms(ops):
    """The four forms of k_plc_wino; one entry where the process runs the direct kernel (the flags do not reach it)."""
    return FORMS if ops.plc_algo() == "winograd" else FORMS[:1]


_dev = {}


def _pair_dev(ops, d):
    key = (d.shape, d.variant)
    if key not in _dev:
        _dev[key] = (d.parent.to(DEV), ops.plc_fused_pack1(d.w1.to(DEV), d.b1.to(DEV)), ops.conv_f16x3_pack(d.w2.to(DEV)), d.b2.to(DEV))
    return _dev[key]


def run_pair(ops, d, act, bias, flags=0, parent=None):
    par, pk1, pk2, b2 = _pair_dev(ops, d)
    ops.set_diagnostics(1, None, flags=flags)
    try:
        y = ops.plc_fused(par if parent is None else parent.to(DEV), pk1, pk2, b2 if bias else None, X.CMID, X.COUT, act=act)
        torch.cuda.synchronize()
    finally:
        ops.set_diagnostics(1, None, flags=0)
    return y.cpu()


# ------------------------------------------------------------------------------------------------ group 1: scale covariance
def pair_covariance(ops, flags):
    """-> [(what, equal, largest difference)] of every bit-for-bit comparison of group 1 for the pair under `flags`."""
    out = []
    for shape in X.PARENTS:
        d0 = X.pair_inputs(shape, "b1zero")
        for act in COV_ACTS:
            y = run_pair(ops, d0, act, False, flags)
            assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
            for k in (-24, 24):
                yk = run_pair(ops, d0, act, False, flags, parent=d0.parent * 2.0 ** k)
                out.append(("%s act%d 2^%d" % (shape, act, k), torch.equal(yk, y * 2.0 ** k), float((yk * 2.0 ** -k - y).abs().max())))
            mids = X.middle_tiles(d0.hp, d0.wp)
            if mids:
                dr = X.pair_inputs(shape, "regions")
                assert torch.equal(dr.parent, d0.parent * X.region_gain(d0.hp, d0.wp)) and torch.equal(dr.w2, d0.w2)
                yr = run_pair(ops, dr, act, False, flags)
                for r, y0, x0 in mids:
                    for p in range(X.P):
                        g = 2.0 ** X.REGION_EXP[p][r]
                        a, b = yr[p, :, :, y0:y0 + X.TH, x0:x0 + X.TW], y[p, :, :, y0:y0 + X.TH, x0:x0 + X.TW] * g
                        out.append(("%s act%d region %d plane %d" % (shape, act, r, p), torch.equal(a, b), float((a / g - b / g).abs().max())))
    return out


def _assert_covariant(rows, tag):
    bad = [r for r in rows if not r[1]]
    print("\n[%s] %d bit-for-bit comparisons, %d differ" % (tag, len(rows), len(bad)))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("form", [f[0] for f in FORMS])
def test_pair_scale_covariance_bit_for_bit(form):
    ops = _ops()
    forms = dict(_in_process_forms(ops))
    if form not in forms:
        pytest.skip("this process runs the direct kernel: one form")
    _assert_covariant(pair_covariance(ops, forms[form]), form)


def test_conv_scale_covariance_bit_for_bit():
    """lldwt_conv3x3_f16x3 with the planes times 2^0, 2^-30, 2^30 (no bias; slots handed in and computed) and lldwt_conv3x3_f16in with
    xscale times 2^0, 2^-10, 2^10: one power-of-two scale per plane, so each plane's output scales exactly."""
    ops = _ops()
    c = X.CONV_CASES[0]
    d = X.conv_inputs(c)
    gain = (2.0 ** torch.tensor(X.PLANE_EXP, dtype=torch.float32)).view(-1, 1, 1, 1, 1)
    x0 = d.x / gain
    assert torch.equal(x0 * gain, d.x)
    packed = ops.conv_f16x3_pack(d.w.to(DEV))
    for act in COV_ACTS:
        ya = ops.conv3x3_f16x3(x0.to(DEV), packed, None, c.cout, act=act).cpu()
        for slots in (None, ops.absmax_slots(d.x.to(DEV))):
            yb = ops.conv3x3_f16x3(d.x.to(DEV), packed, None, c.cout, act=act, slots=slots).cpu()
            for p in range(c.planes):
                same = torch.equal(yb[p], ya[p] * gain[p])
                print("conv planes3 act%d plane %d (2^%d) slots %s: %s" % (act, p, X.PLANE_EXP[p], "computed" if slots is None else "given", "equal" if same else "DIFFERS"))
                assert same, (act, p)
    c16 = X.IN16_CASES[0]
    d16 = X.conv_inputs(c16)
    pk = ops.conv_f16x3_pack(d16.w.to(DEV))
    k = torch.tensor([0.0, -10.0, 10.0])
    ya = ops.conv3x3_f16in(d16.x16.to(DEV), pk, None, c16.cout, d16.xscale.to(DEV)).cpu()
    yb = ops.conv3x3_f16in(d16.x16.to(DEV), pk, None, c16.cout, (d16.xscale * 2.0 ** k).to(DEV)).cpu()
    for p in range(c16.planes):
        same = torch.equal(yb[p], ya[p] * 2.0 ** -float(k[p]))
        print("in16 plane %d xscale x 2^%d: %s" % (p, int(k[p]), "equal" if same else "DIFFERS"))
        assert same, p


# ------------------------------------------------------------------------------------------------ group 2: the pair against float64
_evals = {}


def _pair_eval(c):
    """(ref, f32s) of a pair case, tiled for the region inputs; the 1e-40 parent is held to the bar of the bias-only pair."""
    if c.name not in _evals:
        e = X.pair_evaluate(X.pair_case(c.shape, "zero", c.act, c.bias) if c.variant == "tiny" else c)
        _evals[c.name] = X.tiled_eval(*e) if c.tiles else e
    return _evals[c.name]


def check_pair(c, y, tag):
    ref, f32s = _pair_eval(c)
    assert bool(torch.isfinite(y).all()), (c.name, tag)
    got = [X.tiled(y[p]) if c.tiles else y[p] for p in range(X.P)]
    return R.check("%s %s" % (c.name, tag), "y", got, ref, f32s, floor=R.VALUE_FLOOR, row_dims=X.TILE_DIMS if c.tiles else None)


@pytest.mark.parametrize("c", X.PAIR_CASES, ids=lambda c: c.name)
def test_pair_against_float64(c):
    ops = _ops()
    d = X.pair_inputs(c.shape, c.variant)
    bad = []
    for form, flags in _in_process_forms(ops):
        bad += check_pair(c, run_pair(ops, d, c.act, c.bias, flags), form)
    assert not bad, bad


def _child_main(out):
    """Runs in the child process: groups 1 and 2 of the pair with the kernel the environment selects; the outputs go back in a file."""
    ops = _ops()
    res = {"algo": ops.plc_algo(), "shape": ops.plc_shape(), "cov": pair_covariance(ops, 0), "y": {}}
    for c in X.PAIR_CASES:
        res["y"][c.name] = run_pair(ops, X.pair_inputs(c.shape, c.variant), c.act, c.bias)
    torch.save(res, out)


@pytest.mark.parametrize("setting", list(CHILDREN))
def test_pair_in_a_child_process(setting):
    if os.environ.get("LLDWT_PLC_ALGO") or os.environ.get("LLDWT_PLC_SHAPE"):
        pytest.skip("already inside a run with a process-wide kernel choice")
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_f16x3_domain as t\nt._child_main(sys.argv[1])\n" % (REPO, os.path.join(REPO, "tests")))
    with tempfile.TemporaryDirectory() as td:
        f = os.path.join(td, "out.pt")
        r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, **CHILDREN[setting]), capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        res = torch.load(f, weights_only=False)
    assert res["algo"] == "direct" and res["shape"] == (16 if setting == "shape16" else 32), (res["algo"], res["shape"])
    _assert_covariant(res["cov"], setting)
    bad = []
    for c in X.PAIR_CASES:
        bad += check_pair(c, res["y"][c.name], setting)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ group 3: dense conv, fp16 storage
def _check_conv(c, d, y, tag, floor=R.VALUE_FLOOR):
    ref, f32s = X.conv_evaluate(c, d)
    assert bool(torch.isfinite(y).all())
    return R.check("%s %s" % (c.name, tag), "y", [y[p] for p in range(c.planes)], ref, f32s, floor=floor, row_dims=X.ROW_DIMS if c.rows else None)


@pytest.mark.parametrize("c", X.CONV_CASES, ids=lambda c: c.name)
def test_conv_against_float64(c):
    ops = _ops()
    d = X.conv_inputs(c)
    x, packed = d.x.to(DEV), ops.conv_f16x3_pack(d.w.to(DEV))
    b = d.b.to(DEV) if c.bias else None
    bad = _check_conv(c, d, ops.conv3x3_f16x3(x, packed, b, c.cout, act=c.act).cpu(), "slots computed")
    bad += _check_conv(c, d, ops.conv3x3_f16x3(x, packed, b, c.cout, act=c.act, slots=ops.absmax_slots(x)).cpu(), "slots given")
    assert not bad, bad


def test_f16in_exact_on_integers():
    ops = _ops()
    g = torch.Generator().manual_seed(21)
    Pn, cin, cout, h, wd = 3, 37, 150, 11, 45
    x = torch.randint(-4, 5, (Pn, X.B, cin, h, wd), generator=g).float()
    w = torch.randint(-3, 4, (Pn, cout, cin, 3, 3), generator=g).float()
    b = torch.randint(-5, 6, (Pn, cout), generator=g).float()
    xscale = torch.tensor([1.0, 64.0, 0.125])
    x16 = (x * xscale.view(-1, 1, 1, 1, 1)).half()
    y = ops.conv3x3_f16in(x16.to(DEV), ops.conv_f16x3_pack(w.to(DEV)), b.to(DEV), cout, xscale.to(DEV)).cpu()
    for p in range(Pn):
        assert torch.equal(y[p].double(), X.conv3(x[p].double(), w[p].double()) + b[p].double().view(1, -1, 1, 1)), p


@pytest.mark.parametrize("c", X.IN16_CASES, ids=lambda c: c.name)
def test_f16in_against_float64_on_the_stored_values(c):
    """Against float64 on x16 / xscale the error is the weight split's alone: the values bar applies."""
    ops = _ops()
    d = X.conv_inputs(c)
    if c.variant == "f16out":                     # the input as _plc_pair produces it: the first tree conv stored as fp16 x oscale
        pd = X.pair_inputs("7x19")
        par, w1, b1 = pd.parent.to(DEV), pd.w1.to(DEV), pd.b1.to(DEV)
        bound = ops.absmax_slots(par).amax(dim=1) * w1.abs().sum(dim=(2, 3, 4)).amax(dim=1) + b1.abs().amax(dim=1)
        oscale = torch.exp2(14.0 - torch.ceil(torch.log2(bound.clamp_min(1e-30)))).contiguous()
        t16 = ops.conv2d_f16out(par, w1, b1, 3, oscale, act=ops.ACT_LRELU, upsample2=True)
        d = types.SimpleNamespace(w=d.w, b=d.b, x16=t16.cpu(), xscale=oscale.cpu())
        d.x = d.x16.float() / d.xscale.view(-1, 1, 1, 1, 1)
        assert tuple(d.x16.shape) == (c.planes, X.B, c.cin) + tuple(c.hw) and float(d.x16.float().abs().max()) > 2.0 ** 10
    y = ops.conv3x3_f16in(d.x16.to(DEV), ops.conv_f16x3_pack(d.w.to(DEV)), d.b.to(DEV) if c.bias else None, c.cout, d.xscale.to(DEV),
                          act=c.act).cpu()
    bad = _check_conv(c, d, y, "")
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ group 4: the one-product class
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", ["7x19", "4x144"])
def test_one_product_class(shape, prec):
    """The pair under set_precision('fp16' / 'bf16'): 4 x the one-product evaluation (operands rounded to the type, fp32 accumulation)
    plus the floor, per plane."""
    ops = _ops()
    d = X.pair_inputs(shape)
    lin64, _ = X.pair_lins(d)
    one = X.pair_split(d.parent, d.w1, d.b1, d.w2, "direct", prec=1 if prec == "fp16" else 2)
    ref = {"y": [X.epilogue(lin64[p], d.b2[p].double(), X.ACT_NONE) for p in range(X.P)]}
    f32s = [{"y": [X.epilogue(one[p], d.b2[p], X.ACT_NONE) for p in range(X.P)]}]
    saved = ops.get_precision()
    ops.set_precision(prec)
    try:
        y = run_pair(ops, d, X.ACT_NONE, True)
    finally:
        ops.set_precision(saved)
    assert bool(torch.isfinite(y).all())
    bad = R.check("one-product %s %s" % (prec, shape), "y", [y[p] for p in range(X.P)], ref, f32s, floor=R.VALUE_FLOOR)
    assert not bad, bad
    full = run_pair(ops, d, X.ACT_NONE, True)
    assert not torch.equal(full, y), "the precision switch did not reach the kernel"


# ------------------------------------------------------------------------------------------------ group 5: backward
@pytest.mark.parametrize("c", X.BWD_CASES, ids=lambda c: c.name)
def test_backward_data_against_float64(c, monkeypatch):
    """dx of autograd.conv (ACT_NONE): lldwt_conv3x3_f16x3 on dy with the transposed, flipped weight and one scale per plane from
    absmax_slots(dy), against the float64 adjoint conv under the gradient rule; the six-decade row ramp row by row."""
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import autograd as AG
    ops = _ops()
    d = X.conv_inputs(c)
    calls = []
    real = ops.conv3x3_f16x3
    monkeypatch.setattr(ops, "conv3x3_f16x3", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(c.planes, X.B, c.cin, *c.hw, generator=g) - 0.5).to(DEV).requires_grad_(True)
    w = d.w.to(DEV).requires_grad_(True)
    y = AG.conv(x, w, d.b.to(DEV), 3)
    y.backward(d.x.to(DEV))
    assert len(calls) == 2, "forward and backward-data did not run the split-fp16 kernel"
    bad = _check_conv(c, d, x.grad.cpu(), "dx", floor=R.GRAD_FLOOR)
    assert not bad, bad


@pytest.mark.parametrize("c", X.WGRAD_CASES, ids=lambda c: c.name)
def test_wgrad_against_float64(c):
    ops = _ops()
    d = X.conv_inputs(c)
    ref, f32s = X.conv_evaluate(c, d)
    x, dy = d.x.to(DEV), d.dy.to(DEV)
    shape = (c.planes, c.cout, c.cin, 3, 3)
    bad = []
    for tag, kw in (("slots computed", {}), ("slots given", dict(x_slots=ops.absmax_slots(x), dy_slots=ops.absmax_slots(dy)))):
        dw, db = ops.conv3x3_wgrad_f16x3(x, dy, shape, **kw)
        assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())
        bad += R.check("%s %s" % (c.name, tag), "dw", [dw[p].cpu() for p in range(c.planes)], ref, f32s, floor=R.GRAD_FLOOR)
        bad += R.check("%s %s" % (c.name, tag), "db", [db[p].cpu() for p in range(c.planes)], ref, f32s, floor=R.GRAD_FLOOR)
    assert not bad, bad
