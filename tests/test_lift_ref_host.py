"""CPU: tests/lift_ref.py (the float64 reference of the lifting kernels) against the unpatched fp32 oracle, the reference
project's own outputs under tests/golden/, and central differences.  Prints every yardstick (pytest -s)."""
import pytest
import torch

import lift_ref as R
from helpers import filled, load_golden
from oracle import lifting, model, weights

EPS32 = 2.0 ** -24


def _sds(K=5, planes=1, **kw):
    cfg = dict(model.DEFAULT_CFG, filtersize=K, dwtlevels=1, **kw)
    return cfg, [filled(weights.autoencoder_template(cfg), "lr%d." % p) for p in range(planes)]


def _rand(shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) - 0.5


@pytest.mark.parametrize("dtype", [R.F32, R.F64])
@pytest.mark.parametrize("K,linear", [(5, False), (3, False), (3, True)])
def test_step_restates_the_oracle_bit_for_bit(K, linear, dtype):
    """step() is skip_filter + p_block with the intermediates kept: same operations in the same order, so torch.equal."""
    cfg, (sd,) = _sds(K)
    sd = R.cast_sd(sd, dtype)
    src, dst = _rand((2, 1, 19, 45), 1).to(dtype), _rand((2, 1, 19, 45), 2).to(dtype)
    for sign in (1.0, -1.0):
        f = R.step(src, dst, R.tap_of(sd, 1), R.block_of(sd, "U_blocks.0."), sign, True, linear)
        skip = lifting.skip_filter(src, sd["preProcessingList.1.weight"])
        ref = dst + sign * (skip + lifting.p_block(skip, sd, "U_blocks.0.", 0 if linear else 1) * 0.1)
        assert torch.equal(f["out"], ref) and torch.equal(f["skip"], skip)
        # the other orientation is the same step on the transposed arrays
        ft = R.step(src.transpose(2, 3).contiguous(), dst.transpose(2, 3).contiguous(), R.tap_of(sd, 1),
                    R.block_of(sd, "U_blocks.0."), sign, False, linear)
        for k in R.STEP_KEYS:
            assert torch.equal(ft[k].transpose(2, 3), f[k]), k
    with R.oracle_tanh(torch.tanh):
        assert lifting.torch is torch
    with R.oracle_tanh(R.declared_tanh):
        assert lifting.torch is not torch
    assert lifting.torch is torch


def test_declared_tanh_is_tanh_to_fp32_rounding():
    """The formula the kernels declare, over the whole argument range (saturation and +-0 included): a few ulp of 1 from tanh in
    either dtype, odd, exactly +-1 once exp2 overflows, and its derivative is 1 - t^2."""
    x = torch.cat([torch.linspace(-30, 30, 20001, dtype=R.F64), torch.tensor([0.0, -0.0, 1e-30, 88.0, -200.0, 1e4], dtype=R.F64)])
    for dtype, tol in ((R.F64, 4 * 2.0 ** -53), (R.F32, 4 * EPS32)):
        t = R.declared_tanh(x.to(dtype))
        e = float((t.double() - torch.tanh(x)).abs().max())
        print("declared tanh in %s: max |t - tanh| = %.2e" % (dtype, e))
        assert e <= tol and bool(torch.isfinite(t).all())
        assert torch.equal(R.declared_tanh(-x.to(dtype)), -t)
    xg = torch.linspace(-4, 4, 101, dtype=R.F64).requires_grad_(True)
    (gr,) = torch.autograd.grad(R.declared_tanh(xg).sum(), xg)
    assert float((gr - (1 - torch.tanh(xg.detach()) ** 2)).abs().max()) < 1e-14


@pytest.mark.parametrize("hw", [(19, 45), (70, 150), (200, 250)])
def test_fp32_oracle_step_against_float64(hw):
    """What fp32 costs one step: every accumulation is at most 25 * 16 products of operands below 1 in magnitude, its result scaled
    by 0.1 into the output -- 16 ulp of the largest output bound the sum of all roundings with room to spare."""
    cfg, sds = _sds(5, 3)
    src, dst = _rand((3, 2, 1) + hw, 11), _rand((3, 2, 1) + hw, 12)

    def fn(p, dtype, tanh):
        sd = R.cast_sd(sds[p], dtype)
        return R.step(src[p].to(dtype), dst[p].to(dtype), R.tap_of(sd, 1), R.block_of(sd, "U_blocks.0."), 1.0, True, False,
                      tanh=tanh)
    ref, f32s = R.evaluate(fn, 3)
    for k in R.STEP_KEYS:
        y = R.yardstick(ref, f32s, k)
        plain = R.errors(f32s[0][k], ref[k])
        mx = max(float(t.abs().max()) for t in ref[k])
        print("step %-9s %-5s fp32 oracle %.2e  with the declared tanh %.2e  max|f64| %.3g" % (
            hw, k, max(map(float, plain)), max(map(float, y)), mx))
        assert max(map(float, y)) <= 16 * EPS32 * max(1.0, mx), k


def test_fp32_oracle_transform_against_float64():
    """L = 3 at 64 x 96: 12 chained steps per level pair of passes; the bound of one step per chained step."""
    cfg = dict(model.DEFAULT_CFG, filtersize=5, dwtlevels=3)
    sd = filled(weights.autoencoder_template(cfg), "lrT.")
    x = _rand((2, 1, 64, 96), 13)
    ref, f32s = R.evaluate(lambda p, dtype, tanh: R.transform(x.to(dtype), R.cast_sd(sd, dtype), cfg, tanh), 1)
    for k in ref:
        y = float(R.yardstick(ref, f32s, k)[0])
        mx = float(ref[k][0].abs().max())
        print("transform L=3 64x96 %-4s fp32 yardstick %.2e  max|f64| %.3g" % (k, y, mx))
        assert y <= 24 * 16 * EPS32 * max(1.0, mx), k
    assert float((ref["xr"][0] - x.double()).abs().max()) < 1e-13            # perfect reconstruction in float64


@pytest.mark.parametrize("name,lin", [("ref_pblock_k3", 1), ("ref_pblock_k5", 1), ("ref_pblock_linear", 0)])
def test_reference_projects_p_block(name, lin):
    """The reference project's own fp32 P_block output against the float64 evaluation: inside the value bar, like a kernel."""
    g = load_golden(name)
    k = 3 if "k3" in name or "linear" in name else 5
    tpl = {}
    for n, (co, ci) in zip(range(1, 5), [(16, 1), (16, 16), (16, 16), (1, 16)]):
        tpl["P_blocks.0.conv%d.weight" % n] = torch.zeros(co, ci, k, k)
        tpl["P_blocks.0.conv%d.bias" % n] = torch.zeros(co)
    sd = filled(tpl)

    def fn(p, dtype, tanh):
        with R.oracle_tanh(tanh):
            return {"y": lifting.p_block(g["x"].to(dtype), R.cast_sd(sd, dtype), "P_blocks.0.", lin)}
    ref, f32s = R.evaluate(fn, 1)
    assert not R.check(name, "y", [g["y"]], ref, f32s)


def test_reference_projects_skip_filters():
    g = load_golden("ref_skip_filters")
    sd = weights.autoencoder_template(dict(model.DEFAULT_CFG, dwtlevels=1))
    for j in range(4):
        w = sd["preProcessingList.%d.weight" % j]
        for n in ("imp", "ramp"):
            fn = lambda p, dtype, tanh: {"y": lifting.skip_filter(g[n].to(dtype), w.to(dtype))}
            ref, f32s = R.evaluate(fn, 1)
            assert not R.check("skip filter %d %s" % (j, n), "y", [g["%s%d" % (n, j)]], ref, f32s)


@pytest.mark.parametrize("name", ["ref_lifting_L2_k5", "ref_lifting_L3_k3_rect", "ref_lifting_L2_scale_berk",
                                  "ref_lifting_L2_different", "ref_lifting_L2_linear"])
def test_reference_projects_one_level(name):
    """One level forward and its inverse as the reference project computed them, against the oracle in float64."""
    g = load_golden(name)
    cfg = g["cfg"]
    sd = filled(weights.autoencoder_template(cfg))

    def fn(p, dtype, tanh):
        with R.oracle_tanh(tanh):
            s = R.cast_sd(sd, dtype)
            sub = lifting.one_level_forward(g["x"].to(dtype), s, cfg, 0)
            rec = lifting.one_level_inverse(*[g[n].to(dtype) for n in ("LL", "LH", "HL", "HH")], s, cfg, lifting._inv_off(cfg, 0))
        return dict(zip(("LL", "LH", "HL", "HH"), sub), rec1=rec)
    ref, f32s = R.evaluate(fn, 1)
    bad = []
    for k in ("LL", "LH", "HL", "HH", "rec1"):
        bad += R.check(name, k, [g[k]], ref, f32s)
    assert not bad, bad


def _directional(loss, params, grads, seed, eps=1e-6):
    """<grads, d> against (loss(p + eps d) - loss(p - eps d)) / 2 eps for one random direction d over all of `params`."""
    gen = torch.Generator().manual_seed(seed)
    d = {k: torch.rand(v.shape, generator=gen, dtype=R.F64) - 0.5 for k, v in params.items()}
    ana = sum(float((grads[k] * d[k]).sum()) for k in params)
    up = loss({k: v + eps * d[k] for k, v in params.items()})
    dn = loss({k: v - eps * d[k] for k, v in params.items()})
    return ana, (up - dn) / (2 * eps)


@pytest.mark.parametrize("vertical", [True, False])
@pytest.mark.parametrize("K,linear,tanh", [(5, False, torch.tanh), (5, False, R.declared_tanh), (3, False, torch.tanh),
                                           (3, True, torch.tanh)])
def test_step_gradients_against_central_differences(K, linear, tanh, vertical):
    """step_grads in float64: every input gradient through a directional central difference (step 1e-6: truncation ~1e-12,
    rounding ~1e-10 of the loss), and the chain tensors through the same difference on sum(net * g)."""
    cfg, (sd,) = _sds(K)
    sd = R.cast_sd(sd, R.F64)
    shp = (2, 1, 13, 21)
    src, dst, g = _rand(shp, 3).double(), _rand(shp, 4).double(), _rand(shp, 5).double()
    tap, blk = R.tap_of(sd, 0), R.block_of(sd, "P_blocks.0.")
    gr = R.step_grads(src, dst, tap, blk, g, -1.0, vertical, linear, tanh=tanh)
    assert torch.equal(gr["gdin"], g)
    params = dict(blk, src=src, dst=dst, tap=tap)
    grads = {k: gr["d" + k] for k in R.W_KEYS}
    grads.update(src=gr["gsrc"], dst=gr["gdin"], tap=gr["dtaps"])

    def loss(p):
        f = R.step(p["src"], p["dst"], p["tap"], {k: p[k] for k in R.W_KEYS}, -1.0, vertical, linear, tanh=tanh)
        return float((f["out"] * g).sum())
    for seed in (1, 2):
        ana, num = _directional(loss, params, grads, seed)
        print("step K=%d linear=%d vertical=%d: <grad, d> %.12g  central difference %.12g" % (K, linear, vertical, ana, num))
        assert abs(ana - num) <= 1e-7 * max(1.0, abs(ana))
    # chain: perturb the intermediate itself
    pad = K // 2
    f = R.step(src, dst, tap, blk, -1.0, True, linear, tanh=tanh) if vertical else None
    if vertical:
        import torch.nn.functional as F
        act = (lambda v: v) if linear else tanh
        tails = {"dt3": (f["t3"], lambda v: F.conv2d(v, blk["w4"], blk["b4"], padding=pad)),
                 "dpre2": (f["pre2"], lambda v: F.conv2d(F.conv2d(act(v), blk["w3"], blk["b3"], padding=pad) + f["r"],
                                                         blk["w4"], blk["b4"], padding=pad))}
        for k, (at, tail) in tails.items():
            ana, num = _directional(lambda p: float((tail(p["v"]) * g).sum()), {"v": at}, {"v": gr[k]}, 7)
            assert abs(ana - num) <= 1e-7 * max(1.0, abs(ana)), k


@pytest.mark.parametrize("K,prop,scale", [(5, "same", 0), (3, "different", 1)])
def test_transform_gradients_against_central_differences(K, prop, scale):
    cfg = dict(model.DEFAULT_CFG, filtersize=K, dwtlevels=2, block_property=prop, scale=scale)
    sd = R.cast_sd(filled(weights.autoencoder_template(cfg), "lrG."), R.F64)
    x = _rand((1, 1, 16, 24), 21).double()
    gen = torch.Generator().manual_seed(22)
    gouts = [torch.rand(1, 1, 4, 6, generator=gen, dtype=R.F64) - 0.5] + \
            [torch.rand(1, 3, 16 >> (i + 1), 24 >> (i + 1), generator=gen, dtype=R.F64) - 0.5 for i in range(2)]
    gx = torch.rand(1, 1, 16, 24, generator=gen, dtype=R.F64) - 0.5
    fwd, inv = R.transform_grads(x, sd, cfg, gouts, gx)

    def coeffs(p):
        ll, yh = lifting.lifting_forward(p["x"], {k: p.get(k, v) for k, v in sd.items()}, cfg)
        return [ll] + [t[:, 0] for t in yh]
    ana, num = _directional(lambda p: sum(float((o * g_).sum()) for o, g_ in zip(coeffs(p), gouts)),
                            dict({k: sd[k] for k in fwd if k != "x"}, x=x), fwd, 3)
    print("forward L=2 K=%d %s scale=%d: <grad, d> %.12g  central difference %.12g" % (K, prop, scale, ana, num))
    assert abs(ana - num) <= 1e-7 * max(1.0, abs(ana))
    c0 = [c.detach() for c in coeffs({"x": x})]
    names = ["ll", "yh0", "yh1"]

    def inv_loss(p):
        c = [p[n] for n in names]
        xr = lifting.lifting_inverse(c[0], [t.unsqueeze(1) for t in c[1:]], {k: p.get(k, v) for k, v in sd.items()}, cfg)
        return float((xr * gx).sum())
    params = dict({k: sd[k] for k in inv if k not in names}, **dict(zip(names, c0)))
    ana, num = _directional(inv_loss, params, inv, 4)
    print("inverse L=2 K=%d %s scale=%d: <grad, d> %.12g  central difference %.12g" % (K, prop, scale, ana, num))
    assert abs(ana - num) <= 1e-7 * max(1.0, abs(ana))
