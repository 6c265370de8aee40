"""CPU: proves the float64 conv reference (tests/conv_ref.py) and the inputs of the GPU tables of tests/test_gpu_conv_domain.py
and tests/test_gpu_wgrad_domain.py.

  * the reference equals F.conv2d / F.conv_transpose2d / torch autograd in float64 to 1e-12 of the output scale, for every
    descriptor field alone and for every row of the GPU tables (torch_forward below is built from those torch calls only and
    shares no code with the reference);
  * on every integer row an fp32 torch evaluation equals the float64 one bit for bit and stays below 2^24;
  * planted faults (conv_ref.FAULTS): for every row and image, each fault that applies -- that changes the operator on generic
    real inputs of the row's shapes -- is rejected on the row's own inputs: torch.equal fails on the integer rows, the bar is
    exceeded on the float rows.  Printed per row (pytest -s): which faults applied and that each was rejected."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as CR
import lift_ref as R
import test_gpu_conv_domain as TC
import test_gpu_wgrad_domain as TW

P, B = 2, 2
F64 = torch.float64
FWD_FAULTS = [f for f in CR.FAULTS if f not in ("bias_x", "batch_drop")]
WG_FAULTS = [f for f in CR.FAULTS if f != "epi_after"]


# ------------------------------------------------------------------------------------------------ torch's own statement
def torch_lin(c, x, w):
    """conv(x) of one plane from torch calls alone: x (B,xtot,hi,wi), w as handed in -> (B,cout,h,w)."""
    if c.ic_block:
        x = torch.stack([x[:, (i // c.ic_block) * c.ic_stride + c.ic_off + i % c.ic_block] for i in range(c.cin)], dim=1)
    if c.ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    if c.swap:
        w = w.transpose(-1, -2)
    m = torch.tensor([float((c.mask >> t) & 1) for t in range(c.K * c.K)], dtype=x.dtype).view(c.K, c.K)
    if c.transposed:                      # the mask names the taps of the operator, which are the flipped taps of the weight
        return F.conv_transpose2d(x, w * m.flip(0, 1), None, padding=c.K // 2, groups=c.groups)
    return F.conv2d(x, w * m, None, padding=c.K // 2, groups=c.groups)


def torch_forward(c, x, w, b, res, aux, out0):
    v = torch_lin(c, x, w)
    out = out0.clone()
    for oc in range(c.cout):
        ocp = (oc // c.oc_block) * c.oc_stride + c.oc_off + oc % c.oc_block
        t = v[:, oc] + (b[oc] if b is not None else 0)
        if c.epi:
            a = aux[:, ocp]
            t = t * ((1 - a * a) if c.epi == CR.EPI_TANH_BWD else torch.where(a > 0, torch.ones_like(a), torch.full_like(a, 0.01)))
        if res is not None:
            t = t + res[:, ocp]
        if c.act == CR.ACT_TANH:
            t = torch.tanh(t)
        elif c.act == CR.ACT_LRELU:
            t = F.leaky_relu(t, 0.01)
        elif c.act == CR.ACT_RELU:
            t = F.relu(t)
        out[:, ocp] = t
    return out


def torch_wgrad(c, x, dy, alpha):
    """dw / dbias of one plane by autograd of torch_lin with respect to the weight in its handed-in layout."""
    w = torch.zeros(c.cout, c.cin_g, c.K, c.K, dtype=x.dtype, requires_grad=True)
    b = torch.zeros(c.cout, dtype=x.dtype, requires_grad=True)
    y = torch_lin(c, x, w) + b.view(1, -1, 1, 1)
    g = torch.stack([dy[:, (oc // c.oc_block) * c.oc_stride + c.oc_off + oc % c.oc_block] for oc in range(c.cout)], dim=1)
    dw, db = torch.autograd.grad((y * g).sum(), [w, b])
    return alpha * dw, alpha * db


def _plane(d, p, dt=F64):
    opt = lambda t: None if t is None else t[p].to(dt)
    return d.x[p].to(dt), d.w[p].to(dt), opt(d.bias), opt(d.res), opt(d.aux), d.out0[p].to(dt)


FIELDS = [
    CR.case("plain", 5, 7, 3), CR.case("k1", 6, 4, 1), CR.case("k5", 3, 5, 5), CR.case("groups", 6, 9, 3, groups=3),
    CR.case("ups", 3, 4, 3, ups=True), CR.case("transposed", 5, 7, 3, transposed=True),
    CR.case("transposed-groups", 6, 9, 5, groups=3, transposed=True), CR.case("mask", 4, 5, 3, mask=TC.mask_bits(3, "A")),
    CR.case("mask-asym-transposed", 4, 5, 3, mask=TC.mask_bits(3, "asym"), transposed=True), CR.case("swap", 4, 5, 5, swap=True),
    CR.case("swap-mask", 4, 5, 3, swap=True, mask=TC.mask_bits(3, "asym")), CR.case("oplace", 4, 6, 3, op=(2, 3, 1, 10)),
    CR.case("iplace", 6, 4, 3, ip=(2, 3, 1, 10)), CR.case("res", 4, 5, 3, res=True), CR.case("nobias", 4, 5, 3, bias=False),
    CR.case("tanh", 4, 5, 3, act=CR.ACT_TANH), CR.case("lrelu", 4, 5, 3, act=CR.ACT_LRELU), CR.case("relu", 4, 5, 3, act=CR.ACT_RELU),
    CR.case("epi-tanh", 4, 5, 3, epi=CR.EPI_TANH_BWD, res=True), CR.case("epi-lrelu", 4, 5, 3, epi=CR.EPI_LRELU_BWD),
]


def _close(a, b):
    return float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("c", FIELDS + TC.INT_CASES + TC.FLOAT_CASES, ids=lambda c: c.name)
def test_forward_reference_equals_torch(c):
    hw = (6, 8) if c.hw is None and c in FIELDS else CR.geometries(c)[-1]
    cc = CR.at(c, hw)
    d = CR.inputs(cc, P, B, generic=True)
    for p in range(P):
        x, w, b, res, aux, out0 = _plane(d, p)
        assert _close(CR.forward(x, w, b, cc, res, aux, out0), torch_forward(cc, x, w, b, res, aux, out0))
        assert _close(CR.forward(x, w, b, cc, res, aux, out0, lin=CR.conv_lin_torch), torch_forward(cc, x, w, b, res, aux, out0))


WG_FIELDS = [c for c in FIELDS if not c.transposed and not c.epi and not c.res and c.act == CR.ACT_NONE]


@pytest.mark.parametrize("c", WG_FIELDS + [c for _, c in TW.ROWS + TW.FLOAT_ROWS], ids=lambda c: c.name)
def test_wgrad_reference_equals_torch(c):
    hw = c.hw or ((6, 8) if c in WG_FIELDS else TW.geos(c)[-2])
    cc = CR.at(c, hw)
    d = CR.inputs(cc, P, B, generic=True)
    x, dy = d.x[0], d.dy[0]
    tw, tb = torch_wgrad(cc, x, dy, cc.alpha)
    z = torch.zeros(c.cout, c.cin_g, c.K, c.K, dtype=F64)
    for fn in (lambda: CR.wgrad(x, dy, cc, z, torch.zeros(c.cout, dtype=F64), cc.alpha, cc.swap),
               lambda: CR.wgrad_torch(x, dy, cc, cc.alpha, cc.swap)):
        dw, db = fn()
        assert _close(dw, tw) and _close(db, tb)


def test_helpers_equal_torch():
    g = torch.Generator().manual_seed(3)
    t = torch.randn(2, 3, 6, 8, generator=g, dtype=F64)
    assert _close(CR.downsum2(t), F.avg_pool2d(t, 2) * 4)
    for act, fn in ((CR.ACT_TANH, torch.tanh), (CR.ACT_LRELU, lambda v: F.leaky_relu(v, 0.01)), (CR.ACT_RELU, F.relu), (CR.ACT_NONE, lambda v: v)):
        v = torch.randn(50, generator=g, dtype=F64).requires_grad_(True)
        dy = torch.randn(50, generator=g, dtype=F64)
        y = fn(v)
        assert _close(CR.act_bwd(dy, y.detach(), act), torch.autograd.grad((y * dy).sum(), v)[0])


def test_plan_and_dispatch_tables():
    TC.test_plan_table()
    TW.test_dispatch_table()


# ------------------------------------------------------------------------------------------------ integer rows are exact
@pytest.mark.parametrize("c", TC.INT_CASES, ids=lambda c: c.name)
def test_forward_integer_rows_exact_in_fp32(c):
    for hw in CR.geometries(c):
        cc = CR.at(c, hw)
        d = CR.inputs(cc, P, B)
        for p in range(P):
            ref = CR.forward(*_plane(d, p)[:2], _plane(d, p)[2], cc, *_plane(d, p)[3:])
            f32 = CR.forward(*_plane(d, p, torch.float32)[:2], _plane(d, p, torch.float32)[2], cc, *_plane(d, p, torch.float32)[3:],
                             lin=CR.conv_lin_torch)
            assert float(ref.abs().max()) < 2 ** 24 and torch.equal(f32.double(), ref) and bool(torch.isfinite(ref).all())


@pytest.mark.parametrize("c", [c for _, c in TW.ROWS], ids=lambda c: c.name)
def test_wgrad_integer_rows_exact_in_fp32(c):
    hw = TW.geos(c)[-1]
    cc = CR.at(c, hw)
    d = CR.inputs(cc, P, B)
    rw, rb = CR.wgrad(d.x[0].double(), d.dy[0].double(), cc, d.dw0[0].double(), d.db0[0].double(), cc.alpha, cc.swap)
    fw, fb = CR.wgrad_torch(d.x[0], d.dy[0], cc, cc.alpha, cc.swap)
    assert float(rw.abs().max()) < 2 ** 24 and bool(torch.isfinite(rw).all())
    assert torch.equal((d.dw0[0] + fw).double(), rw) and torch.equal((d.db0[0] + fb).double(), rb)


# ------------------------------------------------------------------------------------------------ planted faults
_applied = {}


def _inert(c, f, wgrad):
    """Faults whose code path the case cannot reach (the probe is skipped for these only)."""
    nblk_o, nblk_i = -(-c.cout // c.oc_block), (-(-c.cin // c.ic_block) if c.ic_block else 1)
    return ((f in ("khkw", "halo_edge") and c.K == 1) or (f == "ups_round" and not c.ups) or (f == "dead_live" and c.ntaps == c.K * c.K) or
            (f == "epi_after" and not (c.epi and c.res)) or (f == "chunk_drop" and c.cin_g % CR.plan(c)[4] == 0) or
            (f == "place_block" and nblk_o <= 1 and nblk_i <= 1) or (f == "bias_x" and not c.want_bias) or
            (f == "oc_neighbour" and (c.cout_g == 1 or c.cout_g % (16 if wgrad else CR.plan(c)[1]) == 0)))


def _differs(a, b):
    return float((a - b).abs().max()) > 1e-9 * max(1.0, float(b.abs().max()))


def _fwd_faults(c, hw):
    cc = CR.at(c, hw)
    gen = CR.inputs(cc, 1, B, generic=True)
    gx = _plane(gen, 0)
    clean = CR.forward(gx[0], gx[1], gx[2], cc, gx[3], gx[4], gx[5], act=False)
    d = CR.inputs(cc, P, B)
    if c.kind == "int":
        refs = [CR.forward(*_plane(d, p)[:3], cc, *_plane(d, p)[3:]) for p in range(P)]
        bar = [0.0] * P
    else:
        ref, f32s = CR.forward_evaluate(cc, d, P)
        refs, bar = ref["y"], CR.bars(ref, f32s, "y", R.VALUE_FLOOR)
    applied = []
    for f in FWD_FAULTS:
        if _inert(c, f, False) or not _differs(CR.forward(gx[0], gx[1], gx[2], cc, gx[3], gx[4], gx[5], fault=f, act=False), clean):
            continue
        applied.append(f)
        rejected = False
        for p in range(P):
            a = _plane(d, p)
            bad = CR.forward(a[0], a[1], a[2], cc, a[3], a[4], a[5], fault=f)
            rejected |= (not torch.equal(bad, refs[p])) if c.kind == "int" else float((bad - refs[p]).abs().max()) > bar[p]
        assert rejected, "%s %s: the inputs do not reject the planted fault %s" % (c.name, hw, f)
    return applied


@pytest.mark.parametrize("c", TC.INT_CASES + TC.FLOAT_CASES, ids=lambda c: c.name)
def test_forward_rows_reject_planted_faults(c):
    for hw in CR.geometries(c):
        applied = _fwd_faults(c, hw)
        _applied.setdefault("fwd", set()).update(applied)
        print("%-44s %-8s applied and rejected: %s" % (c.name, hw, " ".join(applied) or "-"))


def _wg_faults(c, hw):
    cc = CR.at(c, hw)
    gen = CR.inputs(cc, 1, B, generic=True)
    zb = lambda dt: torch.zeros(c.cout, dtype=dt) if c.want_bias else None
    z = torch.zeros(c.cout, c.cin_g, c.K, c.K, dtype=F64)
    clean = CR.wgrad(gen.x[0], gen.dy[0], cc, z, zb(F64), cc.alpha, cc.swap)
    d = CR.inputs(cc, P, B)
    pl = lambda p: (d.x[p].double(), d.dy[p].double(), cc, d.dw0[p].double(), d.db0[p].double() if c.want_bias else None, cc.alpha, cc.swap)
    if c.kind == "int":
        refs = [CR.wgrad(*pl(p)) for p in range(P)]
    else:
        ref, f32s = CR.wgrad_evaluate(cc, d, P)
        refs = [(ref["dw"][p], ref["db"][p] if c.want_bias else None) for p in range(P)]
        bw, bb = CR.bars(ref, f32s, "dw", R.GRAD_FLOOR), (CR.bars(ref, f32s, "db", R.GRAD_FLOOR) if c.want_bias else None)
    applied = []
    for f in WG_FAULTS:
        if _inert(c, f, True):
            continue
        bad = CR.wgrad(gen.x[0], gen.dy[0], cc, z, zb(F64), cc.alpha, cc.swap, fault=f)
        if not (_differs(bad[0], clean[0]) or (c.want_bias and _differs(bad[1], clean[1]))):
            continue
        applied.append(f)
        rejected = False
        for p in range(P):
            bw_, bb_ = CR.wgrad(*pl(p), fault=f)
            if c.kind == "int":
                rejected |= not torch.equal(bw_, refs[p][0]) or (c.want_bias and not torch.equal(bb_, refs[p][1]))
            else:
                rejected |= float((bw_ - refs[p][0]).abs().max()) > bw[p] or (c.want_bias and float((bb_ - refs[p][1]).abs().max()) > bb[p])
        assert rejected, "%s %s: the inputs do not reject the planted fault %s" % (c.name, hw, f)
    return applied


@pytest.mark.parametrize("c", [c for _, c in TW.ROWS + TW.FLOAT_ROWS], ids=lambda c: c.name)
def test_wgrad_rows_reject_planted_faults(c):
    for hw in ([c.hw] if c.hw else TW.geos(c)):
        applied = _wg_faults(c, hw)
        _applied.setdefault("wg", set()).update(applied)
        print("%-24s %-8s applied and rejected: %s" % (c.name, hw, " ".join(applied) or "-"))


def test_every_fault_applied_somewhere():
    """No planted fault is vacuous over the tables (collected by the two tests above; run alone, it walks the tables itself)."""
    if "fwd" not in _applied:
        for c in TC.INT_CASES + TC.FLOAT_CASES:
            _applied.setdefault("fwd", set()).update(_fwd_faults(c, CR.geometries(c)[-1]))
    if "wg" not in _applied:
        for _, c in TW.ROWS + TW.FLOAT_ROWS:
            _applied.setdefault("wg", set()).update(_wg_faults(c, c.hw or TW.geos(c)[-1]))
    assert _applied["fwd"] == set(FWD_FAULTS), set(FWD_FAULTS) - _applied["fwd"]
    assert _applied["wg"] == set(WG_FAULTS), set(WG_FAULTS) - _applied["wg"]
