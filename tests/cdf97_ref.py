"""float64 reference for the fixed CDF 9/7 kernels (csrc/cdf97.hip) and their adjoints: the yardstick of
tests/test_cdf97_ref_host.py and tests/test_gpu_cdf97_domain.py.  No device code.

Reference.  oracle.cdf97.dwt_forward / dwt_inverse with periodic=True in float64: the formula of the kernel file's header at
every length, dtype-generic and differentiable.  Adjoints are float64 autograd through it (A^T g is the gradient of
sum(g * A(x)) with respect to x; the inverse likewise): there is no second hand-written formula here.

Yardstick.  The same oracle in fp32 on the same inputs, the larger error of two forms: periodic=True and, where every level
input has 10 or more samples, the conv form periodic=False, which sums in another order.

Bar, per plane (one H x W image of the Z = P * B * C a call holds) and per output tensor (ll, and LH / HL / HH of every level,
separately), no element left out:
    |kernel - f64| <= 4 * yardstick + floor * max(max|f64 of that tensor|, max|input of that plane|)
    floor = 2e-7 for values, 5e-7 for adjoints / gradients                          (lift_ref.VALUE_FLOOR, GRAD_FLOOR)
The second argument of the max: on a constant or checkerboard plane a detail band cancels to about 1e-12 in float64 while an
honest fp32 evaluation leaves rounding noise of the size of the terms that cancel, so max|f64| alone is a bar no fp32 kernel
can meet.  For the inverse the plane's input is the largest magnitude over all its coefficient tensors.

Tensors travel as dicts of (Z, h, w) arrays: 'll', 'lh0', 'hl0', 'hh0', 'lh1', ... (finest level first) for coefficients,
'x' for an image.

expected_kernel restates the dispatch of lldwt_cdf97_forward / lldwt_cdf97_inverse for one level."""
import contextlib

import torch

import lift_ref as R
from oracle import cdf97

F64, F32 = torch.float64, torch.float32
FACTOR, VALUE_FLOOR, GRAD_FLOOR = 4.0, R.VALUE_FLOOR, R.GRAD_FLOOR
BANDS = ("lh", "hl", "hh")


# ------------------------------------------------------------------------------------------------ layouts
def coeff_keys(levels):
    return ["ll"] + [b + str(i) for i in range(levels) for b in BANDS]


def levels_of(co):
    return (len(co) - 1) // 3


def to_dict(ll, yh):
    """ll (..., h, w), yh_i (..., 3, h_i, w_i), as the oracle or ops.cdf97_forward return them -> dict of (Z, h, w)."""
    out = {"ll": ll.reshape(-1, *ll.shape[-2:])}
    for i, t in enumerate(yh):
        t = t.reshape(-1, 3, *t.shape[-2:])
        for j, b in enumerate(BANDS):
            out[b + str(i)] = t[:, j]
    return out


def from_dict(co, lead=None):
    """dict of (Z, h, w) -> (ll (*lead, h, w), [yh_i (*lead, 3, h_i, w_i)]); lead defaults to (Z, 1), the oracle's (B, C)."""
    lead = tuple(lead) if lead is not None else (co["ll"].shape[0], 1)
    ll = co["ll"].reshape(*lead, *co["ll"].shape[-2:])
    yh = []
    for i in range(levels_of(co)):
        t = torch.stack([co[b + str(i)] for b in BANDS], 1)
        yh.append(t.reshape(*lead, 3, *t.shape[-2:]))
    return ll, yh


def cast(d, dtype):
    return {k: v.to(dtype) for k, v in d.items()}


def conv_form_applies(H, W, levels):
    """Every level input has 10 or more samples on both sides: the oracle's conv form is then the same transform."""
    return (min(H, W) >> (levels - 1)) >= 10


def level_inputs(H, W, levels):
    return [(H >> i, W >> i) for i in range(levels)]


# ------------------------------------------------------------------------------------------------ the transform
def analysis(x, levels, dtype, periodic=True):
    """x (..., H, W) -> coefficient dict in `dtype`."""
    x = x.reshape(-1, 1, *x.shape[-2:]).to(dtype)
    return to_dict(*cdf97.dwt_forward(x, levels, periodic=periodic))


def synthesis(co, dtype, periodic=True):
    """coefficient dict -> {'x': (Z, H, W)} in `dtype`."""
    ll, yh = from_dict(cast(co, dtype))
    return {"x": cdf97.dwt_inverse(ll, yh, periodic=periodic)[:, 0]}


def analysis_adjoint(g, dtype, periodic=True):
    """A^T g for a coefficient-shaped dict g -> {'x': (Z, H, W)}: autograd of sum(g * A(x))."""
    levels = levels_of(g)
    Z, h, w = g["ll"].shape
    x = torch.zeros(Z, h << levels, w << levels, dtype=dtype, requires_grad=True)
    out = analysis(x, levels, dtype, periodic)
    loss = sum((out[k] * g[k].to(dtype)).sum() for k in out)
    return {"x": torch.autograd.grad(loss, x)[0]}


def synthesis_adjoint(gx, levels, dtype, periodic=True):
    """S^T gx for an image-shaped gx (Z, H, W) -> coefficient dict: autograd of sum(gx * S(c))."""
    Z, H, W = gx.shape
    co = {"ll": torch.zeros(Z, H >> levels, W >> levels, dtype=dtype, requires_grad=True)}
    for i in range(levels):
        for b in BANDS:
            co[b + str(i)] = torch.zeros(Z, H >> (i + 1), W >> (i + 1), dtype=dtype, requires_grad=True)
    loss = (synthesis(co, dtype, periodic)["x"] * gx.to(dtype)).sum()
    return dict(zip(co, torch.autograd.grad(loss, list(co.values()))))


@contextlib.contextmanager
def perturbed_taps(table, index, factor):
    """oracle.cdf97 with tap `index` of filter `table` ('DEC_LO', ...) multiplied by `factor` for the duration (both forms
    read the module-level lists when they are called)."""
    saved = getattr(cdf97, table)
    taps = list(saved)
    taps[index] = taps[index] * factor
    setattr(cdf97, table, taps)
    try:
        yield
    finally:
        setattr(cdf97, table, saved)


# ------------------------------------------------------------------------------------------------ reference + yardstick
def evaluate(fn, conv):
    """fn(dtype, periodic) -> dict of (Z, ...) tensors.  -> (ref, f32s): the float64 periodic evaluation and the list of the
    fp32 evaluations that make the yardstick (periodic; the conv form too if `conv`)."""
    det = lambda d: {k: v.detach() for k, v in d.items()}
    f32s = [det(fn(F32, True))]
    if conv:
        f32s.append(det(fn(F32, False)))
    return det(fn(F64, True)), f32s


def plane_max(t):
    """(Z, ...) -> (Z,) float64 max |t| per plane."""
    return t.detach().double().abs().flatten(1).amax(1)


def input_max(d):
    """Per plane, the largest magnitude over all tensors of a dict (the coefficient tensors of an inverse's input)."""
    return torch.stack([plane_max(v) for v in d.values()]).amax(0)


def check(tag, got, ref, f32s, inmax, floor=VALUE_FLOOR, stats=None):
    """The bar for every tensor of `ref` on every plane.  got: dict like ref (any float dtype, CPU); inmax: (Z,) max|input|.
    Prints, per tensor, the plane closest to (or furthest past) its bar.  -> list of (tag, key, plane, error, yardstick, bar)
    for the planes outside; stats (a dict) collects the worst (error / bar, error, yardstick, bar) per tag prefix."""
    bad = []
    for key in ref:
        assert got[key].shape == ref[key].shape, (tag, key, got[key].shape, ref[key].shape)
        err = torch.stack([torch.as_tensor(e) for e in R.errors(got[key].detach().cpu(), ref[key])])
        yard = torch.stack(R.yardstick(ref, f32s, key))
        bar = FACTOR * yard + floor * torch.maximum(plane_max(ref[key]), inmax)
        ok = err <= bar                                                       # NaN (an element no lane wrote) is not <=
        ratio = torch.where(ok, err / bar.clamp_min(1e-300), torch.full_like(err, float("inf")))
        p = int(torch.argmax(ratio))
        print("%-64s %-4s kernel %.2e  yardstick %.2e  bar %.2e  (plane %d)" % (tag, key, float(err[p]), float(yard[p]),
                                                                             float(bar[p]), p))
        if stats is not None:
            name = tag.split(" ")[0]
            if name not in stats or float(ratio[p]) > stats[name][0]:
                stats[name] = (float(ratio[p]), float(err[p]), float(yard[p]), float(bar[p]), tag, key)
        bad += [(tag, key, int(q), float(err[q]), float(yard[q]), float(bar[q])) for q in torch.nonzero(~ok).flatten()]
    return bad


# ------------------------------------------------------------------------------------------------ dispatch
CT = 32                                                                       # csrc/cdf97.hip: subband tile edge
KERNELS = ("afb/sfb", "fwd_level[mod]", "fwd_level[wrap]", "fwd_v<8,32>", "fwd_v<16,32>", "fwd_v<32,32>", "inv_level",
           "inv_v<16,32>", "inv_v<32,32>")


def _cdiv(a, b):
    return -(-a // b)


def square_tiles(Z, h, w):
    """The tile count both directions dispatch on: 32 x 32 subband tiles (64 x 64 pixels) of one h x w level over Z planes."""
    return _cdiv(w // 2, CT) * _cdiv(h // 2, CT) * Z


def expected_kernel(direction, adj, Z, h, w):
    """The launch lldwt_cdf97_forward (direction 'forward': h x w is the level's input) or lldwt_cdf97_inverse ('inverse':
    h x w is the level's output) makes for one level of Z planes, restated from their bodies (rows are contiguous there)."""
    assert direction in ("forward", "inverse")
    if adj:
        return "afb/sfb"                                                      # three k_afb (forward) / k_sfb (inverse) launches
    tiles = square_tiles(Z, h, w)
    hh, wh = h // 2, w // 2
    if direction == "forward":
        if h >= 2 * CT and w >= 2 * CT and w % 4 == 0:
            return "fwd_v<32,32>" if tiles >= 4096 else "fwd_v<8,32>" if tiles < 200 else "fwd_v<16,32>"
        return "fwd_level[mod]" if (h < 2 * CT + 8 or w < 2 * CT + 8) else "fwd_level[wrap]"
    if hh >= CT and wh >= CT and wh % 2 == 0:
        return "inv_v<32,32>" if tiles >= 4096 else "inv_v<16,32>"
    return "inv_level"
