"""float64 reference for the general conv layer (lldwt_conv_desc) and its weight gradients: the yardstick of
tests/test_conv_ref_host.py, tests/test_gpu_conv_domain.py and tests/test_gpu_wgrad_domain.py.  No device code.

Reference.  A plain torch statement of the comment block of include/lldwt.h, per plane and in the dtype of its arguments:
    y[b, oc'] = act((sum_{ic, live tap} W[oc, ic, tap] x[b, ic', . + tap - K/2] + bias[oc]) * epi(aux[b, oc']) + residual[b, oc'])
    dw[oc, ic, tap] += alpha sum_{b, p} dy[b, oc', p] x[b, ic', p + tap - K/2],   dbias[oc] += alpha sum_{b, p} dy[b, oc', p]
with oc' / ic' the output / input placement, x read through the nearest 2x upsampling when upsample2, W the weight handed in
(ConvTranspose2d layout with flipped taps when transposed, (kh, kw)-transposed when swap_hw), dead taps of tap_mask skipped
whatever the weight holds there.  Both are written as the contraction itself, one einsum per live tap over shifted views of the
zero-padded input; the host test pins them to F.conv2d / F.conv_transpose2d / torch autograd in float64.

Yardstick (the pattern of tests/lift_ref.py, whose evaluate / yardstick / check / declared_tanh are used as they are): per plane
and per tensor the largest error against float64 of these fp32 evaluations on the same inputs
  1. torch fp32 (F.conv2d, autograd for the gradients) with torch.tanh and with the kernels' declared tanh;
  2. one sequential fp32 chain in the engine's declared accumulation order.  Forward (csrc/conv_mfma.hip): chunks of CK input
     channels, tap-major inside a chunk, then channel, one accumulator per output, bias added last.  Weight gradient
     (csrc/conv_bwd.hip): one accumulator per dW element over the pixels in the order of the 8 x 16 chunks (32-pixel segments
     for k_wgrad1x1), chunk q in slice q % S for a few fixed slice counts S, the slices' partial sums added at the end as the
     atomics do.  torch's blocked conv sums in a tree and is several times closer to float64 than any single chain is, so a bar
     built on leg 1 alone would fail a correct fmaf chain; the chain here rounds product and sum separately where the matrix
     core rounds once, so it bounds the kernel from above.
Bars are lift_ref's: values 4 * yardstick + 2e-7 * max|f64|, gradients 4 * yardstick + 5e-7 * max|f64|, per plane and tensor.

Planted faults (FAULTS): the reference evaluated with one deliberate mistake of the kind a kernel can make.  A fault APPLIES to a
case when it changes the operator on generic real inputs of the case's shapes (no activation); the host test asserts that every
applicable fault is rejected on the case's own inputs -- the condition that keeps a symmetric or degenerate input from hiding it."""
import types
import zlib

import torch
import torch.nn.functional as F

import lift_ref as R

F64, F32 = torch.float64, torch.float32
ACT_NONE, ACT_TANH, ACT_LRELU, ACT_RELU = 0, 1, 2, 3
EPI_NONE, EPI_TANH_BWD, EPI_LRELU_BWD = 0, 1, 2
SENTINEL = -777.25

FAULTS = ("tap_col", "tap_row", "khkw", "chunk_drop", "oc_neighbour", "halo_edge", "ups_round", "place_block", "dead_live",
          "bias_x", "batch_drop", "epi_after")


# ------------------------------------------------------------------------------------------------ cases
def case(name, cin, cout, K, groups=1, act=ACT_NONE, ups=False, transposed=False, mask=None, swap=False, op=None, ip=None,
         epi=EPI_NONE, bias=True, res=False, kind="int", alpha=1.0, hw=None, acc=False, want_bias=None):
    """One descriptor.  op = (oc_block, oc_stride, oc_off, ytot) or None (dense); ip = (ic_block, ic_stride, ic_off, xtot) or None.
    mask: live-tap bits (None = dense).  kind: 'int' (exact) or 'float'.  alpha / acc (accumulate into non-zero dw) / want_bias
    belong to the weight-gradient cases, hw is the output size (h, w) where the table fixes one."""
    full = (1 << (K * K)) - 1
    c = types.SimpleNamespace(name=name, cin=cin, cout=cout, K=K, groups=groups, act=act, ups=bool(ups), transposed=bool(transposed),
                              mask=full if mask is None else mask & full, swap=bool(swap), epi=epi, bias=bool(bias), res=bool(res),
                              kind=kind, alpha=alpha, hw=hw, acc=bool(acc), want_bias=bool(bias) if want_bias is None else want_bias)
    c.oc_block, c.oc_stride, c.oc_off, c.ytot = op if op is not None else (cout, 0, 0, cout)
    c.ic_block, c.ic_stride, c.ic_off, c.xtot = ip if ip is not None else (0, 0, 0, cin)
    c.cin_g, c.cout_g = cin // groups, cout // groups
    c.taps = [(t // K, t % K) for t in range(K * K) if (c.mask >> t) & 1]
    c.ntaps = len(c.taps)
    return c


def at(c, hw):
    """The case at output size hw."""
    d = types.SimpleNamespace(**vars(c))
    d.hw = tuple(hw)
    return d


def placed(n, blk, stride, off):
    """Memory channel of logical channels 0 .. n-1 under a block placement."""
    i = torch.arange(n)
    return (i // blk) * stride + off + i % blk


def oc_index(c, fault=None):
    idx = placed(c.cout, c.oc_block, c.oc_stride, c.oc_off)
    nblk = -(-c.cout // c.oc_block)
    if fault == "place_block" and nblk > 1:                                   # every block lands where its successor belongs
        i = torch.arange(c.cout)
        idx = ((i // c.oc_block + 1) % nblk) * c.oc_stride + c.oc_off + i % c.oc_block
    return idx


def ic_index(c, fault=None):
    if not c.ic_block:
        return torch.arange(c.cin)
    nblk = -(-c.cin // c.ic_block)
    if fault == "place_block" and -(-c.cout // c.oc_block) <= 1 and nblk > 1:
        i = torch.arange(c.cin)
        return ((i // c.ic_block + 1) % nblk) * c.ic_stride + c.ic_off + i % c.ic_block
    return placed(c.cin, c.ic_block, c.ic_stride, c.ic_off)


# ------------------------------------------------------------------------------------------------ the engine's plan (documented rule)
OC_BLOCKS = (16, 32, 64, 96, 128)
OC_EFF = (0.6, 0.75, 0.9, 1.0, 1.0)


def plan(c):
    """csrc/conv_mfma.hip make_plan / launch_ks as their comments state them: the oc block with the least padded channels per unit
    of efficiency (ties to the larger block); pixel tile 16 x 32 for the 16-block, 8 x 32 for 32 / 64, 8 x 16 for 96 / 128 except
    the 128-block at K = 3 (8 x 32); chunks of 32 input channels at K = 1, else 4 when cin_g <= 4, else 8.
    -> (cfg, oc block, TH, TW, CK, dense)."""
    best, cost = 0, 1e30
    for i, (blk, eff) in enumerate(zip(OC_BLOCKS, OC_EFF)):
        k = -(-c.cout_g // blk) * blk / eff
        if k <= cost:
            best, cost = i, k
    th, tw = ((16, 32), (8, 32), (8, 32), (8, 16), (8, 32) if c.K == 3 else (8, 16))[best]
    ck = 32 if c.K == 1 else (4 if c.cin_g <= 4 else 8)
    return best, OC_BLOCKS[best], th, tw, ck, c.ntaps == c.K * c.K


def geometries(c):
    """The five images of a case: 1 x 1, one row / one column one pixel past the tile, one tile, one pixel past it both ways
    (their even neighbours with upsample2)."""
    _, _, th, tw, _, _ = plan(c)
    if c.ups:
        return [(2, 2), (2, tw + 2), (th + 2, 2), (th, tw), (th + 2, tw + 2)]
    return [(1, 1), (1, tw + 1), (th + 1, 1), (th, tw), (th + 1, tw + 1)]


# ------------------------------------------------------------------------------------------------ inputs
def _gen(c, salt=""):
    return torch.Generator().manual_seed(zlib.crc32(("%s|%s|%s" % (c.name, c.hw, salt)).encode()))


def _ints(shape, lo, hi, g):
    """Integers of magnitude lo .. hi with random sign (no zero: a zero would hide a misplaced tap)."""
    v = torch.randint(lo, hi + 1, shape, generator=g).float()
    s = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return v * s


def w_shape(c, P):
    return (P, c.cin, c.cout_g, c.K, c.K) if c.transposed else (P, c.cout, c.cin_g, c.K, c.K)


def inputs(c, P=2, B=2, generic=False):
    """fp32 inputs of a case at c.hw: x (P,B,xtot,hi,wi) with NaN in the channels the placement does not name, w (dead taps
    non-zero), bias (P,cout) or None, res / aux (P,B,ytot,h,w) or None, out0 (P,B,ytot,h,w) filled with the sentinel, dy
    (P,B,ytot,h,w) with NaN in the channels the placement does not name, dw0 / db0 the gradients' starting values.
    generic: float64 normal values everywhere (the applicability probe of the planted faults)."""
    h, w = c.hw
    hi, wi = (h // 2, w // 2) if c.ups else (h, w)
    g = _gen(c, "generic" if generic else "")
    intk = c.kind == "int" and not generic
    d = types.SimpleNamespace()
    if generic:
        rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64)
        xv, wv, bv, rv, dyv = rnd(P, B, c.cin, hi, wi), rnd(*w_shape(c, P)), rnd(P, c.cout), rnd(P, B, c.cout, h, w), rnd(P, B, c.cout, h, w)
        av = torch.tanh(rnd(P, B, c.cout, h, w))
    elif intk:
        xv, wv = _ints((P, B, c.cin, hi, wi), 1, 4, g), _ints(w_shape(c, P), 1, 3, g)
        bv, rv = _ints((P, c.cout), 1, 5, g), _ints((P, B, c.cout, h, w), 1, 6, g)
        dyv = _ints((P, B, c.cout, h, w), 1, 4, g)
        av = torch.randint(-2, 3, (P, B, c.cout, h, w), generator=g).float() * 0.5        # 0, +-0.5, +-1: 1 - aux^2 is exact
    else:
        u = lambda *s: torch.rand(*s, generator=g) * 2 - 1
        xv = u(P, B, c.cin, hi, wi) * 2
        wv = u(*w_shape(c, P)) * (2.0 / (c.cin_g * c.ntaps) ** 0.5)
        bv, rv = u(P, c.cout), u(P, B, c.cout, h, w)
        dyv = u(P, B, c.cout, h, w) * 1e-3
        pre = u(P, B, c.cout, h, w) * 2                               # aux = a forward output: both signs, values near 0
        av = R.declared_tanh(pre) if c.epi == EPI_TANH_BWD else torch.where(pre >= 0, pre, 0.01 * pre)
        flat = xv.view(P, B, -1)
        n = flat.shape[2]
        for p in range(P):                                            # planted: 0 and +-1e3, one at the last pixel of an image
            flat[p, 0, n - 1] = 1e3 if p == 0 else -1e3
            flat[p, 1, 0] = -1e3 if p == 0 else 1e3
            flat[p, 1, n // 2] = 0.0
            if n > 3:
                flat[p, 0, n // 3] = 0.0
    dt = F64 if generic else F32
    d.x = torch.full((P, B, c.xtot, hi, wi), float("nan"), dtype=dt)
    d.x[:, :, ic_index(c)] = xv
    d.w = wv
    d.bias = bv if c.bias else None
    ocp = oc_index(c)
    full = lambda t, fill: torch.full((P, B, c.ytot, h, w), fill, dtype=dt).index_copy_(2, ocp, t)
    d.res = full(rv, 0.0) if c.res else None
    d.aux = full(av, 0.0) if c.epi else None
    d.out0 = torch.full((P, B, c.ytot, h, w), SENTINEL, dtype=dt)
    d.dy = full(dyv, float("nan"))
    if c.acc and not generic:
        d.dw0, d.db0 = _ints((P, c.cout, c.cin_g, c.K, c.K), 1, 9, g), _ints((P, c.cout), 1, 9, g)
    else:
        d.dw0, d.db0 = torch.zeros(P, c.cout, c.cin_g, c.K, c.K, dtype=dt), torch.zeros(P, c.cout, dtype=dt)
    return d


# ------------------------------------------------------------------------------------------------ the statement
def w_eff(w, c, fault=None):
    """The weight handed in -> (groups, cout_g, cin_g, K, K) of the operator: Conv2d layout, taps as the conv applies them."""
    if c.transposed:                       # (cin, cout_g, K, K), input channel g * cin_g + ic: ConvTranspose2d, taps flipped
        w = w.view(c.groups, c.cin_g, c.cout_g, c.K, c.K).transpose(1, 2).flip(-1, -2)
    else:
        w = w.view(c.groups, c.cout_g, c.cin_g, c.K, c.K)
    if c.swap != (fault == "khkw"):
        w = w.transpose(-1, -2)
    return w


def live_taps(c, fault=None):
    return [(t // c.K, t % c.K) for t in range(c.K * c.K)] if fault == "dead_live" else c.taps


def source(x, c, fault=None):
    """x (B,xtot,hi,wi) -> (B,groups,cin_g,h,w): the named channels, through the nearest 2x upsampling."""
    v = x[:, ic_index(c, fault)]
    if c.ups:
        hi, wi = v.shape[-2:]
        iy, ix = torch.arange(2 * hi), torch.arange(2 * wi)
        if fault == "ups_round":
            iy, ix = ((iy + 1) >> 1).clamp_max(hi - 1), ((ix + 1) >> 1).clamp_max(wi - 1)
        else:
            iy, ix = iy >> 1, ix >> 1
        v = v[:, :, iy][:, :, :, ix]
    if fault == "chunk_drop" and c.cin_g % plan(c)[4]:
        v = v.clone()
        v[:, c.cin_g - 1::c.cin_g] = 0                       # the last channel of the partial chunk of every group
    return v.reshape(v.shape[0], c.groups, c.cin_g, *v.shape[-2:])


class Patches:
    """Shifted views of the zero-padded source: tap (ky, kx) of output pixel p reads the source at p + (ky, kx) - K/2."""

    def __init__(self, src, c, fault=None):
        self.R, self.h, self.w, self.fault = c.K // 2, src.shape[-2], src.shape[-1], fault
        pad = self.R + 1
        s = src.reshape(src.shape[0], -1, self.h, self.w)
        if fault == "halo_edge":
            s = F.pad(s, (pad, pad, pad, pad), mode="replicate")
        else:
            s = F.pad(s, (pad, pad, pad, pad))
        self.p = s.reshape(*src.shape[:3], self.h + 2 * pad, self.w + 2 * pad)
        self.bad = c.taps[-1]                                # the tap the tap_col / tap_row faults move

    def __call__(self, ky, kx):
        oy = 1 + (1 if self.fault == "tap_row" and (ky, kx) == self.bad else 0)
        ox = 1 + (1 if self.fault == "tap_col" and (ky, kx) == self.bad else 0)
        return self.p[..., ky + oy:ky + oy + self.h, kx + ox:kx + ox + self.w]


def conv_lin(x, w, c, fault=None):
    """sum over input channels and live taps -> (B, cout, h, w)."""
    src = source(x, c, fault)
    pt, we = Patches(src, c, fault), w_eff(w, c, fault)
    y = 0
    for ky, kx in live_taps(c, fault):
        y = y + torch.einsum("goi,bgihw->bgohw", we[:, :, :, ky, kx], pt(ky, kx))
    y = y.reshape(x.shape[0], c.cout, *src.shape[-2:])
    if fault == "oc_neighbour" and c.cout_g % plan(c)[1] and c.cout_g > 1:
        y = y.clone()
        y[:, c.cout_g - 1::c.cout_g] = y[:, c.cout_g - 2::c.cout_g]
    return y


def conv_lin_torch(x, w, c):
    """The same operator through F.conv2d (leg 1 of the yardstick)."""
    src = source(x, c)
    we = w_eff(w, c) * _mask_tensor(c, w.dtype)
    return F.conv2d(src.reshape(src.shape[0], c.cin, *src.shape[-2:]), we.reshape(c.cout, c.cin_g, c.K, c.K), None,
                    padding=c.K // 2, groups=c.groups)


def _mask_tensor(c, dtype):
    return torch.tensor([float((c.mask >> t) & 1) for t in range(c.K * c.K)], dtype=dtype).view(c.K, c.K)


def conv_lin_chain(x, w, c):
    """fp32, one sequential chain per output in the engine's order: chunks of CK channels, tap-major inside a chunk, then channel."""
    src = source(x, c)
    pt, we, ck = Patches(src, c), w_eff(w, c), plan(c)[4]
    acc = torch.zeros(src.shape[0], c.groups, c.cout_g, *src.shape[-2:], dtype=x.dtype)
    for c0 in range(0, c.cin_g, ck):
        for ky, kx in c.taps:
            p = pt(ky, kx)
            for ic in range(c0, min(c0 + ck, c.cin_g)):
                acc = acc + we[None, :, :, ic, ky, kx, None, None] * p[:, :, ic:ic + 1]
    return acc.reshape(src.shape[0], c.cout, *src.shape[-2:])


def act_apply(v, act, tanh=torch.tanh):
    if act == ACT_TANH:
        return tanh(v)
    if act == ACT_LRELU:
        return torch.where(v >= 0, v, 0.01 * v)
    if act == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    return v


def epilogue(lin, bias, c, res=None, aux=None, out0=None, tanh=torch.tanh, fault=None, act=True):
    """(B,cout,h,w) sums -> the (B,ytot,h,w) tensor: bias, epi(aux), residual, activation, placement into out0."""
    ocp = oc_index(c, fault)
    v = lin if bias is None else lin + bias.view(1, -1, 1, 1)
    r = res[:, ocp] if res is not None else None
    if c.epi and aux is not None:
        a = aux[:, ocp]
        f = 1 - a * a if c.epi == EPI_TANH_BWD else torch.where(a > 0, torch.ones_like(a), torch.full_like(a, 0.01))
        if fault == "epi_after" and r is not None:
            v, r = (v + r) * f, None
        else:
            v = v * f
    if r is not None:
        v = v + r
    if act:
        v = act_apply(v, c.act, tanh)
    out = torch.full((lin.shape[0], c.ytot, *lin.shape[-2:]), SENTINEL, dtype=lin.dtype) if out0 is None else out0.clone()
    out[:, ocp] = v
    return out


def forward(x, w, bias, c, res=None, aux=None, out0=None, tanh=torch.tanh, fault=None, lin=conv_lin, act=True):
    """One plane of lldwt_conv2d in the dtype of the arguments.  x (B,xtot,hi,wi) -> (B,ytot,h,w)."""
    l = lin(x, w, c, fault) if lin is conv_lin else lin(x, w, c)
    return epilogue(l, bias, c, res, aux, out0, tanh, fault, act)


# ------------------------------------------------------------------------------------------------ weight gradient
def _dw_store(c, dw, ky, kx, val, swap):
    a, b = (kx, ky) if swap else (ky, kx)
    dw[:, :, a, b] = dw[:, :, a, b] + val.reshape(c.cout, c.cin_g)


def wgrad(x, dy, c, dw0, db0, alpha=1.0, swap=False, fault=None):
    """One plane of lldwt_conv2d_wgrad in the dtype of the arguments.  x (B,xtot,hi,wi), dy (B,ytot,h,w) -> (dw, dbias)
    accumulated into copies of dw0 (cout,cin_g,K,K) / db0 (cout) (db0 None: no bias gradient)."""
    if fault == "batch_drop":
        x, dy = x[:-1], dy[:-1]
    src = source(x, c, fault)
    pt = Patches(src, c, fault)
    g = dy[:, oc_index(c, fault)].reshape(dy.shape[0], c.groups, c.cout_g, *dy.shape[-2:])
    dw = dw0.clone()
    for ky, kx in live_taps(c, fault):
        _dw_store(c, dw, ky, kx, alpha * torch.einsum("bgohw,bgihw->goi", g, pt(ky, kx)), swap != (fault == "khkw"))
    if fault == "oc_neighbour" and c.cout_g % 16 and c.cout_g > 1:
        dw[c.cout_g - 1::c.cout_g] = dw[c.cout_g - 2::c.cout_g]
    db = None
    if db0 is not None:
        db = db0 + alpha * g.sum(dim=(0, 3, 4)).reshape(-1)
        if fault == "bias_x" and x.shape[0] > 0:
            db = db + alpha * g[0, :, :, 0, 0].reshape(-1) * src[0, 0, 0, 0, 0]
    return dw, db


def wgrad_torch(x, dy, c, alpha=1.0, swap=False):
    """dw / dbias (from zero) by torch autograd of F.conv2d in the dtype of the arguments (leg 1)."""
    src = source(x, c)
    src = src.reshape(src.shape[0], c.cin, *src.shape[-2:])
    w = torch.zeros(c.cout, c.cin_g, c.K, c.K, dtype=x.dtype, requires_grad=True)
    b = torch.zeros(c.cout, dtype=x.dtype, requires_grad=True)
    y = F.conv2d(src, w, b, padding=c.K // 2, groups=c.groups)
    dw, db = torch.autograd.grad((y * dy[:, oc_index(c)]).sum(), [w, b])
    dw = dw * _mask_tensor(c, x.dtype)
    return alpha * (dw.transpose(-1, -2) if swap else dw), alpha * db


def uses_wgrad1x1(c):
    """The dispatch of lldwt_conv2d_wgrad for the whole-dW 1x1 tiles (32-pixel segments of the flattened image)."""
    nb = c.cin_g + (1 if c.want_bias else 0)
    plain = c.K == 1 and not c.ups and c.oc_block >= c.cout and c.oc_off == 0 and c.ytot == c.cout and not c.ic_block
    return plain and c.cout_g > 16 and 64 < nb <= 192


def chunk_order(c, B, h, w):
    """Pixel indices (b, y, x) of every K chunk in the kernels' order."""
    out = []
    if uses_wgrad1x1(c):
        for b in range(B):
            for p0 in range(0, h * w, 32):
                p = torch.arange(p0, min(p0 + 32, h * w))
                out.append((b, p // w, p % w))
        return out
    for b in range(B):
        for y0 in range(0, h, 8):
            for x0 in range(0, w, 16):
                yy, xx = torch.meshgrid(torch.arange(y0, min(y0 + 8, h)), torch.arange(x0, min(x0 + 16, w)), indexing="ij")
                out.append((b, yy.reshape(-1), xx.reshape(-1)))
    return out


def wgrad_chain(x, dy, c, alpha, swap, slices):
    """fp32: one accumulator per dW element and slice over that slice's chunks pixel by pixel, slices added at the end."""
    src = source(x, c)
    pt = Patches(src, c)
    B, h, w = dy.shape[0], dy.shape[-2], dy.shape[-1]
    g = dy[:, oc_index(c)].reshape(B, c.groups, c.cout_g, h, w)
    xt = torch.stack([pt(ky, kx) for ky, kx in c.taps], dim=3)                 # (B, G, cin_g, ntaps, h, w)
    chunks = chunk_order(c, B, h, w)
    S = max(1, min(slices, len(chunks)))
    accw = [torch.zeros(c.groups, c.cout_g, c.cin_g, c.ntaps, dtype=x.dtype) for _ in range(S)]
    accb = [torch.zeros(c.groups, c.cout_g, dtype=x.dtype) for _ in range(S)]
    for q, (b, yy, xx) in enumerate(chunks):
        s = q % S
        gq, xq = g[b][:, :, yy, xx], xt[b][:, :, :, yy, xx]                    # (G, cout_g, n), (G, cin_g, ntaps, n)
        for j in range(gq.shape[-1]):
            accw[s] = accw[s] + gq[:, :, None, None, j] * xq[:, None, :, :, j]
            accb[s] = accb[s] + gq[:, :, j]
    tw, tb = torch.zeros_like(accw[0]), torch.zeros_like(accb[0])
    for s in range(S):
        tw, tb = tw + alpha * accw[s], tb + alpha * accb[s]
    dw = torch.zeros(c.cout, c.cin_g, c.K, c.K, dtype=x.dtype)
    for t, (ky, kx) in enumerate(c.taps):
        _dw_store(c, dw, ky, kx, tw[..., t], swap)
    return dw, tb.reshape(-1)


# ------------------------------------------------------------------------------------------------ elementwise helpers
def act_bwd(dy, y, act):
    """dx = dy * act'(y) from the forward OUTPUT y, in the dtype of the arguments."""
    if act == ACT_TANH:
        return dy * (1 - y * y)
    if act == ACT_LRELU:
        return torch.where(y > 0, dy, 0.01 * dy)
    if act == ACT_RELU:
        return torch.where(y > 0, dy, torch.zeros_like(dy))
    return dy


def downsum2(g):
    """(.., h, w) -> (.., h/2, w/2): the sum of every 2 x 2 block, as (p00 + p01) + (p10 + p11)."""
    return (g[..., 0::2, 0::2] + g[..., 0::2, 1::2]) + (g[..., 1::2, 0::2] + g[..., 1::2, 1::2])


# ------------------------------------------------------------------------------------------------ reference + yardstick per case
WGRAD_SLICES = (1, 2, 4)


def forward_evaluate(c, d, P=2):
    """lift_ref.evaluate for the forward of case c on inputs d -> (ref, f32s), tensor key 'y' (B,ytot,h,w) per plane."""
    opt = lambda t, p, dt: None if t is None else t[p].to(dt)

    def args(p, dt):
        return (d.x[p].to(dt), d.w[p].to(dt), opt(d.bias, p, dt), c, opt(d.res, p, dt), opt(d.aux, p, dt), d.out0[p].to(dt))

    def fn(p, dtype, tanh):
        return {"y": forward(*args(p, dtype), tanh=tanh, lin=conv_lin if dtype == F64 else conv_lin_torch)}

    def chain(p):
        return {"y": forward(*args(p, F32), tanh=R.declared_tanh, lin=conv_lin_chain)}
    return R.evaluate(fn, P, extra=(chain,))


def wgrad_evaluate(c, d, P=2):
    """lift_ref.evaluate for the weight gradient of case c (from d.dw0 / d.db0) -> (ref, f32s), keys 'dw' and 'db'."""
    def pack(dw, db, p, dt):
        out = {"dw": d.dw0[p].to(dt) + dw}
        if c.want_bias:
            out["db"] = d.db0[p].to(dt) + db
        return out

    def fn(p, dtype, tanh):
        x, dy = d.x[p].to(dtype), d.dy[p].to(dtype)
        if dtype == F64:
            z = torch.zeros_like(d.dw0[p], dtype=F64)
            dw, db = wgrad(x, dy, c, z, torch.zeros(c.cout, dtype=F64), c.alpha, c.swap)
        else:
            dw, db = wgrad_torch(x, dy, c, c.alpha, c.swap)
        return pack(dw, db, p, dtype)

    def chain(s):
        return lambda p: pack(*wgrad_chain(d.x[p], d.dy[p], c, c.alpha, c.swap, s), p, F32)
    return R.evaluate(fn, P, extra=tuple(chain(s) for s in WGRAD_SLICES))


def bars(ref, f32s, key, floor):
    """Per plane: 4 * yardstick + floor * max|f64| (the rule of lift_ref.check, for the planted-fault test)."""
    yard = R.yardstick(ref, f32s, key)
    return [4.0 * float(yard[p]) + floor * float(ref[key][p].abs().max()) for p in range(len(ref[key]))]
