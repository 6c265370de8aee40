"""float64 reference, fp32 yardstick and planted faults for the split-fp16 3x3 conv family of csrc/conv_f16x3.hip (the dense conv
lldwt_conv3x3_f16x3, its fp16-storage form lldwt_conv3x3_f16in, the fused tree-context pair lldwt_plc_fused in its direct and row-wise
Winograd forms) and the split-fp16 backward of autograd.ConvFn (the adjoint conv, lldwt_conv3x3_wgrad_f16x3): the yardstick of
tests/test_f16x3_ref_host.py and tests/test_gpu_f16x3_domain.py.  No device code.

Reference.  Plain torch statements in the dtype of their arguments, one einsum per tap over shifted views of the zero-padded input:
    conv   y = act(conv3x3(x, w) + b)
    pair   y = act2(conv3x3(LeakyReLU_0.01(conv3x3(up2(parent), w1) + b1), w2) + b2)      up2 the nearest 2x upsampling; the upsampled
           image is zero-padded for the first conv and t is zero-padded for the second (the padding is NOT LeakyReLU(b1))
    adjoint  dx = conv3x3(dpre, w.transpose(0, 1).flip(-1, -2))                            the weight ConvFn.backward forms
    wgrad  dw[o, i, ky, kx] = alpha sum_{b, p} dy[b, o, p] x[b, i, p + (ky, kx) - 1],  db[o] = alpha sum_{b, p} dy[b, o, p]
The host test pins them to F.conv2d / F.interpolate / torch autograd in float64.

Yardstick (the pattern of tests/lift_ref.py, whose evaluate / yardstick / check / declared_tanh are used as they are): per plane and
tensor the largest error against float64 of these fp32 evaluations on the same inputs
  (a) torch fp32 (F.conv2d, F.interpolate) with torch.tanh and with the kernels' declared tanh;
  (b) one sequential fp32 chain per output in the kernels' declared order: chunks of 32 channels (16 for k_plc_wino: both are legs),
      tap-major inside a chunk, then channel, bias last;
  (c) the split evaluation: tools/winograd_numerics.py restated in torch and extended to what the kernels declare -- pow2_scale as
      in csrc/split_f16.h (amax 2^n lands on 2^14), a round-to-nearest hi / lo fp16 split, the three products lo*hi, hi*lo, hi*hi
      accumulated in fp32 chunk by chunk.  The pair takes its scales per 8 x 32 output tile and image from the tile's 6 x 18 parent
      patch: s_p from the patch |max|, sx from amax * L1max + bmax with L1max / bmax as k_f1_pack forms them (half of that sx and the
      U / V transforms for the Winograd form); its first conv is itself split, the weights under sw1, and its result goes through
      fma(t, sx / (s_p sw1), b1 sx) and max(v, 0.01 v).  The dense conv takes one scale per plane; the fp16-storage form reads fp16
      values times xscale[plane] and has two products; the weight gradient scales x and dy per plane to 2^14.  The one-product
      evaluation (operands rounded to fp16 / bf16) is the yardstick of the PREC 1 / PREC 2 class only.
Bars are lift_ref's: values 4 * yardstick + 2e-7 * max|f64|, gradients 4 * yardstick + 5e-7 * max|f64|, per plane and tensor; per
output tile for the region inputs and per image row for the row ramps (yardstick and floor over the same block).

Planted faults (FAULTS): one deliberate mistake of the kind a kernel can make.  OPERATOR faults change the operator and are planted
in the float64 statement; they apply to a case when they change it on generic inputs of the case's shapes and fields.  ARITHMETIC
faults leave the operator alone in exact arithmetic and are planted in the split evaluation: a dropped product and an epilogue scale
off by two apply everywhere, the three misplaced scales (shared by the launch, the neighbouring tile's, the neighbouring plane's)
apply to the cases whose inputs are declared to tell scales apart (case.scales: the region inputs and the plane-magnitude inputs).
The host test asserts that every applicable fault is rejected on the case's own inputs under the case's own bar."""
import types
import zlib

import torch
import torch.nn.functional as F

import lift_ref as R

F64, F32 = torch.float64, torch.float32
ACT_NONE, ACT_TANH, ACT_LRELU, ACT_RELU = 0, 1, 2, 3
TH, TW, OCB = 8, 32, 128

ARITH_FAULTS = ("scale_launch", "scale_tile", "scale_plane", "epi_scale", "hilo_drop", "lo1_drop")
OPER_FAULTS = ("pad_lrelu", "ups_round", "chunk_live", "bias_block", "relu_lrelu", "slope", "wino_swap", "tap_swap")
FAULTS = ARITH_FAULTS + OPER_FAULTS
SCALE_FAULTS = ("scale_launch", "scale_tile", "scale_plane")


# ------------------------------------------------------------------------------------------------ the statements
def act_apply(v, act, tanh=torch.tanh, fault=None):
    if act == ACT_TANH:
        return tanh(v)
    if act == ACT_LRELU or (act == ACT_RELU and fault == "relu_lrelu"):
        return torch.where(v >= 0, v, 0.01 * v)
    if act == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    return v


def conv3_padded(xp, w, fault=None):
    """xp (B,cin,h+2,w+2) already padded, w (cout,cin,3,3) -> (B,cout,h,w)."""
    h, wd = xp.shape[-2] - 2, xp.shape[-1] - 2
    y = 0
    for ky in range(3):
        for kx in range(3):
            a, b = (kx, ky) if fault == "tap_swap" else (ky, kx)
            y = y + torch.einsum("oi,bihw->bohw", w[:, :, ky, kx], xp[..., a:a + h, b:b + wd])
    return y


def conv3(x, w, fault=None):
    if fault == "chunk_live" and w.shape[1] % 16:          # the last channel of the partial chunk counted twice
        w = w.clone()
        w[:, -1] = 2 * w[:, -1]
    return conv3_padded(F.pad(x, (1, 1, 1, 1)), w, fault)


def up2(parent, fault=None):
    hp, wp = parent.shape[-2:]
    iy, ix = torch.arange(2 * hp), torch.arange(2 * wp)
    if fault == "ups_round":
        iy, ix = ((iy + 1) >> 1).clamp_max(hp - 1), ((ix + 1) >> 1).clamp_max(wp - 1)
    else:
        iy, ix = iy >> 1, ix >> 1
    return parent[..., iy, :][..., ix]


def bias_of(b, fault=None):
    if b is not None and fault == "bias_block" and b.shape[0] > OCB:      # channel block 1 takes block 0's bias
        b = b.clone()
        b[OCB:2 * OCB] = b[:b.shape[0] - OCB][:OCB]
    return b


def epilogue(lin, b, act, tanh=torch.tanh, fault=None):
    b = bias_of(b, fault)
    v = lin if b is None else lin + b.view(1, -1, 1, 1)
    y = act_apply(v, act, tanh, fault)
    if fault == "wino_swap":
        y = torch.stack([y[..., 1::2], y[..., 0::2]], dim=-1).reshape(y.shape)
    return y


def pair_lin(parent, w1, b1, w2, fault=None):
    """One plane: parent (B,3,hp,wp) -> conv3x3(LeakyReLU(conv3x3(up2(parent)) + b1)) without the second bias, (B,cout,2hp,2wp)."""
    v = conv3(up2(parent, fault), w1) + b1.view(1, -1, 1, 1)
    slope = 0.1 if fault == "slope" else 0.01
    t = torch.where(v >= 0, v, slope * v)
    tp = F.pad(t, (1, 1, 1, 1))
    if fault == "pad_lrelu":
        rim = torch.where(b1 >= 0, b1, slope * b1).view(1, -1, 1, 1).expand_as(tp).clone()
        rim[..., 1:-1, 1:-1] = t
        tp = rim
    if fault == "chunk_live" and w2.shape[1] % 16:
        w2 = w2.clone()
        w2[:, -1] = 2 * w2[:, -1]
    return conv3_padded(tp, w2, fault)


def adjoint_weight(w):
    """(cout,cin,3,3) -> (cin,cout,3,3): the weight of the adjoint conv as autograd.ConvFn.backward forms it."""
    return w.transpose(0, 1).flip(-1, -2).contiguous()


def wgrad(x, dy, alpha=1.0, fault=None):
    """One plane: x (B,cin,h,w), dy (B,cout,h,w) -> (dw (cout,cin,3,3), db (cout))."""
    h, wd = x.shape[-2:]
    xp = F.pad(x, (1, 1, 1, 1))
    dw = torch.zeros(dy.shape[1], x.shape[1], 3, 3, dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            a, b = (kx, ky) if fault == "tap_swap" else (ky, kx)
            dw[:, :, ky, kx] = alpha * torch.einsum("bohw,bihw->oi", dy, xp[..., a:a + h, b:b + wd])
    return dw, alpha * dy.sum(dim=(0, 2, 3))


# ------------------------------------------------------------------------------------------------ fp32 legs (a) and (b)
def conv3_torch(x, w):
    return F.conv2d(x, w, None, padding=1)


def pair_lin_torch(parent, w1, b1, w2):
    t = F.leaky_relu(F.conv2d(F.interpolate(parent, scale_factor=2, mode="nearest"), w1, b1, padding=1), 0.01)
    return F.conv2d(t, w2, None, padding=1)


def conv3_chain(x, w, ck):
    """One sequential accumulator per output: chunks of ck channels, tap-major inside a chunk, then channel."""
    h, wd = x.shape[-2:]
    xp = F.pad(x, (1, 1, 1, 1))
    acc = torch.zeros(x.shape[0], w.shape[0], h, wd, dtype=x.dtype)
    for c0 in range(0, x.shape[1], ck):
        for ky in range(3):
            for kx in range(3):
                for ic in range(c0, min(c0 + ck, x.shape[1])):
                    acc = acc + w[None, :, ic, ky, kx, None, None] * xp[:, ic:ic + 1, ky:ky + h, kx:kx + wd]
    return acc


def pair_lin_chain(parent, w1, b1, w2, ck):
    v = conv3_chain(up2(parent), w1, 32) + b1.view(1, -1, 1, 1)
    return conv3_chain(torch.where(v >= 0, v, 0.01 * v), w2, ck)


def wgrad_chain(x, dy, alpha, slices):
    """One accumulator per dW element and slice over the pixels in the order of the 2 x 32 pixel chunks of csrc/conv_wgrad_f16x3.hip,
    chunk q in slice q % slices, the slices added at the end as the atomics do."""
    Bn, _, h, wd = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    xt = torch.stack([xp[..., ky:ky + h, kx:kx + wd] for ky in range(3) for kx in range(3)], dim=2)      # (B,cin,9,h,w)
    accw = [torch.zeros(dy.shape[1], x.shape[1], 9, dtype=x.dtype) for _ in range(slices)]
    accb = [torch.zeros(dy.shape[1], dtype=x.dtype) for _ in range(slices)]
    q = 0
    for b in range(Bn):
        for y0 in range(0, h, 2):
            for x0 in range(0, wd, 32):
                s = q % slices
                q += 1
                for yy in range(y0, min(y0 + 2, h)):
                    for xx in range(x0, min(x0 + 32, wd)):
                        accw[s] = accw[s] + dy[b, :, yy, xx, None, None] * xt[b, None, :, :, yy, xx]
                        accb[s] = accb[s] + dy[b, :, yy, xx]
    tw, tb = torch.zeros_like(accw[0]), torch.zeros_like(accb[0])
    for s in range(slices):
        tw, tb = tw + alpha * accw[s], tb + alpha * accb[s]
    return tw.reshape(dy.shape[1], x.shape[1], 3, 3), tb


# ------------------------------------------------------------------------------------------------ leg (c): the split evaluation
def pow2_scale(amax, top=15):
    """csrc/split_f16.h pow2_scale<TOP>: 2^k with amax * 2^k in [2^(TOP-1), 2^TOP), k clamped to +-120; 1 for 0 / non-finite."""
    a = torch.as_tensor(amax, dtype=F32)
    ok = (a > 0) & (a < 3.0e38)
    _, e = torch.frexp(torch.where(ok, a, torch.ones_like(a)))
    k = (top - e).clamp(-120, 120).to(torch.int32)
    return torch.where(ok, torch.ldexp(torch.ones_like(a), k), torch.ones_like(a))


def split(v):
    hi = v.half().float()
    return hi, (v - hi).half().float()


def round_to(v, prec):
    return v.half().float() if prec == 1 else v.bfloat16().float()


def mac3(acc, eq, wh, wl, xh, xl, fault=None):
    """acc + the three split products in the kernels' order (w_lo x_hi, w_hi x_lo, w_hi x_hi), each product exact in fp32."""
    acc = acc + torch.einsum(eq, wl, xh)
    if fault != "hilo_drop":
        acc = acc + torch.einsum(eq, wh, xl)
    return acc + torch.einsum(eq, wh, xh)


def wino_u(w):
    """(cout,cin,3,3) -> U (cout,cin,3 dy,4 xi) in float64 (k_f3w_pack)."""
    w = w.double()
    g0, g1, g2 = w[..., 0], w[..., 1], w[..., 2]
    return torch.stack([g0, (g0 + g1 + g2) * 0.5, (g0 - g1 + g2) * 0.5, g2], dim=-1)


def conv_split(x, w, amax, fault=None, in16_scale=None):
    """One plane of the dense conv: x (B,cin,h,w) fp32, w (cout,cin,3,3) fp32, amax the |max| its scale comes from -> acc * out_scale.
    in16_scale: the fp16-storage form -- x holds the stored fp16 values, the scale is xscale[plane], two products."""
    h, wd = x.shape[-2:]
    sw = pow2_scale(w.abs().max())
    wh, wl = split(w * sw)
    if in16_scale is not None:
        sx = torch.as_tensor(in16_scale, dtype=F32)
        xh, xl = F.pad(x, (1, 1, 1, 1)), None
    else:
        sx = pow2_scale(amax)
        xh, xl = split(F.pad(x * sx, (1, 1, 1, 1)))
    acc = torch.zeros(x.shape[0], w.shape[0], h, wd, dtype=F32)
    for c0 in range(0, x.shape[1], 32):
        c = slice(c0, min(c0 + 32, x.shape[1]))
        for ky in range(3):
            for kx in range(3):
                a = xh[:, c, ky:ky + h, kx:kx + wd]
                if xl is None:
                    if fault != "hilo_drop":
                        acc = acc + torch.einsum("oi,bihw->bohw", wl[:, c, ky, kx], a)
                    acc = acc + torch.einsum("oi,bihw->bohw", wh[:, c, ky, kx], a)
                else:
                    acc = mac3(acc, "oi,bihw->bohw", wh[:, c, ky, kx], wl[:, c, ky, kx], a, xl[:, c, ky:ky + h, kx:kx + wd], fault)
    out_scale = (1.0 / sx) * (1.0 / sw)
    return acc * (out_scale * (2.0 if fault == "epi_scale" else 1.0))


def pair_tiles(hp, wp):
    """(y0, x0) of the 8 x 32 output tiles of a parent of hp x wp, in the kernels' order (row-major)."""
    return [(y0, x0) for y0 in range(0, 2 * hp, TH) for x0 in range(0, 2 * wp, TW)]


def _patches(parent):
    """parent (..,3,hp,wp) -> list over tiles of the 6 x 18 zero-padded parent patch (..,3,6,18)."""
    hp, wp = parent.shape[-2:]
    pp = F.pad(parent, (1, 18, 1, 6))
    return [pp[..., (y0 >> 1):(y0 >> 1) + 6, (x0 >> 1):(x0 >> 1) + 18] for y0, x0 in pair_tiles(hp, wp)]


def pair_split(parent, w1, b1, w2, form="wino", fault=None, prec=0):
    """All planes: parent (P,B,3,hp,wp), w1 (P,cmid,3,3,3), b1 (P,cmid), w2 (P,cout,cmid,3,3), fp32 -> acc * out_scale (P,B,cout,2hp,2wp).
    form 'wino' (k_plc_wino) or 'direct' (k_conv3_f16x3<2>); prec 1 / 2: one product on fp16 / bf16 operands (direct form)."""
    Pn, Bn, _, hp, wp = parent.shape
    cmid, cout, h, wd = w1.shape[1], w2.shape[1], 2 * hp, 2 * wp
    tiles, patches = pair_tiles(hp, wp), _patches(parent)
    amax = torch.stack([pt.abs().amax(dim=(-1, -2, -3)) for pt in patches], dim=-1)          # (P,B,tiles)
    iy, ix = torch.arange(12) >> 1, torch.arange(36) >> 1
    out = torch.zeros(Pn, Bn, cout, h, wd, dtype=F32)
    for p in range(Pn):
        sw1 = pow2_scale(w1[p].abs().max())
        l1 = w1[p].abs().reshape(cmid, 27).sum(dim=1).max()
        bmax = b1[p].abs().max()
        w1s = w1[p] * sw1
        if prec:
            w1h, w1l = round_to(w1s, prec), None
            sw = pow2_scale(w2[p].abs().max())
            w2h, w2l = round_to(w2[p] * sw, prec), None
        else:
            w1h, w1l = split(w1s)
            if form == "wino":
                u = wino_u(w2[p])
                sw = pow2_scale(u.float().abs().max())
                w2h, w2l = split((u * sw.double()).float())
            else:
                sw = pow2_scale(w2[p].abs().max())
                w2h, w2l = split(w2[p] * sw)
        for t, (y0, x0) in enumerate(tiles):
            am = amax[p, :, t]
            if fault == "scale_launch":
                am = amax.max().expand(Bn)
            elif fault == "scale_tile":
                am = amax[p, :, (t + 1) % len(tiles)]
            elif fault == "scale_plane":
                am = amax[(p + 1) % Pn, :, t]
            am = am.view(Bn, 1, 1, 1)
            s_p = pow2_scale(am)
            sx = pow2_scale(am * l1 + bmax) * (0.5 if form == "wino" and not prec else 1.0)
            u12 = patches[t][p][..., iy, :][..., ix] * s_p                                  # (B,3,12,36): the upsampled patch
            if prec:
                uh = round_to(u12, prec)
                tacc = F.conv2d(uh, w1h)
            else:
                uh, ul = split(u12)
                tacc = F.conv2d(uh, w1l)
                if fault != "lo1_drop":
                    tacc = tacc + F.conv2d(ul, w1h)
                tacc = tacc + F.conv2d(uh, w1h)
            inv1sx = (1.0 / s_p) * (1.0 / sw1) * sx
            v = (tacc.double() * inv1sx.double() + (b1[p].view(1, -1, 1, 1) * sx).double()).float()      # fmaf(t, inv1sx, b1 * sx)
            d = torch.maximum(v, v * 0.01)
            gy, gx = torch.arange(y0 - 1, y0 + 9), torch.arange(x0 - 1, x0 + 33)
            pin = ((gy >= 0) & (gy < h)).view(-1, 1) & ((gx >= 0) & (gx < wd)).view(1, -1)
            d = torch.where(pin, d, torch.zeros_like(d))                                  # (B,cmid,10,34), scaled by sx
            if prec or form != "wino":
                dh, dl = (round_to(d, prec), None) if prec else split(d)
                acc = torch.zeros(Bn, cout, TH, TW, dtype=F32)
                for c0 in range(0, cmid, 32):
                    c = slice(c0, min(c0 + 32, cmid))
                    for ky in range(3):
                        for kx in range(3):
                            a = dh[:, c, ky:ky + TH, kx:kx + TW]
                            if prec:
                                acc = acc + torch.einsum("oi,bihw->bohw", w2h[:, c, ky, kx], a)
                            else:
                                acc = mac3(acc, "oi,bihw->bohw", w2h[:, c, ky, kx], w2l[:, c, ky, kx], a,
                                           dl[:, c, ky:ky + TH, kx:kx + TW], fault)
                lin = acc
            else:
                dk = [d[..., k:k + TW:2] for k in range(4)]                                # d_k of the 16 pixel pairs
                vv = torch.stack([dk[0] - dk[2], dk[1] + dk[2], dk[2] - dk[1], dk[1] - dk[3]], dim=-1)    # (B,cmid,10,16,4)
                vh, vl = split(vv)
                m = [torch.zeros(Bn, cout, TH, TW // 2, dtype=F32) for _ in range(4)]
                for c0 in range(0, cmid, 16):
                    c = slice(c0, min(c0 + 16, cmid))
                    for ky in range(3):
                        for xi in range(4):
                            m[xi] = mac3(m[xi], "oi,bihw->bohw", w2h[:, c, ky, xi], w2l[:, c, ky, xi], vh[:, c, ky:ky + TH, :, xi],
                                         vl[:, c, ky:ky + TH, :, xi], fault)
                lin = torch.stack([(m[0] + m[1]) + m[2], (m[1] - m[2]) - m[3]], dim=-1).reshape(Bn, cout, TH, TW)
            out_scale = (1.0 / sx) * (1.0 / sw) * (2.0 if fault == "epi_scale" else 1.0)
            y1, x1 = min(y0 + TH, h), min(x0 + TW, wd)
            out[p, :, :, y0:y1, x0:x1] = (lin * out_scale)[:, :, :y1 - y0, :x1 - x0]
    return out


def wgrad_split(x, dy, ax, ay, alpha=1.0, fault=None):
    """One plane of lldwt_conv3x3_wgrad_f16x3: both operands scaled to 2^14 by a power of two, three products, fp32 accumulation;
    the bias gradient is a plain fp32 sum of dy."""
    h, wd = x.shape[-2:]
    sx, sy = pow2_scale(ax, 14), pow2_scale(ay, 14)
    xh, xl = split(F.pad(x * sx, (1, 1, 1, 1)))
    yh, yl = split(dy * sy)
    dw = torch.zeros(dy.shape[1], x.shape[1], 3, 3, dtype=F32)
    for ky in range(3):
        for kx in range(3):
            a, b = (kx, ky) if fault == "tap_swap" else (ky, kx)
            acc = mac3(torch.zeros(dy.shape[1], x.shape[1], dtype=F32), "bohw,bihw->oi", yh, yl, xh[..., a:a + h, b:b + wd],
                       xl[..., a:a + h, b:b + wd], fault)
            dw[:, :, ky, kx] = acc * (alpha * (1.0 / sx) * (1.0 / sy) * (2.0 if fault == "epi_scale" else 1.0))
    return dw, alpha * dy.sum(dim=(0, 2, 3))


# ------------------------------------------------------------------------------------------------ inputs: the pair
P, B, CMID, COUT = 2, 2, 40, 130
PARENTS = {"7x19": (7, 19), "4x144": (4, 144), "36x16": (36, 16)}
# Region inputs: the parent times 2^k on three regions along the long axis of the image, a different order per plane.  Chosen by the
# host test (test_region_exponents_are_needed_and_enough): a step of 2^24 between neighbours leaves the split about three bits in its
# lo half when a scale comes from the wrong region, which every misplaced-scale fault needs to leave the 4 x yardstick bar.
REGION_EXP = ((0, -24, 24), (24, 0, -24))


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32("|".join(str(k) for k in key).encode()))


def region_slices(hp, wp):
    """Three regions along the long axis: [(dim, slice)]."""
    dim, n = (-1, wp) if wp >= hp else (-2, hp)
    e = [0, n // 3, 2 * (n // 3), n]
    return [(dim, slice(e[r], e[r + 1])) for r in range(3)]


def region_gain(hp, wp, exps=REGION_EXP):
    """(P,1,1,hp,wp) of exact powers of two."""
    g = torch.ones(len(exps), 1, 1, hp, wp)
    for p, ex in enumerate(exps):
        for (dim, sl), k in zip(region_slices(hp, wp), ex):
            if dim == -1:
                g[p, ..., sl] = 2.0 ** k
            else:
                g[p, ..., sl, :] = 2.0 ** k
    return g


def middle_tiles(hp, wp):
    """[(region, y0, x0)] of the tiles whose whole 6 x 18 parent patch lies inside one region (none on the ragged parent)."""
    out = []
    for r, (dim, sl) in enumerate(region_slices(hp, wp)):
        for y0, x0 in pair_tiles(hp, wp):
            lo, n = ((x0 >> 1) - 1, 18) if dim == -1 else ((y0 >> 1) - 1, 6)
            if lo >= sl.start and lo + n <= sl.stop:
                out.append((r, y0, x0))
    return out


VARIANTS = ("base", "b1zero", "regions", "zero", "zero_region", "down24", "up24", "tiny", "spike", "bigb1", "w1decades", "wino_cancel",
            "w2zero_oc")
_pair_cache = {}


def pair_inputs(shape, variant="base"):
    """fp32 inputs of the pair: parent (P,B,3,hp,wp), w1 (P,CMID,3,3,3), b1 (P,CMID), w2 (P,COUT,CMID,3,3), b2 (P,COUT).  The planes carry
    distinct weights of distinct magnitude (plane 1: w1 / 2, w2 x 4), so a header read from the wrong plane is off by a factor."""
    key = (shape, variant)
    if key in _pair_cache:
        return _pair_cache[key]
    hp, wp = PARENTS[shape]
    g = _gen("pair", shape)
    u = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    d = types.SimpleNamespace(shape=shape, variant=variant, hp=hp, wp=wp)
    d.parent = u(P, B, 3, hp, wp) * 2
    d.w1 = u(P, CMID, 3, 3, 3) * 0.3
    d.b1 = u(P, CMID) * 0.5
    d.w2 = u(P, COUT, CMID, 3, 3) * (1.0 / (CMID * 9) ** 0.5)
    d.b2 = u(P, COUT) * 0.5
    d.w1[1] *= 0.5
    d.w2[1] *= 4.0
    regs = region_slices(hp, wp)
    if variant == "b1zero" or variant.startswith("regions"):
        d.b1 = torch.zeros_like(d.b1)
    if variant.startswith("regions"):           # "regions": REGION_EXP; "regions<step>": the same order with another step (the host probe)
        step = int(variant[7:] or 24)
        d.parent = d.parent * region_gain(hp, wp, tuple(tuple(k * step // 24 for k in ex) for ex in REGION_EXP))
    elif variant == "zero":
        d.parent = torch.zeros_like(d.parent)
    elif variant == "zero_region":
        dim, sl = regs[1]
        if dim == -1:
            d.parent[..., sl] = 0
        else:
            d.parent[..., sl, :] = 0
    elif variant == "down24":
        d.parent = d.parent * 2.0 ** -24
    elif variant == "up24":
        d.parent = d.parent * 2.0 ** 24
    elif variant == "tiny":
        d.parent = torch.full_like(d.parent, 1e-40)
    elif variant == "spike":
        d.parent[0, 1, 2, hp // 2, wp // 3] = 10000.37           # not a multiple of its fp16 ulp: the sample has a lo half
        d.parent[1, 0, 0, hp - 1, wp - 1] = -10000.37
    elif variant == "bigb1":
        for p in range(P):
            top = float(conv3(up2(d.parent[p].double()), d.w1[p].double()).abs().max())
            d.b1[p] = torch.sign(d.b1[p]) * (1.0 + d.b1[p].abs()) * 100.0 * top
    elif variant == "w1decades":
        d.w1 = d.w1 * (10.0 ** (-6.0 * torch.arange(CMID) / (CMID - 1))).view(1, CMID, 1, 1, 1)
    elif variant == "wino_cancel":
        d.w2[..., 1, 1] *= 64.0
        d.parent[..., 1::2] = 0
    elif variant == "w2zero_oc":
        d.w2[:, 7] = 0
        d.w2[:, COUT - 1] = 0
    elif variant not in ("base", "b1zero"):
        raise ValueError(variant)
    _pair_cache[key] = d
    return d


# What an input of the numeric domain cannot see, by construction: a zero (1e-40) parent nulls every fault on the parent's path (these
# two are the corner amax == 0 of the scales); with the parent at 2^-24 of b1, or b1 at a hundred times the first conv, the first
# conv's share of t is below or near the fp32 resolution of t and so are its lo image and (at 2^-24) its upsampling index; with the parent at 2^24 of b1 so is LeakyReLU(b1).
_PARENT_PATH = ("hilo_drop", "lo1_drop", "ups_round", "wino_swap", "tap_swap")
BLIND = {"zero": _PARENT_PATH, "tiny": _PARENT_PATH, "down24": ("lo1_drop", "ups_round"), "bigb1": ("lo1_drop",), "up24": ("pad_lrelu",)}


def pair_case(shape, variant, act, bias):
    c = types.SimpleNamespace(kind="pair", shape=shape, variant=variant, act=act, bias=bool(bias), cin=CMID, cout=COUT)
    c.name = "pair-%s-%s-act%d-%s" % (shape, variant, act, "b2" if bias else "nob2")
    c.tiles = variant.startswith("regions")             # compared per output tile
    c.scales = variant.startswith("regions")            # the inputs tell scales apart
    c.blind = BLIND.get(variant, ())                    # the faults this input nulls by construction
    return c


# group 2 of tests/test_gpu_f16x3_domain.py: every activation with and without b2 at the three parents ...
PAIR_BASE = [pair_case(s, "base", a, b) for s in PARENTS for a in (0, 1, 2, 3) for b in (True, False)]
# ... the numeric domain at 7x19 and 4x144 ...
_DOMAIN = [("zero", 0, True), ("zero_region", 3, True), ("down24", 2, True), ("up24", 0, False), ("tiny", 1, True), ("spike", 3, False),
           ("bigb1", 2, False), ("w1decades", 0, True), ("wino_cancel", 3, True), ("w2zero_oc", 1, True)]
PAIR_DOMAIN = [pair_case(s, v, a, b) for s in ("7x19", "4x144") for v, a, b in _DOMAIN]
# ... and the region inputs (b1 = 0, no b2: the pair is homogeneous), per tile
PAIR_REGIONS = [pair_case(s, "regions", a, False) for s in ("4x144", "36x16") for a in (0, 2, 3)]
PAIR_CASES = PAIR_BASE + PAIR_DOMAIN + PAIR_REGIONS


def applies(c, fault):
    """Whether the planted fault applies to case c (see the module docstring)."""
    pair = c.kind == "pair"
    if pair and fault in c.blind:
        return False
    if fault in SCALE_FAULTS:
        return c.scales and (pair or fault != "scale_tile")
    if fault in ("epi_scale", "hilo_drop", "tap_swap"):
        return True
    if fault == "bias_block":
        return c.bias and c.cout > OCB and c.kind in ("pair", "conv", "in16")
    if fault == "relu_lrelu":
        return c.act == ACT_RELU and c.kind != "wgrad"
    if fault == "pad_lrelu":
        return pair and c.variant != "b1zero" and not c.variant.startswith("regions")
    if fault == "chunk_live":
        return c.kind != "wgrad" and (c.cout if c.kind == "adjoint" else c.cin) % 16 != 0
    if fault in ("lo1_drop", "slope", "ups_round", "wino_swap"):
        return pair
    raise ValueError(fault)


# ------------------------------------------------------------------------------------------------ evaluation of the pair
_pair_lins = {}


def pair_lins(d):
    """The pre-bias sums of one input set, computed once: float64, then the fp32 legs (torch, chain 32, chain 16, split direct, split
    Winograd).  -> (lin64 [P], [leg][P])."""
    key = (d.shape, d.variant)
    if key not in _pair_lins:
        a64 = lambda p: (d.parent[p].double(), d.w1[p].double(), d.b1[p].double(), d.w2[p].double())
        a32 = lambda p: (d.parent[p], d.w1[p], d.b1[p], d.w2[p])
        lin64 = [pair_lin(*a64(p)) for p in range(P)]
        sd, sw = pair_split(d.parent, d.w1, d.b1, d.w2, "direct"), pair_split(d.parent, d.w1, d.b1, d.w2, "wino")
        legs = [[pair_lin_torch(*a32(p)) for p in range(P)], [pair_lin_chain(*a32(p), 32) for p in range(P)],
                [pair_lin_chain(*a32(p), 16) for p in range(P)], [sd[p] for p in range(P)], [sw[p] for p in range(P)]]
        _pair_lins[key] = (lin64, legs)
    return _pair_lins[key]


def evaluate_epilogues(lin64, legs, bias, act, planes):
    """lift_ref.evaluate over cached pre-bias sums -> (ref, f32s) with key 'y': leg 0 (torch fp32) runs with torch.tanh and with the
    declared tanh, every further leg with the declared tanh."""
    bz = lambda p, dt: None if bias is None else bias[p].to(dt)

    def fn(p, dtype, tanh):
        src = lin64 if dtype == F64 else legs[0]
        return {"y": epilogue(src[p], bz(p, dtype), act, tanh)}
    extra = tuple((lambda p, leg=leg: {"y": epilogue(leg[p], bz(p, F32), act, R.declared_tanh)}) for leg in legs[1:])
    return R.evaluate(fn, planes, extra=extra)


def pair_evaluate(c):
    d = pair_inputs(c.shape, c.variant)
    lin64, legs = pair_lins(d)
    return evaluate_epilogues(lin64, legs, d.b2 if c.bias else None, c.act, P)


_pair_fault = {}


def pair_faulty(c, fault):
    """The pair of case c with one planted fault -> [P] tensors (float64 for the operator faults, fp32 for the arithmetic ones)."""
    d = pair_inputs(c.shape, c.variant)
    b2 = d.b2 if c.bias else None
    epi_fault = fault in ("bias_block", "relu_lrelu", "wino_swap")
    key = (d.shape, d.variant, None if epi_fault else fault)
    if key not in _pair_fault:
        if epi_fault:
            _pair_fault[key] = pair_lins(d)[0]
        elif fault in ARITH_FAULTS:
            lin = pair_split(d.parent, d.w1, d.b1, d.w2, "wino", fault)
            _pair_fault[key] = [lin[p] for p in range(P)]
        else:
            _pair_fault[key] = [pair_lin(d.parent[p].double(), d.w1[p].double(), d.b1[p].double(), d.w2[p].double(), fault)
                                for p in range(P)]
    lins = _pair_fault[key]
    dt = lins[0].dtype
    return [epilogue(lins[p], None if b2 is None else b2[p].to(dt), c.act, R.declared_tanh if dt == F32 else torch.tanh,
                     fault if epi_fault else None) for p in range(P)]


def tiled(t):
    """(B,C,h,w) with h % 8 == 0 and w % 32 == 0 -> (B,C,h/8,8,w/32,32); reduce over TILE_DIMS for one value per output tile."""
    b, c, h, w = t.shape
    return t.reshape(b, c, h // TH, TH, w // TW, TW)


TILE_DIMS, ROW_DIMS = (0, 1, 3, 5), (0, 1, 3)


def tiled_eval(ref, f32s):
    return {k: [tiled(t) for t in v] for k, v in ref.items()}, [{k: [tiled(t) for t in v] for k, v in d.items()} for d in f32s]


def exceeds(got, ref, f32s, key, floor, row_dims=None):
    """Whether `got` (list over planes) leaves the bar 4 * yardstick + floor * max|f64| somewhere, and the largest error / bar."""
    yard = R.yardstick(ref, f32s, key, row_dims)
    worst = 0.0
    for p in range(len(got)):
        e = R._pmax(got[p].double() - ref[key][p], row_dims)
        bar = 4.0 * torch.as_tensor(yard[p]) + floor * R._pmax(ref[key][p], row_dims)
        e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
        ratio = torch.where(e > bar, e / bar.clamp_min(1e-300), torch.zeros_like(e))
        worst = max(worst, float(ratio.max()))
    return worst > 0.0, worst


# ------------------------------------------------------------------------------------------------ the dense conv, its fp16-storage form, backward
CP, CIN, CCOUT, CH, CW = 3, 37, 150, 11, 45
PLANE_EXP = (0, -30, 30)


def conv_case(name, variant, act=ACT_NONE, bias=True, kind="conv", cin=CIN, cout=CCOUT, hw=(CH, CW), planes=CP, rows=False, scales=False):
    return types.SimpleNamespace(kind=kind, name=name, variant=variant, act=act, bias=bool(bias), cin=cin, cout=cout, hw=hw, planes=planes,
                                 rows=rows, scales=scales, tiles=False)


CONV_CASES = [conv_case("conv-planes3-none", "planes3", ACT_NONE, False, scales=True),
              conv_case("conv-planes3-relu", "planes3", ACT_RELU, False, scales=True),
              conv_case("conv-rows6-lrelu", "rows6", ACT_LRELU, False, rows=True),
              conv_case("conv-ragged-tanh", "ragged", ACT_TANH, True), conv_case("conv-ragged-relu", "ragged", ACT_RELU, True)]
IN16_CASES = [conv_case("in16-xscale-none", "xscale", ACT_NONE, True, kind="in16"), conv_case("in16-xscale-relu", "xscale", ACT_RELU, True, kind="in16"),
              conv_case("in16-f16out-lrelu", "f16out", ACT_LRELU, True, kind="in16", cin=CMID, cout=COUT, hw=(14, 38), planes=P)]
BWD_CASES = [conv_case("bwd-64to64-random", "dy", kind="adjoint", cin=64, cout=64, hw=(12, 40), planes=2),
             conv_case("bwd-70to97-random", "dy", kind="adjoint", cin=70, cout=97, hw=(12, 40), planes=2),
             conv_case("bwd-64to64-rows6", "dyrows6", kind="adjoint", cin=64, cout=64, hw=(12, 40), planes=2, rows=True),
             conv_case("bwd-70to97-rows6", "dyrows6", kind="adjoint", cin=70, cout=97, hw=(12, 40), planes=2, rows=True)]
WG_EXP_X, WG_EXP_DY = (-20, 0, 12), (12, -20, 0)
WGRAD_CASES = [conv_case("wgrad-70to97-magnitudes", "magnitudes", kind="wgrad", cin=70, cout=97, hw=(12, 40), planes=3, scales=True)]
_conv_cache = {}


def conv_inputs(c):
    """x (P,B,cin,h,w), w (P,cout,cin,3,3), b (P,cout) fp32 (adjoint: x is dpre (P,B,cout,h,w), w the forward weight; wgrad: x and dy;
    in16: x16 the stored fp16 values and xscale (P))."""
    if c.name in _conv_cache:
        return _conv_cache[c.name]
    g = _gen("conv", c.variant, c.cin, c.cout, c.hw)
    u = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    h, wd = c.hw
    Pn = c.planes
    d = types.SimpleNamespace()
    d.w = u(Pn, c.cout, c.cin, 3, 3) * (1.0 / (c.cin * 9) ** 0.5)
    for p in range(Pn):
        d.w[p] *= 2.0 ** p
    d.b = u(Pn, c.cout) * 0.5
    ramp = (10.0 ** (-6.0 * torch.arange(h) / (h - 1))).view(1, 1, 1, h, 1)
    if c.kind == "adjoint":
        d.x = u(Pn, B, c.cout, h, wd) * 1e-3
        if c.variant == "dyrows6":
            d.x = d.x * ramp
    elif c.kind == "wgrad":
        d.x = u(Pn, B, c.cin, h, wd) * 2 * (2.0 ** torch.tensor(WG_EXP_X, dtype=F32)).view(Pn, 1, 1, 1, 1)
        d.dy = u(Pn, B, c.cout, h, wd) * (2.0 ** torch.tensor(WG_EXP_DY, dtype=F32)).view(Pn, 1, 1, 1, 1)
    elif c.kind == "in16":
        d.xscale = 2.0 ** torch.tensor([9.0, 3.0, 12.0][:Pn])
        d.x16 = (u(Pn, B, c.cin, h, wd) * 2 * d.xscale.view(Pn, 1, 1, 1, 1)).half()       # f16out: replaced by the producer's output
        d.x = d.x16.float() / d.xscale.view(Pn, 1, 1, 1, 1)
    else:
        d.x = u(Pn, B, c.cin, h, wd) * 2
        if c.variant == "planes3":
            d.x = d.x * (2.0 ** torch.tensor(PLANE_EXP, dtype=F32)).view(Pn, 1, 1, 1, 1)
        elif c.variant == "rows6":
            d.x = d.x * ramp
    _conv_cache[c.name] = d
    return d


def conv_weight(c, d, p, dt):
    w = d.w[p].to(dt)
    return adjoint_weight(w) if c.kind == "adjoint" else w


def conv_evaluate(c, d):
    """(ref, f32s) with key 'y' for the conv / in16 / adjoint cases; 'dw', 'db' for the weight gradient."""
    Pn = c.planes
    if c.kind == "wgrad":
        def fn(p, dtype, tanh):
            if dtype == F64:
                dw, db = wgrad(d.x[p].double(), d.dy[p].double())
            else:
                w = torch.zeros(c.cout, c.cin, 3, 3, requires_grad=True)
                bz = torch.zeros(c.cout, requires_grad=True)
                dw, db = torch.autograd.grad((F.conv2d(d.x[p], w, bz, padding=1) * d.dy[p]).sum(), [w, bz])
            return {"dw": dw, "db": db}
        ax, ay = d.x.abs().amax(dim=(1, 2, 3, 4)), d.dy.abs().amax(dim=(1, 2, 3, 4))
        extra = tuple((lambda p, s=s: dict(zip(("dw", "db"), wgrad_chain(d.x[p], d.dy[p], 1.0, s)))) for s in (1, 4))
        extra += (lambda p: dict(zip(("dw", "db"), wgrad_split(d.x[p], d.dy[p], ax[p], ay[p]))),)
        return R.evaluate(fn, Pn, extra=extra)
    amax = d.x.abs().amax(dim=(1, 2, 3, 4))
    bias = d.b if c.bias and c.kind != "adjoint" else None
    lin64 = [conv3(d.x[p].double(), conv_weight(c, d, p, F64)) for p in range(Pn)]
    legs = [[conv3_torch(d.x[p], conv_weight(c, d, p, F32)) for p in range(Pn)],
            [conv3_chain(d.x[p], conv_weight(c, d, p, F32), 32) for p in range(Pn)]]
    if c.kind == "in16":
        legs.append([conv_split(d.x16[p].float(), d.w[p], None, in16_scale=d.xscale[p]) for p in range(Pn)])
    else:
        legs.append([conv_split(d.x[p], conv_weight(c, d, p, F32), amax[p]) for p in range(Pn)])
    return evaluate_epilogues(lin64, legs, bias, c.act, Pn)


def conv_faulty(c, d, fault):
    """The case with one planted fault -> dict of lists over planes."""
    Pn = c.planes
    nb = lambda p: (p + 1) % Pn
    if c.kind == "wgrad":
        ax, ay = d.x.abs().amax(dim=(1, 2, 3, 4)), d.dy.abs().amax(dim=(1, 2, 3, 4))
        if fault == "scale_launch":
            ax, ay = ax.max().expand(Pn), ay.max().expand(Pn)
        elif fault == "scale_plane":
            ax, ay = ax.roll(-1), ay.roll(-1)
        out = [wgrad_split(d.x[p], d.dy[p], ax[p], ay[p], fault=fault) for p in range(Pn)]
        return {"dw": [o[0] for o in out], "db": [o[1] for o in out]}
    bias = d.b if c.bias and c.kind != "adjoint" else None
    bz = lambda p, dt: None if bias is None else bias[p].to(dt)
    if fault in OPER_FAULTS:
        f_lin = fault if fault in ("chunk_live", "tap_swap") else None
        return {"y": [epilogue(conv3(d.x[p].double(), conv_weight(c, d, p, F64), f_lin), bz(p, F64), c.act, torch.tanh,
                               None if f_lin else fault) for p in range(Pn)]}
    if c.kind == "in16":
        xs = d.xscale.roll(-1) if fault == "scale_plane" else d.xscale
        lins = [conv_split(d.x16[p].float(), d.w[p], None, fault, in16_scale=xs[p]) for p in range(Pn)]
    else:
        amax = d.x.abs().amax(dim=(1, 2, 3, 4))
        if fault == "scale_launch":
            amax = amax.max().expand(Pn)
        elif fault == "scale_plane":
            amax = amax.roll(-1)
        lins = [conv_split(d.x[p], conv_weight(c, d, p, F32), amax[p], fault) for p in range(Pn)]
    return {"y": [epilogue(lins[p], bz(p, F32), c.act, R.declared_tanh) for p in range(Pn)]}


def bars(ref, f32s, key, floor):
    """Per plane: 4 * yardstick + floor * max|f64| (the rule of lift_ref.check)."""
    yard = R.yardstick(ref, f32s, key)
    return [4.0 * float(yard[p]) + floor * float(ref[key][p].abs().max()) for p in range(len(ref[key]))]
