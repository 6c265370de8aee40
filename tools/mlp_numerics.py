"""Host emulation of the split-fp16 subband MLP (csrc/subband_mlp_f16.hip) beside a plain fp32 one, against float64.

The emulation uses what the kernel uses: layers 0 and 3 in fp32; for the two 32 x 32 layers the weights times the power of
two s with max|W| s in [2^14, 2^15), the activations times 2^14, a round-to-nearest hi / lo fp16 split of both, the three
products lo*hi + hi*lo + hi*hi (each exact in fp32) accumulated in fp32 (each product summed in float64 and rounded once: the
MFMA keeps more than fp32 inside a k-step), the exact unscale 1 / (s 2^14) in the fma that adds the bias, and the tanh of
common.h (exp2 / rcp form) evaluated in fp32.  "fp32" is the same network with fp32 products accumulated in fp32.
Weights: the template weights of tests/test_gpu_ops.py::test_subband_mlp (Yh_ae.0, ae_down, plane prefix q0.), then the same
with every weight (not the biases) times 4 and times 16 (tanh saturation), inputs uniform in +-2 and in +-1e4.
Run: python tools/mlp_numerics.py  (numpy + the oracle's weight templates, no GPU)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
H = 32
f32 = np.float32


def pow2_scale(amax):
    """power of two s with amax * s in [2^14, 2^15), exponent clamped as in lldwt_subband_mlp_pack; 1 for 0 / non-finite"""
    if not (0.0 < amax < 3.0e38):
        return 1.0
    return float(2.0 ** min(max(15 - int(np.frexp(f32(amax))[1]), -113), 112))


def split(v):
    v = v.astype(f32)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(f32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def tanh32(x):
    """common.h fast_tanh in fp32 (numpy's exp2 stands for v_exp_f32, 1/x for v_rcp_f32: both within 1 ulp)"""
    x = x.astype(f32)
    with np.errstate(over="ignore"):                           # a huge |x| gives e = inf, r = 0, t = 1, as in the kernel
        e = np.exp2(np.abs(x) * f32(2.88539008177792681472)).astype(f32)
        r = (f32(1.0) / (e + f32(1.0))).astype(f32)
    t = (f32(1.0) - f32(2.0) * r).astype(f32)                 # fma(-2, r, 1): 2r is exact, one rounding
    return np.copysign(t, x)


def layer_split(W, b, h):
    """W (C,H,H) fp32, h (C,H,N) fp32 activations -> pre-activation, the kernel's arithmetic"""
    out = np.empty_like(h)
    for c in range(W.shape[0]):
        s = pow2_scale(float(np.abs(W[c]).max()))
        wh, wl = split(W[c] * f32(s))
        ah, al = split(h[c] * f32(16384.0))
        acc = (wl @ ah).astype(f32)
        acc = (acc + (wh @ al).astype(f32)).astype(f32)
        acc = (acc + (wh @ ah).astype(f32)).astype(f32)
        inv = f32(1.0 / (s * 16384.0))
        out[c] = (acc.astype(np.float64) * np.float64(inv) + b[c][:, None].astype(np.float64)).astype(f32)   # one fma
    return out


def layer_f32(W, b, h):
    out = np.empty_like(h)
    for c in range(W.shape[0]):
        acc = np.broadcast_to(b[c][:, None], h[c].shape).astype(f32)
        for k in range(H):                                       # fp32 accumulation in k order, bias first
            acc = (acc + (W[c][:, k:k + 1] * h[c][k:k + 1, :]).astype(f32)).astype(f32)
        out[c] = acc
    return out


def mlp(ws, x, layer):
    """ws: w0 (C,H) b0 (C,H) w1 (C,H,H) b1 w2 b2 w3 (C,H) b3 (C); x (C,N).  layer = None: float64."""
    w0, b0, w1, b1, w2, b2, w3, b3 = ws
    if layer is None:
        d = [a.astype(np.float64) for a in ws]
        h = np.tanh(d[0][:, :, None] * x[:, None, :].astype(np.float64) + d[1][:, :, None])
        h = np.tanh(np.einsum("cok,ckn->con", d[2], h) + d[3][:, :, None])
        h = np.tanh(np.einsum("cok,ckn->con", d[4], h) + d[5][:, :, None])
        return np.einsum("ck,ckn->cn", d[6], h) + d[7][:, None]
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)
    h = tanh32(fma(w0[:, :, None], x[:, None, :].astype(f32), b0[:, :, None]))
    h = tanh32(layer(w1, b1, h))
    h = tanh32(layer(w2, b2, h))
    o = np.zeros(x.shape, f32)
    for k in range(H):
        o = fma(w3[:, k:k + 1], h[:, k, :], o)
    return (o + b3[:, None]).astype(f32)


def template_weights():
    from oracle import model, weights
    cfg = dict(model.DEFAULT_CFG, dwtlevels=1)
    tpl = weights.autoencoder_template(cfg)
    get = lambda k: weights.fill_value("q0." + k, tpl[k]).to(tpl[k].dtype).reshape(tpl[k].shape).numpy().astype(f32)
    C = 3
    raw = [get("Yh_ae.0.ae_down.%d.%s" % (n, k)) for n in (0, 2, 4, 6) for k in ("weight", "bias")]
    return [raw[0].reshape(C, H), raw[1].reshape(C, H), raw[2].reshape(C, H, H), raw[3].reshape(C, H), raw[4].reshape(C, H, H),
            raw[5].reshape(C, H), raw[6].reshape(C, H), raw[7].reshape(C)]


def main():
    base = template_weights()
    rng = np.random.RandomState(0)
    N = 4096
    print("%-28s %-10s %-12s %-12s %s" % ("weights / inputs", "max|y|", "split-fp16", "fp32", "ratio"))
    for wname, k in (("template", 1.0), ("template x4", 4.0), ("template x16", 16.0)):
        ws = [a * f32(k) if i % 2 == 0 else a for i, a in enumerate(base)]
        for xname, amp in (("|x| <= 2", 2.0), ("|x| <= 1e4", 1e4)):
            x = ((rng.rand(3, N) * 2 - 1) * amp).astype(f32)
            x[:, 0] = 0.0
            ref = mlp(ws, x, None)
            es = float(np.abs(mlp(ws, x, layer_split) - ref).max())
            ef = float(np.abs(mlp(ws, x, layer_f32) - ref).max())
            print("%-28s %-10.3g %-12.3e %-12.3e %.2f" % (wname + ", " + xname, np.abs(ref).max(), es, ef, es / ef))


if __name__ == "__main__":
    main()
