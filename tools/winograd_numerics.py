"""Host emulation of the split-fp16 ("f16x3") second tree conv, direct vs row-wise Winograd F(2,3).

Both forms use what the kernels use: power-of-two operand scales (the Winograd input V = B^T d spans up to 2 max|d|, so
its scale is half the direct one; the weight scale comes from max|U|), a round-to-nearest hi / lo fp16 split, three
products per MAC (hi*hi + hi*lo + lo*hi, each exact in fp32) and fp32 accumulation.  Errors are relative to max|y| of a
float64 reference.  Run: python tools/winograd_numerics.py  (numpy only, no GPU)."""
import numpy as np


def pow2_scale(amax):
    """power of two s with amax * s in [2^14, 2^15) (the kernels' pow2_scale_for)"""
    if not amax > 0:
        return 1.0
    _, e = np.frexp(amax)
    return float(2.0 ** (15 - int(e)))


def split(v):
    hi = v.astype(np.float16)
    lo = (v.astype(np.float32) - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float32), lo.astype(np.float32)


def mac3(a, b, eq):
    """sum of the three split products of einsum(eq, a, b), each product exact, accumulated in fp32"""
    ah, al = split(a)
    bh, bl = split(b)
    out = np.einsum(eq, al, bh, dtype=np.float32)
    out = out + np.einsum(eq, ah, bl, dtype=np.float32)
    return out + np.einsum(eq, ah, bh, dtype=np.float32)


def winograd_weights(w):
    """(cout, cin, 3, 3) -> U (cout, cin, 3 dy, 4 xi), in float64"""
    w = w.astype(np.float64)
    g0, g1, g2 = w[..., 0], w[..., 1], w[..., 2]
    return np.stack([g0, (g0 + g1 + g2) / 2, (g0 - g1 + g2) / 2, g2], axis=-1)


def conv_direct(x, w):
    cin, h, wd = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1)))
    sx, sw = pow2_scale(np.abs(x).max()), pow2_scale(np.abs(w).max())
    xs, ws = (xp * sx).astype(np.float32), (w * sw).astype(np.float32)
    y = np.zeros((w.shape[0], h, wd), np.float32)
    for dy in range(3):
        for dx in range(3):
            y += mac3(ws[:, :, dy, dx], xs[:, dy:dy + h, dx:dx + wd], "oc,chw->ohw")
    return y / np.float32(sx * sw)


def conv_winograd(x, w):
    cin, h, wd = x.shape
    wpair = (wd + 1) // 2
    xp = np.zeros((cin, h + 2, 2 * wpair + 2), np.float32)      # one-pixel rim, overhanging pair reads zeros
    xp[:, 1:h + 1, 1:wd + 1] = x
    u = winograd_weights(w)
    sx, sw = pow2_scale(np.abs(x).max()) / 2, pow2_scale(np.abs(u).max())
    us = (u * sw).astype(np.float32)
    d = [xp[:, :, k:k + 2 * wpair:2] for k in range(4)]         # d_k of every pixel pair, (cin, h + 2, wpair)
    v = np.stack([d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]], axis=-1) * np.float32(sx)   # fp32, then scaled
    m = np.zeros((4, w.shape[0], h, wpair), np.float32)
    for dy in range(3):
        for xi in range(4):
            m[xi] += mac3(us[:, :, dy, xi], v[:, dy:dy + h, :, xi], "oc,chw->ohw")
    y = np.empty((w.shape[0], h, 2 * wpair), np.float32)
    y[:, :, 0::2] = m[0] + m[1] + m[2]
    y[:, :, 1::2] = m[1] - m[2] - m[3]
    return y[:, :, :wd] / np.float32(sx * sw)


def ref64(x, w):
    cin, h, wd = x.shape
    xp = np.pad(x.astype(np.float64), ((0, 0), (1, 1), (1, 1)))
    y = np.zeros((w.shape[0], h, wd))
    for dy in range(3):
        for dx in range(3):
            y += np.einsum("oc,chw->ohw", w[:, :, dy, dx].astype(np.float64), xp[:, dy:dy + h, dx:dx + wd])
    return y


def case(rng, cin, cout, h, wd):
    """a first-conv-like input (LeakyReLU of a random field) and the second conv's weights, as the tests draw them"""
    x = rng.uniform(-2.0, 2.0, (cin, h, wd)).astype(np.float32)
    x = np.where(x > 0, x, 0.01 * x).astype(np.float32)
    w = ((rng.random((cout, cin, 3, 3)) - 0.5) * (2.0 / (cin * 9) ** 0.5)).astype(np.float32)
    r = ref64(x, w)
    s = np.abs(r).max()
    return (float(np.abs(conv_direct(x, w) - r).max() / s), float(np.abs(conv_winograd(x, w) - r).max() / s))


def main():
    rng = np.random.default_rng(3)
    shapes = [(17, 5, 2, 2), (64, 40, 6, 9), (100, 129, 14, 33), (243, 243, 16, 35), (256, 40, 80, 140), (243, 243, 8, 1)]
    print("%-22s %12s %12s" % ("cin cout h w", "direct", "winograd"))
    worst = 0.0
    for cin, cout, h, wd in shapes:
        ed, ew = case(rng, cin, cout, h, wd)
        worst = max(worst, ew)
        print("%-22s %12.3g %12.3g" % ("%d %d %d %d" % (cin, cout, h, wd), ed, ew))
    print("worst winograd error / max|y|: %.3g" % worst)


if __name__ == "__main__":
    main()
