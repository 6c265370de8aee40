"""How the branch cuts of the centroid kernel (csrc/recon.hip) were chosen: the kernel's three regimes restated
in numpy float32 -- every operation rounded to fp32, erfcxf / erff taken from scipy in float64 and rounded, which is the best a
device library can do -- and scanned over the cuts against the float64 reference tests/centroid_ref.py on 600 000 seeded
(a, s).  Host only; the figure a cut is finally held to is measured on the device (tests/test_gpu_centroid_domain.py).

    python tools/centroid_cuts.py

Prints, per (S_CUT, D_CUT, Gauss-Legendre nodes, X_CUT, continued-fraction depth), the largest error of each regime in steps."""
import math
import os
import sys

import numpy as np
from scipy.special import erf, erfcx

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import centroid_ref as cr  # noqa: E402

f32 = np.float32


def mills32(x, x_cut, depth):
    big = x >= f32(x_cut)
    xs = np.where(big, f32(x_cut), x)
    r = f32(math.sqrt(math.pi / 2)) * erfcx((xs * f32(1 / math.sqrt(2))).astype(np.float64)).astype(f32)
    xb = np.where(big, x, f32(x_cut))
    y = f32(1) / xb
    z = y * y
    num, den = f32(1) + f32(depth) * z, np.ones_like(y)
    for n in range(depth - 1, 1, -1):
        num, den = num + f32(n) * z * den, num
    return np.where(big, y * num / (num + z * den), r), np.where(big, y * den / num, f32(1) / r - xs)


def delta32(a, s, s_cut, d_cut, x_cut, nodes, depth):
    w = f32(1) / s
    D = a * w * w
    wide = (s > f32(s_cut)) & (D < f32(d_cut))
    zero = ~wide & (a < f32(0.5))
    gamma = f32(0.5) * w * w
    x, wt = np.polynomial.legendre.leggauss(nodes)
    num, den = np.zeros_like(a), np.zeros_like(a)
    with np.errstate(all="ignore"):
        for xi, wi in zip((0.25 * (x + 1)).astype(f32), (0.25 * wt).astype(f32)):
            g = wi * np.exp(-(gamma * (xi * xi)))
            e = np.exp(D * xi)
            ie = f32(1) / e
            num += g * xi * (e - ie)
            den += g * (e + ie)
        l, h = (a - f32(0.5)) / s, (a + f32(0.5)) / s
        r2 = f32(1 / math.sqrt(2))
        mass = f32(0.5) * (erf((h * r2).astype(np.float64)).astype(f32) + erf((-l * r2).astype(np.float64)).astype(f32))
        d_zero = a - s * (np.exp(-(f32(0.5) * l * l)) * f32(1 / math.sqrt(2 * math.pi))) * -np.expm1(-D) / mass
        lt = np.maximum(l, f32(0))
        Rl, Kl = mills32(lt, x_cut, depth)
        Rh, Kh = mills32(lt + w, x_cut, depth)
        r = np.exp(-D) * (Rh / Rl)
        d_tail = f32(0.5) - s * ((Kl - r * (Kh + w)) / (f32(1) - r))
    return np.where(wide, num / den, np.where(zero, d_zero, d_tail)), wide, zero


def main():
    g = np.random.default_rng(2)
    n = 600000
    s = np.exp(g.uniform(math.log(0.11), math.log(16.0), n)).astype(f32)
    a = np.where(g.random(n) < 0.6, g.uniform(0, 12, n), np.exp(g.uniform(math.log(1e-3), math.log(4096.0), n))).astype(f32)
    ref = cr.delta(a.astype(np.float64), s.astype(np.float64))
    for s_cut in (0.5, 0.75, 1.0, 1.5, 2.0, 3.0):
        for d_cut in (2.0, 4.0, 8.0):
            for nodes in (4, 5, 6):
                for x_cut, depth in ((2.0, 16), (2.0, 24), (3.0, 8), (3.0, 12), (3.0, 16), (4.0, 8)):
                    d, wide, zero = delta32(a, s, s_cut, d_cut, x_cut, nodes, depth)
                    e = np.abs(d.astype(np.float64) - ref)
                    tail = ~wide & ~zero
                    print("S_CUT %.2f D_CUT %g GL %d X_CUT %g CF %2d | wide %.2e zero %.2e tail %.2e | max %.2e"
                          % (s_cut, d_cut, nodes, x_cut, depth, e[wide].max(), e[zero].max(), e[tail].max(), e.max()))


if __name__ == "__main__":
    main()
