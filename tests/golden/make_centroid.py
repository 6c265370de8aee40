"""Generates tests/golden/centroid_delta.npz with mpmath (1.3.0) at 60 digits: the centroid offset of DESIGN.md 7.1.13,

    delta(a, s) = a - E[X | a - 1/2 <= X <= a + 1/2],   X ~ N(0, s^2),

on a grid of (a, s), rounded to float64.  For a >= 1/2 the density is integrated over z = x - lo in [0, 1] SCALED by its value at
the bin's inner edge lo = a - 1/2, g(z) = exp(-(lo z + z^2 / 2) / s^2), so that nothing underflows however far out the bin
lies (the unscaled density is 0 in any fixed exponent range at s = 0.11, a = 40), and delta = 1/2 - int z g / int g.  For
a < 1/2 the mode lies inside the bin and the density is scaled by its value there (1).  The integrals are tanh-sinh quadratures
split at multiples of the decay length of g; each point is checked against the closed form in erfc, evaluated at 120 digits
where its cancellations do no harm.  Run from the repository root: python tests/golden/make_centroid.py"""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 60
A = [0.0, 1e-6, 0.25, 0.5 - 2.0 ** -20, 0.5, 0.5 + 2.0 ** -20, 1.0, 1.5, 2.0, 3.0, 8.0, 8.37, 40.0, 100.0, 1000.0, 4095.0, 4095.5]
S = np.geomspace(0.11, 2.0 ** 22, 102)
S[0], S[-1] = 0.11, 2.0 ** 22
S = np.concatenate((S, [0.5, 1.0, 1.5, 2.0, 4.0, 16.0, 256.0, 256.0 * 16 * 81]))       # round scales and the widest under layers


def splits(lo, hi, rate):
    """[lo, hi] cut at lo + 2^k / rate: an integrand that decays at ``rate`` is flat on every piece in units of its own length."""
    pts, step = [lo], 1 / rate
    while pts[-1] + step < hi and len(pts) < 64:
        pts.append(pts[-1] + step)
        step *= 2
    return pts + [hi]


def delta_quad(a, s):
    a, s = mp.mpf(a), mp.mpf(s)
    if a >= mp.mpf(1) / 2:
        lo = a - mp.mpf(1) / 2
        g = lambda z: mp.exp(-(lo * z + z * z / 2) / (s * s))
        pts = splits(mp.mpf(0), mp.mpf(1), max(lo / (s * s), 1 / s, mp.mpf(1)))
        return mp.mpf(1) / 2 - mp.quad(lambda z: z * g(z), pts) / mp.quad(g, pts)
    g = lambda x: mp.exp(-x * x / (2 * s * s))                     # the mode is inside: scaled by the density at 0
    neg = [-p for p in reversed(splits(mp.mpf(0), mp.mpf(1) / 2 - a, 1 / s))]
    pts = neg[:-1] + splits(mp.mpf(0), a + mp.mpf(1) / 2, 1 / s)
    return a - mp.quad(lambda x: x * g(x), pts) / mp.quad(g, pts)


def delta_closed(a, s):
    with mp.workdps(120):
        a, s = mp.mpf(a), mp.mpf(s)
        l, h = (a - mp.mpf(1) / 2) / s, (a + mp.mpf(1) / 2) / s
        mass = (mp.erfc(l / mp.sqrt(2)) - mp.erfc(h / mp.sqrt(2))) / 2
        return a - s * (mp.npdf(l) - mp.npdf(h)) / mass


def main():
    out = np.empty((len(A), len(S)), dtype=np.float64)
    worst = mp.mpf(0)
    for i, a in enumerate(A):
        for j, s in enumerate(S):
            d = delta_quad(a, float(s))
            worst = max(worst, abs(d - delta_closed(a, float(s))))
            assert -mp.mpf(10) ** -40 <= d <= mp.mpf(1) / 2, (a, s, d)
            out[i, j] = 0.0 if a == 0 else float(d)                # delta(0, s) = 0 by symmetry, the quadrature leaves 1e-60
    assert worst < mp.mpf(10) ** -40, worst
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "centroid_delta.npz")
    np.savez_compressed(path, a=np.array(A, dtype=np.float64), s=S.astype(np.float64), delta=out)
    print("ok mpmath %s, %d x %d points, quadrature against closed form: %s" % (mp.__version__, len(A), len(S), mp.nstr(worst, 3)))


if __name__ == "__main__":
    main()
