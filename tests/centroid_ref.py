"""float64 restatement of the centroid offset of DESIGN.md 7.1.13, in numpy and ``math`` alone (no mpmath, no scipy):

    delta(a, s) = a - E[X | a - 1/2 <= X <= a + 1/2],   X ~ N(0, s^2),   a >= 0, s > 0        (0 <= delta <= 1/2, delta(0, s) = 0)

the distance, in steps, by which the mean-square-optimal reconstruction of a bin lies inside the bin's centre.  The three regimes
of csrc/recon.hip, with the same branch cuts (D = a / s^2 is the drop of the exponent across the bin):

  wide    s > S_CUT and D < D_CUT: the density over the bin is exp(-beta y - gamma y^2), y in [-1/2, 1/2], beta = D and
          gamma = 1 / (2 s^2) -- a uniform density tilted by beta and bent by gamma.  Folding y and -y together,
              delta = int_0^1/2 y exp(-gamma y^2) sinh(beta y) dy / int_0^1/2 exp(-gamma y^2) cosh(beta y) dy,
          delta itself and not a - E, every term positive; Gauss-Legendre on [0, 1/2] (the integrands are entire and flat there).
          gamma -> 0 gives the tilted uniform's coth(beta / 2) / 2 - 1 / beta, beta -> 0 gives a / (12 s^2).
  zero    otherwise, a < 1/2 (the bin holds the mode): a - s phi(l) (1 - exp(-D)) / (Phi(h) - Phi(l)) with the mass an erf SUM.
  tail    otherwise (a >= 1/2): everything divided by the density at the inner edge lo = a - 1/2.  With l = lo / s, w = 1 / s,
          h = l + w, t = exp(-D), the Mills ratio R(x) = (1 - Phi(x)) / phi(x) and K(x) = 1 / R(x) - x,
              delta = 1/2 - s (K(l) R(l) - t R(h) (K(h) + w)) / (R(l) - t R(h)),
          which tends to 1/2 - s K(l) = 1/2 - s^2 / lo + ... in the far tail, where both masses underflow.  K(x) is its continued
          fraction 1 / (x + 2 / (x + 3 / (x + ...))) for x >= X_CUT and 1 / R(x) - x below.
"""
import math

import numpy as np

S_CUT = 0.75                         # the cuts of csrc/recon.hip (DESIGN.md 7.1.13 says how they were chosen)
D_CUT = 4.0
X_CUT = 3.0
S_MIN = 0.11                         # the floor of the scale in steps, as the quantiser's
_GL = 16                             # Gauss-Legendre nodes of the wide regime here (the kernel takes fewer)
_CF = 120                            # depth of the continued fraction here
_SQRT_HALF_PI = math.sqrt(math.pi / 2.0)
_SQRT2 = math.sqrt(2.0)
_erf = np.frompyfunc(math.erf, 1, 1)
_erfc = np.frompyfunc(math.erfc, 1, 1)


def _mills(x):
    """(R, K) of x >= 0 (float64 array): the Mills ratio and K = 1 / R - x."""
    big = x >= X_CUT
    xs = np.where(big, X_CUT, x)                                    # below the cut: erfc scaled back up (no underflow here)
    r_small = _SQRT_HALF_PI * np.exp(0.5 * xs * xs) * _erfc(xs / _SQRT2).astype(np.float64)
    xb = np.where(big, x, X_CUT)
    k = np.zeros_like(xb)
    for n in range(_CF, 1, -1):                                     # K = 1 / (x + 2 / (x + 3 / (x + ...)))
        k = n / (xb + k)
    k_big = 1.0 / (xb + k)
    K = np.where(big, k_big, 1.0 / r_small - xs)
    R = np.where(big, 1.0 / (xb + k_big), r_small)
    return R, K


def _wide(a, s):
    beta, gamma = a / (s * s), 0.5 / (s * s)
    x, wt = np.polynomial.legendre.leggauss(_GL)
    num = np.zeros_like(a)
    den = np.zeros_like(a)
    for xi, wi in zip(0.25 * (x + 1.0), 0.25 * wt):
        g = wi * np.exp(-gamma * xi * xi)
        num += g * xi * np.sinh(beta * xi)
        den += g * np.cosh(beta * xi)
    return num / den


def _zero(a, s):
    l, h = (a - 0.5) / s, (a + 0.5) / s                             # l < 0 < h
    mass = 0.5 * (_erf(h / _SQRT2).astype(np.float64) + _erf(-l / _SQRT2).astype(np.float64))
    phi_l = np.exp(-0.5 * l * l) / math.sqrt(2.0 * math.pi)
    return a - s * phi_l * -np.expm1(-a / (s * s)) / mass


def _tail(a, s):
    l, w = (a - 0.5) / s, 1.0 / s
    t = np.exp(-a / (s * s))
    Rl, Kl = _mills(l)
    Rh, Kh = _mills(l + w)
    return 0.5 - s * (Kl * Rl - t * Rh * (Kh + w)) / (Rl - t * Rh)


def delta(a, s):
    """delta(a, s) for float64 arrays (or numbers) a >= 0, s > 0 of one shape -> float64 array."""
    a, s = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(s, dtype=np.float64))
    a, s = a.copy(), s.copy()
    wide = (s > S_CUT) & (a < D_CUT * s * s)
    zero = ~wide & (a < 0.5)
    tail = ~wide & ~zero
    out = np.empty_like(a)
    with np.errstate(all="ignore"):
        if wide.any():
            out[wide] = _wide(a[wide], s[wide])
        if zero.any():
            out[zero] = _zero(a[zero], s[zero])
        if tail.any():
            out[tail] = _tail(a[tail], s[tail])
    return np.clip(out, 0.0, 0.5)


def centroid(v, sigma, mu, q):
    """The reconstruction of DESIGN.md 7.1.13 in float64: v - sign(u) q delta(|u|, max(sigma / q, 0.11)), u = (v - mu) / q."""
    v, sigma, mu = (np.asarray(t, dtype=np.float64) for t in (v, sigma, mu))
    u = (v - mu) / q
    return v - np.sign(u) * q * delta(np.abs(u), np.maximum(sigma / q, S_MIN))


def mse_experiment(seed=0, n=65536, s_lo=0.11, s_hi=4.0):
    """The experiment of DESIGN.md 7.1.13: n values y ~ N(0, s^2), s log-uniform in [s_lo, s_hi] steps, quantised at step 1
    -> (y, s, centre MSE, centroid MSE)."""
    g = np.random.default_rng(seed)
    s = np.exp(g.uniform(math.log(s_lo), math.log(s_hi), n))
    y = g.standard_normal(n) * s
    v = np.rint(y)
    c = centroid(v, s, 0.0, 1.0)
    return y, s, float(np.mean((v - y) ** 2)), float(np.mean((c - y) ** 2))
