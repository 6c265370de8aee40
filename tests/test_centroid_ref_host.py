"""Host: the float64 restatement of the centroid offset (tests/centroid_ref.py) against the 60-digit fixture
tests/golden/centroid_delta.npz (tests/golden/make_centroid.py), its range and monotonicity, and the experiment that shows what
the reconstruction is worth when the model is right."""
import os

import numpy as np

import centroid_ref as cr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "centroid_delta.npz")
REQUIRED_A = [0.0, 1e-6, 0.25, 0.5 - 2.0 ** -20, 0.5, 0.5 + 2.0 ** -20, 1.0, 1.5, 2.0, 3.0, 8.0, 8.37, 40.0, 100.0, 1000.0, 4095.0, 4095.5]


def _grid():
    f = np.load(GOLDEN)
    a, s = np.meshgrid(f["a"], f["s"], indexing="ij")
    return f["a"], f["s"], a, s, f["delta"]


def test_the_fixture_holds_the_grid_the_design_asks_for():
    a, s, _, _, d = _grid()
    assert a.tolist() == REQUIRED_A and d.shape == (a.size, s.size) and d.dtype == np.float64
    assert s.min() == 0.11 and s.max() == 2.0 ** 22 and 256.0 * 16 * 81 in s.tolist()
    assert np.diff(np.log(np.sort(s))).max() < np.log(2.0) / 2                  # at least two scales per octave, end to end
    assert os.path.getsize(GOLDEN) < 64 * 1024


def test_the_reference_equals_the_fixture_to_1e_12():
    """float64 against 60 digits: a point that misses means a wrong branch in the reference."""
    _, _, a, s, d = _grid()
    got = cr.delta(a, s)
    err = np.abs(got - d)
    wide = (s > cr.S_CUT) & (a < cr.D_CUT * s * s)
    zero = ~wide & (a < 0.5)
    for name, m in (("wide", wide), ("zero", zero), ("tail", ~wide & ~zero)):
        assert m.any()                                                          # the grid reaches every regime
        k = np.argmax(np.where(m, err, -1.0))
        print("%s: %d points, max |reference - fixture| = %.3g at a = %g, s = %g" % (name, int(m.sum()), err.ravel()[k], a.ravel()[k],
                                                                                      s.ravel()[k]))
    assert float(err.max()) <= 1e-12


def test_range_zero_and_monotonicity():
    _, _, a, s, d = _grid()
    for t in (d, cr.delta(a, s)):
        assert float(t.min()) >= 0.0 and float(t.max()) <= 0.5
        assert np.all(t[0] == 0.0)                                              # delta(0, s) = 0 exactly
        assert np.all(np.diff(t, axis=0) >= 0.0)                                # non-decreasing in a at fixed s
        assert np.all(t[1:] > 0.0)
    # the far tail, where both Gaussian masses underflow even in float64: 1/2 - s^2 / (a - 1/2)
    assert abs(float(cr.delta(40.0, 0.11)) - (0.5 - 0.11 ** 2 / 39.5)) < 1e-6
    # wide sigma: a / (12 s^2)
    assert abs(float(cr.delta(3.0, 4096.0)) * 12 * 4096.0 ** 2 / 3.0 - 1.0) < 1e-6


def test_the_experiment_reproduces():
    """65 536 values from N(0, s^2), s log-uniform in [0.11, 4] steps, quantised at step 1."""
    _, _, centre, centroid = cr.mse_experiment()
    print("centre %.5f centroid %.5f ratio %.3f" % (centre, centroid, centroid / centre))
    assert "%.5f" % centre == "0.06898" and "%.5f" % centroid == "0.06240" and "%.3f" % (centroid / centre) == "0.904"
    _, _, centre, centroid = cr.mse_experiment(s_hi=1.0)                       # narrow scales gain more: 0.838 on this draw
    assert abs(centroid / centre - 0.838) < 5e-4
