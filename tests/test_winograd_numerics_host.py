"""Host: the split-fp16 emulation of tools/winograd_numerics.py -- the row-wise Winograd F(2,3) form of the tree-context conv
(csrc/conv_f16x3.hip k_plc_wino) stays at the direct form's accuracy, well inside the 2e-6-of-max|y| bar of the GPU tests."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import winograd_numerics as wn  # noqa: E402


@pytest.mark.parametrize("cin,cout,h,w", [(17, 5, 1, 1), (17, 5, 2, 3), (64, 40, 6, 9), (243, 243, 8, 35), (243, 20, 3, 1)])
def test_winograd_error_at_the_direct_level(cin, cout, h, w):
    ed, ew = wn.case(np.random.default_rng(cin + h + w), cin, cout, h, w)
    assert ew < 1e-6, (ed, ew)
    assert ew < 3 * ed + 2e-7, (ed, ew)


def test_transforms_are_exact_on_integers():
    """With small integers every product and sum is exact: the Winograd form equals the direct convolution bit for bit."""
    rng = np.random.default_rng(0)
    x = rng.integers(-3, 4, (5, 4, 7)).astype(np.float32)
    w = rng.integers(-2, 3, (6, 5, 3, 3)).astype(np.float32)
    assert np.array_equal(wn.conv_winograd(x, w), wn.ref64(x, w).astype(np.float32))
