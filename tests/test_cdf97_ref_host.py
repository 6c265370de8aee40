"""CPU: tests/cdf97_ref.py (the float64 reference of the CDF 9/7 kernels) against the oracle's conv form, the PyWavelets
fixtures under tests/golden/ and the adjoint identity; that its bar notices a tap wrong by 1e-5; and that the table of
tests/test_gpu_cdf97_domain.py covers the dispatch of csrc/cdf97.hip.  Prints every yardstick (pytest -s)."""
import os

import numpy as np
import pytest
import torch

import cdf97_ref as C
import test_gpu_cdf97_domain as G
from helpers import GOLDEN


def _rand(shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=C.F64) - 0.5


def _multi_level_shapes():
    """Every multi-level shape of the GPU file whose level inputs all have 10 or more samples."""
    rows = [(m[0], m[1], m[2], m[3]) for m in G.MULTI] + [(a[0], a[1], a[2], a[3]) for a in G.ADJOINT] + list(G.FUNCTIONS)
    return sorted({(pbc[0] * pbc[1] * pbc[2], H, W, L) for pbc, H, W, L in rows if L > 1 and C.conv_form_applies(H, W, L)})


def test_periodic_form_equals_conv_form_in_float64():
    """Same transform, other summation order: double rounding over about 40 operations, 1e-12 of the largest value."""
    shapes = _multi_level_shapes()
    assert (4, 144, 208, 4) in shapes and (6, 160, 96, 3) in shapes and (2, 144, 208, 3) in shapes
    for Z, H, W, L in shapes:
        x = _rand((Z, H, W), H + W)
        a, b = C.analysis(x, L, C.F64, True), C.analysis(x, L, C.F64, False)
        for k in a:
            d, m = float((a[k] - b[k]).abs().max()), float(a[k].abs().max())
            print("%dx%dx%d L%d %-4s periodic - conv %.2e  max %.2e" % (Z, H, W, L, k, d, m))
            assert d <= 1e-12 * m, (Z, H, W, L, k)
        xa, xb = C.synthesis(a, C.F64, True)["x"], C.synthesis(a, C.F64, False)["x"]
        assert float((xa - xb).abs().max()) <= 1e-12 * float(xa.abs().max()), (Z, H, W, L)


def test_periodic_form_equals_the_pywavelets_fixtures():
    """To the precision the fixtures are stored in: float64 arrays written by PyWavelets, compared here at 1e-12 of the
    largest coefficient (PyWavelets sums its taps in its own order)."""
    z = np.load(os.path.join(GOLDEN, "cdf97_pywt.npz"))
    x = torch.tensor(z["x"])
    assert x.dtype == C.F64 and z["ll"].dtype == np.float64
    co = C.analysis(x, 2, C.F64)
    want = {"ll": z["ll"]}
    want.update({"%s%d" % (b, i): z["%s%d" % (b, i)] for i in range(2) for b in C.BANDS})
    for k, v in want.items():
        w = torch.tensor(v).reshape(co[k].shape)
        assert float((co[k] - w).abs().max()) <= 1e-12 * float(w.abs().max()), k
    z = np.load(os.path.join(GOLDEN, "cdf97_pywt_small.npz"))
    for name in "abcd":
        x, lev = torch.tensor(z[name + "_x"]), int(z[name + "_levels"])
        assert x.dtype == C.F64
        assert not C.conv_form_applies(x.shape[-2], x.shape[-1], lev)          # the short levels only the periodic form states
        co = C.analysis(x, lev, C.F64)
        ll, yh = C.from_dict(co, lead=x.shape[:2])
        assert float((ll - torch.tensor(z[name + "_ll"])).abs().max()) <= 1e-12 * float(ll.abs().max()), name
        for i in range(lev):
            w = torch.tensor(z["%s_yh%d" % (name, i)])
            assert float((yh[i] - w).abs().max()) <= 1e-12 * max(float(w.abs().max()), float(x.abs().max())), (name, i)
        assert float((C.synthesis(co, C.F64)["x"].reshape(x.shape) - x).abs().max()) <= 1e-10, name


@pytest.mark.parametrize("Z,H,W,L", [(2, 12, 20, 1), (2, 68, 136, 1), (1, 144, 208, 3), (2, 6, 4, 1), (2, 24, 16, 3)])
def test_adjoint_identity(Z, H, W, L):
    """<A x, g> == <x, A^T g> and <S c, gx> == <c, S^T gx> in float64 to 1e-12 ||.|| ||.||: the autograd adjoints are the
    adjoints of the operators they are taken from.  6 x 4 is one short level; 24 x 16 ends on a 6 x 4 level input."""
    x, gx = _rand((Z, H, W), 1), _rand((Z, H, W), 2)
    g = {k: _rand(v.shape, 3 + i) for i, (k, v) in enumerate(C.analysis(x, L, C.F64).items())}
    c = {k: _rand(v.shape, 40 + i) for i, (k, v) in enumerate(g.items())}
    dot = lambda a, b: sum(float((a[k] * b[k]).sum()) for k in a)
    norm = lambda a: sum(float((v * v).sum()) for v in a.values()) ** 0.5
    lhs, rhs = dot(C.analysis(x, L, C.F64), g), dot({"x": x}, C.analysis_adjoint(g, C.F64))
    print("analysis  %dx%dx%d L%d  <Ax,g> - <x,A^T g> = %.2e" % (Z, H, W, L, lhs - rhs))
    assert abs(lhs - rhs) <= 1e-12 * norm({"x": x}) * norm(g)
    lhs, rhs = dot(C.synthesis(c, C.F64), {"x": gx}), dot(c, C.synthesis_adjoint(gx, L, C.F64))
    print("synthesis %dx%dx%d L%d  <Sc,gx> - <c,S^T gx> = %.2e" % (Z, H, W, L, lhs - rhs))
    assert abs(lhs - rhs) <= 1e-12 * norm(c) * norm({"x": gx})
    if C.conv_form_applies(H, W, L):                                           # the conv form differentiates to the same adjoint
        a, b = C.analysis_adjoint(g, C.F64, True)["x"], C.analysis_adjoint(g, C.F64, False)["x"]
        assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())
        a, b = C.synthesis_adjoint(gx, L, C.F64, True), C.synthesis_adjoint(gx, L, C.F64, False)
        assert all(float((a[k] - b[k]).abs().max()) <= 1e-12 * float(a[k].abs().max()) for k in a)


def test_the_bar_has_teeth():
    """An fp32 evaluation with one tap wrong by 1e-5 relative -- a slip in one of the two copies of the taps in csrc/cdf97.hip
    -- is outside the bar on 3 x 68 x 136 and inside the 5e-5 the suite asked before; the unchanged fp32 evaluation is inside
    the bar.  Analysis: DEC_LO[5]; synthesis: REC_LO[4], judged by the inverse's bar."""
    x = G.make_input("uniform", 3, 68, 136)
    ref, f32s = C.evaluate(lambda dt, per: C.analysis(x, 1, dt, per), True)
    assert not C.check("analysis, fp32 oracle", f32s[0], ref, f32s, C.plane_max(x))
    with C.perturbed_taps("DEC_LO", 5, 1 + 1e-5):
        wrong = C.analysis(x, 1, C.F32)
    assert wrong["ll"].dtype == C.F32
    bad = C.check("analysis, DEC_LO[5] * (1 + 1e-5)", wrong, ref, f32s, C.plane_max(x))
    assert {b[1] for b in bad} == {"ll", "lh0", "hl0"} and {b[2] for b in bad} == {0, 1, 2}  # the bands the low-pass filter feeds
    assert max(float((wrong[k].double() - ref[k]).abs().max()) for k in ref) < 5e-5
    assert torch.equal(C.analysis(x, 1, C.F32)["ll"], f32s[0]["ll"])           # the taps are restored

    co = C.cast(ref, C.F32)
    iref, if32s = C.evaluate(lambda dt, per: C.synthesis(co, dt, per), True)
    assert not C.check("synthesis, fp32 oracle", if32s[0], iref, if32s, C.input_max(co))
    with C.perturbed_taps("REC_LO", 4, 1 + 1e-5):
        wrong = C.synthesis(co, C.F32)
    bad = C.check("synthesis, REC_LO[4] * (1 + 1e-5)", wrong, iref, if32s, C.input_max(co))
    assert {b[2] for b in bad} == {0, 1, 2}
    assert float((wrong["x"].double() - iref["x"]).abs().max()) < 5e-5


def test_an_unwritten_element_is_outside_the_bar():
    x = G.make_input("uniform", 3, 12, 20)
    ref, f32s = C.evaluate(lambda dt, per: C.analysis(x, 1, dt, per), True)
    got = {k: v.clone() for k, v in f32s[0].items()}
    got["hh0"][1, 2, 3] = float("nan")
    assert [b[:3] for b in C.check("NaN", got, ref, f32s, C.plane_max(x))] == [("NaN", "hh0", 1)]


def test_the_table_covers_the_dispatch():
    """The GPU file's rows name every value expected_kernel can return, each row states its own dispatch, and every threshold
    of lldwt_cdf97_forward / lldwt_cdf97_inverse has a row on either side."""
    rows = [(p[0] * p[1] * p[2], H, W, f, i) for p, H, W, f, i, _ in G.ROWS]
    for Z, H, W, f, i in rows:
        assert C.expected_kernel("forward", False, Z, H, W) == f and C.expected_kernel("inverse", False, Z, H, W) == i
    named = {r[3] for r in rows} | {r[4] for r in rows}
    named |= {C.expected_kernel("forward", True, a[0][0] * a[0][1] * a[0][2], a[1], a[2]) for a in G.ADJOINT}
    assert named == set(C.KERNELS)
    for kernel in C.KERNELS[1:]:                                               # the scaled and special planes reach every branch
        assert any(kernel in (f, i) for _, _, _, f, i, extra in G.ROWS if extra), kernel
    fast = [(C.square_tiles(Z, H, W), f, i) for Z, H, W, f, i in rows if f in (G.V8, G.V16, G.V32)]
    # 199 / 200 tiles (forward only) and 4095 / 4096 tiles (both directions): the nearest counts on either side that whole
    # planes give (one tile per 64 x 64 plane, six per 68 x 136 plane)
    assert (199, G.V8, G.I16) in fast and (200, G.V16, G.I16) in fast
    assert (4092, G.V16, G.I16) in fast and (4098, G.V32, G.I32) in fast
    assert C.expected_kernel("forward", False, 4095, 64, 64) == G.V16 and C.expected_kernel("forward", False, 4096, 64, 64) == G.V32
    assert C.expected_kernel("inverse", False, 4095, 64, 64) == G.I16 and C.expected_kernel("inverse", False, 4096, 64, 64) == G.I32
    shape = {(H, W): (f, i) for Z, H, W, f, i in rows if Z <= 3}
    # 62 / 64 samples: the size limit of the fast kernels in both directions
    assert shape[(62, 64)] == (G.MOD, G.INV) and shape[(64, 64)] == (G.V8, G.I16)
    # w % 4: 66 x 70 and 72 x 74 against 70 x 72 and 68 x 136; 72 samples: mod against conditional wrap
    assert shape[(66, 70)][0] == G.MOD and shape[(72, 70)][0] == G.MOD and shape[(72, 74)][0] == G.WRAP
    assert shape[(70, 72)][0] == G.V8 and 70 % 4 == 2 and 74 % 4 == 2 and 72 % 4 == 0
    # wh % 2: 72 x 70 (35 wide subbands) against 70 x 72 (36 wide), both with subband sides of 32 or more
    assert shape[(72, 70)][1] == G.INV and shape[(70, 72)][1] == G.I16
    # the generic inverse below and above its 36-sample patch
    assert any(i == G.INV and min(H, W) // 2 < 36 for _, H, W, _, i in rows)
    assert any(i == G.INV and min(H, W) // 2 >= 36 for _, H, W, _, i in rows)
    # the multi-level rows mix kernels: two levels on the fast kernels, two on the generic ones
    pbc, H, W, L, _ = G.MULTI[0]
    per_level = [C.expected_kernel("forward", False, pbc[0] * pbc[1] * pbc[2], h, w) for h, w in C.level_inputs(H, W, L)]
    assert per_level == [G.V8, G.V8, G.MOD, G.MOD]
    # more than 2048 rows for grid2d's row loop
    assert any(a[1] > 2 * 2048 for a in G.ADJOINT)
