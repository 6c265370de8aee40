"""Host: the float64 reference of the context MLP (tests/cgp_ref.py) against the oracle, its backward against central differences,
and the figures the GPU file (tests/test_gpu_cgp_domain.py) is read against: the fp32 yardstick of every input set and, for every
weight set, the error of the emulated split chain (cgp_ref.chain_split) beside it.  No device code runs here."""
import types

import pytest
import torch
import torch.nn.functional as F

import cgp_ref as R
from oracle import entropy, weights

F64, F32 = torch.float64, torch.float32
G = 3
SHAPES = ((3, 5), (8, 8), (37, 53), (33, 64))


def _level_sd(seed_prefix="model0.entropymodel."):
    cfg = dict(dwtlevels=2, clrch=1, entropy_layer="conditioned2ZTsepSubbands")
    sd = weights.entropy_template(cfg)
    filled = weights.fill_by_name({seed_prefix + k: v for k, v in sd.items()})
    return {k[len(seed_prefix):]: v for k, v in filled.items()}, cfg


def _oracle_level_inputs(sd, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(2, G, h, w, generator=g) * 4
    x1 = torch.randn(2, G, h // 2, w // 2, generator=g) * 4
    xe = torch.randn(2, 1, h // 2, w // 2, generator=g) * 4
    # the oracle's own lines for the tree context (conditioned2_forward :208-215)
    con = entropy.upsample2(entropy.quantize(x1, "dequantize"))
    plc = F.conv2d(con, sd["plc_list.0.0.weight"], sd["plc_list.0.0.bias"], padding=1)
    plc = F.conv2d(F.leaky_relu(plc, 0.01), sd["plc_list.0.2.weight"], sd["plc_list.0.2.bias"], padding=1)
    return xe, x0, x1, plc, entropy.quantize(x0, "dequantize")


def test_unfolded_restatement_is_the_oracle_bit_for_bit():
    """cgp_ref.unfolded_forward in fp32 against conditioned2_forward: the rate-domain residual x - mu (dbg) and the bits of every
    coefficient of the tree level, by torch.equal."""
    sd, cfg = _level_sd()
    xe, x0, x1, plc, xq = _oracle_level_inputs(sd, 12, 20, 1)
    dbg = {}
    _, si, _, _ = entropy.conditioned2_forward(xe, [x0, x1], sd, cfg, dbg=dbg)
    params = R.unfolded_forward(plc, xq, sd, 0)
    sigma, mu = params[:, 0::2], params[:, 1::2]
    assert torch.equal(x0 - mu, dbg[0])
    _, p = entropy.gaussian_conditional_forward(x0, sigma, mu, False)
    assert torch.equal(-torch.log2(p), si[0])


def _abs_bound(cat, ws, bs, eps):
    """What rounding every folded layer-0 weight and bias to fp32 (relative eps) can move params by: the perturbation of layer 0's
    output carried through |W_1|, |W_2|, |W_3| (LeakyReLU is 1-Lipschitz)."""
    t = eps * F.conv2d(cat.abs(), ws[0].abs()[:, :, None, None], bs[0].abs(), groups=G)
    for l in (1, 2, 3):
        t = F.conv2d(t, ws[l].abs()[:, :, None, None], None, groups=G)
    return t


def test_folded_reference_equals_the_unfolded_oracle_path(monkeypatch):
    """The project's _fold_csc_into_cgp gives cgp_ref.fold's tensors, and the reference on them equals the unfolded path in
    float64 up to the fold's own rounding of layer 0 to fp32 (bounded element by element, 2^-24 per weight)."""
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models import LiftingBasedDWT_net as net
    sd, _ = _level_sd()
    got = {}

    def capture(ws, bs, groups):                                # the fp32 pack needs a device: keep what it would have packed
        got.update(ws=ws, bs=bs)
        return None, (93, 162, 54, 18)
    monkeypatch.setattr(ops, "cgp_pack", capture)
    monkeypatch.setattr(ops, "cgp16_supported", lambda ws, groups, bs=None: False)
    mod = lambda w, b: types.SimpleNamespace(weight=w, bias=b, kernel_size=(5, 5), tap_bits=lambda: R.TAP_BITS)
    convs = [[mod(sd["cgp_out_xo_list.0.%d.weight" % n], sd["cgp_out_xo_list.0.%d.bias" % n])] for n in (0, 2, 4, 6)]
    cs = [mod(sd["csc_list.0.weight"] * sd["csc_list.0.mask"], sd["csc_list.0.bias"])]
    net._fold_csc_into_cgp(convs, cs, G)
    ws, bs = R.fold(sd, 0, G)
    for l in range(4):
        assert torch.equal(got["ws"][l][0, :, :, 0, 0], ws[l]) and torch.equal(got["bs"][l][0], bs[l])
    xe, x0, x1, plc, xq = _oracle_level_inputs(sd, 12, 20, 2)
    sd64 = {k: v.double() for k, v in sd.items()}
    ref = R.unfolded_forward(plc.double(), xq.double(), sd64, 0)
    w64, b64 = [t.double() for t in ws], [t.double() for t in bs]
    out = R.forward(plc.double(), xq.double(), w64, b64)["params"]
    bound = _abs_bound(R.cat_input(plc.double(), R.gather_taps(xq.double())), w64, b64, 2.0 ** -24)
    err = (out - ref).abs()
    print("fold: max |folded - unfolded| %.2e, bound there %.2e, max|params| %.2e" % (
        float(err.max()), float(bound.reshape(-1)[int(err.argmax())]), float(ref.abs().max())))
    assert float(err.max()) > 0 and bool((err <= bound + 1e-13 * ref.abs().max()).all())
    # and in fp32 the two paths are fp32 evaluations of the same function: both inside the other's yardstick class
    f32 = R.forward(plc, xq, ws, bs)["params"]
    u32 = R.unfolded_forward(plc, xq, sd, 0)
    assert float((f32.double() - ref).abs().max()) <= 4 * float((u32.double() - ref).abs().max()) + 2e-7 * float(ref.abs().max())


def test_taps_are_zero_outside_the_image():
    xq = torch.arange(1.0, 1 + 2 * 3 * 4 * 6).reshape(2, 3, 4, 6)
    t = R.gather_taps(xq).reshape(2, 3, 12, 4, 6)
    for j in range(12):
        dy, dx = j // 5 - 2, j % 5 - 2
        for y in range(4):
            for x in range(6):
                inside = 0 <= y + dy < 4 and 0 <= x + dx < 6
                want = xq[:, :, y + dy, x + dx] if inside else torch.zeros(2, 3)
                assert torch.equal(t[:, :, j, y, x], want)


def _small_case(seed):
    g = torch.Generator().manual_seed(seed)
    ws, bs = R.iid_weights(1, G, seed)
    ws, bs = R.plane_weights(ws, bs, 0, F64)
    cat = torch.randn(2, G * 93, 3, 5, generator=g, dtype=F64)
    dp = torch.randn(2, 2 * G, 3, 5, generator=g, dtype=F64)
    return g, ws, bs, cat, dp


def test_backward_against_central_differences():
    """Every output of cgp_ref.backward / param_grads in float64 against (L(v + e d) - L(v - e d)) / 2e of L = <params, dparams>
    along random directions d (the stack is piecewise linear: the quotient is exact unless a unit crosses zero inside +-e d)."""
    g, ws, bs, cat, dp = _small_case(11)
    f = R.stack(cat, ws, bs, G)
    bw = R.backward(dp, f["h1"], f["h2"], f["h3"], ws, G)
    pg = R.param_grads(cat, f["h1"], f["h2"], f["h3"], dp, bw["d1"], bw["d2"], bw["d3"], G)
    B, _, h, w = cat.shape
    dcat = torch.cat([bw["dplc"].reshape(B, G, 81, h, w), bw["dtaps"].reshape(B, G, 12, h, w)], 2).reshape(cat.shape)
    loss = lambda c, W, b: float((R.stack(c, W, b, G)["params"] * dp).sum())
    e = 1e-7
    targets = [("cat", dcat, lambda d, s: loss(cat + s * d, ws, bs))]
    for l in range(4):
        targets.append(("dw%d" % l, pg["dw%d" % l], lambda d, s, l=l: loss(cat, [W + s * d if i == l else W for i, W in enumerate(ws)], bs)))
        targets.append(("db%d" % l, pg["db%d" % l], lambda d, s, l=l: loss(cat, ws, [b + s * d if i == l else b for i, b in enumerate(bs)])))
    for name, grad, fn in targets:
        for _ in range(3):
            d = torch.randn(grad.shape, generator=g, dtype=F64)
            fd = (fn(d, e) - fn(d, -e)) / (2 * e)
            an = float((grad * d).sum())
            assert abs(fd - an) <= 1e-6 * max(abs(an), float(grad.abs().max())), (name, fd, an)
    # the hidden gradients: d_l is the gradient at layer l's pre-activation, i.e. at its bias, pixel by pixel
    for l, key in ((0, "d1"), (1, "d2"), (2, "d3")):
        assert torch.allclose(bw[key].sum(dim=(0, 2, 3)), pg["db%d" % l], rtol=1e-12, atol=0)


def test_backward_takes_the_gates_from_the_tensors_handed_in():
    g, ws, bs, cat, dp = _small_case(12)
    f = R.stack(cat, ws, bs, G)
    flipped = -f["h2"]
    a = R.backward(dp, f["h1"], f["h2"], f["h3"], ws, G)
    b = R.backward(dp, f["h1"], flipped, f["h3"], ws, G)
    assert not torch.equal(a["d2"], b["d2"]) and torch.equal(a["d3"], b["d3"])
    zero = R.backward(dp, f["h1"], torch.zeros_like(f["h2"]), f["h3"], ws, G)             # h == 0 gates with 0.01, as hv > 0 does
    assert torch.allclose(zero["d2"], 0.01 * R._convT(a["d3"], ws[2], G), rtol=1e-14, atol=0)


def test_rescaled_sets_are_the_same_function_in_float64():
    sets = R.weight_sets(2, G, 5)
    plc, xq = R.input_sets(2, 2, G, 8, 8, 3)["taps4_feat1"]
    for p in range(2):
        ref = R.forward(plc[p].double(), xq[p].double(), *R.plane_weights(*sets["iid"], p, F64))["params"]
        for name in sets:
            if name.startswith("rescaled"):
                out = R.forward(plc[p].double(), xq[p].double(), *R.plane_weights(*sets[name], p, F64))["params"]
                assert float((out - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), name


def _evaluate(plc, xq, ws, bs, extra=()):
    """-> ref (P, ...) float64 params, [fp32 evaluations]."""
    P = plc.shape[0]
    ref = torch.stack([R.forward(plc[p].double(), xq[p].double(), *R.plane_weights(ws, bs, p, F64))["params"] for p in range(P)])
    f32 = torch.stack([R.forward(plc[p], xq[p], *R.plane_weights(ws, bs, p))["params"] for p in range(P)])
    return ref, [f32] + [torch.stack([e(plc[p], xq[p], *R.plane_weights(ws, bs, p))["params"] for p in range(P)]) for e in extra]


@pytest.mark.parametrize("h,w", SHAPES)
def test_print_yardsticks_of_the_input_domain(h, w):
    """The fp32 yardstick of params for every input set the GPU file runs (i.i.d. weights), and the emulated chain held to the
    bar on them: the emulation must pass where the kernels are required to."""
    ws, bs = R.iid_weights(2, G, 100 + h)
    bad = []
    for name, (plc, xq) in R.input_sets(2, 2, G, h, w, 7 * h + w).items():
        ref, f32s = _evaluate(plc, xq, ws, bs)
        emu = torch.stack([R.chain_split(plc[p], xq[p], *R.plane_weights(ws, bs, p))["params"] for p in range(2)])
        per_pixel = name == "six_decades"
        bad += R.check("%dx%d %s (emulated)" % (h, w, name), "params", emu, ref, f32s + ([emu] if per_pixel else []), G,
                       reduce=R.PER_PIXEL if per_pixel else R.PER_ROW)
    assert not bad, bad


def test_print_emulated_chain_over_the_weight_domain():
    """For every weight set of the GPU file at 37 x 53: the emulated chain's error beside the fp32 yardstick, and the headroom
    measure of ops.cgp16_supported.  Asserted only where the kernels are required to hold the bar (i.i.d., benchmark weights,
    dead unit, dead tap); the rescaled and large-bias sets are DESIGN.md 2.3's sweep."""
    P = 3
    sets = R.weight_sets(P, G, 41)
    plc, xq = R.input_sets(P, 2, G, 37, 53, 9)["taps4_feat1"]
    bad = []
    for name, (ws, bs) in sets.items():
        ref, f32s = _evaluate(plc, xq, ws, bs)
        emu = torch.stack([R.chain_split(plc[p], xq[p], *R.plane_weights(ws, bs, p))["params"] for p in range(P)])
        hr = max(float(R.headroom(*R.plane_weights(ws, bs, p), G).max()) for p in range(P))
        miss = R.check("%-18s headroom %5.1f (emulated)" % (name, hr), "params", emu, ref, f32s, G, reduce=R.PER_ROW)
        if name in ("iid", "bench", "dead_unit", "dead_tap", "positive"):
            bad += miss
    assert not bad, bad


def test_supported_limit_over_the_weight_domain():
    """ops.cgp16_headroom is cgp_ref.headroom, and ops.cgp16_supported keeps the sets every form must serve (i.i.d., benchmark
    weights, dead unit, dead tap, 2^3 on one layer, a bias of 1e2) and refuses the ones the chain was measured to miss on."""
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    sets = R.weight_sets(3, G, 41)
    for name, (ws, bs) in sets.items():
        want = max(float(R.headroom(*R.plane_weights(ws, bs, p), G).max()) for p in range(3))
        got = ops.cgp16_headroom(ws, bs, G)
        assert abs(got - want) < 1e-4, (name, got, want)
        print("%-20s headroom %5.2f supported %s" % (name, got, ops.cgp16_supported(ws, G, bs)))
    yes = ("iid", "bench", "dead_unit", "dead_tap", "positive", "rescaled_3_0_0", "rescaled_0_3_0", "rescaled_0_0_3", "bias_1e+02")
    for name in sets:
        assert ops.cgp16_supported(sets[name][0], G, sets[name][1]) == (name in yes), name
    assert not ops.cgp16_supported([w[:, :, :40] for w in sets["iid"][0]], G, sets["iid"][1])    # other widths: as before
