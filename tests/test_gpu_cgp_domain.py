"""GPU: the context-MLP kernels against the float64 reference of tests/cgp_ref.py over their input and weight domain
 -- k_cgp16 in its streaming, persistent, TRAIN and wavefront forms, k_cgp16_bwd (csrc/cgp_f16x3.hip), the fp32-MFMA
k_cgp_rate / k_cgp_bwd (csrc/cgp_fused.hip) and k_wgrad1x1.

Bars (cgp_ref.check): |kernel - f64| <= 4 * yardstick + 2e-7 (values) or 5e-7 (gradients) * max|f64|, the yardstick being the fp32
evaluation of the same formula on the same inputs; per plane and group, params per output row, the six-decade cases per pixel.
Every output tensor an op allocates is filled with NaN before the launch (the `nan_outputs` fixture), so an element no lane
writes fails its bar.  Distinct random weights per (plane, group); B = 2 so that the persistent form's waves stride over images.

Weights beyond what the split chain represents (ops.cgp16_supported is False: DESIGN.md 2.3) must be refused by the chain's
dispatch and meet the same bars on the fp32 kernels; inside the limit every form of the chain meets them."""
import ctypes as C
import types

import pytest
import torch

import cgp_ref as R
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV, G = "cuda:0", 3
FORCE_STREAM, FORCE_PERSISTENT = 1 << 2, 2 << 2             # ops.set_diagnostics(2, None, flags)
SHAPES = ((3, 5), (8, 8), (37, 53), (33, 64))
CHAIN_FORMS = ("stream", "persistent", "train")
REQUIRED = ("iid", "bench", "dead_unit", "dead_tap", "positive")        # weight sets every form of the chain must hold the bars on
_CACHE = {}


class _NanTorch:
    """`torch` for ops.py with every floating-point torch.empty / empty_like filled with NaN."""

    @staticmethod
    def _fill(t):
        return t.fill_(float("nan")) if t.is_floating_point() else t

    def empty(self, *a, **k):
        return self._fill(torch.empty(*a, **k))

    def empty_like(self, *a, **k):
        return self._fill(torch.empty_like(*a, **k))

    def __getattr__(self, name):
        return getattr(torch, name)


@pytest.fixture(autouse=True)
def nan_outputs(monkeypatch):
    monkeypatch.setattr(ops, "torch", _NanTorch())


def _dev(t):
    return t.to(DEV).contiguous()


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _weights(P, seed=41):
    return _cached(("weights", P, seed), lambda: R.weight_sets(P, G, seed))


def _inputs(P, h, w):
    return _cached(("inputs", P, h, w), lambda: R.input_sets(P, 2, G, h, w, 7 * h + w))


def _evaluate(plc, xq, ws, bs):
    """-> (ref, f32): dicts params, h1, h2, h3 with a leading plane axis; float64 and the fp32 oracle."""
    ref, f32 = {}, {}
    for p in range(plc.shape[0]):
        a = R.forward(plc[p].double(), xq[p].double(), *R.plane_weights(ws, bs, p, R.F64))
        b = R.forward(plc[p], xq[p], *R.plane_weights(ws, bs, p))
        for k in a:
            ref.setdefault(k, []).append(a[k])
            f32.setdefault(k, []).append(b[k])
    return {k: torch.stack(v) for k, v in ref.items()}, {k: torch.stack(v) for k, v in f32.items()}


def _emulate(plc, xq, ws, bs):
    out = {}
    for p in range(plc.shape[0]):
        for k, v in R.chain_split(plc[p], xq[p], *R.plane_weights(ws, bs, p), want_hidden=True).items():
            out.setdefault(k, []).append(v)
    return {k: torch.stack(v) for k, v in out.items()}


def _run(form, plc, xq, ws, bs):
    """One form on the device -> dict of host tensors (params, and h1 .. h3 where the form writes them)."""
    wsd, bsd, plc, xq = [_dev(t) for t in ws], [_dev(t) for t in bs], _dev(plc), _dev(xq)
    if form == "f32":
        packed, dims = ops.cgp_pack(wsd, bsd, G)
        _, params, h1, h2, h3 = ops.cgp_rate_train_ctx(plc, xq, xq, packed, dims, torch.zeros_like(xq), R.K, R.TAP_BITS)
        out = dict(params=params, h1=h1, h2=h2, h3=h3)
    elif form == "train":
        out = dict(zip(("params", "h1", "h2", "h3"), ops.cgp16_params_train(plc, xq, ops.cgp16_pack(wsd, bsd, G), R.K, R.TAP_BITS)))
    else:
        packed = ops.cgp16_pack(wsd, bsd, G)
        ops.set_diagnostics(2, None, FORCE_PERSISTENT if form == "persistent" else FORCE_STREAM)
        try:
            out = dict(params=ops.cgp16_params(plc, xq, packed, R.K, R.TAP_BITS))
            torch.cuda.synchronize()
        finally:
            ops.set_diagnostics(2, None, 0)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _check_forward(tag, out, ref, f32, extra=None, per_pixel=False):
    bad = []
    for k in ("params", "h1", "h2", "h3"):
        if k in out:
            yard = [f32[k]] + ([extra[k]] if extra is not None else [])
            reduce = R.PER_PIXEL if per_pixel else R.PER_ROW if k == "params" else R.PER_GROUP
            bad += R.check(tag, k, out[k], ref[k], yard, G, R.VALUE_FLOOR, reduce)
    return bad


# ------------------------------------------------------------------------------------------------ forms x input domain
@pytest.mark.parametrize("h,w", SHAPES)
def test_every_form_over_the_input_domain(h, w):
    """3x5: one partial block; 8x8: two blocks, fewer than the waves; 37x53: 1961 pixels, the last block has 9; 33x64: taps across
    rows at a width that is a multiple of 32.  Streaming, persistent and TRAIN forms of the chain and the fp32 kernels, on every
    input set of cgp_ref.input_sets.  six_decades is compared pixel by pixel: the chain holds ONE scale per 32-pixel block, and
    fp16 has no exponent below 2^-24, so its small pixels keep fewer than 22 bits -- for that case, and for the chain's forms
    only, the emulated chain (cgp_ref.chain_split) joins the yardstick (DESIGN.md 2.3 gives both figures)."""
    ws, bs = _weights(2)["iid"]
    bad = []
    for name, (plc, xq) in _inputs(2, h, w).items():
        ref, f32 = _evaluate(plc, xq, ws, bs)
        six = name == "six_decades"
        emu = _emulate(plc, xq, ws, bs) if six else None
        for form in CHAIN_FORMS + ("f32",):
            out = _run(form, plc, xq, ws, bs)
            if six and form != "f32":
                _check_forward("%dx%d %s %s [fp32 yardstick alone]" % (h, w, name, form), out, ref, f32, None, True)
            bad += _check_forward("%dx%d %s %s" % (h, w, name, form), out, ref, f32, emu if form != "f32" else None, six)
    assert not bad, bad


def test_all_zero_image_gives_the_bias_chain():
    """amax == 0: scale 1, and (sigma, mu) of every pixel is the network's answer to a zero input."""
    ws, bs = _weights(2)["iid"]
    plc, xq = _inputs(2, 8, 8)["all_zero"]
    out = _run("stream", plc, xq, ws, bs)["params"]
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0
    assert bool((out == out[:, :1, :, :1, :1]).all())


def test_values_at_the_bound_do_not_overflow():
    """Weights and biases all positive, every input 1: away from the border h1, h2, h3 of a pixel EQUAL the bounds the chain's
    scales come from (max input x largest row L1 norm + largest bias holds with equality for the largest row), the largest value
    a scale of 2^15 / bound must carry in fp16.  A scale taken one layer early overflows here."""
    ws, bs = _weights(2)["positive"]
    plc, xq = torch.ones(2, 2, G * R.CPLC, 8, 8), torch.ones(2, 2, G, 8, 8)
    ref, f32 = _evaluate(plc, xq, ws, bs)
    w0, b0 = R.plane_weights(ws, bs, 0)
    top = (w0[0].sum(dim=1) + b0[0]).reshape(G, -1).amax(dim=1)                            # a unit close to layer 0's bound exists
    assert bool((ref["h1"][0].reshape(2, G, -1).amax(dim=(0, 2)) > 0.9 * top).all())
    bad = []
    for form in CHAIN_FORMS + ("f32",):
        bad += _check_forward("at the bound 8x8 %s" % form, _run(form, plc, xq, ws, bs), ref, f32)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the wavefront step
def _table63():
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import get_scale_table
    return torch.as_tensor(get_scale_table()).float()[:63].contiguous()


def test_wavefront_step_against_float64():
    """One decoder-mode step of lldwt_cgp16_wavefront_step_q (unit step, sigma_out) on a state whose every pixel is non-zero: the
    step's (sigma, mu) are the whole-image values at its pixels (all 12 taps of a pixel lie on earlier steps).  First step, last
    step and the longest diagonal of 24 x 40."""
    P, B, H, W = 2, 2, 24, 40
    ws, bs = _weights(2)["iid"]
    plc, xq = _inputs(2, H, W)["taps4_feat1"]
    ref, f32 = _evaluate(plc, xq, ws, bs)
    lib = _lib.load()
    packed = ops.cgp16_pack([_dev(t) for t in ws], [_dev(t) for t in bs], G)
    plc_d, state, table = _dev(plc), _dev(xq), _dev(_table63())
    slope = R.K // 2 + 1
    steps = {t: [y for y in range(H) if 0 <= t - slope * y < W] for t in range(W + slope * (H - 1))}
    longest = max(steps, key=lambda t: len(steps[t]))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda a: C.c_void_p(a.data_ptr())
    bad = []
    for t in (0, longest, max(steps)):
        rows = torch.tensor(steps[t])
        cols = t - slope * rows
        n = len(rows)
        idx = torch.full((P * B, n, G), -1, device=DEV, dtype=torch.int32)
        mu = torch.full((P * B, G, n), float("nan"), device=DEV)
        sg = torch.full((P * B, G, n), float("nan"), device=DEV)
        before = state.clone()
        ops.check(lib.lldwt_cgp16_wavefront_step_q(p(plc_d), p(state), None, p(packed), p(table), p(idx), None, p(mu), p(sg), P, B,
                                                   H, W, G, R.K, R.TAP_BITS, t, n, 0, 1.0, 1.0, st), "wavefront_step_q")
        torch.cuda.synchronize()
        assert torch.equal(state, before) and int(idx.min()) >= 0                 # the decoder's step leaves the state alone
        got = torch.stack([sg.cpu().reshape(P, B, G, n), mu.cpu().reshape(P, B, G, n)], dim=3).reshape(P, B, 2 * G, 1, n)
        pick = lambda a: a[..., rows, cols].reshape(P, B, 2 * G, 1, n)
        bad += R.check("wavefront 24x40 step %d (%d pixels)" % (t, n), "params", got, pick(ref["params"]), [pick(f32["params"])],
                       G, R.VALUE_FLOOR, R.PER_ROW)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ weight domain
@pytest.mark.parametrize("name", R.WEIGHT_SET_NAMES)
def test_weight_domain(name):
    """Every weight set of cgp_ref.weight_sets at 37 x 53 (P = 3).  Supported by the chain (ops.cgp16_supported): its streaming
    and TRAIN forms hold the bars on (sigma, mu) and h1 .. h3.  Not supported: the fp32 kernels hold them, and the chain's own
    figures are printed beside (the sweep of DESIGN.md 2.3).  The rescaled sets compute the i.i.d. set's function: their float64
    outputs equal it to 1e-12."""
    sets = _weights(3)
    ws, bs = sets[name]
    plc, xq = _inputs(3, 37, 53)["taps4_feat1"]
    ref, f32 = _cached(("wd", name), lambda: _evaluate(plc, xq, ws, bs))
    if name.startswith("rescaled"):
        base, _ = _cached(("wd", "iid"), lambda: _evaluate(plc, xq, *sets["iid"]))
        assert float((ref["params"] - base["params"]).abs().max()) <= 1e-12 * float(base["params"].abs().max())
    supported = ops.cgp16_supported(ws, G, bs)
    hr = max(float(R.headroom(*R.plane_weights(ws, bs, p), G).max()) for p in range(3))
    print("%s: headroom %.1f binades, cgp16_supported %s" % (name, hr, supported))
    assert supported or name not in REQUIRED
    bad = []
    for form in ("stream", "train"):
        miss = _check_forward("%s %s" % (name, form), _run(form, plc, xq, ws, bs), ref, f32)
        bad += miss if supported else []
    if not supported:
        bad += _check_forward("%s f32" % name, _run("f32", plc, xq, ws, bs), ref, f32)
    assert not bad, bad


def test_unsupported_weights_take_the_fp32_path():
    """_fold_csc_into_cgp yields packed16 = None for a weight set beyond the limit (and a pack for the benchmark weights), so the
    eval and training paths take the fp32 kernels and the coder its host-stepped schedule on them (code_tree_level_generic)."""
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models import LiftingBasedDWT_net as net
    from oracle import weights
    tmpl = weights.entropy_template(dict(dwtlevels=2, clrch=1, entropy_layer="conditioned2ZTsepSubbands"))
    sd = weights.fill_by_name({"model0.entropymodel." + k: v for k, v in tmpl.items()})
    sd = {k[len("model0.entropymodel."):]: v for k, v in sd.items()}

    def fold(sd):
        mod = lambda w, b: types.SimpleNamespace(weight=_dev(w), bias=_dev(b), kernel_size=(5, 5), tap_bits=lambda: R.TAP_BITS)
        convs = [[mod(sd["cgp_out_xo_list.0.%d.weight" % n], sd["cgp_out_xo_list.0.%d.bias" % n])] for n in (0, 2, 4, 6)]
        return net._fold_csc_into_cgp(convs, [mod(sd["csc_list.0.weight"] * sd["csc_list.0.mask"], sd["csc_list.0.bias"])], G)
    assert fold(sd)[2] is not None
    loud = {k: v.clone() for k, v in sd.items()}
    for n in (0, 2, 4):
        loud["cgp_out_xo_list.0.%d.weight" % n][5] *= 2.0 ** 10
    packed, dims, packed16 = fold(loud)
    assert packed16 is None and packed is not None


def test_training_path_refuses_the_chain_outside_its_range(monkeypatch):
    """CgpRateCtxFn takes lldwt_cgp_rate_train_ctx / lldwt_cgp_bwd_split for a weight set beyond the limit and the chain for the
    i.i.d. set: the calls of the chain's two entry points are recorded -- forward and backward once each for the i.i.d. set, none
    for the set beyond the limit."""
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import autograd as ag
    sets = _weights(2)
    plc, xq = _inputs(2, 8, 8)["taps4_feat1"]

    def run(name):
        ws, bs = sets[name]
        wb = [_dev(t).requires_grad_(True) for pair in zip(ws, bs) for t in pair]
        x = _dev(xq)
        bits = ag.CgpRateCtxFn.apply(_dev(plc).requires_grad_(True), x, x, torch.zeros_like(x), G, R.K, R.TAP_BITS, *wb)
        bits.sum().backward()
        torch.cuda.synchronize()
        return bits
    calls = []
    real_fwd, real_bwd = ops.cgp16_params_train, ops.cgp16_bwd
    monkeypatch.setattr(ops, "cgp16_params_train", lambda *a: (calls.append("fwd"), real_fwd(*a))[1])
    monkeypatch.setattr(ops, "cgp16_bwd", lambda *a: (calls.append("bwd"), real_bwd(*a))[1])
    assert bool(torch.isfinite(run("iid")).all()) and calls == ["fwd", "bwd"]
    del calls[:]
    assert bool(torch.isfinite(run("rescaled_6_6_6")).all()) and calls == []


# ------------------------------------------------------------------------------------------------ backward
BWD_SETS = ("iid", "dead_unit") + tuple("rescaled_%d_%d_%d" % r for r in R.RESCALES)      # the forward's rescaled sets, all of them
BWD_KEYS = ("d3", "d2", "d1", "dplc", "dtaps")


def _dparams(P, h, w):
    g = torch.Generator().manual_seed(5)
    rnd = torch.randn(P, 2, 2 * G, h, w, generator=g)
    zero = rnd.clone().reshape(P, 2, 2 * G, h * w)
    zero[..., R.BLOCK:2 * R.BLOCK] = 0.0
    ramp = torch.logspace(0, -6, R.BLOCK).repeat(-(-h * w // R.BLOCK))[:h * w].reshape(h, w)
    return {"random": rnd, "zero_block": zero.reshape(rnd.shape), "six_decades": rnd * ramp}


def _backward_reference(name):
    """h1 .. h3 from the float64 forward rounded to fp32, then the float64 / fp32 / emulated backward of every dparams case."""
    P = 2
    ws, bs = _weights(P)[name]
    plc, xq = _inputs(P, 37, 53)["taps4_feat1"]
    ref, _ = _evaluate(plc, xq, ws, bs)
    hs = [ref[k].float() for k in ("h1", "h2", "h3")]
    cases = {}
    for case, dp in _dparams(P, 37, 53).items():
        r, f, e = {}, {}, {}
        for p in range(P):
            w64, _ = R.plane_weights(ws, bs, p, R.F64)
            w32, _ = R.plane_weights(ws, bs, p)
            for dst, val in ((r, R.backward(dp[p].double(), *[t[p].double() for t in hs], w64, G)),
                             (f, R.backward(dp[p], *[t[p] for t in hs], w32, G)),
                             (e, R.chain_split_bwd(dp[p], *[t[p] for t in hs], w32, G) if case == "six_decades" else {})):
                for k, v in val.items():
                    dst.setdefault(k, []).append(v)
        cases[case] = tuple({k: torch.stack(v) for k, v in d.items()} for d in (r, f, e)) + (dp,)
    return ws, hs, cases


@pytest.mark.parametrize("kernel", ["cgp16_bwd", "cgp_bwd_split"])
@pytest.mark.parametrize("name", BWD_SETS)
def test_backward_data_against_float64(name, kernel):
    """lldwt_cgp16_bwd (split chain) and lldwt_cgp_bwd_split (fp32 MFMA) on d1, d2, d3, dplc, dtaps at 37 x 53, gates from the
    stored activations handed in.  dparams: random; one whole block zero; six decades across the pixels of every block, compared
    pixel by pixel (for the chain with its emulation, cgp_ref.chain_split_bwd, in the yardstick: one scale per block).  The
    backward bounds are the transposed layers' L1 norms, so the rescaled sets spend the chain's binades here as well: outside
    ops.cgp16_supported the chain's figures are printed and the fp32 kernel is held to the bars."""
    ws, hs, cases = _cached(("bwd", name), lambda: _backward_reference(name))
    wsd = [_dev(t) for t in ws]
    supported = ops.cgp16_supported(ws, G, _weights(2)[name][1])
    bad = []
    for case, (ref, f32, emu, dp) in cases.items():
        args = (_dev(dp), _dev(hs[0]), _dev(hs[1]), _dev(hs[2]))
        if kernel == "cgp16_bwd":
            got = ops.cgp16_bwd(*args, ops.cgp16_pack_bwd(wsd, G), G)
        else:
            got = ops.cgp_bwd_split(*args, ops.cgp_pack_bwd(wsd, G), R.C[:4], G, R.NTAPS)
        torch.cuda.synchronize()
        out = dict(zip(("dplc", "dtaps", "d1", "d2", "d3"), [t.cpu() for t in got]))
        six = case == "six_decades"
        for k in BWD_KEYS:
            yard = [f32[k]] + ([emu[k]] if six and kernel == "cgp16_bwd" else [])
            if six and kernel == "cgp16_bwd":
                R.check("%s %s %s [fp32 yardstick alone]" % (name, kernel, case), k, out[k], ref[k], [f32[k]], G, R.GRAD_FLOOR, R.PER_PIXEL)
            miss = R.check("%s %s %s" % (name, kernel, case), k, out[k], ref[k], yard, G, R.GRAD_FLOOR,
                           R.PER_PIXEL if six else R.PER_GROUP)
            bad += miss if (supported or kernel == "cgp_bwd_split") else []
    assert not bad, bad


def test_wgrad1x1_split_against_float64():
    """lldwt_wgrad1x1_split on [plc | taps] x d1 over 2 x 1961 pixels (no multiple of its 32-pixel K tile), weight rows and the
    bias column.  Every entry is ONE fp32 sum over the pixels in no fixed order -- a workgroup adds four pixels per fp32 MFMA to
    one accumulator, chunk after chunk, and the workgroups meet in fp32 atomics -- so the yardstick takes the worst of a few
    fixed orders: lift_ref.BIAS_ORDERS and, for the kernel's own granularity, partial sums of 4 pixels added one after another."""
    P = 2
    ws, hs, cases = _cached(("bwd", "iid"), lambda: _backward_reference("iid"))
    plc, xq = _inputs(P, 37, 53)["taps4_feat1"]
    d1 = cases["random"][0]["d1"].float()
    taps = torch.stack([R.gather_taps(xq[p]) for p in range(P)])
    dw, db = ops.wgrad1x1_split(_dev(plc), _dev(taps), _dev(d1), G)
    torch.cuda.synchronize()
    orders = R.BIAS_ORDERS + ((4, False), (4, True))
    ref, f32s = [], [[] for _ in range(1 + len(orders))]
    for p in range(P):
        cat = R.cat_input(plc[p], taps[p])
        ref.append(R.wgrad_ordered(cat.double(), d1[p].double(), G, 1 << 20, False))
        f32s[0].append(torch.cat([R.wgrad(cat, d1[p], G), d1[p].sum(dim=(0, 2, 3))[:, None]], dim=1))
        for i, (chunk, rev) in enumerate(orders):
            f32s[1 + i].append(R.wgrad_ordered(cat, d1[p], G, chunk, rev))
    ref, f32s = torch.stack(ref), [torch.stack(t) for t in f32s]
    bad = R.check("wgrad1x1_split 2 x 1961 pixels", "dw0", dw.cpu()[:, :, :, 0, 0], ref[:, :, :93], [t[:, :, :93] for t in f32s], G,
                  R.GRAD_FLOOR)
    bad += R.check("wgrad1x1_split 2 x 1961 pixels", "db0", db.cpu(), ref[:, :, 93], [t[:, :, 93] for t in f32s], G, R.GRAD_FLOOR)
    assert not bad, bad
