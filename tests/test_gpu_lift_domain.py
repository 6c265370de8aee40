"""GPU: every hand-written form of the learned lifting step -- the three fp32-MFMA launches (csrc/lifting.hip), the fused
split-fp16 kernel on its composed 9x9 path, on its sequential TRAIN path and in BWD mode (csrc/lifting_f16.hip) -- against the
float64 evaluation of the oracle, over the numeric domain and at run lengths above 1 (the vertical hand-down of T1 / T2 rows).

Reference, yardstick and bars come from tests/lift_ref.py:
    values      |kernel - f64| <= 4 * yardstick + 2e-7 * max|f64|
    gradients   |kernel - f64| <= 4 * yardstick + 5e-7 * max|f64|
per plane and per tensor, no element left out; the yardstick is the fp32 oracle's own distance from float64 on the same inputs
(the larger of torch.tanh and the kernels' declared tanh formula).  Every comparison prints its error, yardstick and bar
(pytest -s).  P = 3 planes with distinct weights, B = 2; the fused paths need K = 5, C = 16.

Run lengths.  The launch (lift_f16_launch) takes a run length above 1 only when Z * tiles_x * tiles_y exceeds the CU count: of the
shapes here 200 x 250 (eval) and the 140 x 300 level of the TRAIN forward / step backward do so on 256 CUs by the dispatch's own
choice.  The run length is otherwise forced: LLDWT_LF_RL (and LLDWT_WGRAD16_MIN for the split-fp16 weight gradients) are read
once per process, so test_forced_run_lengths starts one fresh child per setting, which runs the step, TRAIN-forward and
step-backward tests of this file at 70 x 150 (five tile rows: runs of 3 + 2 and 2 + 2 + 1) and 40 x 45."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import lift_ref as R
from helpers import filled
from oracle import lifting, model, weights

pytestmark = pytest.mark.gpu

P, B, C = 3, 2, 16
CHILD = os.environ.get("LLDWT_LIFT_DOMAIN_CHILD") == "1"          # inside a child of test_forced_run_lengths
STEP_SHAPES = [(70, 150), (40, 45)] if CHILD else [(8, 12), (19, 45), (70, 150)]
LEVEL_SHAPES = [(140, 300), (80, 90)] if CHILD else [(38, 90), (140, 300)]      # x of one level: row pass H/2 x W, columns H/2 x W/2


def _ops():
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    import gpu_util
    return ops, gpu_util


_cache = {}


def _weights(K=5, variant=None):
    """Per-plane state dicts (distinct weights), device taps (4,P,3) and eval packs (P,2,2,total): built once per variant."""
    key = ("w", K, variant)
    if key not in _cache:
        _, gu = _ops()
        cfg = dict(model.DEFAULT_CFG, filtersize=K, dwtlevels=1)
        sds = [filled(weights.autoencoder_template(cfg), "dom%d." % p) for p in range(P)]
        for sd in sds:
            for blk in ("P_blocks.0.", "P_blocks.1.", "U_blocks.0.", "U_blocks.1."):
                if variant == "x4":             # conv2 / conv3 weights x 4: saturated tanh, large t3
                    sd[blk + "conv2.weight"] = sd[blk + "conv2.weight"] * 4.0
                    sd[blk + "conv3.weight"] = sd[blk + "conv3.weight"] * 4.0
                elif variant == "w2zero":       # a zero conv: the pack's scale of an all-zero tensor
                    sd[blk + "conv2.weight"] = torch.zeros_like(sd[blk + "conv2.weight"])
        taps, packed = gu.lifting_params(sds)
        _cache[key] = (cfg, sds, taps, packed)
    return _cache[key]


def _inputs(hw, seed=0):
    g = torch.Generator().manual_seed(9000 + 131 * hw[0] + hw[1] + seed)
    return torch.rand(P, B, 1, *hw, generator=g) - 0.5, torch.rand(P, B, 1, *hw, generator=g) - 0.5


# which step of the lifting pair a test runs: (skip-filter index, block prefix, index into packed[:, block, is_u])
STEP_OF = {1: (1, "U_blocks.0.", (0, 1)), 0: (2, "P_blocks.1.", (1, 0))}          # by `vertical`


def _step_reference(sds, src, dst, vertical, sign, linear=False, cache_key=None):
    """float64 step and its fp32 evaluations, per plane (lift_ref.evaluate); cached for the tests that share inputs."""
    if cache_key is not None and cache_key in _cache:
        return _cache[cache_key]
    j, prefix, _ = STEP_OF[vertical]

    def fn(p, dtype, tanh):
        sd = R.cast_sd(sds[p], dtype)
        f = R.step(src[p].to(dtype), dst[p].to(dtype), R.tap_of(sd, j), R.block_of(sd, prefix), sign, bool(vertical), linear,
                   tanh=tanh)
        return {"out": f["out"]}
    res = R.evaluate(fn, P)
    if cache_key is not None:
        _cache[cache_key] = res
    return res


def _kernel_step(w, src, dst, K, vertical, sign, linear=False, flags=0):
    ops, gu = _ops()
    _, _, taps, packed = w
    j, _, (blk, u) = STEP_OF[vertical]
    h, wd = src.shape[-2:]
    Z = P * B
    src_d, dst_d = gu.dev(src), gu.dev(dst)
    out_d = torch.empty_like(dst_d)
    v = lambda t: ops.view_of(t, Z, h, wd)
    try:
        ops.set_diagnostics(0, None, flags)
        ops.lift_step(v(src_d), v(dst_d), v(out_d), Z, B, h, wd, taps[j].contiguous(), packed[:, blk, u].contiguous(), C, K,
                      vertical, sign, 0.1, linear)
        torch.cuda.synchronize()
    finally:
        ops.set_diagnostics(0, None, 0)
    out = out_d.cpu()
    return [out[p] for p in range(P)]


# ------------------------------------------------------------------------------------------------ 1. eval step, three forms
FORMS = {0: "composed", 16: "sequential", 32: "composed, no hand-down"}


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("vertical", [1, 0])
@pytest.mark.parametrize("hw", STEP_SHAPES)
def test_eval_step_three_forms(hw, vertical, sign):
    """8 x 12 is smaller than a tile, 19 x 45 all border, 70 x 150 interior tiles and ragged last tiles (40 x 45 in the children:
    three tile rows).  Diagnostics flags 0 / 16 / 32 select the composed path, the sequential evaluation and the composed path
    without the hand-down; each is held against float64, not against the others."""
    w = _weights()
    src, dst = _inputs(hw)
    ref, f32s = _step_reference(w[1], src, dst, vertical, sign)
    bad = []
    for flags, name in FORMS.items():
        got = _kernel_step(w, src, dst, 5, vertical, sign, flags=flags)
        bad += R.check("eval step %s v=%d s=%+.0f %s" % (hw, vertical, sign, name), "out", got, ref, f32s)
    assert not bad, bad


@pytest.mark.skipif(CHILD, reason="the dispatch's own choice: not part of the forced runs")
@pytest.mark.parametrize("vertical", [1, 0])
def test_eval_step_runs_chosen_by_the_dispatch(vertical):
    """200 x 250, Z = 6: 13 x 8 tiles per image, 624 in all -- on 256 CUs the cost rule of lift_f16_launch takes runs of three with a
    last run of one tile, so T1 / T2 rows are handed down twice per run without any diagnostics setting."""
    w = _weights()
    src, dst = _inputs((200, 250))
    ref, f32s = _step_reference(w[1], src, dst, vertical, 1.0)
    got = _kernel_step(w, src, dst, 5, vertical, 1.0)
    bad = R.check("eval step (200, 250) v=%d dispatch's runs" % vertical, "out", got, ref, f32s)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 2. the numeric domain
def _domain_case(name, hw):
    """-> (weights variant, src, dst, per-plane row norms or None).  Finite inputs only."""
    src, dst = _inputs(hw, seed=7)
    h, wd = hw
    variant, rows = None, None
    if name.startswith("scale"):
        s = 2.0 ** int(name[5:])
        src, dst = src * s, dst * s
    elif name == "src_zero":
        src = torch.zeros_like(src)
    elif name == "zero_block":
        # 48 x 64 zeros from (8, 16): at 70 x 150 the 32 x 48 skip patch of tile row 1 or 2, tile column 1 is zero for either filter
        # direction (pow2_scale(0) = 1); at 19 x 45 the zeros take the lower right of the image
        src = src.clone()
        src[..., 8:56, 16:80] = 0.0
    elif name == "outlier":
        src = src.clone()
        src[..., h // 2 + 1, wd // 2 - 3] = 1e4                    # one sample sets its tile's operand scale
    elif name == "rows":
        ramp = 10.0 ** torch.linspace(-3, 3, h, dtype=torch.float64)
        src, dst = (src.double() * ramp[:, None]).float(), (dst.double() * ramp[:, None]).float()
        rows = [ramp] * P
    elif name in ("x4", "w2zero"):
        variant = name
    elif name == "planes":
        s = torch.tensor([0.01, 1.0, 4.0]).view(P, 1, 1, 1, 1)
        src, dst = src * s, dst * s
    else:
        raise KeyError(name)
    assert bool(torch.isfinite(src).all()) and bool(torch.isfinite(dst).all())
    return variant, src, dst, rows


DOMAIN = ["scale-12", "scale-4", "scale6", "scale12", "src_zero", "zero_block", "outlier", "rows", "x4", "w2zero", "planes"]


@pytest.mark.skipif(CHILD, reason="not part of the forced runs")
@pytest.mark.parametrize("vertical,sign", [(1, 1.0), (0, -1.0)])
@pytest.mark.parametrize("hw", [(19, 45), (70, 150)])
@pytest.mark.parametrize("name", DOMAIN)
def test_eval_step_domain(name, hw, vertical, sign):
    """The fused eval step away from U(-0.5, 0.5) inputs and `filled` weights: inputs far from 1, zero patches, an outlier that
    sets a tile's scale, six decades down the image (compared row by row, error and yardstick normalised by the row's factor),
    saturated tanh, a zero conv, planes of different magnitude."""
    variant, src, dst, rows = _domain_case(name, hw)
    w = _weights(5, variant)
    ref, f32s = _step_reference(w[1], src, dst, vertical, sign)
    got = _kernel_step(w, src, dst, 5, vertical, sign)
    kw = dict(row_dims=(0, 1, 3), row_norm=rows) if rows is not None else {}
    bad = R.check("domain %-10s %s v=%d" % (name, hw, vertical), "out", got, ref, f32s, **kw)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 3. the fp32 launches
@pytest.mark.skipif(CHILD, reason="not part of the forced runs")
@pytest.mark.parametrize("vertical,sign", [(1, -1.0), (0, 1.0)])
@pytest.mark.parametrize("hw", [(19, 45), (70, 150)])
@pytest.mark.parametrize("K,linear,f32mode", [(5, False, True), (3, False, False), (5, True, False), (3, True, False)])
def test_fp32_launches(K, linear, f32mode, hw, vertical, sign):
    """The three fp32-MFMA launches: what lift mode f32 runs at K = 5, and what K = 3 and the linear blocks always run."""
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import _lib
    w = _weights(K)
    src, dst = _inputs(hw, seed=3)
    ref, f32s = _step_reference(w[1], src, dst, vertical, sign, linear)
    lib = _lib.load()
    try:
        if f32mode:
            lib.lldwt_set_lift_mode(0)
        got = _kernel_step(w, src, dst, K, vertical, sign, linear)
    finally:
        lib.lldwt_set_lift_mode(0 if os.environ.get("LLDWT_LIFT_MODE") == "f32" else 1)
    bad = R.check("fp32 launches K=%d linear=%d %s v=%d" % (K, linear, hw, vertical), "out", got, ref, f32s)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 4. TRAIN forward
def _train_pack(sds):
    """(P, 2, 2, total): the pack autograd.py's training forward reads (no composed kernels)."""
    ops, gu = _ops()
    blocks = []
    for b in range(2):
        pu = []
        for kind in ("P_blocks", "U_blocks"):
            a = [gu.stack(sds, "%s.%d.conv%d.%s" % (kind, b, n, k)) for n in (1, 2, 3, 4) for k in ("weight", "bias")]
            pu.append(ops.pack_pblock(*a, train=not ops.train_lift_f16(), compose=False))
        blocks.append(torch.stack(pu, 1))
    return torch.stack(blocks, 1).contiguous()


def _op_views(op):
    return {"src": (op.buf_src, op.off_src, op.sz_src, op.sy_src, op.sx_src),
            "din": (op.buf_din, op.off_din, op.sz_din, op.sy_din, op.sx_din),
            "dout": (op.buf_dout, op.off_dout, op.sz_dout, op.sy_dout, op.sx_dout)}


def _run_program(prog, x, sd, dtype, tanh):
    """The step program of one level on the host for ONE plane (x: (B,1,H,W)): every op is lift_ref.step on strided views of the
    program's symbolic buffers.  -> dict 'op<i>.<src|skip|t1|t2|t3|out>' plus the final 'll' and 'yh0'."""
    Bn, _, H, W = x.shape
    size = {}
    for op in prog:
        for buf, off, sz, sy, sx in _op_views(op).values():
            size[buf] = max(size.get(buf, 0), off + (Bn - 1) * sz + (op.h - 1) * sy + (op.w - 1) * sx + 1)
    bufs = {b: torch.zeros(n, dtype=dtype) for b, n in size.items()}
    bufs[0] = x.to(dtype).reshape(-1).clone()
    sd = R.cast_sd(sd, dtype)
    out = {}
    for i, op in enumerate(prog):
        assert op.kind == 0
        vs = {k: torch.as_strided(bufs[buf], (Bn, 1, op.h, op.w), (sz, 0, sy, sx), off)
              for k, (buf, off, sz, sy, sx) in _op_views(op).items()}
        f = R.step(vs["src"], vs["din"], R.tap_of(sd, op.tap), R.block_of(sd, "%s_blocks.%d." % ("U" if op.is_u else "P", op.block)),
                   float(op.sign), bool(op.vertical), False, tanh=tanh)
        out["op%d.src" % i] = vs["src"].clone()
        for k in R.STEP_KEYS:
            out["op%d.%s" % (i, k)] = f[k].contiguous()
        vs["dout"].copy_(f["out"])
    h2, w2 = H // 2, W // 2
    out["ll"] = bufs[7][:Bn * h2 * w2].view(Bn, 1, h2, w2).clone()
    out["yh0"] = bufs[8][:Bn * 3 * h2 * w2].view(Bn, 3, h2, w2).clone()
    return out


def _level(hw):
    """One level of the TRAIN forward at x of `hw`: program, kernel outputs and `saved`, float64 chain and fp32 chains.  Shared by
    the TRAIN-forward and step-backward tests, never modified."""
    key = ("level", hw)
    if key in _cache:
        return _cache[key]
    ops, gu = _ops()
    cfg, sds, taps, _ = _weights()
    g = torch.Generator().manual_seed(4242 + hw[0])
    x = torch.rand(P, B, 1, *hw, generator=g) - 0.5
    Z = P * B
    prog, nsaved = ops.lifting_program(Z, hw[0], hw[1], 1, False, 0, False, C, False)
    # the program views a plane-major (Z, ...) buffer; one plane's host run sees B images of it
    pack = _train_pack(sds)
    saved = torch.full((nsaved,), float("nan"), device=gu.DEV)
    ll, yh = ops.lifting_forward_train(gu.dev(x), taps, pack, 1, C, 5, 0.1, False, False, 0, saved)
    torch.cuda.synchronize()
    ref, f32s = R.evaluate(lambda p, dtype, tanh: _run_program(prog, x[p], sds[p], dtype, tanh), P)
    # the host run of the program is the oracle's transform (float64: to rounding)
    for p in range(P):
        o = R.transform(x[p].double(), R.cast_sd(sds[p], R.F64), dict(cfg, dwtlevels=1))
        assert float((ref["ll"][p] - o["ll"]).abs().max()) < 1e-13 and float((ref["yh0"][p] - o["yh0"]).abs().max()) < 1e-13
    _cache[key] = dict(prog=prog, x=x, pack=pack, saved=saved, ll=ll, yh=yh, ref=ref, f32s=f32s)
    return _cache[key]


def _saved_slices(lv, i):
    """The slice src | skip | t1 | t2 | t3 of op i in `saved`, as device views (P, B, c, h, w)."""
    op = lv["prog"][i]
    h, w = op.h, op.w
    n = P * B * h * w
    base = lv["saved"][op.saved_off:op.saved_off + n * (2 + 3 * C)]
    cut = {"src": (0, 1), "skip": (n, 1), "t1": (2 * n, C), "t2": ((2 + C) * n, C), "t3": ((2 + 2 * C) * n, C)}
    return base, {k: base[o:o + n * c].view(P, B, c, h, w) for k, (o, c) in cut.items()}


@pytest.mark.parametrize("hw", LEVEL_SHAPES)
def test_train_forward_saved_intermediates(hw):
    """ops.lifting_forward_train at one level: for every op of ops.lifting_program its slice src | skip | t1 | t2 | t3 of `saved`
    and the level's outputs against the float64 chain (yardstick: the fp32 chains).  At 140 x 300 the row pass has 5 x 10 tiles
    on each of 6 images -- 300 runs of length 1 would not fit 256 CUs, so it runs at length 2 on its own: the tile above stores
    rows 22, 23 of t1 and rows 20 .. 23 of t2 for the tile below."""
    lv = _level(hw)
    bad = []
    for i, op in enumerate(lv["prog"]):
        _, sl = _saved_slices(lv, i)
        for k in ("src", "skip", "t1", "t2", "t3"):
            got = sl[k].cpu()
            bad += R.check("TRAIN %s op %d (%dx%d v=%d)" % (hw, i, op.h, op.w, op.vertical), "op%d.%s" % (i, k),
                           [got[p] for p in range(P)], lv["ref"], lv["f32s"])
    ll, yh = lv["ll"].cpu(), lv["yh"][0].cpu()
    bad += R.check("TRAIN %s outputs" % (hw,), "ll", [ll[p] for p in range(P)], lv["ref"], lv["f32s"])
    bad += R.check("TRAIN %s outputs" % (hw,), "yh0", [yh[p] for p in range(P)], lv["ref"], lv["f32s"])
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 5. step backward
PIXEL_GRADS = ("dsk", "dt3", "dpre2", "dr", "gsrc")


def _backward_reference(lv, i, g, key):
    if key in _cache:
        return _cache[key]
    op = lv["prog"][i]
    _, sds, _, _ = _weights()
    src = lv["ref"]["op%d.src" % i]                      # float64 copies of the fp32 values every chain starts from

    def fn(p, dtype, tanh):
        sd = R.cast_sd(sds[p], dtype)
        blk = R.block_of(sd, "%s_blocks.%d." % ("U" if op.is_u else "P", op.block))
        # dst_in enters the loss linearly: its value does not matter to any gradient
        gr = R.step_grads(src[p].to(dtype), torch.zeros_like(src[p]).to(dtype), R.tap_of(sd, op.tap), blk, g[p].to(dtype),
                          float(op.sign), bool(op.vertical), False, tanh=tanh)
        if dtype == R.F32 and tanh is torch.tanh:
            plain32[p] = gr
        return gr

    plain32 = {}

    def ordered(chunk, reverse):        # the bias gradients' fp32 atomics have no fixed order: the worst of a few orders
        return lambda p: R.step_bias_grads_ordered(plain32[p], g[p], float(op.sign), chunk, reverse)

    def split(p):           # the fused BWD launch's operand images (lift_ref.step_grads_split): joins that form's yardstick only
        blk = R.block_of(sds[p], "%s_blocks.%d." % ("U" if op.is_u else "P", op.block))
        return R.step_grads_split(src[p], R.tap_of(sds[p], op.tap), blk, g[p], float(op.sign), bool(op.vertical))
    _cache[key] = R.evaluate(fn, P, extra=[split] + [ordered(*o) for o in R.BIAS_ORDERS])
    return _cache[key]


def _kernel_backward(lv, i, g, fused):
    ops, gu = _ops()
    op = lv["prog"][i]
    _, sds, taps, _ = _weights()
    h, w = op.h, op.w
    Z, n = P * B, P * B * h * w
    dev = torch.device(gu.DEV)
    base, _ = _saved_slices(lv, i)
    keys = R.W_KEYS
    prefix = "%s_blocks.%d." % ("U" if op.is_u else "P", op.block)
    Wd = {"w%d" % k: gu.stack(sds, prefix + "conv%d.weight" % k) for k in (1, 2, 3, 4)}
    Wd.update({"b%d" % k: gu.stack(sds, prefix + "conv%d.bias" % k) for k in (1, 2, 3, 4)})
    pack = lv["pack"]
    tot = pack.shape[3]
    pk = ctypes.c_void_p(pack.data_ptr() + 4 * (op.block * 2 + op.is_u) * tot)
    bpk = tid = None
    if fused:
        # the backward pack is read with the FORWARD pack's plane stride (include/lldwt.h): same (P, 2, 2, total) layout, this
        # step's block in its own slot
        bpack = torch.zeros_like(pack)
        bpack[:, op.block, op.is_u] = ops.pack_pblock_bwd(Wd["w1"], Wd["w2"], Wd["w3"], Wd["w4"])
        assert bpack.shape == pack.shape and bpack.is_contiguous()
        bpk = ctypes.c_void_p(bpack.data_ptr() + 4 * (op.block * 2 + op.is_u) * tot)
        tid = torch.tensor([0.0, 1.0, 0.0], device=dev).repeat(P, 1).contiguous()
    gout = gu.dev(g.reshape(Z, h, w))
    gdin, gsrc = torch.zeros(Z, h, w, device=dev), torch.zeros(Z, h, w, device=dev)
    dW = [torch.zeros_like(Wd[k]) for k in keys]
    tp = taps[op.tap].contiguous()
    dtaps = torch.zeros_like(tp)
    v = lambda t: ops.View(ctypes.c_void_p(t.data_ptr()), h * w, w, 1)
    ops.lift_step_bwd(v(gout), v(gdin), v(gsrc), base, P, B, h, w, tp, dtaps, pk, pack.shape[1] * 2 * tot, dW, C, 5, 0.1,
                      float(op.sign), bool(op.vertical), False,
                      packed_bwd=bpk, taps_id=tid)
    torch.cuda.synchronize()
    ws = ops.workspace(0, dev).view(torch.float32)
    out = {"dsk": ws[n:2 * n].view(P, B, 1, h, w), "dt3": ws[2 * n:2 * n + n * C].view(P, B, C, h, w),
           "dpre2": ws[2 * n + n * C:2 * n + 2 * n * C].view(P, B, C, h, w),
           "dr": ws[2 * n + 2 * n * C:2 * n + 3 * n * C].view(P, B, C, h, w)}
    out = {k: t.clone() for k, t in out.items()}
    out.update(gsrc=gsrc.view(P, B, 1, h, w), gdin=gdin.view(P, B, 1, h, w), dtaps=dtaps)
    out.update({"d" + k: t for k, t in zip(keys, dW)})
    return {k: t.cpu() for k, t in out.items()}


def _bwd_ops(prog):
    """One row-pass op and one column-pass op (the last of each pass)."""
    vert = [i for i, op in enumerate(prog) if op.vertical]
    horz = [i for i, op in enumerate(prog) if not op.vertical]
    return [vert[-1], horz[-1]]


@pytest.mark.parametrize("ramp", [False, True], ids=["random", "ramp"])
@pytest.mark.parametrize("which", [0, 1], ids=["rowpass", "colpass"])
@pytest.mark.parametrize("hw", LEVEL_SHAPES)
def test_step_backward_on_the_saved_forward(hw, which, ramp):
    """Both forms of ops.lift_step_bwd -- the fused BWD launch and the fp32 launches -- on the `saved` slice that the TRAIN forward
    wrote (consistent src, skip, t1, t2, t3, unlike random tensors): G[src], dtaps, dw1 .. db4 and the chain's dsk, dt3, dpre2, dr
    against float64 autograd of that step, G[dst_in] == g exactly.  With the row ramp g grows by six decades down the image, so the
    tiles of a run differ in their operand scales and the handed-down rows are rescaled; the per-pixel gradients are then compared
    row by row, normalised by the row's factor."""
    ops, gu = _ops()
    lv = _level(hw)
    i = _bwd_ops(lv["prog"])[which]
    op = lv["prog"][i]
    h, w = op.h, op.w
    gen = torch.Generator().manual_seed(77 + i)
    g = (torch.rand(P, B, 1, h, w, generator=gen) - 0.5) * 3.0
    rows = None
    if ramp:
        r = 10.0 ** torch.linspace(-3, 3, h, dtype=torch.float64)
        g = (g.double() * r[:, None]).float()
        rows = [r] * P
    ref, f32s = _backward_reference(lv, i, g, ("bwd", hw, i, ramp))
    bad = []
    forms = [("fp32 launches", False)] + ([("fused BWD", True)] if ops.bwd_lift_f16() else [])
    for name, fused in forms:
        got = _kernel_backward(lv, i, g, fused)
        assert torch.equal(got["gdin"], g), name
        tag = "bwd %s op %d (%dx%d v=%d) %s %s" % (hw, i, h, w, op.vertical, "ramp" if ramp else "rand", name)
        for k in R.CHAIN_KEYS + ("gsrc", "dtaps") + tuple("d" + k for k in R.W_KEYS):
            kw = dict(row_dims=(0, 1, 3), row_norm=rows) if (ramp and k in PIXEL_GRADS) else {}
            bad += R.check(tag, k, [got[k][p] for p in range(P)], ref, f32s if fused else f32s[:2] + f32s[3:], floor=R.GRAD_FLOOR, **kw)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 6. whole transform
@pytest.mark.skipif(CHILD, reason="not part of the forced runs")
def test_whole_transform_eval():
    """Eval lifting_forward / lifting_inverse at L = 3, 64 x 96: coefficients and the reconstruction from the kernel's own
    coefficients against float64 (whose reconstruction is x)."""
    ops, gu = _ops()
    cfg = dict(model.DEFAULT_CFG, filtersize=5, dwtlevels=3)
    _, sds, taps, packed = _weights()
    x = torch.rand(P, B, 1, 64, 96, generator=torch.Generator().manual_seed(606)) - 0.5
    ref, f32s = R.evaluate(lambda p, dtype, tanh: R.transform(x[p].to(dtype), R.cast_sd(sds[p], dtype), cfg, tanh), P)
    ll, yh = ops.lifting_forward(gu.dev(x), taps, packed, 3, C, 5, 0.1)
    xr = ops.lifting_inverse(ll, yh, taps, packed, C, 5, 0.1)
    got = {"ll": ll.cpu(), "xr": xr.cpu()}
    got.update({"yh%d" % i: t.cpu() for i, t in enumerate(yh)})
    bad = []
    for k in got:
        bad += R.check("transform L=3 64x96", k, [got[k][p] for p in range(P)], ref, f32s)
    assert not bad, bad


def _stacks(sds, nblocks, gu):
    taps = torch.stack([torch.stack([sd["preProcessingList.%d.weight" % j].reshape(3) for sd in sds], 0) for j in range(4)], 0)
    W = []
    for n in (1, 2, 3, 4):
        for k in ("weight", "bias"):
            W.append(torch.stack([torch.stack([torch.stack([sd["%s.%d.conv%d.%s" % (kind, b, n, k)] for sd in sds], 0)
                                               for kind in ("P_blocks", "U_blocks")], 0) for b in range(nblocks)], 0))
    return gu.dev(taps), [gu.dev(t) for t in W]


@pytest.mark.skipif(CHILD, reason="not part of the forced runs")
@pytest.mark.parametrize("K,different,scale", [(5, False, False), (3, True, True)])
def test_whole_transform_gradients(K, different, scale):
    """LiftingFn / LiftingInvFn at L = 2, 64 x 96: the gradient of every input, tap, block parameter and gain against float64
    autograd of the oracle."""
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import autograd as ag
    ops, gu = _ops()
    L = 2
    cfg = dict(model.DEFAULT_CFG, dwtlevels=L, filtersize=K, block_property="different" if different else "same",
               scale=1 if scale else 0)
    nblocks = 2 * 2 * L if different else 2
    sds = [filled(weights.autoencoder_template(cfg), "domg%d." % p) for p in range(P)]
    gen = torch.Generator().manual_seed(808)
    x = torch.rand(P, B, 1, 64, 96, generator=gen) - 0.5
    gouts = [torch.rand(P, B, 1, 16, 24, generator=gen) - 0.5] + \
            [torch.rand(P, B, 3, 64 >> (i + 1), 96 >> (i + 1), generator=gen) - 0.5 for i in range(L)]
    gx = torch.rand(P, B, 1, 64, 96, generator=gen) - 0.5

    def fn(p, dtype, tanh):
        fwd, inv = R.transform_grads(x[p].to(dtype), R.cast_sd(sds[p], dtype), cfg, [t[p] for t in gouts], gx[p], tanh)
        out = {"fwd." + k: v for k, v in fwd.items()}
        out.update({"inv." + k: v for k, v in inv.items()})
        return out
    def ordered(chunk, reverse):        # the bias gradients' fp32 atomics have no fixed order: lift_ref.oracle_bias_order
        def run(p):
            with R.oracle_bias_order(chunk, reverse):
                return fn(p, R.F32, torch.tanh)
        return run
    ref, f32s = R.evaluate(fn, P, extra=[ordered(*o) for o in R.BIAS_ORDERS])

    def gains():
        if not scale:
            return None, None
        nh = torch.stack([lifting.LIFTING_COEFF[4] + sd["nh"].reshape(()) * 0.1 for sd in sds]).float()
        nl = torch.stack([lifting.LIFTING_COEFF[5] + sd["nl"].reshape(()) * 0.1 for sd in sds]).float()
        return gu.dev(nh).requires_grad_(True), gu.dev(nl).requires_grad_(True)
    meta = dict(levels=L, C=C, K=K, rw=0.1, linear=False, different=different)
    got = {}
    for side in ("fwd", "inv"):
        nh, nl = gains()
        taps, Wt = _stacks(sds, nblocks, gu)
        taps.requires_grad_(True)
        for t in Wt:
            t.requires_grad_(True)
        if side == "fwd":
            xd = gu.dev(x).requires_grad_(True)
            outs = ag.LiftingFn.apply(xd, taps, meta, nh, nl, *Wt)
            torch.autograd.backward(outs, [gu.dev(t) for t in gouts])
            got["fwd.x"] = xd.grad
            coeffs = [o.detach() for o in outs]
        else:
            cin = [c.clone().requires_grad_(True) for c in coeffs]
            xr = ag.LiftingInvFn.apply(taps, meta, L, nh, nl, *cin, *Wt)
            xr.backward(gu.dev(gx))
            got["inv.ll"] = cin[0].grad
            got.update({"inv.yh%d" % i: c.grad for i, c in enumerate(cin[1:])})
        for j in range(4):
            got["%s.preProcessingList.%d.weight" % (side, j)] = taps.grad[j].reshape(P, 1, 1, 3, 1)
        idx = 0
        for n in (1, 2, 3, 4):
            for k in ("weight", "bias"):
                for b in range(nblocks):
                    for u, kind in enumerate(("P_blocks", "U_blocks")):
                        got["%s.%s.%d.conv%d.%s" % (side, kind, b, n, k)] = Wt[idx].grad[b, u]
                idx += 1
        if scale:       # d/d(sd.nh) = 0.1 d/d(gain)
            got[side + ".nh"], got[side + ".nl"] = nh.grad * 0.1, nl.grad * 0.1
    bad = []
    for k in sorted(got):
        t = got[k].cpu()
        if k not in ref:        # a block this configuration's pass does not use
            assert float(t.abs().max()) == 0.0, k
            continue
        bad += R.check("gradients L=2 64x96 K=%d %s" % (K, cfg["block_property"]), k,
                       [t[p].reshape(ref[k][p].shape) for p in range(P)], ref, f32s, floor=R.GRAD_FLOOR)
    assert set(ref) <= set(got), sorted(set(ref) - set(got))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 7. forced run lengths
@pytest.mark.skipif(CHILD, reason="already inside a child run")
def test_forced_run_lengths():
    """Fresh child processes (the settings are read once per process), one after the other, each under its own time limit: run
    length 2, then run length 3 with the split-fp16 weight gradients at every size.  A child that ends by a signal or at its time
    limit fails the test and nothing more is started."""
    for env in ({"LLDWT_LF_RL": "2"}, {"LLDWT_LF_RL": "3", "LLDWT_WGRAD16_MIN": "1"}):
        cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-m", "gpu",
               "-p", "no:cacheprovider", "-k", "eval_step_three_forms or train_forward or step_backward"]
        r = subprocess.run(cmd, env=dict(os.environ, LLDWT_LIFT_DOMAIN_CHILD="1", **env), capture_output=True, text=True)
        tail = r.stdout[-6000:] + r.stderr[-2000:]
        print("\n[forced runs] %s: exit status %d\n%s" % (env, r.returncode, "\n".join(
            ln for ln in r.stdout.splitlines() if " kernel " in ln or "passed" in ln or "failed" in ln)))
        assert r.returncode >= 0 and r.returncode not in (124, 137, 134, 139), (env, r.returncode, tail)
        assert r.returncode == 0, (env, tail)
        assert " passed" in r.stdout and " skipped" not in r.stdout.splitlines()[-1], tail
