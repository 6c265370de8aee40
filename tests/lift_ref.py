"""float64 reference for the learned lifting step and transform: the yardstick of tests/test_lift_ref_host.py and
tests/test_gpu_lift_domain.py.  No device code.

The formulas are the oracle's (oracle/lifting.py is dtype-agnostic): skip_filter, p_block, lifting_forward / lifting_inverse run
on float64 copies of the fp32 weights and inputs.  p_block does not return its intermediates, so `step` restates it line by line
with the intermediates kept (skip, t1, t2, t3, out -- what the TRAIN forward saves for the backward); the host test pins that
restatement to p_block bit for bit in both dtypes.

Yardstick.  The same functions in fp32 on the same inputs are the fp32 oracle, and its distance from float64 is what fp32 costs
the formula.  The kernels declare one deviation from it: tanh is copysign(1 - 2 / (exp2(2 log2(e) |x|) + 1), x) (csrc/common.h
fast_tanh, csrc/lifting_f16.hip tanh_scaled), so the fp32 oracle is evaluated a second time with that formula in fp32 torch ops.
The yardstick of a compared tensor is the larger of the two errors, per plane.  Bars (the rules of test_gpu_conv_f16x3.
test_accuracy_is_fp32_level and test_wgrad_f16x3_vs_float64_and_fp32_kernel for the same split arithmetic):
    values      |kernel - f64| <= 4 * yardstick + 2e-7 * max|f64|
    gradients   |kernel - f64| <= 4 * yardstick + 5e-7 * max|f64|
with every maximum taken per plane and per tensor, no element left out.

Restated properties of the declared arithmetic (further fp32 evaluations that join the yardstick of the kernel that declares them,
see DESIGN.md 2.2 for the cases that needed them):
  * step_grads_split: the fused BWD launch keeps its gradient images as split fp16 (hi + lo) under ONE power-of-two scale per
    16 x 32 tile, taken from a bound (max|g| of the tile's patch x the L1 norms of the transposed weights).  fp16 has no exponent
    below 2^-24, so a value far below its tile's bound keeps fewer than 22 bits -- six decades inside one tile leave the small
    rows about 12;
  * oracle_bias_order: a bias gradient is one fp32 number summed over every pixel by one fp32 atomic per workgroup, in no fixed
    order.  A single number's fp32 error is one draw, not a maximum over many elements, so the yardstick takes the worst of a
    few fixed orders (partial sums of 64 / 256 / 1024 values added one after another, forwards or backwards)."""
import contextlib

import torch
import torch.nn.functional as F

from oracle import lifting

F64, F32 = torch.float64, torch.float32
RW = 0.1                                                     # res_connection_weight of every configuration here
TWO_LOG2E = 2.88539008177792681472
W_KEYS = ("w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4")
STEP_KEYS = ("skip", "t1", "t2", "t3", "out")
CHAIN_KEYS = ("dsk", "dt3", "dpre2", "dr")


# ------------------------------------------------------------------------------------------------ the declared tanh
class _DeclaredTanh(torch.autograd.Function):
    """The kernels' tanh in the dtype of its argument; derivative 1 - t^2 from the output, as the backward kernels take it."""

    @staticmethod
    def forward(ctx, x):
        e = torch.exp2(x.abs() * TWO_LOG2E)
        t = torch.copysign(1.0 - 2.0 / (e + 1.0), x)
        ctx.save_for_backward(t)
        return t

    @staticmethod
    def backward(ctx, g):
        (t,) = ctx.saved_tensors
        return g * (1.0 - t * t)


def declared_tanh(x):
    return _DeclaredTanh.apply(x)


class _TorchWith:
    """`torch` with another tanh, for oracle.lifting's module-level name."""

    def __init__(self, tanh):
        self.tanh = tanh

    def __getattr__(self, name):
        return getattr(torch, name)


@contextlib.contextmanager
def oracle_tanh(tanh):
    """oracle.lifting evaluated with `tanh` in place of torch.tanh for the duration."""
    saved = lifting.torch
    lifting.torch = saved if tanh is torch.tanh else _TorchWith(tanh)
    try:
        yield
    finally:
        lifting.torch = saved


# ------------------------------------------------------------------------------------------------ parameters
def block_of(sd, prefix, dtype=None):
    """The eight tensors of P/U block `prefix` ('U_blocks.0.') of an oracle state dict, keyed like the C-ABI (w1 .. b4)."""
    out = {}
    for n in (1, 2, 3, 4):
        out["w%d" % n] = sd[prefix + "conv%d.weight" % n]
        out["b%d" % n] = sd[prefix + "conv%d.bias" % n]
    return {k: (v if dtype is None else v.to(dtype)) for k, v in out.items()}


def tap_of(sd, j, dtype=None):
    t = sd["preProcessingList.%d.weight" % j].reshape(3)
    return t if dtype is None else t.to(dtype)


def cast_sd(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------ one step
def step(src, dst, tap, blk, sign, vertical=True, linear=False, rw=RW, tanh=torch.tanh):
    """One lifting step (wavelet_forward_v2.py:60-74 with P_block_v2.py:40-55) in the dtype of its arguments.
    src, dst: (B, 1, h, w) as the kernels see them; a step with vertical == False filters along w, which the oracle does on the
    transposed arrays.  -> dict skip, t1, t2, t3, out (+ r, pre2: the pre-activations) in the layout of the arguments:
    skip, out (B, 1, h, w); the others (B, C, h, w).  linear: t1 = r, t2 = pre2 (linearity_flag == 0)."""
    s, d = (src, dst) if vertical else (src.transpose(2, 3), dst.transpose(2, 3))
    res = _step_oriented(s, d, tap, blk, sign, linear, rw, tanh)
    return res if vertical else {k: v.transpose(2, 3) for k, v in res.items()}


def _step_oriented(s, d, tap, blk, sign, linear, rw, tanh):
    """The step in the oracle's orientation (the filter runs along dim 2)."""
    pad = blk["w1"].shape[-1] // 2
    skip = lifting.skip_filter(s, tap.reshape(1, 1, 3, 1))
    r = F.conv2d(skip, blk["w1"], blk["b1"], padding=pad)
    t1 = r if linear else tanh(r)
    pre2 = F.conv2d(t1, blk["w2"], blk["b2"], padding=pad)
    t2 = pre2 if linear else tanh(pre2)
    t3 = F.conv2d(t2, blk["w3"], blk["b3"], padding=pad)
    t3 = t3 + r
    net = F.conv2d(t3, blk["w4"], blk["b4"], padding=pad)
    out = d + sign * (skip + net * rw)
    return dict(skip=skip, r=r, t1=t1, pre2=pre2, t2=t2, t3=t3, net=net, out=out)


def step_grads(src, dst, tap, blk, g, sign, vertical=True, linear=False, rw=RW, tanh=torch.tanh):
    """Autograd of one step in the dtype of its arguments, for the loss sum(out * g).  -> dict
         gsrc, gdin          dL/d src, dL/d dst_in (== g)
         dtaps, dw1 .. db4   dL/d taps, dL/d block parameters
         dsk, dt3, dpre2, dr the backward-data chain of the kernels: gradients of sum(net * g) (the P block alone, without
                             sign * rw) with respect to skip, t3, conv2's pre-activation and conv1's pre-activation."""
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    src_, dst_, tap_ = leaf(src), leaf(dst), leaf(tap)
    blk_ = {k: leaf(v) for k, v in blk.items()}
    tr = (lambda t: t) if vertical else (lambda t: t.transpose(2, 3))
    f = _step_oriented(tr(src_), tr(dst_), tap_, blk_, sign, linear, rw, tanh)
    chain = torch.autograd.grad((f["net"] * tr(g)).sum(), [f["skip"], f["t3"], f["pre2"], f["r"]], retain_graph=True)
    ins = [src_, dst_, tap_] + [blk_[k] for k in W_KEYS]
    gr = torch.autograd.grad((f["out"] * tr(g)).sum(), ins)
    out = dict(zip(CHAIN_KEYS, [tr(c) for c in chain]))
    out.update(gsrc=gr[0], gdin=gr[1], dtaps=gr[2])
    out.update({"d" + k: t for k, t in zip(W_KEYS, gr[3:])})
    return {k: v.detach() for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ restated: split-fp16 tiles
TILE_H, TILE_W = 16, 32


def pow2_scale(amax):
    """csrc/lifting_f16.hip pow2_scale: s = 2^k with amax * s in [2^14, 2^15); 1 for amax == 0."""
    _, e = torch.frexp(amax)
    s = torch.ldexp(torch.ones_like(amax), (15 - e).clamp(-120, 120))
    return torch.where(amax > 0, s, torch.ones_like(amax))


def split_fp16(v, s):
    """v as the kernels hold an operand: hi = fp16(v s), lo = fp16(v s - hi), read back as (hi + lo) / s."""
    x = v * s
    hi = x.half().float()
    return (hi + (x - hi).half().float()) / s


def tile_max(a, th, tw, halo):
    """(B, c, h, w) -> (B, 1, h, w): for every pixel max|a| over its own th x tw tile grown by `halo` pixels on every side."""
    Bn, _, h, w = a.shape
    m = a.abs().amax(dim=1, keepdim=True)
    out = torch.empty_like(m)
    for y0 in range(0, h, th):
        for x0 in range(0, w, tw):
            patch = m[:, :, max(0, y0 - halo):y0 + th + halo, max(0, x0 - halo):x0 + tw + halo]
            out[:, :, y0:y0 + th, x0:x0 + tw] = patch.amax(dim=(2, 3), keepdim=True)
    return out


def step_grads_split(src, tap, blk, g, sign, vertical=True, rw=RW):
    """The backward-data chain of one step in fp32 with every operand image (g, dt3, dpre2, dr) held as the fused BWD launch holds
    it: split fp16 under one scale per tile -- pow2_scale of max|g| over the tile's 32 x 48 patch for g, of that maximum times the
    largest row L1 norm of conv4^T (and of conv3^T) for dt3 (and dpre2), of max|dr| over the tile's 20 x 36 region for dr.  Each pixel
    takes the scale of the tile that owns it.  -> dict dt3, dpre2, dr, dsk, gsrc (layout of step_grads)."""
    tr = (lambda t: t) if vertical else (lambda t: t.transpose(2, 3))
    th, tw = (TILE_H, TILE_W) if vertical else (TILE_W, TILE_H)             # the tiles lie in the kernels' (h, w) frame
    src, g, tap = src.float(), tr(g.float()), tap.float()
    blk = {k: v.float() for k, v in blk.items()}
    f = _step_oriented(tr(src), torch.zeros_like(tr(src)), tap, blk, sign, False, rw, torch.tanh)
    pad = blk["w1"].shape[-1] // 2
    convT = lambda x, w: F.conv_transpose2d(x, w, None, padding=pad)
    l1a = blk["w4"].abs().sum(dim=(0, 2, 3)).max()
    l1b = blk["w3"].abs().sum(dim=(0, 2, 3)).max()
    m = tile_max(g, th, tw, 8)
    dt3 = convT(split_fp16(g, pow2_scale(m)), blk["w4"])
    dpre2 = (1 - f["t2"] ** 2) * convT(split_fp16(dt3, pow2_scale(m * l1a)), blk["w3"])
    dr = (1 - f["t1"] ** 2) * convT(split_fp16(dpre2, pow2_scale(m * l1a * l1b)), blk["w2"]) + dt3
    dsk = convT(split_fp16(dr, pow2_scale(tile_max(dr, th, tw, 2))), blk["w1"])
    gsrc = F.conv_transpose2d(sign * (g + rw * dsk), tap.reshape(1, 1, 3, 1), None, padding=(1, 0))
    return {k: tr(v) for k, v in dict(dt3=dt3, dpre2=dpre2, dr=dr, dsk=dsk, gsrc=gsrc).items()}


# ------------------------------------------------------------------------------------------------ restated: bias-sum orders
def ordered_sum(t, chunk, reverse):
    """(B, C, h, w) -> (C,): per channel, partial sums of `chunk` consecutive values, added one after another in the dtype of t."""
    t = t.transpose(0, 1).reshape(t.shape[1], -1)
    t = F.pad(t, (0, -t.shape[1] % chunk))
    part = t.view(t.shape[0], -1, chunk).sum(dim=2)
    if reverse:
        part = part.flip(1)
    acc = torch.zeros_like(part[:, 0])
    for j in range(part.shape[1]):
        acc = acc + part[:, j]
    return acc


def step_bias_grads_ordered(gr, g, sign, chunk, reverse, rw=RW):
    """db1 .. db4 of one step from the chain of step_grads (db4 = sign rw sum g, db3 = .. sum dt3, db2 = .. sum dpre2, db1 = ..
    sum dr), summed in the given order in the dtype of the chain."""
    a = sign * rw
    return {"db4": a * ordered_sum(g.to(gr["dr"].dtype), chunk, reverse), "db3": a * ordered_sum(gr["dt3"], chunk, reverse),
            "db2": a * ordered_sum(gr["dpre2"], chunk, reverse), "db1": a * ordered_sum(gr["dr"], chunk, reverse)}


class _BiasAddOrdered(torch.autograd.Function):
    """y + b with the bias gradient summed as partial sums of `chunk` consecutive values added one after another in fp32."""

    @staticmethod
    def forward(ctx, y, b, chunk, reverse):
        ctx.order = (chunk, reverse)
        return y + b.view(1, -1, 1, 1)

    @staticmethod
    def backward(ctx, g):
        return g, ordered_sum(g, *ctx.order), None, None


class _FunctionalWith:
    def __init__(self, conv2d):
        self.conv2d = conv2d

    def __getattr__(self, name):
        return getattr(F, name)


BIAS_ORDERS = ((64, False), (256, False), (256, True), (1024, False))


@contextlib.contextmanager
def oracle_bias_order(chunk, reverse):
    """oracle.lifting with every conv's bias gradient summed in the given fp32 order for the duration."""
    def conv2d(x, w, b=None, stride=1, padding=0):
        y = F.conv2d(x, w, None, stride=stride, padding=padding)
        return y if b is None else _BiasAddOrdered.apply(y, b, chunk, reverse)
    saved = lifting.F
    lifting.F = _FunctionalWith(conv2d)
    try:
        yield
    finally:
        lifting.F = saved


# ------------------------------------------------------------------------------------------------ whole transform
def transform(x, sd, cfg, tanh=torch.tanh):
    """oracle lifting_forward and lifting_inverse of its own coefficients, in the dtype of x / sd.
    -> dict ll (B,1,h,w), yh0 .. (B,3,h,w), xr."""
    with oracle_tanh(tanh):
        ll, yh = lifting.lifting_forward(x, sd, cfg)
        xr = lifting.lifting_inverse(ll, yh, sd, cfg)
    out = {"ll": ll, "xr": xr}
    out.update({"yh%d" % i: t[:, 0] for i, t in enumerate(yh)})
    return out


def transform_grads(x, sd, cfg, gouts, gx, tanh=torch.tanh):
    """Autograd of the whole transform in the dtype of x / sd: the forward under the loss sum_i <out_i, gouts_i> (outputs in the
    order ll, yh0, ...), then the inverse of the forward's own (detached) coefficients under <xr, gx>.
    -> (fwd, inv): dicts 'x' (forward) or 'll', 'yh0', .. (inverse) plus one entry per state-dict key that received a gradient."""
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    with oracle_tanh(tanh):
        sd1, x1 = {k: leaf(v) for k, v in sd.items()}, leaf(x)
        ll, yh = lifting.lifting_forward(x1, sd1, cfg)
        outs = [ll] + [t[:, 0] for t in yh]
        torch.autograd.backward(outs, [g.to(x.dtype) for g in gouts])
        fwd = {"x": x1.grad}
        fwd.update({k: v.grad for k, v in sd1.items() if v.grad is not None})
        sd2 = {k: leaf(v) for k, v in sd.items()}
        cin = [leaf(o) for o in outs]
        xr = lifting.lifting_inverse(cin[0], [t.unsqueeze(1) for t in cin[1:]], sd2, cfg)
        xr.backward(gx.to(x.dtype))
        inv = {"ll": cin[0].grad}
        inv.update({"yh%d" % i: c.grad for i, c in enumerate(cin[1:])})
        inv.update({k: v.grad for k, v in sd2.items() if v.grad is not None})
    return fwd, inv


# ------------------------------------------------------------------------------------------------ reference + yardstick
def _pmax(t, dims=None):
    """max |t| of one plane's tensor, or per row (dims = the axes to reduce) for the row-normalised comparisons."""
    t = t.double().abs()
    return t.amax(dim=dims) if dims is not None else t.max()


def evaluate(fn, planes, extra=()):
    """fn(p, dtype, tanh) -> dict of tensors for plane p.  Evaluates float64 (the reference), fp32 and fp32 with the declared
    tanh, plus every further fp32 evaluation in `extra` (callables like fn without the dtype / tanh arguments: a restated
    property of the kernels' declared arithmetic).
    -> (ref, f32s): ref[k] is the list over planes of float64 tensors, f32s the list of such dicts for the fp32 evaluations."""
    ref, f32s = {}, [{} for _ in range(2 + len(extra))]
    for p in range(planes):
        for k, v in fn(p, F64, torch.tanh).items():
            ref.setdefault(k, []).append(v.detach())
        runs = [fn(p, F32, torch.tanh), fn(p, F32, declared_tanh)] + [e(p) for e in extra]
        for d, run in zip(f32s, runs):
            for k, v in run.items():
                d.setdefault(k, []).append(v.detach())
    return ref, f32s


def errors(got, ref, row_dims=None, row_norm=None):
    """max |got - ref| per plane (a float), or per row when row_dims is given; divided by row_norm[p] if that is given."""
    out = []
    for p, (a, b) in enumerate(zip(got, ref)):
        e = _pmax(a.double() - b, row_dims)
        out.append(e / row_norm[p] if row_norm is not None else e)
    return out


def yardstick(ref, f32s, key, row_dims=None, row_norm=None):
    """Per plane: the largest error of the fp32 evaluations against float64 for tensor `key`."""
    per = [errors(d[key], ref[key], row_dims, row_norm) for d in f32s if key in d]
    return [torch.stack([torch.as_tensor(e[p]) for e in per]).amax(dim=0) for p in range(len(ref[key]))]


VALUE_FLOOR, GRAD_FLOOR = 2e-7, 5e-7


def check(tag, key, got, ref, f32s, floor=VALUE_FLOOR, row_dims=None, row_norm=None):
    """Asserts the bar for tensor `key` on every plane (got: list over planes of tensors in the layout of ref[key]) and prints the
    worst plane's error beside its yardstick and bar.  Row-normalised form: errors, yardstick and max|f64| all per row of the
    normalised tensors."""
    err = errors(got, ref[key], row_dims, row_norm)
    yard = yardstick(ref, f32s, key, row_dims, row_norm)
    worst, bad = None, []
    for p in range(len(err)):
        mx = _pmax(ref[key][p], row_dims)
        if row_norm is not None:
            mx = mx / row_norm[p]
        bar = 4.0 * yard[p] + floor * mx
        e = torch.as_tensor(err[p])
        i = int(torch.argmax((e / bar.clamp_min(1e-300)).reshape(-1)))              # the element closest to (or furthest past) its bar
        ev, yv, bv = float(e.reshape(-1)[i]), float(torch.as_tensor(yard[p]).reshape(-1)[i]), float(bar.reshape(-1)[i])
        if worst is None or ev * max(worst[2], 1e-300) > worst[0] * max(bv, 1e-300):
            worst = (ev, yv, bv, p)
        if not bool((e <= bar).all()):
            bad.append((p, ev, yv, bv))
    print("%-58s %-6s kernel %.2e  yardstick %.2e  bar %.2e  (plane %d)" % (tag, key, worst[0], worst[1], worst[2], worst[3]))
    return [(tag, key) + b for b in bad]
