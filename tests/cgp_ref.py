"""float64 reference for the context MLP (cgp_out_xo_list with the masked context conv folded into its first layer): the yardstick
of tests/test_cgp_ref_host.py and tests/test_gpu_cgp_domain.py.  No device code.

Per subband g the stack sees [81 tree-context features | 12 causal taps of the quantised subband, zero outside the image] and runs
93 -> 162 -> 54 -> 18 -> 2 = (sigma, mu) as four grouped 1x1 convs with LeakyReLU(0.01) between them -- oracle/entropy.py
conditioned2_forward lines :212-224 after _fold_csc_into_cgp.  Everything here is dtype-agnostic torch on the host: the same
functions on float64 copies are the reference, on fp32 the fp32 oracle, and their distance is the yardstick of a compared tensor.
Bars (the rules of 2.1 / 2.2 of DESIGN.md):
    values      |kernel - f64| <= 4 * yardstick + 2e-7 * max|f64|
    gradients   |kernel - f64| <= 4 * yardstick + 5e-7 * max|f64|
every maximum per plane, per group and per tensor -- for params per output row (sigma and mu apart), for the six-decade cases per
pixel -- no element left out.

Layouts are one plane's: plc (B, G*81, h, w), xq (B, G, h, w), ws[l] (G*c_{l+1}, c_l), bs[l] (G*c_{l+1}); a weight SET holds a
leading plane axis and the trailing (1, 1) of the conv weights, as ops.cgp16_pack takes it.

Restated properties of the declared arithmetic:
  * chain_split: csrc/cgp_f16x3.hip's forward chain in fp32 torch ops -- one power-of-two scale per 32-pixel block for the input
    (from its maximum) and for every hidden layer (from the bound bound_l = bound_{l-1} maxrow|W_l|_1 + max|b_l| of the pack's
    header), operands split into fp16 hi + lo (subnormals included), three products per MAC, fp32 accumulators;
  * ordered_sum: a bias gradient is one fp32 number summed by fp32 atomics in no fixed order, so its yardstick takes the worst of
    a few fixed orders (lift_ref.BIAS_ORDERS)."""
import torch
import torch.nn.functional as F

from lift_ref import BIAS_ORDERS, pow2_scale
from oracle import entropy

F64, F32 = torch.float64, torch.float32
C = (93, 162, 54, 18, 2)
CPLC, NTAPS, K = 81, 12, 5
LIVE = tuple(range(NTAPS))                                   # the live taps of the 5x5 type-A mask: rows 0, 1 and two of row 2
TAP_BITS = (1 << NTAPS) - 1
VALUE_FLOOR, GRAD_FLOOR = 2e-7, 5e-7
SLOPE = 0.01


# ------------------------------------------------------------------------------------------------ inputs
def gather_taps(xq):
    """(B, G, h, w) -> (B, G*12, h, w): tap j of subband g = xq[g] shifted by (j // 5 - 2, j % 5 - 2), zero outside the image."""
    B, G, h, w = xq.shape
    xp = F.pad(xq, (K // 2, K // 2, K // 2, K // 2))
    taps = [xp[:, :, (t // K):(t // K) + h, (t % K):(t % K) + w] for t in LIVE]
    return torch.stack(taps, dim=2).reshape(B, G * NTAPS, h, w)


def cat_input(plc, taps):
    """[plc_g | taps_g] per subband: (B, G*81, h, w), (B, G*12, h, w) -> (B, G*93, h, w)."""
    B, _, h, w = plc.shape
    G = taps.shape[1] // NTAPS
    return torch.cat([plc.reshape(B, G, CPLC, h, w), taps.reshape(B, G, NTAPS, h, w)], dim=2).reshape(B, G * C[0], h, w)


# ------------------------------------------------------------------------------------------------ forward
def stack(cat, ws, bs, G):
    """The four grouped 1x1 layers on the concatenated input (the oracle's loop, intermediates kept)
    -> dict params (B, 2G, h, w) = (sigma, mu) interleaved per subband, h1 (B, G*162, ..), h2, h3 after LeakyReLU."""
    out, t = {}, cat
    for l in range(4):
        t = F.conv2d(t, ws[l].reshape(ws[l].shape[0], -1, 1, 1), bs[l], groups=G)
        if l < 3:
            t = F.leaky_relu(t, SLOPE)
            out["h%d" % (l + 1)] = t
    out["params"] = t
    return out


def forward(plc, xq, ws, bs):
    """One plane in the dtype of its arguments -> dict params, h1, h2, h3."""
    G = xq.shape[1]
    return stack(cat_input(plc, gather_taps(xq)), ws, bs, G)


def unfolded_forward(plc, xq, sd, i):
    """The oracle's own path for tree level i of an entropy-model state dict (conditioned2_forward :212-224): masked 5x5 conv of
    xq, regroup with plc, the grouped stack on the 162-wide input -> params (B, 2G, h, w)."""
    g = xq.shape[1]
    csc = entropy.masked_conv(xq, sd, "csc_list.%d." % i, groups=g)
    p, c = plc.chunk(g, dim=1), csc.chunk(g, dim=1)
    t = torch.cat([z for k in range(g) for z in (p[k], c[k])], dim=1)
    ws = [sd["cgp_out_xo_list.%d.%d.weight" % (i, n)] for n in (0, 2, 4, 6)]
    bs = [sd["cgp_out_xo_list.%d.%d.bias" % (i, n)] for n in (0, 2, 4, 6)]
    return stack(t, ws, bs, g)["params"]


def fold(sd, i, G):
    """_fold_csc_into_cgp of one plane's state dict in float64 -> (ws, bs) fp32, ws[l] (G*c_{l+1}, c_l)."""
    W0 = sd["cgp_out_xo_list.%d.0.weight" % i].double()[:, :, 0, 0]
    b0 = sd["cgp_out_xo_list.%d.0.bias" % i].double()
    Wc = (sd["csc_list.%d.weight" % i] * sd["csc_list.%d.mask" % i]).double()
    bc = sd["csc_list.%d.bias" % i].double()
    c1, cc = W0.shape[0] // G, Wc.shape[0] // G
    cpl = W0.shape[1] - cc
    rw, rb = [], []
    for g in range(G):
        W0g = W0[g * c1:(g + 1) * c1]
        Wcg = Wc[g * cc:(g + 1) * cc, 0].reshape(cc, K * K)[:, list(LIVE)]
        rw.append(torch.cat([W0g[:, :cpl], W0g[:, cpl:] @ Wcg], 1))
        rb.append(b0[g * c1:(g + 1) * c1] + W0g[:, cpl:] @ bc[g * cc:(g + 1) * cc])
    ws = [torch.cat(rw, 0).float()] + [sd["cgp_out_xo_list.%d.%d.weight" % (i, n)][:, :, 0, 0] for n in (2, 4, 6)]
    bs = [torch.cat(rb, 0).float()] + [sd["cgp_out_xo_list.%d.%d.bias" % (i, n)] for n in (2, 4, 6)]
    return ws, bs


# ------------------------------------------------------------------------------------------------ backward
def gate(h):
    """lrelu' from the stored activation, as both backward kernels take it: h > 0 ? 1 : 0.01."""
    return torch.where(h > 0, torch.ones_like(h), torch.full_like(h, SLOPE))


def _convT(d, w, G):
    """Grouped transposed 1x1: d (B, G*co, h, w), w (G*co, ci) -> (B, G*ci, h, w)."""
    B, _, h, wd = d.shape
    co, ci = w.shape[0] // G, w.shape[1]
    return torch.einsum("bgohw,goi->bgihw", d.reshape(B, G, co, h, wd), w.reshape(G, co, ci)).reshape(B, G * ci, h, wd)


def backward(dparams, h1, h2, h3, ws, G):
    """Backward-data from dparams and the GIVEN activations, in the dtype of the arguments
    -> dict d3, d2, d1 (gradients at the pre-activations), dplc (B, G*81, ..), dtaps (B, G*12, ..)."""
    d3 = gate(h3) * _convT(dparams, ws[3], G)
    d2 = gate(h2) * _convT(d3, ws[2], G)
    d1 = gate(h1) * _convT(d2, ws[1], G)
    dcat = _convT(d1, ws[0], G)
    B, _, h, w = dcat.shape
    dcat = dcat.reshape(B, G, C[0], h, w)
    return dict(d3=d3, d2=d2, d1=d1, dplc=dcat[:, :, :CPLC].reshape(B, G * CPLC, h, w),
                dtaps=dcat[:, :, CPLC:].reshape(B, G * NTAPS, h, w))


def wgrad(xin, dy, G):
    """Weight gradient of a grouped 1x1 layer: xin (B, G*ci, h, w), dy (B, G*co, h, w) -> (G*co, ci)."""
    B, _, h, w = xin.shape
    ci, co = xin.shape[1] // G, dy.shape[1] // G
    return torch.einsum("bgop,bgip->goi", dy.reshape(B, G, co, h * w), xin.reshape(B, G, ci, h * w)).reshape(G * co, ci)


def ordered_sum(t, chunk, reverse):
    """(B, c, h, w) -> (c,): per channel, partial sums of `chunk` consecutive values added one after another in the dtype of t."""
    t = t.transpose(0, 1).reshape(t.shape[1], -1)
    t = F.pad(t, (0, -t.shape[1] % chunk))
    part = t.view(t.shape[0], -1, chunk).sum(dim=2)
    if reverse:
        part = part.flip(1)
    acc = torch.zeros_like(part[:, 0])
    for j in range(part.shape[1]):
        acc = acc + part[:, j]
    return acc


def param_grads(cat, h1, h2, h3, dparams, d1, d2, d3, G):
    """The eight weight and bias gradients from the chain of `backward` -> dict dw0 .. dw3 (G*c_{l+1}, c_l), db0 .. db3."""
    out = {}
    for l, (xin, dy) in enumerate(((cat, d1), (h1, d2), (h2, d3), (h3, dparams))):
        out["dw%d" % l] = wgrad(xin, dy, G)
        out["db%d" % l] = dy.sum(dim=(0, 2, 3))
    return out


# ------------------------------------------------------------------------------------------------ restated: the split chain
BLOCK = 32


def pack_header(ws, bs, G):
    """k_cgp16_pack's header quantities per group, fp32: (sw, l1, mb), each (4, G) -- the weight scale 2^k with max|W_l| 2^k in
    [2^14, 2^15), the largest row L1 norm and the largest |bias| of layer l."""
    sw, l1, mb = [], [], []
    for l in range(4):
        w = ws[l].float().reshape(G, C[l + 1], C[l]).abs()
        sw.append(pow2_scale(w.amax(dim=(1, 2))))
        l1.append(w.sum(dim=2).amax(dim=1))
        mb.append(bs[l].float().reshape(G, C[l + 1]).abs().amax(dim=1))
    return torch.stack(sw), torch.stack(l1), torch.stack(mb)


def _split_parts(x):
    hi = x.half().float()
    return hi, (x - hi).half().float()


def chain_split(plc, xq, ws, bs, want_hidden=False):
    """The declared arithmetic of k_cgp16 on one plane, fp32 -> params (B, 2G, h, w) (+ h1, h2, h3 as the TRAIN form stores them).
    Blocks are 32 consecutive pixels of one (image, subband); the last block of an image may be partial."""
    B, G, h, w = xq.shape
    hw = h * w
    x = cat_input(plc.float(), gather_taps(xq.float())).reshape(B, G, C[0], hw)
    nblk = -(-hw // BLOCK)
    x = x[..., torch.arange(nblk * BLOCK).clamp_max(hw - 1)]             # lanes past the image read its last pixel
    x = x.reshape(B, G, C[0], nblk, BLOCK)
    sw, l1, mb = pack_header(ws, bs, G)
    bc = lambda v: v.reshape(1, G, 1, 1, 1)                                        # a per-group scalar over (B, G, c, blk, pix)
    amax = x.abs().amax(dim=(2, 4), keepdim=True)
    s = [pow2_scale(amax)]
    bound = amax
    for l in range(3):
        bound = bound * bc(l1[l]) + bc(mb[l])
        s.append(pow2_scale(bound))
    op_hi, op_lo = _split_parts(x * s[0])
    out = {}
    for l in range(4):
        wl = ws[l].float().reshape(G, C[l + 1], C[l]) * sw[l].reshape(G, 1, 1)
        w_hi, w_lo = _split_parts(wl)
        mm = lambda a, b: torch.einsum("goi,bgikp->bgokp", a, b)
        acc = mm(w_lo, op_hi) + mm(w_hi, op_lo) + mm(w_hi, op_hi)
        inv = (1.0 / s[l]) * (1.0 / bc(sw[l]))
        bias = bs[l].float().reshape(1, G, C[l + 1], 1, 1)
        if l == 3:
            t = acc * inv + bias
            out["params"] = t.reshape(B, G * 2, nblk * BLOCK)[:, :, :hw].reshape(B, 2 * G, h, w)
            break
        t = acc * (inv * s[l + 1]) + bias * s[l + 1]
        v = torch.maximum(t, SLOPE * t)
        if want_hidden:
            hl = (v / s[l + 1]).reshape(B, G * C[l + 1], nblk * BLOCK)[:, :, :hw]
            out["h%d" % (l + 1)] = hl.reshape(B, G * C[l + 1], h, w)
        op_hi, op_lo = _split_parts(v)
    return out


def chain_split_bwd(dparams, h1, h2, h3, ws, G):
    """The declared arithmetic of k_cgp16_bwd on one plane, fp32 -> dict d3, d2, d1, dplc, dtaps.  One scale per 32-pixel block
    for dparams (from its maximum) and for d3, d2, d1 (from that maximum times the transposed layers' largest row L1 norms)."""
    B, _, h, w = dparams.shape
    hw = h * w
    nblk = -(-hw // BLOCK)
    idx = torch.arange(nblk * BLOCK).clamp_max(hw - 1)
    live = (torch.arange(nblk * BLOCK) < hw).reshape(1, 1, 1, nblk, BLOCK)
    blocks = lambda t, c: t.float().reshape(B, G, c, hw)[..., idx].reshape(B, G, c, nblk, BLOCK)
    bc = lambda v: v.reshape(1, G, 1, 1, 1)
    wt = [ws[l].float().reshape(G, C[l + 1], C[l]) for l in range(4)]
    sw = [pow2_scale(t.abs().amax(dim=(1, 2))) for t in wt]
    l1t = [t.abs().sum(dim=1).amax(dim=1) for t in wt]                             # largest COLUMN L1 norm of the forward layer
    v = blocks(dparams, 2) * live                                                 # lanes past the image carry zero
    amax = v.abs().amax(dim=(2, 4), keepdim=True)
    s, bound = [pow2_scale(amax)], amax
    for l in (3, 2, 1):
        bound = bound * bc(l1t[l])
        s.append(pow2_scale(bound))
    gates = [None, blocks(gate(h3.float()), C[3]), blocks(gate(h2.float()), C[2]), blocks(gate(h1.float()), C[1])]
    op_hi, op_lo = _split_parts(v * s[0])
    out, names = {}, ("d3", "d2", "d1")
    for b, l in enumerate((3, 2, 1, 0)):
        w_hi, w_lo = _split_parts(wt[l] * sw[l].reshape(G, 1, 1))
        mm = lambda a, x: torch.einsum("goi,bgokp->bgikp", a, x)
        acc = mm(w_lo, op_hi) + mm(w_hi, op_lo) + mm(w_hi, op_hi)
        inv = (1.0 / s[b]) * (1.0 / bc(sw[l]))
        if b == 3:
            t = (acc * inv).reshape(B, G, C[0], nblk * BLOCK)[..., :hw].reshape(B, G, C[0], h, w)
            out["dplc"] = t[:, :, :CPLC].reshape(B, G * CPLC, h, w)
            out["dtaps"] = t[:, :, CPLC:].reshape(B, G * NTAPS, h, w)
            break
        val = acc * (inv * s[b + 1]) * gates[b + 1]
        out[names[b]] = (val / s[b + 1]).reshape(B, G * C[l], nblk * BLOCK)[..., :hw].reshape(B, G * C[l], h, w)
        op_hi, op_lo = _split_parts(val)
    return out


def wgrad_ordered(xin, dy, G, chunk, reverse):
    """wgrad with the pixels summed as partial sums of `chunk` consecutive pixels added one after another in the dtype of the
    arguments; the bias gradient rides as one more input row of ones -> (G*co, ci + 1)."""
    B, _, h, w = xin.shape
    ci, co = xin.shape[1] // G, dy.shape[1] // G
    x = torch.cat([xin.reshape(B, G, ci, h * w), torch.ones(B, G, 1, h * w, dtype=xin.dtype)], dim=2)
    x = x.permute(1, 2, 0, 3).reshape(G, ci + 1, -1)
    d = dy.reshape(B, G, co, h * w).permute(1, 2, 0, 3).reshape(G, co, -1)
    n = x.shape[2]
    x, d = F.pad(x, (0, -n % chunk)), F.pad(d, (0, -n % chunk))
    part = torch.einsum("gokc,gikc->kgoi", d.reshape(G, co, -1, chunk), x.reshape(G, ci + 1, -1, chunk))
    if reverse:
        part = part.flip(0)
    acc = torch.zeros_like(part[0])
    for j in range(part.shape[0]):
        acc = acc + part[j]
    return acc.reshape(G * co, ci + 1)


def headroom(ws, bs, G):
    """Binades of the chain's 18 that the bounds of layers 0 .. 2 spend beyond an even network, per group (G,) -- the measure
    of ops.cgp16_supported: sum over the layers of log2(max row L1 norm / median row L1 norm), with a layer's largest |bias|
    counted as the L1 norm of one more row (a bias enters the bound as a row does)."""
    tot = torch.zeros(G, dtype=F64)
    for l in range(3):
        rows = ws[l].double().reshape(G, C[l + 1], C[l]).abs().sum(dim=2)
        med = rows.median(dim=1).values
        top = torch.maximum(rows.amax(dim=1), bs[l].double().reshape(G, C[l + 1]).abs().amax(dim=1))
        tot += torch.log2(top / med).clamp_min(0.0)
    return tot


# ------------------------------------------------------------------------------------------------ weight and input sets
def iid_weights(P, G, seed, bias=0.1):
    """The tests' usual set: randn / sqrt(c_in) per (plane, group), biases 0.1 randn (sigma's + 1): ws (P, G*c_{l+1}, c_l, 1, 1)."""
    g = torch.Generator().manual_seed(seed)
    ws = [torch.randn(P, G * C[l + 1], C[l], 1, 1, generator=g) / C[l] ** 0.5 for l in range(4)]
    bs = [torch.randn(P, G * C[l + 1], generator=g) * bias for l in range(4)]
    bs[3] = bs[3] + torch.tensor([1.0, 0.0] * G)
    return ws, bs


UNIT = (5, 7, 3)                                              # the unit of layer 0, 1, 2 that the variants below touch, in every group


def _clone(ws, bs):
    return [w.clone() for w in ws], [b.clone() for b in bs]


def rescaled(ws, bs, G, log2b):
    """The same function with unit UNIT[l] of layer l louder by 2^log2b[l]: its row and bias times 2^b, its column in layer l + 1
    times 2^-b (powers of two and a positively homogeneous activation: exact)."""
    ws, bs = _clone(ws, bs)
    for l, b in enumerate(log2b):
        if b:
            for g in range(G):
                u = g * C[l + 1] + UNIT[l]
                ws[l][:, u] *= 2.0 ** b
                bs[l][:, u] *= 2.0 ** b
                ws[l + 1][:, g * C[l + 2]:(g + 1) * C[l + 2], UNIT[l]] *= 2.0 ** -b
    return ws, bs


def big_bias(ws, bs, G, value):
    """A layer-0 unit with bias `value` whose column in layer 1 is zero: it feeds nothing, but enters the bound."""
    ws, bs = _clone(ws, bs)
    for g in range(G):
        bs[0][:, g * C[1] + UNIT[0]] = value
        ws[1][:, g * C[2]:(g + 1) * C[2], UNIT[0]] = 0.0
    return ws, bs


def dead_unit(ws, bs, G):
    """A layer-0 unit with an all-zero row AND a zero bias (its activation is exactly 0: the backward's gate at h == 0 is 0.01)
    and a layer-1 unit with an all-zero row that keeps its bias."""
    ws, bs = _clone(ws, bs)
    for g in range(G):
        ws[0][:, g * C[1] + UNIT[0]] = 0.0
        bs[0][:, g * C[1] + UNIT[0]] = 0.0
        ws[1][:, g * C[2] + UNIT[1]] = 0.0
    return ws, bs


def positive(ws, bs, G):
    """|w| and |b| of the set: with inputs that are all equal and positive every hidden unit of a pixel away from the image's
    border sits AT the bound its layer's scale is taken from (max input x row L1 norm + bias, signs aligned)."""
    return [w.abs() for w in ws], [b.abs() for b in bs]


def dead_tap(ws, bs, G):
    ws, bs = _clone(ws, bs)
    ws[0][:, :, CPLC + 3] = 0.0
    return ws, bs


def bench_weights(G=3, level=0):
    """oracle.weights.fill_by_name on the benchmark model (conditioned2ZTsepSubbands, four levels), tree level `level`, the three
    colour planes' entropy models folded -> ws, bs as a weight set (P = 3)."""
    from oracle import weights
    cfg = dict(dwtlevels=4, clrch=1, entropy_layer="conditioned2ZTsepSubbands")
    per = []
    for p in range(3):
        sd = weights.entropy_template(cfg)
        sd = {k[len("model%d.entropymodel." % p):]: v
              for k, v in weights.fill_by_name({"model%d.entropymodel.%s" % (p, k): v for k, v in sd.items()}).items()}
        per.append(fold(sd, level, G))
    ws = [torch.stack([per[p][0][l] for p in range(3)])[:, :, :, None, None].contiguous() for l in range(4)]
    bs = [torch.stack([per[p][1][l] for p in range(3)]).contiguous() for l in range(4)]
    return ws, bs


RESCALES = ((3, 0, 0), (0, 3, 0), (0, 0, 3), (3, 3, 3), (6, 0, 0), (0, 6, 0), (0, 0, 6), (6, 6, 6),
            (10, 0, 0), (0, 10, 0), (0, 0, 10), (10, 10, 10))
BIASES = (1e2, 1e4, 1e6)


WEIGHT_SET_NAMES = (("iid",) + tuple("rescaled_%d_%d_%d" % r for r in RESCALES) + tuple("bias_%.0e" % v for v in BIASES) +
                    ("dead_unit", "dead_tap", "positive", "bench"))


def weight_sets(P, G, seed):
    """name -> (ws, bs): the weight domain of DESIGN.md 2.3.  'rescaled_*' compute the same function as 'iid'."""
    base = iid_weights(P, G, seed)
    sets = {"iid": base}
    for r in RESCALES:
        sets["rescaled_%d_%d_%d" % r] = rescaled(*base, G, r)
    for v in BIASES:
        sets["bias_%.0e" % v] = big_bias(*base, G, v)
    sets["dead_unit"] = dead_unit(*base, G)
    sets["dead_tap"] = dead_tap(*base, G)
    sets["positive"] = positive(*base, G)
    sets["bench"] = bench_weights(G)
    assert tuple(sets) == WEIGHT_SET_NAMES
    return sets


def plane_weights(ws, bs, p, dtype=None):
    """Plane p of a weight set as `forward` takes it."""
    w = [t[p, :, :, 0, 0] for t in ws]
    b = [t[p] for t in bs]
    return ([t.to(dtype) for t in w], [t.to(dtype) for t in b]) if dtype is not None else (w, b)


def input_sets(P, B, G, h, w, seed):
    """name -> (plc (P, B, G*81, h, w), xq (P, B, G, h, w)), fp32; xq non-zero at every pixel unless the case says otherwise."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)

    def taps(scale, lim=None):
        t = (rn(P, B, G, h, w) * scale).round()
        t = torch.where(t == 0, torch.ones_like(t), t)
        return t if lim is None else t.clamp(-lim, lim)
    plc1 = rn(P, B, G * CPLC, h, w)
    sets = {"taps4_feat1": (plc1, taps(4.0)),
            "taps4_feat1e-3": (plc1 * 1e-3, taps(4.0)),
            "taps4_feat1e-6": (plc1 * 1e-6, taps(4.0)),
            "taps4095_feat1": (plc1, taps(2000.0, 4095.0)),
            "all_zero": (torch.zeros_like(plc1), torch.zeros(P, B, G, h, w))}
    hw = h * w
    if hw >= 3 * BLOCK:
        # block 1 of every image all zero: its features, and every pixel its 12 taps reach (rows above, columns beside)
        pz, xz = plc1.clone().reshape(P, B, G * CPLC, hw), taps(4.0)
        pz[..., BLOCK:2 * BLOCK] = 0.0
        y0, y1 = BLOCK // w, (2 * BLOCK - 1) // w
        xz[..., max(0, y0 - 2):y1 + 1, :] = 0.0
        sets["zero_block"] = (pz.reshape(plc1.shape), xz)
    # six decades across the 32 pixels of every block: features and subband values of pixel p times 10^(-6 (p % 32) / 31)
    ramp = torch.logspace(0, -6, BLOCK).repeat(-(-hw // BLOCK))[:hw].reshape(h, w)
    sets["six_decades"] = (plc1 * ramp, taps(4.0) * ramp)
    big = plc1.clone()
    big[:, :, 7, h // 2, w // 2] = 1e4
    sets["feature_1e4"] = (big, taps(4.0))
    # large taps with small features: the block's scale comes from the taps and the features fall into the low halves of the split
    sets["taps4095_feat1e-3"] = (plc1 * 1e-3, taps(2000.0, 4095.0))
    sets["taps4095_feat1e-6"] = (plc1 * 1e-6, taps(2000.0, 4095.0))
    return sets


# ------------------------------------------------------------------------------------------------ errors, yardstick, bar
PER_GROUP, PER_ROW, PER_PIXEL = (1, 3, 4), (1, 4), (3,)


def _units(t, G, reduce):
    """(P, B, G*c, h, w) or (P, G*co, ci) -> max |t| over the axes `reduce` of the (P, B, G, c, hw) view."""
    t = t.double().abs()
    if t.dim() == 3:                                                                # a weight gradient: rows of a group
        P = t.shape[0]
        return t.reshape(P, G, -1).amax(dim=2)
    if t.dim() == 2:                                                                # a bias gradient: the numbers of a group
        return t.reshape(t.shape[0], G, -1).amax(dim=2)
    P, B = t.shape[:2]
    return t.reshape(P, B, G, t.shape[2] // G, -1).amax(dim=reduce)


def measure(got, ref, f32s, G, floor=VALUE_FLOOR, reduce=PER_GROUP):
    """got, ref, every f32s[i]: tensors with a leading plane axis -> (error, yardstick, bar, error / bar) of the unit closest to
    (or furthest past) its bar, and whether any unit is past it (a NaN is)."""
    ref = ref.double()
    err = _units(got.double() - ref, G, reduce)
    yard = torch.stack([_units(f.double() - ref, G, reduce) for f in f32s]).amax(dim=0)
    bar = 4.0 * yard + floor * _units(ref, G, reduce)
    nan = torch.isnan(err)
    ratio = torch.where(nan, torch.full_like(err, float("inf")), err / bar.clamp_min(1e-300))
    i = int(torch.argmax(ratio.reshape(-1)))
    pick = lambda t: float(t.reshape(-1)[i])
    return pick(err), pick(yard), pick(bar), pick(ratio), bool((nan | (err > bar)).any())


def check(tag, key, got, ref, f32s, G, floor=VALUE_FLOOR, reduce=PER_GROUP):
    """Prints the worst unit's error beside its yardstick and bar; -> the list of misses (empty: the bar holds everywhere)."""
    e, y, b, r, bad = measure(got, ref, f32s, G, floor, reduce)
    print("%-46s %-7s kernel %.2e  yardstick %.2e  bar %.2e  ratio %6.2f" % (tag, key, e, y, b, r))
    return [(tag, key, e, y, b)] if bad else []
