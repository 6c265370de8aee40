"""GPU: the split-fp16 subband MLP (csrc/subband_mlp_f16.hip) against a float64 evaluation of the same weights on the host, its
weight pack against a numpy statement of the layout, and its block walk (looping waves, tails, image boundaries).

Bar.  OLD_ERR holds max|y - float64| of the fp32-MFMA kernel this one replaced (k_subband_mlp_mfma, parent commit), measured on
an MI355X on exactly these cases.  The new kernel must stay within 2x of it per case: split operands carry 2^-22
against fp32's 2^-24, but the error of both forms is set by the fp32 tanh and bias arithmetic they share.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

P, B, H = 2, 3, 32
SHAPES = [(9, 21), (1, 64 * 3 + 1), (70, 70)]       # one partial block; three blocks + 1; several workgroups, looping waves
WEIGHTS = ["default", "x8", "zero_layer"]
CASES = [(C, hw, wk, tr) for C in (1, 3) for hw in SHAPES for wk in WEIGHTS for tr in (False, True)]

# max|y - float64| of the replaced fp32 kernel, per case id (measured at the parent commit on an MI355X by running
# measure_errors() of this file against it; the figures are also in DESIGN.md 2.4)
OLD_ERR = {
    "C1-9x21-default-down": 1.1358e-07,
    "C1-9x21-default-up": 6.0266e-07,
    "C1-9x21-x8-down": 3.6817e-06,
    "C1-9x21-x8-up": 4.5290e-05,
    "C1-9x21-zero_layer-down": 1.1358e-07,
    "C1-9x21-zero_layer-up": 4.8286e-07,
    "C1-1x193-default-down": 9.3730e-08,
    "C1-1x193-default-up": 6.0125e-07,
    "C1-1x193-x8-down": 2.9447e-06,
    "C1-1x193-x8-up": 2.6717e-05,
    "C1-1x193-zero_layer-down": 8.4215e-08,
    "C1-1x193-zero_layer-up": 5.5256e-07,
    "C1-70x70-default-down": 1.2421e-07,
    "C1-70x70-default-up": 7.1563e-07,
    "C1-70x70-x8-down": 4.5037e-06,
    "C1-70x70-x8-up": 3.8674e-05,
    "C1-70x70-zero_layer-down": 1.2226e-07,
    "C1-70x70-zero_layer-up": 6.5526e-07,
    "C3-9x21-default-down": 1.3790e-07,
    "C3-9x21-default-up": 5.8778e-07,
    "C3-9x21-x8-down": 5.4832e-06,
    "C3-9x21-x8-up": 3.0310e-05,
    "C3-9x21-zero_layer-down": 1.3790e-07,
    "C3-9x21-zero_layer-up": 5.8778e-07,
    "C3-1x193-default-down": 1.0884e-07,
    "C3-1x193-default-up": 6.4186e-07,
    "C3-1x193-x8-down": 4.9422e-06,
    "C3-1x193-x8-up": 3.7121e-05,
    "C3-1x193-zero_layer-down": 1.0884e-07,
    "C3-1x193-zero_layer-up": 6.4186e-07,
    "C3-70x70-default-down": 1.4616e-07,
    "C3-70x70-default-up": 8.5575e-07,
    "C3-70x70-x8-down": 6.8731e-06,
    "C3-70x70-x8-up": 4.5374e-05,
    "C3-70x70-zero_layer-down": 1.3538e-07,
    "C3-70x70-zero_layer-up": 8.5575e-07,
}


def case_id(case):
    C, (h, w), wk, tr = case
    return "C%d-%dx%d-%s-%s" % (C, h, w, wk, "up" if tr else "down")


def _ops():
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    return ops


_memo = {}


def weights_of(C, wk, transposed):
    """Stacked (P, ...) host weights w0, b0, w1, b1, w2, b2, w3, b3 of P default-initialised SubbandAutoEncoders."""
    key = (C, wk, transposed)
    if key not in _memo:
        from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.layers.lifting_dwt_nets import \
            SubbandAutoEncoder
        torch.manual_seed(1000 + C)
        aes = [SubbandAutoEncoder(in_ch=C) for _ in range(P)]
        seqs = [(a.ae_up if transposed else a.ae_down) for a in aes]
        ws = []
        for n in (0, 2, 4, 6):
            ws.append(torch.stack([s[n].weight.detach() for s in seqs], 0).flatten(1).contiguous().clone())
            ws.append(torch.stack([s[n].bias.detach() for s in seqs], 0).contiguous().clone())
        if wk == "x8":
            for i in (0, 2, 4, 6):
                ws[i] *= 8.0
        if wk == "zero_layer":                      # (plane 1, channel 0): an all-zero 32 x 32 first hidden layer
            ws[2].view(P, C, H, H)[1, 0] = 0.0
        _memo[key] = ws
    return _memo[key]


def input_of(C, hw):
    key = ("x", C, hw)
    if key not in _memo:
        h, w = hw
        g = torch.Generator().manual_seed(7 + C + h)
        x = (torch.rand(P, B, C, h, w, generator=g) - 0.5) * 4
        flat = x.view(P, B, C, -1)
        flat[:, :, :, 0] = 0.0
        flat[:, 0, :, 5] = 1e4
        flat[:, 1, :, -1] = -1e4                    # the last coefficient of an image: the tail of a partial block
        flat[:, 2, :, h * w // 2] = 1e4
        _memo[key] = x
    return _memo[key]


def reference64(x, ws, transposed):
    """float64 on the host, written from the layer definition (grouped 1x1 convs, tanh between)."""
    key = ("ref", id(x), id(ws[0]))
    if key not in _memo:
        w0, b0, w1, b1, w2, b2, w3, b3 = [t.double() for t in ws]
        Pn, Bn, C = x.shape[:3]
        v = x.double().reshape(Pn, Bn, C, 1, -1)
        hcur = torch.tanh(w0.view(Pn, 1, C, H, 1) * v + b0.view(Pn, 1, C, H, 1))
        for wl, bl in ((w1, b1), (w2, b2)):
            W = wl.view(Pn, C, H, H)
            if transposed:                          # ConvTranspose2d keeps (in, out / groups)
                W = W.transpose(-1, -2)
            hcur = torch.tanh(torch.einsum("pcok,pbcki->pbcoi", W, hcur) + bl.view(Pn, 1, C, H, 1))
        y = torch.einsum("pck,pbcki->pbci", w3.view(Pn, C, H), hcur) + b3.view(Pn, 1, C, 1)
        _memo[key] = y.reshape(x.shape)
    return _memo[key]


def run_case(case):
    """-> (y on the host, max|y - float64|)."""
    C, hw, wk, tr = case
    ops = _ops()
    ws, x = weights_of(C, wk, tr), input_of(C, hw)
    y = ops.subband_mlp(x.cuda(), *[t.cuda() for t in ws], transposed=tr).cpu()
    return y, float((y.double() - reference64(x, ws, tr)).abs().max())


def measure_errors():
    """{case id: max error} of whatever kernel ops.subband_mlp runs (how OLD_ERR was taken at the parent commit)."""
    return {case_id(c): run_case(c)[1] for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_within_twice_the_fp32_kernel(case):
    y, err = run_case(case)
    old = OLD_ERR[case_id(case)]
    print("%s: max|y - float64| = %.3e, fp32 kernel %.3e, ratio %.2f" % (case_id(case), err, old, err / old))
    assert bool(torch.isfinite(y).all())
    assert err <= 2.0 * old


def _pack_reference(ws, transposed):
    """The pack's layout in numpy (include/lldwt.h, csrc/subband_mlp_f16.hip) -> uint32 words (P * C, 2216)."""
    w0, b0, w1, b1, w2, b2, w3, b3 = [t.numpy() for t in ws]
    pairs = b3.size
    lane = np.arange(64)
    col, kk = lane & 15, lane >> 4
    j = np.arange(8)
    chan = (j[None, :] >> 2) * 16 + 4 * kk[:, None] + (j[None, :] & 3)              # (lane, j)
    out = np.zeros((pairs, 2216), np.uint32)
    for pc in range(pairs):
        frags, scales = [], []
        for wl in (w1, w2):
            W = wl.reshape(pairs, H, H)[pc]
            if transposed:
                W = W.T                                                              # W[oc][ic]
            amax = float(np.abs(W).max())
            k = 0
            if 0.0 < amax < 3.0e38:
                k = min(max(15 - int(np.frexp(np.float32(amax))[1]), -113), 112)
            s = np.float32(2.0 ** k)
            scales.append(s)
            for m in range(2):
                v = (W[(m * 16 + col)[:, None], chan] * s).astype(np.float32)
                hi = v.astype(np.float16)
                lo = (v - hi.astype(np.float32)).astype(np.float16)
                frags += [hi, lo]
        out[pc, :2048] = np.stack(frags).reshape(-1).view(np.uint32)
        ch4 = (j[None, :] >> 2) * 16 + 4 * np.arange(4)[:, None] + (j[None, :] & 3)  # (kk, j)
        vecs = [a.reshape(pairs, H)[pc][ch4] for a in (w0, b0, b1, b2, w3)]
        out[pc, 2048:2208] = np.stack(vecs).astype(np.float32).reshape(-1).view(np.uint32)
        tail = np.array([scales[0], scales[1], 1.0 / (scales[0] * 16384.0), 1.0 / (scales[1] * 16384.0),
                         b3.reshape(-1)[pc], 0, 0, 0], np.float32)
        out[pc, 2208:] = tail.view(np.uint32)
    return out


@pytest.mark.parametrize("transposed", [False, True], ids=["down", "up"])
@pytest.mark.parametrize("wk", ["default", "zero_layer"])
def test_pack_layout_bit_equal(wk, transposed):
    ops = _ops()
    C = 3
    ws = [t.clone() for t in weights_of(C, wk, transposed)]
    ws[4].view(P, C, H, H)[0, 1] *= 2.0 ** -20          # one small layer: it gets its own scale
    ws[2].view(P, C, H, H)[0, 0, :4] *= 2.0 ** -14      # weights far below their layer's maximum: subnormal fp16 low halves
    ws[4].view(P, C, H, H)[0, 2, 3, 5] = float("inf")   # a non-finite weight: scale 1, no NaN scale
    pack = ops.subband_mlp_pack(*[t.cuda() for t in ws], transposed=transposed)
    got = pack.cpu().numpy().view(np.uint32).reshape(P * C, 2216)
    with np.errstate(over="ignore", invalid="ignore"):
        want = _pack_reference(ws, transposed)
    assert np.isfinite(got[:, 2208:2213].view(np.float32)).all()
    assert got[2, 2209:2210].view(np.float32)[0] == 1.0 and (want[:, 2209].view(np.float32)[2] == 1.0)
    halves = want[:, :2048].copy().view(np.float16).reshape(P * C, 2048, 2)
    nan_word = np.isnan(halves).any(-1)                 # inf - inf in the low half of the inf weight: a NaN of any payload
    assert nan_word.sum() == 1 and np.isnan(got[:, :2048].copy().view(np.float16).reshape(P * C, 2048, 2)[nan_word]).any()
    same = got == want
    same[:, :2048] |= nan_word
    assert same.all(), [tuple(i) for i in np.argwhere(~same)[:8]]


def test_deterministic_and_images_never_mix():
    ops = _ops()
    C, hw = 3, (70, 70)
    ws = [t.cuda() for t in weights_of(C, "default", False)]
    x = input_of(C, hw).cuda()
    y = ops.subband_mlp(x, *ws)
    assert torch.equal(y, ops.subband_mlp(x, *ws))
    for b in range(B):
        assert torch.equal(y[:, b:b + 1], ops.subband_mlp(x[:, b:b + 1].contiguous(), *ws))


def test_cached_pack_follows_the_parameters():
    """ae_planes keeps the pack on the module: an optimizer-style in-place update must rebuild it."""
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.layers.lifting_dwt_nets import (
        SubbandAutoEncoder, ae_planes)
    torch.manual_seed(5)
    aes = [SubbandAutoEncoder(in_ch=3).cuda() for _ in range(P)]
    x = input_of(3, (9, 21)).cuda()
    with torch.no_grad():
        for decode in (False, True):
            y0 = ae_planes(aes, x, decode)
            assert torch.equal(y0, ae_planes(aes, x, decode))
            seq = aes[1].ae_up if decode else aes[1].ae_down
            seq[2].weight.mul_(1.5)
            y1 = ae_planes(aes, x, decode)
            ws = [torch.stack([getattr((a.ae_up if decode else a.ae_down)[n], k).detach() for a in aes], 0)
                  for n in (0, 2, 4, 6) for k in ("weight", "bias")]
            ws = [t.flatten(1).contiguous() if i % 2 == 0 else t.contiguous() for i, t in enumerate(ws)]
            assert torch.equal(y1, ops_direct(x, ws, decode))
            assert not torch.equal(y0[1], y1[1]) and torch.equal(y0[0], y1[0])


def ops_direct(x, ws, transposed):
    return _ops().subband_mlp(x, *ws, transposed=transposed)
