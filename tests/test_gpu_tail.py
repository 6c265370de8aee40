"""GPU: the end-of-step "tail" (the coarsest level's two context stacks in one launch per layer, the vectorised sum kernel)
against the launches it replaces, which LLDWT_TAIL=legacy keeps.

The switch is read when the library loads, so each leg runs in a fresh child process (this file, run as a script) on the same
seeded weights and input and writes its tensors to a file; the parent process compares them.

Bound on the rate tensors: none is needed -- equality.  A workgroup of the pair launch computes one group's outputs with the
plan, chunk order and fp32 MFMA chain of the single launch, so si_xe and si_xo[L-1] are the same bits (measured on MI355X at
both sizes below and on bench.py's 8x3x512x512 dump against the parent commit: max |diff| = 0 for every array).  The lifting
kernels are not reached by the switch today, so that half of the comparison cannot fail yet; it stays as
the guard for the day LLDWT_TAIL selects a lifting schedule: their outputs are compared at a size where every launch is under-filled and every tile
a border tile (2x3x128x128, L=4) and at 1x3x512x512.  Each leg counts its ops.conv_stack_pair calls, so a default leg that
quietly stopped taking the pair launch fails; the launch itself is pinned against ops.conv2d layer by layer.

ops.sum_into accumulates in float64; its order of summation differs from torch's, each of the n additions rounds at 2^-53
relative, and the terms are non-negative, so 1e-12 relative leaves three orders of magnitude at n = 4 718 592.
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(2, 128, 128), (1, 512, 512)]
LEVELS = 4


def _leg(out_path, B, H, W):
    """One leg, in its own process: encode + entropy-model forward of seeded weights and input -> out_path."""
    sys.path.insert(0, REPO)
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.layers.lifting_dwt_nets import encode_planes
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
        LiftingBasedDWTNetWrapper
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
    cfg = make_config(dwtlevels=LEVELS, mode="validate")
    torch.manual_seed(1337)
    net = LiftingBasedDWTNetWrapper(cfg).to(DEV).eval()
    nets = net.nets()
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(7)).to(DEV)
    calls = {"pair": 0}
    pair = ops.conv_stack_pair

    def counted(*a, **kw):
        calls["pair"] += 1
        return pair(*a, **kw)
    ops.conv_stack_pair = counted        # the model calls it through the module attribute
    with torch.no_grad():
        y = ops.rgb_to_ycc(x)
        out_xe, out_xo = encode_planes([n.autoencoder for n in nets], y)
        em = [n.entropymodel for n in nets]
        # x 8: the coefficients of the initial weights are < 1 and would all quantise to 0 / +-1
        gxe, gxo = (out_xe * 8.0).contiguous(), [(t * 8.0).contiguous() for t in out_xo]
        si_xe, si_xo, xe_q, xo_q = type(em[0]).forward_planes(em, gxe, gxo, False)
    torch.cuda.synchronize()
    torch.save({"mode": ops.tail_mode(), "pair_calls": calls["pair"], "out_xe": out_xe.cpu(), "out_xo": [t.cpu() for t in out_xo], "si_xe": si_xe.cpu(),
                "si_xo": [t.cpu() for t in si_xo], "xe_q": xe_q.cpu(), "xo_q": [t.cpu() for t in xo_q]}, out_path)


def _run_leg(tmp_path, name, tail, B, H, W):
    out = str(tmp_path / ("%s.pt" % name))
    env = dict(os.environ)
    env.pop("LLDWT_TAIL", None)
    if tail:
        env["LLDWT_TAIL"] = tail
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out, str(B), str(H), str(W)], env=env, cwd=REPO,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "leg %s failed (rc=%d):\n%s" % (name, r.returncode, r.stderr[-3000:])
    return torch.load(out)


@pytest.mark.parametrize("B,H,W", CASES)
def test_tail_equals_legacy(tmp_path, B, H, W):
    new = _run_leg(tmp_path, "fused", None, B, H, W)
    old = _run_leg(tmp_path, "legacy", "legacy", B, H, W)
    assert new["mode"] == "fused" and old["mode"] == "legacy"
    # the default leg really took the pair launch (one call for both stacks), the legacy leg never
    assert new["pair_calls"] == 1 and old["pair_calls"] == 0
    # lifting outputs: same bits
    assert torch.equal(new["out_xe"], old["out_xe"])
    assert len(new["out_xo"]) == LEVELS
    for a, b in zip(new["out_xo"], old["out_xo"]):
        assert torch.equal(a, b)
    # quantised tensors and rates: same bits (see the module docstring); print the figure before asserting it
    pairs = [("si_xe", new["si_xe"], old["si_xe"]), ("xe_q", new["xe_q"], old["xe_q"])]
    pairs += [("si_xo_%d" % i, a, b) for i, (a, b) in enumerate(zip(new["si_xo"], old["si_xo"]))]
    pairs += [("xo_q_%d" % i, a, b) for i, (a, b) in enumerate(zip(new["xo_q"], old["xo_q"]))]
    for name, a, b in pairs:
        print("%dx3x%dx%d %s: max |fused - legacy| = %.3g, sum %.6f" % (B, H, W, name, float((a - b).abs().max()),
                                                                       float(a.double().sum())))
    assert float(new["si_xe"].sum()) > 0 and float(new["si_xo"][LEVELS - 1].sum()) > 0
    for name, a, b in pairs:
        assert torch.equal(a, b), name


@pytest.mark.parametrize("ga,gb", [(3, 1), (1, 3)])
def test_conv_stack_pair_equals_conv2d_layer_by_layer(ga, gb):
    """ops.conv_stack_pair against ops.conv2d run layer by layer on each stack alone: same bits.  Odd image size (ragged tiles),
    per-group widths 1 -> 9 -> 27 -> 2 (a first layer narrower than a chunk, partial last chunks of 9 = 8 + 1 and 27 = 24 + 3
    input channels), masked taps (type A then type B), two planes with different weights, either stack as the larger one."""
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    P, B, h, w = 2, 2, 13, 19
    widths = [1, 9, 27, 2]
    masks = [0b000001111, 0b000011111, 0b000011111]
    gen = torch.Generator().manual_seed(100 * ga + gb)
    rnd = lambda *shape: (torch.rand(*shape, generator=gen) - 0.5).to(DEV)
    xs = {g: (rnd(P, B, g * widths[0], h, w) * 8.0).round().contiguous() for g in (ga, gb)}
    ws = {g: [rnd(P, g * widths[i + 1], widths[i], 3, 3) for i in range(3)] for g in (ga, gb)}
    bs = {g: [rnd(P, g * widths[i + 1]) for i in range(3)] for g in (ga, gb)}
    ref = {}
    for g in (ga, gb):
        t = xs[g]
        for i in range(3):
            t = ops.conv2d(t, ws[g][i], bs[g][i], 3, groups=g, act=ops.ACT_NONE if i == 2 else ops.ACT_LRELU, tap_mask=masks[i])
        ref[g] = t
    layers = []
    for i in range(3):
        pa = ops.conv_pack(ws[ga][i], 3, ga, tap_mask=masks[i])
        pb = ops.conv_pack(ws[gb][i], 3, gb, tap_mask=masks[i])
        layers.append((torch.cat([pa, pb], 1).contiguous(), torch.cat([bs[ga][i], bs[gb][i]], 1).contiguous(),
                       (ga + gb) * widths[i], (ga + gb) * widths[i + 1], 3, ops.ACT_NONE if i == 2 else ops.ACT_LRELU, masks[i]))
    ya, yb = ops.conv_stack_pair(xs[ga], xs[gb], layers, ga, gb)
    torch.cuda.synchronize()
    assert ya.shape == ref[ga].shape and yb.shape == ref[gb].shape
    assert float(ref[ga].abs().max()) > 0 and float(ref[gb].abs().max()) > 0
    print("pair (%d, %d): max |ya - ref| = %.3g, max |yb - ref| = %.3g" % (ga, gb, float((ya - ref[ga]).abs().max()),
                                                                          float((yb - ref[gb]).abs().max())))
    assert torch.equal(ya, ref[ga]) and torch.equal(yb, ref[gb])


@pytest.mark.parametrize("n", [1, 3, 1000, 1023, 4718592])
def test_sum_into_vs_float64(n):
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    x = (torch.rand(n, generator=torch.Generator().manual_seed(n)) * 12.0).to(DEV)
    acc = torch.full((1,), 5.0, dtype=torch.float64, device=DEV)         # sum_into ADDS to the accumulator
    ops.sum_into(x, acc)
    ref = float(x.double().sum()) + 5.0
    got = float(acc)
    print("sum_into n=%d: got %.15g ref %.15g rel %.3g" % (n, got, ref, abs(got - ref) / ref))
    assert abs(got - ref) <= 1e-12 * ref


def test_sum_into_unaligned_view():
    """A tensor that does not start on a 16-byte boundary takes the scalar kernel: same sum."""
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    base = (torch.rand(4099, generator=torch.Generator().manual_seed(3)) * 12.0).to(DEV)
    x = base[1:]
    assert x.data_ptr() % 16 != 0 and x.is_contiguous()
    acc = torch.zeros(1, dtype=torch.float64, device=DEV)
    ops.sum_into(x, acc)
    ref = float(x.double().sum())
    assert abs(float(acc) - ref) <= 1e-12 * ref


if __name__ == "__main__":
    _leg(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
