"""Times MS-SSIM on the fused HIP kernels (csrc/msssim.hip) against the same formula composed from ATen grouped convolutions
with torch autograd -- the code one would otherwise have written.

    python tools/bench_msssim.py [--iters 30] [--warmup 5] [--json out.json]

Shapes: 8 x 3 x 256 x 256 (the training patch) and 8 x 3 x 512 x 512.  Device events, median after a warm-up; the fused path and
the composition are timed alternately in one process.  Per scale: a one-scale call at that scale's size (memset + the scale's
kernel + finalize).  Bytes are counted from the shapes (what the algorithm has to move, fp32): the forward reads x and y of every
scale and writes the pooled pair of the next; the backward reads x, y and the coarser gradient and writes the gradient.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import autograd as ag  # noqa: E402
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 8e12
WEIGHTS = ops.MS_SSIM_WEIGHTS


def aten_ms_ssim(x, y, offset=0.5, scales=5):
    """The composition: grouped conv2d with the separable window, avg_pool2d, relu, prod (fp32, on the device)."""
    g = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5) ** 2 / 4.5)
    g = (g / g.sum()).to(x)
    c = x.shape[1]
    gv, gh = g.view(1, 1, 11, 1).expand(c, 1, 11, 1), g.view(1, 1, 1, 11).expand(c, 1, 1, 11)
    filt = lambda t: F.conv2d(F.conv2d(t, gv, groups=c), gh, groups=c)
    X, Y = x + offset, y + offset
    vs = []
    for s in range(scales):
        mx, my = filt(X), filt(Y)
        sxx, syy, sxy = filt(X * X) - mx * mx, filt(Y * Y) - my * my, filt(X * Y) - mx * my
        cs = (2 * sxy + 9e-4) / (sxx + syy + 9e-4)
        if s < scales - 1:
            vs.append(torch.relu(cs.mean((2, 3))))
            pad = (X.shape[2] % 2, X.shape[3] % 2)
            X, Y = F.avg_pool2d(X, 2, padding=pad), F.avg_pool2d(Y, 2, padding=pad)
        else:
            vs.append(torch.relu(((2 * mx * my + 1e-4) / (mx * mx + my * my + 1e-4) * cs).mean((2, 3))))
    w = torch.tensor(WEIGHTS[:scales], device=x.device, dtype=x.dtype).view(-1, 1, 1)
    return torch.prod(torch.stack(vs, 0) ** w, 0)


def sizes(H, W, scales=5):
    out = [(H, W)]
    for _ in range(scales - 1):
        H, W = H // 2 + H % 2, W // 2 + W % 2
        out.append((H, W))
    return out


def traffic_bytes(planes, H, W, scales=5):
    sz = sizes(H, W, scales)
    fwd = sum(2 * h * w for h, w in sz) + sum(2 * h * w for h, w in sz[1:])            # reads of x, y + pooled writes
    fwd += sum(2 * h * w for h, w in sz[:-1])                                          # the pool kernel reads its scale again
    bwd = sum(3 * h * w for h, w in sz) + sum(h * w for h, w in sz[1:])                # x, y, grad out + coarser grad in
    return 4 * planes * fwd, 4 * planes * bwd


def timed(fn, iters, warmup):
    """-> list of per-call milliseconds (device events)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_msssim: no GPU")
    results = []
    for B, H in ((8, 256), (8, 512)):
        gen = torch.Generator(device=DEV).manual_seed(1)
        x = torch.rand(B, 3, H, H, device=DEV, generator=gen) - 0.5
        y = (x + 0.05 * torch.randn(x.shape, device=DEV, generator=gen)).clamp(-0.5, 0.5)
        yg = y.clone().requires_grad_(True)

        def fused_fwd():
            return ops.ms_ssim(x, y)

        def fused_fb():
            yg.grad = None
            ag.MsSsimFn.apply(x, yg).backward()

        def aten_fwd():
            with torch.no_grad():
                return aten_ms_ssim(x, y)

        def aten_fb():
            yg.grad = None
            aten_ms_ssim(x, yg).mean().backward()

        fused_fb()
        g_fused = yg.grad.clone()
        aten_fb()
        agree = dict(value=(fused_fwd().float() - aten_fwd()).abs().max().item(),
                     grad_rel=((g_fused - yg.grad).abs().max() / yg.grad.abs().max()).item())
        t = {k: [] for k in ("fused_fwd", "aten_fwd", "fused_fwd_bwd", "aten_fwd_bwd")}
        for _ in range(3):                                                             # alternate the two in one process
            t["fused_fwd"] += timed(fused_fwd, a.iters, a.warmup)
            t["aten_fwd"] += timed(aten_fwd, a.iters, a.warmup)
            t["fused_fwd_bwd"] += timed(fused_fb, a.iters, a.warmup)
            t["aten_fwd_bwd"] += timed(aten_fb, a.iters, a.warmup)
        per_scale = []
        for h, w in sizes(H, H):
            xs, ys = torch.rand(B, 3, h, w, device=DEV) - 0.5, torch.rand(B, 3, h, w, device=DEV) - 0.5
            per_scale.append(statistics.median(timed(lambda: ops.ms_ssim(xs, ys, scales=1), a.iters, a.warmup)))
        fb, bb = traffic_bytes(B * 3, H, H)
        med = {k: statistics.median(v) for k, v in t.items()}
        res = dict(shape=[B, 3, H, H], ms=med, per_scale_fwd_ms=per_scale, bytes_fwd=fb, bytes_bwd=bb,
                   hbm_fraction_fwd=fb / (med["fused_fwd"] * 1e-3) / HBM_BYTES_PER_S,
                   hbm_fraction_fwd_bwd=(fb + bb) / (med["fused_fwd_bwd"] * 1e-3) / HBM_BYTES_PER_S,
                   speedup_fwd=med["aten_fwd"] / med["fused_fwd"], speedup_fwd_bwd=med["aten_fwd_bwd"] / med["fused_fwd_bwd"],
                   agreement_with_aten_fp32=agree)
        results.append(res)
        print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
