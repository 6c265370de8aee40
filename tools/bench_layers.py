"""Kernel times of the quality layers on HIP events: lldwt_layer_encode, lldwt_layer_rows and
lldwt_layer_apply alone, at the level-0 shape of the BASELINE batch (8 x 3 x 512 x 512: 3 planes x 8 images x 3 subbands of
256 x 256), next to lldwt_gauss_quantise at the same shape in the same run.

    python tools/bench_layers.py [--batch 8] [--size 512] [--reps 200] [--step 3] [--layer 1]

Per kernel: the median (minimum - maximum) of --reps event-timed launches after a warm-up, and the achieved bytes/s with the
bytes computed from the shapes.  Per coefficient the layer encoder reads y, v, sigma and mu and writes symbol, row and value
(28 bytes); the decoder's first half reads v, sigma, mu and writes row and sign (20), its second reads v, symbol and sign and
writes the value (16).  The quantiser's encoder moves 24 bytes per coefficient, its two decoder launches 12 and 20
(tools/bench_quant.py).  The timed calls include the wrappers' allocation of their outputs, as a coder pays it."""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops, quality_layers  # noqa: E402
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import get_scale_table  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps, warm=20):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def report(name, ms, nbytes):
    med = statistics.median(ms)
    print("%-34s %8.1f us (%.1f - %.1f)  %7.1f MB  %6.2f TB/s" % (name, med * 1e3, min(ms) * 1e3, max(ms) * 1e3, nbytes / 1e6,
                                                                  nbytes / (med * 1e-3) / 1e12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step", type=float, default=3.0)
    ap.add_argument("--layer", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_layers: no GPU; kernel times are measured on the device or not at all")
    P, B, G, S = 3, a.batch, 3, a.size // 2
    n16 = int(round(a.step * ops.STEP_DENOM))
    prev, cur = ops.layer_pair(n16, a.layer - 1), ops.layer_pair(n16, a.layer)
    g = torch.Generator().manual_seed(0)
    params = torch.empty(P, B, 2 * G, S, S)
    params[:, :, 0::2] = torch.exp(torch.rand(P, B, G, S, S, generator=g) * 6 - 3)
    params[:, :, 1::2] = torch.rand(P, B, G, S, S, generator=g) - 0.5
    params = params.to(DEV)
    y = ((torch.rand(P, B, G, S, S, generator=g) - 0.5) * 60).to(DEV)
    table = torch.as_tensor(get_scale_table()).float()[:63].contiguous().to(DEV)
    n = P * B * G * S * S
    K = quality_layers.K
    # the base: the quantiser at the previous step, whose values the layer refines
    v = torch.empty_like(y)
    report("gauss_quantise encode, full grid", timed(lambda: ops.gauss_quantise(params, table, v, 0, 0, 1, a.step, y=y), a.reps), 24 * n)
    idx, sym0 = ops.gauss_quantise(params, table, v, 0, 0, 1, a.step, y=y)
    report("gauss_quantise indexes only", timed(lambda: ops.gauss_quantise(params, table, None, 0, 0, 1, a.step), a.reps), 12 * n)
    report("gauss_quantise decode, full grid", timed(lambda: ops.gauss_quantise(params, table, v, 0, 0, 1, a.step, sym=sym0), a.reps), 20 * n)
    vj = v
    for j in range(1, a.layer):                                    # bring v to the step before the timed layer
        _, _, vj = ops.layer_encode(y, vj, params, table, ops.layer_pair(n16, j - 1), ops.layer_pair(n16, j), K)
    report("layer_encode", timed(lambda: ops.layer_encode(y, vj, params, table, prev, cur, K), a.reps), 28 * n)
    sym, row, out = ops.layer_encode(y, vj, params, table, prev, cur, K)
    report("layer_rows", timed(lambda: ops.layer_rows(vj, params, table, prev, K), a.reps), 20 * n)
    row2, sign = ops.layer_rows(vj, params, table, prev, K)
    report("layer_apply", timed(lambda: ops.layer_apply(vj, sym, sign, cur), a.reps), 16 * n)
    assert torch.equal(row, row2) and torch.equal(ops.layer_apply(vj, sym, sign, cur), out)
    share = [float((sym == t).float().mean()) for t in (-1, 0, 1)]
    print("layer %d over step %g: coded symbols -1 / 0 / +1: %.1f / %.1f / %.1f %%" % (a.layer, a.step, *[100 * s for s in share]))


if __name__ == "__main__":
    main()
