"""Kernel times of variable-rate coding on HIP events: lldwt_gauss_quantise and lldwt_code_cost at the
level-0 shape of the BASELINE batch (8 x 3 x 512 x 512: 3 planes x 8 images x 3 subbands of 256 x 256).

    python tools/bench_quant.py [--batch 8] [--size 512] [--reps 200] [--rdo 0.203125]

Per kernel: the median (minimum - maximum) of --reps event-timed launches after a warm-up, and the achieved bytes/s with the
bytes computed from the shapes: per coefficient the encoder reads sigma, mu and y and writes index, symbol and value
(24 bytes), the decoder's two launches move 12 (sigma, mu -> index) and 20 (sigma, mu, symbol -> index, value), and the
cost kernel reads a symbol and an index (8 bytes; its tables stay in cache).  ``pad`` is lldwt_u8hwc_to_ycc_pad on the same
batch in the same process, the copy kernel the other sections of DESIGN.md use as their yardstick.  The ``rdo`` row is the
encoder with rate-distortion optimised quantisation (lldwt_gauss_quantise_rdo): the same 24 bytes per
coefficient plus two table lookups that stay in cache; the line after it gives what the choice does to the ideal code length."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops  # noqa: E402
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.entropy_models import GaussianConditional  # noqa: E402
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models import entropy_coding as ec  # noqa: E402
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
    ap.add_argument("--step", type=float, default=2.5)
    ap.add_argument("--rdo", type=float, default=13 / 64)
    a = ap.parse_args()
    P, B, G, S = 3, a.batch, 3, a.size // 2
    g = torch.Generator().manual_seed(0)
    params = torch.empty(P, B, 2 * G, S, S)
    params[:, :, 0::2] = torch.exp(torch.rand(P, B, G, S, S, generator=g) * 6 - 3)
    params[:, :, 1::2] = torch.rand(P, B, G, S, S, generator=g) - 0.5
    params = params.to(DEV)
    y = ((torch.rand(P, B, G, S, S, generator=g) - 0.5) * 60).to(DEV)
    table = torch.as_tensor(get_scale_table()).float()[:63].contiguous().to(DEV)
    n = P * B * G * S * S
    level = torch.empty_like(y)
    # the per-call empty() of the wrapper's outputs is part of what a coder pays; it does not synchronise
    report("gauss_quantise encode, full grid", timed(lambda: ops.gauss_quantise(params, table, level, 0, 0, 1, a.step, y=y), a.reps), 24 * n)
    idx, sym = ops.gauss_quantise(params, table, level, 0, 0, 1, a.step, y=y)
    report("gauss_quantise indexes only", timed(lambda: ops.gauss_quantise(params, table, None, 0, 0, 1, a.step), a.reps), 12 * n)
    report("gauss_quantise decode, full grid", timed(lambda: ops.gauss_quantise(params, table, level, 0, 0, 1, a.step, sym=sym), a.reps), 20 * n)
    # a ZTBlock phase of the same level: a quarter of the coefficients, level addressed at stride 2
    ph = params[..., :S // 2, :S // 2].contiguous()
    report("gauss_quantise encode, one phase", timed(lambda: ops.gauss_quantise(ph, table, level, 1, 1, 2, a.step, y=y), a.reps), 24 * n // 4)
    em = GaussianConditional(None)
    tabs = ec._Tables(em, get_scale_table())
    ct = ec.device_cost_tables(tabs, torch.device(DEV))
    s2, i2 = sym.reshape(P * B, -1).contiguous(), idx.reshape(P * B, -1).contiguous()
    report("code_cost, %d streams" % (P * B), timed(lambda: ops.code_cost(s2, i2, *ct), a.reps), 8 * n)
    sums, esc = ops.code_cost(s2, i2, *ct)
    ra = (ops.rdo_scale(a.rdo),) + tuple(ct)
    report("gauss_quantise rdo encode, full grid", timed(lambda: ops.gauss_quantise(params, table, level, 0, 0, 1, a.step, y=y, rdo=ra), a.reps), 24 * n)
    _, symr = ops.gauss_quantise(params, table, level, 0, 0, 1, a.step, y=y, rdo=ra)
    sumr, _ = ops.code_cost(symr.reshape(P * B, -1).contiguous(), i2, *ct)
    print("rdo %g: %.2f %% of the symbols moved, ideal code length %.0f -> %.0f bytes (%.2f %% saved)"
          % (a.rdo, 100.0 * float((symr != sym).float().mean()), int(sums.sum()) / ops.COST_ONE_BIT / 8,
             int(sumr.sum()) / ops.COST_ONE_BIT / 8, 100.0 * (1 - int(sumr.sum()) / int(sums.sum()))))
    bits, e = ec.ideal_bits(s2[0].cpu().numpy(), i2[0].cpu().numpy(), tabs)
    print("stream 0: %.1f bits + %d escapes (numpy: %.1f bits, %d escapes)" % ((int(sums[0]) - int(esc[0]) * ops.COST_ESCAPE)
                                                                               / ops.COST_ONE_BIT, int(esc[0]), bits, e))
    img = torch.randint(0, 256, (B, a.size, a.size, 3), dtype=torch.uint8, generator=g).to(DEV)
    report("pad (u8hwc_to_ycc_pad)", timed(lambda: ops.u8hwc_to_ycc_pad(img, a.size, a.size), a.reps), 15 * B * a.size * a.size)


if __name__ == "__main__":
    main()
