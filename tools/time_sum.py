#!/usr/bin/env python
"""k_sum (ops.sum_into) timed the way bench.py's roofline_hbm block times k_rgb_to_ycc and k_gauss_rate: HIP-graph replay of 20
back-to-back calls, fraction of the 8 TB/s HBM peak.  Sizes: the four rate tensors bench.py's default step sums
(8x3x512x512, L=4; the largest is 3 x 8 x 3 x 256 x 256 floats = 19 MB).  The input is read once (4 B/element).  Prints one JSON
line; run it once plain and once with LLDWT_TAIL=legacy (the switch is read when the library loads).
    python tools/time_sum.py"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import bench
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    dev = torch.device("cuda", 0)
    acc = torch.zeros(1, dtype=torch.float64, device=dev)

    def timeit(fn, iters=20):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(iters):
                fn()
        g.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (3 * iters) * 1e-3
    rows = []
    for s in (256, 128, 64, 32):
        x = torch.rand(3, 8, 3, s, s, device=dev)
        t = timeit(lambda: ops.sum_into(x, acc))
        nbytes = x.numel() * 4
        rows.append({"elements": x.numel(), "bytes": nbytes, "us": t * 1e6, "GB/s": nbytes / t / 1e9,
                     "frac": nbytes / t / 1e9 / bench.HBM_PEAK_GBS})
    # the yardstick: the two streaming kernels of bench.py's roofline_hbm block, at batch 8
    x = torch.rand(8, 3, 512, 512, device=dev)
    t = timeit(lambda: ops.rgb_to_ycc(x))
    ref = {"k_rgb_to_ycc": {"us": t * 1e6, "frac": 2 * x.numel() * 4 / t / 1e9 / bench.HBM_PEAK_GBS}}
    cf = torch.randn(3, 8, 3, 256, 256, device=dev) * 3
    prm = torch.rand(3, 8, 6, 256, 256, device=dev) * 2
    t = timeit(lambda: ops.gauss_rate(cf, prm))
    ref["k_gauss_rate"] = {"us": t * 1e6, "frac": cf.numel() * 16 / t / 1e9 / bench.HBM_PEAK_GBS}
    # the yardstick kernel at the SAME traffic as the 19 MB sum (9.4 MB read + 9.4 MB written): what a streaming kernel of this
    # repo reaches when the launch moves 19 MB only (approximate: half of that traffic is written, the sum only reads)
    xs = torch.rand(1, 3, 768, 1024, device=dev)
    t = timeit(lambda: ops.rgb_to_ycc(xs))
    ref["k_rgb_to_ycc at 19 MB of traffic"] = {"us": t * 1e6, "frac": 2 * xs.numel() * 4 / t / 1e9 / bench.HBM_PEAK_GBS}
    print(json.dumps({"tail": ops.tail_mode(), "peak_GB/s": bench.HBM_PEAK_GBS, "k_sum": rows, "yardstick": ref}))


if __name__ == "__main__":
    main()
