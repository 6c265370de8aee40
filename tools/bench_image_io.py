"""Times the image codec's I/O kernels (lldwt_u8hwc_to_ycc_pad, lldwt_ycc_to_u8hwc_crop) with HIP events and prints one JSON
line of GB/s (bytes read + written once).  Default 8 x 2048 x 2048, padded by 16 rows / columns."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops  # noqa: E402


def timeit(fn, iters):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--pad", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    B, H = a.batch, a.size
    Hp = H + a.pad
    img = torch.randint(0, 256, (B, H, H, 3), dtype=torch.uint8, device="cuda:0")
    y = ops.u8hwc_to_ycc_pad(img, Hp, Hp)
    t_in = timeit(lambda: ops.u8hwc_to_ycc_pad(img, Hp, Hp), a.iters)
    t_out = timeit(lambda: ops.ycc_to_u8hwc_crop(y, H, H), a.iters)
    bytes_in = B * H * H * 3 + 3 * B * Hp * Hp * 4
    bytes_out = 3 * B * H * H * 4 + B * H * H * 3          # the crop reads the H x W of each plane it writes
    print(json.dumps({"shape": [B, H, H, 3], "padded": [Hp, Hp],
                      "u8hwc_to_ycc_pad": {"ms": t_in * 1e3, "GB/s": bytes_in / t_in / 1e9},
                      "ycc_to_u8hwc_crop": {"ms": t_out * 1e3, "GB/s": bytes_out / t_out / 1e9}}))


if __name__ == "__main__":
    main()
