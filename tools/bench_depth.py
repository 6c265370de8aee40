"""Measurements of 9- to 16-bit coding (codec.py depth=).  One JSON line per result.

    python tools/bench_depth.py kernels    HIP-event times of the seven kernels of csrc/depth.hip and, in the same process, of
                                           their uint8 forms, at 8 x 2048 x 2048 untiled: --repeats windows of --iters calls per
                                           kernel after a warm-up, the two forms of a kernel alternating inside every repeat, the
                                           median window reported; bytes moved from the shapes (every byte read or written once)
                                           and TB/s, and the 16-bit form's bytes per second over its 8-bit form's
    python tools/bench_depth.py coding     encode + decode wall time (host clock around a device synchronise) of one 3 x 512 x
                                           512 image at depth 16 against the same image at 8 bits (v8 * 257: the same streams),
                                           conditioned2ZTsepSubbands with seeded weights, both coders; median of --repeats after a
                                           warm-up, the two depths alternating inside every repeat
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import codec, ops  # noqa: E402

DEV = "cuda:0"


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / iters


def kernels(a):
    B, H, W, d = 8, 2048, 2048, 16
    px = B * H * W
    grid, reg = (H, W, H, W, 1, 1), (0, 0, H, W)
    v8 = torch.randint(0, 256, (B, H, W, 3), dtype=torch.int32, generator=torch.Generator().manual_seed(0))
    img8, img16 = v8.to(torch.uint8).to(DEV), (v8 * 257).to(torch.uint16).to(DEV)      # converted on the host
    g8, g16 = img8[..., :1].contiguous(), img16[..., :1].contiguous()
    flag = ops.depth_flag(DEV)
    y444 = ops.u8hwc_to_ycc_tiles(img8, H, W, 1, 1, 0, B)
    luma, chroma = ops.u8hwc_to_ycc420_tiles(img8, H, W, 1, 1, 0, B)
    y400 = ops.u8hw_to_y_tiles(g8, H, W, 1, 1, 0, B)
    o8 = {3: torch.empty(B, H, W, 3, dtype=torch.uint8, device=DEV), 1: torch.empty(B, H, W, 1, dtype=torch.uint8, device=DEV)}
    o16 = {3: torch.empty(B, H, W, 3, dtype=torch.uint16, device=DEV), 1: torch.empty(B, H, W, 1, dtype=torch.uint16, device=DEV)}
    af3 = ([0.5, 0.5, 0.5], [0.01, 0.02, 0.03])
    # name -> ((8-bit call, bytes), (16-bit call, bytes)): bytes read + written once, from the shapes
    cases = {
        "to_ycc_tiles (444)": ((lambda: ops.u8hwc_to_ycc_tiles(img8, H, W, 1, 1, 0, B), (3 + 12) * px),
                               (lambda: ops.u16hwc_to_ycc_tiles(img16, H, W, 1, 1, 0, B, d, flag), (6 + 12) * px)),
        "to_ycc420_tiles": ((lambda: ops.u8hwc_to_ycc420_tiles(img8, H, W, 1, 1, 0, B), (3 + 6) * px),
                            (lambda: ops.u16hwc_to_ycc420_tiles(img16, H, W, 1, 1, 0, B, d, flag), (6 + 6) * px)),
        "to_y_tiles (400)": ((lambda: ops.u8hw_to_y_tiles(g8, H, W, 1, 1, 0, B), (1 + 4) * px),
                             (lambda: ops.u16hw_to_y_tiles(g16, H, W, 1, 1, 0, B, d, flag), (2 + 4) * px)),
        "to_f32chw": ((lambda: ops.u8hwc_to_f32chw(img8), (3 + 12) * px),
                      (lambda: ops.u16hwc_to_f32chw(img16, d, flag), (6 + 12) * px)),
        "ycc_tiles_to (444)": ((lambda: ops.ycc_tiles_to_u8hwc(y444, grid, reg, B=B, out=o8[3]), (12 + 3) * px),
                               (lambda: ops.ycc_tiles_to_u16hwc(y444, grid, reg, d, B=B, out=o16[3]), (12 + 6) * px)),
        "ycc_tiles_to (444) affine": ((lambda: ops.ll_tiles_to_u8hwc(y444, grid, reg, af3[0], af3[1], B=B, out=o8[3]), (12 + 3) * px),
                                      (lambda: ops.ycc_tiles_to_u16hwc(y444, grid, reg, d, affine=af3, B=B, out=o16[3]), (12 + 6) * px)),
        "ycc420_tiles_to": ((lambda: ops.ycc420_tiles_to_u8hwc(luma, chroma, grid, reg, B=B, out=o8[3]), (6 + 3) * px),
                            (lambda: ops.ycc420_tiles_to_u16hwc(luma, chroma, grid, reg, d, B=B, out=o16[3]), (6 + 6) * px)),
        "y_tiles_to (400)": ((lambda: ops.y_tiles_to_u8hw(y400, grid, reg, B=B, out=o8[1]), (4 + 1) * px),
                             (lambda: ops.y_tiles_to_u16hw(y400, grid, reg, d, B=B, out=o16[1]), (4 + 2) * px)),
    }
    for name, forms in cases.items():
        for fn, _ in forms:                                      # warm-up: both forms
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        runs = ([], [])
        for _ in range(a.repeats):
            for k, (fn, _) in enumerate(forms):                  # alternating
                runs[k].append(window(fn, a.iters))
        t8, t16 = statistics.median(runs[0]), statistics.median(runs[1])
        r8, r16 = forms[0][1] / t8, forms[1][1] / t16
        print(json.dumps({"kernel": name, "shape": [B, H, W], "depth": d,
                          "u8": {"ms": round(t8 * 1e3, 4), "bytes_per_pixel": forms[0][1] // px, "TB/s": round(r8 / 1e12, 3)},
                          "u16": {"ms": round(t16 * 1e3, 4), "bytes_per_pixel": forms[1][1] // px, "TB/s": round(r16 / 1e12, 3)},
                          "u16_over_u8_bytes_per_s": round(r16 / r8, 3),
                          "ms_all": {"u8": [round(v * 1e3, 4) for v in runs[0]], "u16": [round(v * 1e3, 4) for v in runs[1]]}}))
    assert int(flag.item()) == 0


def coding(a):
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
        LiftingBasedDWTNetWrapper
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
    cfg = make_config(mode="validate", entropy_layer="conditioned2ZTsepSubbands")
    torch.manual_seed(0)
    net = LiftingBasedDWTNetWrapper(cfg).to(DEV).eval()
    H = W = 512
    g = torch.Generator().manual_seed(5)
    low = torch.rand(1, 3, H // 16, W // 16, generator=g)
    x = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False) * 200
    x = (x + torch.rand(1, 3, H, W, generator=g) * 40).clamp(0, 255).round().to(torch.int32).permute(0, 2, 3, 1).contiguous()
    imgs = {8: x.to(torch.uint8), 16: (x * 257).to(torch.uint16)}
    for coder in ("host", "gpu"):
        def once(d):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            blob = codec.encode_images(net, imgs[d], coder=coder, depth=d)[0]
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            out = codec.decode_images(net, [blob])[0]
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            assert out.shape == (H, W, 3)
            return t1 - t0, t2 - t1, len(blob)
        for d in (8, 16):
            once(d)
        runs = {8: [], 16: []}
        for _ in range(a.repeats):
            for d in (8, 16):
                runs[d].append(once(d))
        for d in (8, 16):
            enc, dec = [r[0] for r in runs[d]], [r[1] for r in runs[d]]
            print(json.dumps({"image": [H, W], "coder": coder, "depth": d, "bytes": runs[d][0][2],
                              "encode_s": round(statistics.median(enc), 4), "decode_s": round(statistics.median(dec), 4),
                              "encode_s_all": [round(v, 4) for v in enc], "decode_s_all": [round(v, 4) for v in dec]}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("kernels", "coding"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth.py needs the GPU: nothing here is measured on the host")
    with torch.no_grad():
        (kernels if a.what == "kernels" else coding)(a)


if __name__ == "__main__":
    main()
