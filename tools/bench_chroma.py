"""Measurements of the chroma formats (codec.py chroma=).  One JSON line per result.

    python tools/bench_chroma.py kernels    HIP-event times of the four kernels of csrc/chroma.hip and, in the same process, of
                                            their 4:4:4 siblings, at 8 x 2048 x 2048 untiled and at 32 tiles of 512 (2 x 2048 x
                                            2048 on a 4 x 4 grid); bytes moved from the shapes (every byte read or written once)
                                            and TB/s
    python tools/bench_chroma.py coding     encode + decode wall time (host clock around a device synchronise) and container
                                            bytes of chroma = 444 / 420 / 400 with seeded weights: one 512 x 512 image and one
                                            3840 x 2160 frame tiled at 512, conditioned2ZTsepSubbands, both coders; median of
                                            --repeats after a warm-up, the formats alternating inside every repeat
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


def kernels(a):
    for B, H, W, th, tw in ((8, 2048, 2048, 2048, 2048), (2, 2048, 2048, 512, 512)):
        ny, nx = H // th, W // tw
        T, px, tpx = B * ny * nx, B * H * W, B * ny * nx * th * tw
        grid, reg = (H, W, th, tw, ny, nx), (0, 0, H, W)
        img = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=DEV)
        grey = img[..., :1].contiguous()
        y444 = ops.u8hwc_to_ycc_tiles(img, th, tw, ny, nx, 0, T)
        luma, chroma = ops.u8hwc_to_ycc420_tiles(img, th, tw, ny, nx, 0, T)
        y400 = ops.u8hw_to_y_tiles(grey, th, tw, ny, nx, 0, T)
        out3 = torch.empty(B, H, W, 3, dtype=torch.uint8, device=DEV)
        out1 = torch.empty(B, H, W, 1, dtype=torch.uint8, device=DEV)
        af3, af1 = ([0.5, 0.5, 0.5], [0.01, 0.02, 0.03]), ([0.5], [0.01])
        # name -> (call, bytes read + written once, from the shapes)
        cases = {
            "u8hwc_to_ycc_tiles (444)": (lambda: ops.u8hwc_to_ycc_tiles(img, th, tw, ny, nx, 0, T), 3 * px + 12 * tpx),
            "u8hwc_to_ycc420_tiles": (lambda: ops.u8hwc_to_ycc420_tiles(img, th, tw, ny, nx, 0, T), 3 * px + 6 * tpx),
            "u8hw_to_y_tiles": (lambda: ops.u8hw_to_y_tiles(grey, th, tw, ny, nx, 0, T), px + 4 * tpx),
            "ycc_tiles_to_u8hwc (444)": (lambda: ops.ycc_tiles_to_u8hwc(y444, grid, reg, B=B, out=out3), 12 * px + 3 * px),
            "ycc420_tiles_to_u8hwc": (lambda: ops.ycc420_tiles_to_u8hwc(luma, chroma, grid, reg, B=B, out=out3), 6 * px + 3 * px),
            "ycc420_tiles_to_u8hwc affine": (lambda: ops.ycc420_tiles_to_u8hwc(luma, chroma, grid, reg, affine=af3, B=B, out=out3),
                                             6 * px + 3 * px),
            "y_tiles_to_u8hw": (lambda: ops.y_tiles_to_u8hw(y400, grid, reg, B=B, out=out1), 4 * px + px),
            "y_tiles_to_u8hw affine": (lambda: ops.y_tiles_to_u8hw(y400, grid, reg, affine=af1, B=B, out=out1), 4 * px + px),
        }
        for name, (fn, nbytes) in cases.items():
            t = timeit(fn, a.iters)
            print(json.dumps({"kernel": name, "shape": [B, H, W], "tile": [th, tw], "tiles": T, "ms": round(t * 1e3, 4),
                              "bytes": nbytes, "bytes_per_pixel": round(nbytes / px, 3), "TB/s": round(nbytes / t / 1e12, 3)}))


def _image(H, W, ch, seed):
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(1, ch, H // 16, W // 16, generator=g)
    x = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
    x = x * 200 + torch.rand(1, ch, H, W, generator=g) * 40
    return x.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def coding(a):
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
        LiftingBasedDWTNetWrapper
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
    cfg = make_config(mode="validate", entropy_layer="conditioned2ZTsepSubbands")
    torch.manual_seed(0)
    net = LiftingBasedDWTNetWrapper(cfg).to(DEV).eval()
    formats = ("444", "420", "400")
    for H, W, tile in ((512, 512, None), (2160, 3840, 512)):
        imgs = {f: _image(H, W, 1 if f == "400" else 3, 5) for f in formats}
        for coder in ("host", "gpu"):
            def once(f):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if tile is None:
                    blob = codec.encode_images(net, imgs[f], coder=coder, chroma=f)[0]
                else:
                    blob = codec.encode_tiled(net, imgs[f], tile=tile, coder=coder, chroma=f)[0]
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                out = codec.decode_images(net, [blob])[0] if tile is None else codec.decode_tiled(net, blob)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                assert out.shape[:2] == (H, W)
                return t1 - t0, t2 - t1, len(blob)
            for f in formats:                                    # warm-up: every shape the timed window uses
                once(f)
            runs = {f: [] for f in formats}
            for _ in range(a.repeats):
                for f in formats:                                # alternating
                    runs[f].append(once(f))
            for f in formats:
                enc = [r[0] for r in runs[f]]
                dec = [r[1] for r in runs[f]]
                print(json.dumps({"image": [H, W], "tile": tile, "coder": coder, "chroma": f, "bytes": runs[f][0][2],
                                  "encode_s": round(statistics.median(enc), 4), "decode_s": round(statistics.median(dec), 4),
                                  "encode_s_all": [round(v, 4) for v in enc], "decode_s_all": [round(v, 4) for v in dec]}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("kernels", "coding"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_chroma.py needs the GPU: nothing here is measured on the host")
    with torch.no_grad():
        (kernels if a.what == "kernels" else coding)(a)


if __name__ == "__main__":
    main()
