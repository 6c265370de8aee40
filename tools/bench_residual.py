"""Times the residual layer's kernels (lldwt_resid_analyse, lldwt_resid_contexts, lldwt_resid_apply) with HIP
events at 8 x 2048 x 2048, d = 0, one unit per image, next to the pad / crop kernels of tools/bench_image_io.py in the same
process, and prints one JSON line: per kernel the milliseconds and GB/s (bytes read + written once; the calls go through the
ops wrappers, so the allocation and zero fill of their outputs are inside the time).
--codec also times a 512 x 512 encode and decode of the chosen layer with and without the residual layer, and the layer's own
encode_units / decode_units on the same reconstruction: wall clock, minimum / median / maximum of --codec-reps runs (seeded,
untrained weights: the split of the time is what is measured, the bytes are no quality claim)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import codec, ops  # noqa: E402
from bench_image_io import timeit  # noqa: E402


def codec_share(layer, size, levels, reps):
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import residual
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
        LiftingBasedDWTNetWrapper
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
    torch.manual_seed(0)
    net = LiftingBasedDWTNetWrapper(make_config(dwtlevels=levels, mode="validate", entropy_layer=layer)).to("cuda:0").eval()
    g = torch.Generator().manual_seed(1)
    low = torch.rand(1, 3, size // 16, size // 16, generator=g)
    x = torch.nn.functional.interpolate(low, size=(size, size), mode="bilinear", align_corners=False) * 200
    x = (x + torch.rand(1, 3, size, size, generator=g) * 40).clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    def wall(fn):
        """One warm-up, then reps wall-clock times -> {min, median, max} in seconds, and the last result."""
        fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ts.sort()
        return {"min": ts[0], "median": ts[len(ts) // 2], "max": ts[-1]}, out
    res = {"layer": layer, "size": size, "levels": levels, "reps": reps}
    for name, kw in (("plain", {}), ("lossless", {"near": 0}), ("near2", {"near": 2})):
        te, blobs = wall(lambda: codec.encode_images(net, x, **kw))
        td, img = wall(lambda: codec.decode_images(net, blobs))
        hdr = codec.read_header(blobs[0])
        res[name] = {"encode_s": te, "decode_s": td, "bytes": len(blobs[0]), "bpp": 8.0 * len(blobs[0]) / size / size,
                     "residual_bytes": hdr.get("residual_bytes", 0),
                     "max_err": int((img[0].int() - x[0].int()).abs().max())}
        if kw:
            # the layer alone, on the reconstruction the codec made: its share without the difference of two noisy totals
            d = kw["near"]
            xd = x.to("cuda:0")
            xh = torch.stack(codec.decode_images(net, blobs, refine=False)).to("cuda:0")
            grid = (size, size, size, size, 1, 1)
            tl, units = wall(lambda: residual.encode_units(xd, xh, grid, [0], d, "host"))
            tr, _ = wall(lambda: residual.decode_units(xh.clone(), grid, (0, 0, size, size), [0], units, d, "host"))
            res[name]["layer_encode_s"], res[name]["layer_decode_s"] = tl, tr
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--near", type=int, default=0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--codec", action="store_true")
    ap.add_argument("--layer", default="conditioned2ZTsepSubbands")
    ap.add_argument("--codec-size", type=int, default=512)
    ap.add_argument("--codec-levels", type=int, default=4)
    ap.add_argument("--codec-reps", type=int, default=15)
    a = ap.parse_args()
    B, H, d = a.batch, a.size, a.near
    dev = "cuda:0"
    x = torch.randint(0, 256, (B, H, H, 3), dtype=torch.uint8, device=dev)
    xh = (x.int() + torch.randint(-6, 7, x.shape, device=dev, dtype=torch.int32)).clamp(0, 255).to(torch.uint8)
    grid, region, tiles = (H, H, H, H, 1, 1), (0, 0, H, H), list(range(B))
    sym, ctx, hist, _, _ = ops.resid_analyse(x, xh, grid, region, tiles, d)
    scales = torch.randint(0, 64, (B, 24), dtype=torch.uint8).to(dev)
    out = torch.empty_like(xh)
    px = B * H * H
    t_an = timeit(lambda: ops.resid_analyse(x, xh, grid, region, tiles, d), a.iters)
    t_cx = timeit(lambda: ops.resid_contexts(xh, grid, region, tiles, scales), a.iters)
    t_ap = timeit(lambda: ops.resid_apply(xh, grid, region, tiles, d, sym, out=out), a.iters)
    Hp = H + 16
    y = ops.u8hwc_to_ycc_pad(x, Hp, Hp)
    t_in = timeit(lambda: ops.u8hwc_to_ycc_pad(x, Hp, Hp), a.iters)
    t_out = timeit(lambda: ops.ycc_to_u8hwc_crop(y, H, H), a.iters)
    rate = lambda nbytes, t: {"ms": t * 1e3, "GB/s": nbytes / t / 1e9}
    res = {"shape": [B, H, H, 3], "near": d,
           "resid_analyse": rate(px * (6 + 24), t_an),            # x and xh read, symbols and context ids written
           "resid_contexts": rate(px * (3 + 12), t_cx),           # xh read, table indexes written
           "resid_apply": rate(px * (3 + 12 + 3), t_ap),          # xh and symbols read, the image written
           "u8hwc_to_ycc_pad": rate(px * 3 + 3 * B * Hp * Hp * 4, t_in),
           "ycc_to_u8hwc_crop": rate(3 * px * 4 + px * 3, t_out)}
    if a.codec:
        res["codec"] = codec_share(a.layer, a.codec_size, a.codec_levels, a.codec_reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
