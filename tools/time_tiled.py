"""Wall time of the image codec, untiled (encode_images / decode_images) or tiled (encode_tiled / decode_tiled), on one
seeded-weight net: median of --reps runs after a warm-up, container bytes, peak device memory, and for the decode the time
spent in the host rANS calls (lldwt_rans_decode_multi) and their count (one host round trip each).  One JSON line.

    python tools/time_tiled.py --mode tiled --height 2160 --width 3840 --tile 512
    python tools/time_tiled.py --mode untiled --height 512 --width 512 [--repo DIR]   (DIR: another checkout to time)
    python tools/time_tiled.py --mode tiled --tile 512 --overlap 16     (lapped tiles; also PSNR / MS-SSIM and the seam figure)

The seam figure (tiled): the mean absolute luma step of the decoded image across the adjacent pixel pairs that straddle a
nominal tile border (the middle of each overlap band; for overlap 0 the tile edge), divided by the same mean over all other
adjacent pairs, rows and columns together.  1 means a border is no rougher than the rest of the picture.
"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("untiled", "tiled"), default="tiled")
    ap.add_argument("--layer", default="conditioned2ZTsepSubbands")
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=0)
    ap.add_argument("--tiles-per-call", type=int, default=32)
    ap.add_argument("--region", help="y0,x0,h,w: time a region decode too (tiled)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, a.repo)
    import torch
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import _lib, codec
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
        LiftingBasedDWTNetWrapper
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
    torch.manual_seed(0)
    net = LiftingBasedDWTNetWrapper(make_config(dwtlevels=a.levels, mode="validate", entropy_layer=a.layer)).to("cuda:0").eval()
    g = torch.Generator().manual_seed(1)
    H, W = a.height, a.width
    low = torch.rand(1, 3, H // 16, W // 16, generator=g)
    x = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False) * 200
    x = (x + torch.rand(1, 3, H, W, generator=g) * 40).clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    if a.mode == "tiled":
        kw = {"overlap": a.overlap} if a.overlap else {}
        enc = lambda: codec.encode_tiled(net, x, tile=a.tile, tiles_per_call=a.tiles_per_call, **kw)[0]
        dec = lambda b, r=None: codec.decode_tiled(net, b, region=r, tiles_per_call=a.tiles_per_call)
    else:
        enc = lambda: codec.encode_images(net, x)[0]
        dec = lambda b, r=None: codec.decode_images(net, [b])[0]

    lib = _lib.load()
    real = lib.lldwt_rans_decode_multi
    rans = {"s": 0.0, "calls": 0}

    def timed(*args):
        t0 = time.perf_counter()
        r = real(*args)
        rans["s"] += time.perf_counter() - t0
        rans["calls"] += 1
        return r
    lib.lldwt_rans_decode_multi = timed

    def clock(fn, *args):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*args)
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    blob = enc()                                       # warm-up (caches, packed weights, allocator)
    dec(blob)
    torch.cuda.reset_peak_memory_stats()
    te, td, tr, rs, rc = [], [], [], [], []
    for _ in range(a.reps):
        blob, t = clock(enc)
        te.append(t)
    peak_enc = torch.cuda.max_memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    for _ in range(a.reps):
        rans["s"], rans["calls"] = 0.0, 0
        _, t = clock(dec, blob)
        td.append(t)
        rs.append(rans["s"])
        rc.append(rans["calls"])
    peak_dec = torch.cuda.max_memory_allocated()
    res = {"mode": a.mode, "layer": a.layer, "L": a.levels, "H": H, "W": W, "bytes": len(blob),
           "encode_s": statistics.median(te), "decode_s": statistics.median(td), "encode_all": te, "decode_all": td,
           "decode_host_rans_s": statistics.median(rs), "decode_rans_calls": rc[0],
           "peak_alloc_encode_GB": peak_enc / 1e9, "peak_alloc_decode_GB": peak_dec / 1e9,
           "omp_num_threads": os.environ.get("OMP_NUM_THREADS")}
    if a.mode == "tiled":
        hdr = codec.read_header(blob)
        res.update(tile=[hdr["th"], hdr["tw"]], grid=[hdr["ny"], hdr["nx"]], tiles_per_call=a.tiles_per_call)
        if hasattr(codec, "quality"):
            img = dec(blob)
            q = codec.quality(x[0], img)
            ov = hdr.get("overlap", 0)
            res.update(overlap=ov, psnr=q["psnr"], msssim=q["msssim"],
                       seam=seam_figure(img, hdr["th"], hdr["tw"], ov, hdr["ny"], hdr["nx"]))
        if a.region:
            reg = tuple(int(v) for v in a.region.split(","))
            for _ in range(a.reps):
                _, t = clock(dec, blob, reg)
                tr.append(t)
            res.update(region=reg, region_decode_s=statistics.median(tr))
    print(json.dumps(res))


def seam_figure(img, th, tw, ov, ny, nx):
    """The module docstring's seam figure of a decoded (H,W,3) uint8 image."""
    import torch
    luma = (img.double() * torch.tensor([0.2126, 0.7152, 0.0722], dtype=torch.float64)).sum(-1)
    num = den = 0.0
    cnt_b = cnt_o = 0
    for axis, t, n in ((0, th, ny), (1, tw, nx)):
        d = luma.diff(dim=axis).abs()
        border = torch.zeros(d.shape[axis], dtype=torch.bool)
        for q in range(1, n):
            i = q * (t - ov) + ov // 2 - 1               # the pair (i, i + 1) straddles the border of tiles q - 1 and q
            if 0 <= i < d.shape[axis]:
                border[i] = True
        sel = d[border] if axis == 0 else d[:, border]
        rest = d[~border] if axis == 0 else d[:, ~border]
        num, cnt_b = num + float(sel.sum()), cnt_b + sel.numel()
        den, cnt_o = den + float(rest.sum()), cnt_o + rest.numel()
    if not cnt_b or not den:
        return None
    return (num / cnt_b) / (den / cnt_o)


if __name__ == "__main__":
    main()
