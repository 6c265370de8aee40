"""Times the image codec's I/O kernels (lldwt_u8hwc_to_ycc_pad, lldwt_ycc_to_u8hwc_crop) with HIP events and prints one JSON
line of GB/s (bytes read + written once).  Default 8 x 2048 x 2048, padded by 16 rows / columns.
--tiled times the tile-grid kernels instead (lldwt_u8hwc_to_ycc_tiles over every tile of the batch,
lldwt_ycc_tiles_to_u8hwc writing the whole image from them): default 8 x 3840 x 2160 at tile 512 (480 x 432 tiles).
--lapped times the lapped-grid kernels (lldwt_u8hwc_to_ycc_tiles_lapped over every tile of the batch, and per image
lldwt_ycc_tiles_blend of all its tiles into the image-sized accumulator) at --overlap (default 16) with tiles of
--th x --tw (default here 448 x 496, the grid of tile 512 at overlap 16)."""
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
    ap.add_argument("--tiled", action="store_true")
    ap.add_argument("--lapped", action="store_true")
    ap.add_argument("--overlap", type=int, default=16)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--th", type=int)
    ap.add_argument("--tw", type=int)
    a = ap.parse_args()
    a.th = a.th or (448 if a.lapped else 432)
    a.tw = a.tw or (496 if a.lapped else 480)
    if a.lapped:
        return lapped(a)
    if a.tiled:
        return tiled(a)
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


def tiled(a):
    B, H, W, th, tw = a.batch, a.height, a.width, a.th, a.tw
    ny, nx = -(-H // th), -(-W // tw)
    T = B * ny * nx
    img = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda:0")
    y = ops.u8hwc_to_ycc_tiles(img, th, tw, ny, nx, 0, T)
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device="cuda:0")
    grid = (H, W, th, tw, ny, nx)
    t_in = timeit(lambda: ops.u8hwc_to_ycc_tiles(img, th, tw, ny, nx, 0, T), a.iters)
    t_out = timeit(lambda: ops.ycc_tiles_to_u8hwc(y, grid, (0, 0, H, W), B=B, out=out), a.iters)
    tile_px = T * th * tw
    bytes_in = B * H * W * 3 + 3 * tile_px * 4         # each source byte read once (no padding at the default grid)
    bytes_out = 3 * B * H * W * 4 + B * H * W * 3      # the scatter reads the in-image part of every tile
    print(json.dumps({"shape": [B, H, W, 3], "tile": [th, tw], "grid": [ny, nx], "tiles": T,
                      "u8hwc_to_ycc_tiles": {"ms": t_in * 1e3, "GB/s": bytes_in / t_in / 1e9},
                      "ycc_tiles_to_u8hwc": {"ms": t_out * 1e3, "GB/s": bytes_out / t_out / 1e9}}))


def lapped(a):
    B, H, W, th, tw, ov = a.batch, a.height, a.width, a.th, a.tw, a.overlap
    count = lambda size, t: 1 if t >= size else -(-(size - t) // (t - ov)) + 1
    ny, nx = count(H, th), count(W, tw)
    T = B * ny * nx
    img = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda:0")
    y = ops.u8hwc_to_ycc_tiles_lapped(img, th, tw, ov, ny, nx, 0, T)
    acc = torch.zeros(3, 1, 1, H, W, device="cuda:0")
    grid = (H, W, th, tw, ov, ny, nx)
    per = ny * nx
    ys = [y[:, b * per:(b + 1) * per].contiguous() for b in range(B)]
    lst = list(range(per))

    def blend():                                       # one launch per image (the accumulator holds one image)
        for b in range(B):
            ops.ycc_tiles_blend(ys[b], grid, (0, 0, H, W), lst, acc)
    t_in = timeit(lambda: ops.u8hwc_to_ycc_tiles_lapped(img, th, tw, ov, ny, nx, 0, T), a.iters)
    t_out = timeit(blend, a.iters)
    cover = lambda size, t, n: sum(min(size, q * (t - ov) + t) - q * (t - ov) for q in range(n))
    in_px = cover(H, th, ny) * cover(W, tw, nx)        # tile samples inside the image: each is read once by the blend
    bytes_in = B * H * W * 3 + 3 * T * th * tw * 4     # source bytes once (band re-reads hit the cache), every tile written
    bytes_out = B * (3 * in_px * 4 + 2 * 3 * H * W * 4)    # tile samples read, the accumulator read and written
    print(json.dumps({"shape": [B, H, W, 3], "tile": [th, tw], "overlap": ov, "grid": [ny, nx], "tiles": T,
                      "u8hwc_to_ycc_tiles_lapped": {"ms": t_in * 1e3, "GB/s": bytes_in / t_in / 1e9},
                      "ycc_tiles_blend": {"ms": t_out * 1e3, "GB/s": bytes_out / t_out / 1e9,
                                          "launches": B, "includes_slot_table_upload": True}}))


if __name__ == "__main__":
    main()
