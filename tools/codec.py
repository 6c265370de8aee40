"""Command-line image codec on the HIP path (imagecompressionlearnedliftingandlearnedtreebasedmodels_amd/codec.py).

    python tools/codec.py encode --config cfg.json [--checkpoint ckpt.pth.tar] in.png out.lld
    python tools/codec.py decode --config cfg.json [--checkpoint ckpt.pth.tar] in.lld out.png
    python tools/codec.py info in.lld                      (CPU only: prints the header and the bytes a decode reads
                                                            at each reduce factor)

    encode --tile N [--tiles-per-call K]   writes a tiled (LLDT) container: N x N target tiles, each an independent image
    encode --tile N --overlap V            writes a lapped (LLDO) container: neighbouring tiles share V pixels (a power of
                                           two, 2^dwtlevels <= V <= half a tile) and the decoder cross-fades them
    decode --region y0,x0,h,w              decodes only that region (tiled containers only)
    decode --reduce k                      decodes the image at 1/2^k of each side from the coarse levels only (0 <= k <=
                                           dwtlevels; with --region, the region is in the reduced image's coordinates)
    python tools/codec.py compare a.png b.png              (prints PSNR, MS-SSIM and MS-SSIM in dB of two image files)

    decode --compare SRC                   after decoding, prints the same three figures for the decoded image against SRC
    encode --coder gpu                     codes the streams with the interleaved device coder (irans32); decode reads the
                                           coder from the header

    encode --step Q                        quantises the levels below the coarsest with the step Q = n / 16 in [0.25, 64]
                                           (1: the trained operating point); decode reads the step from the header
    encode --target-bytes T | --target-bpp R   chooses the finest step of the quarter-octave grid whose container is at most
                                           T bytes (R bits per pixel: T = floor(R * H * W / 8)); info prints the step
    encode --target-psnr DB | --target-msssim M   chooses a step of the same grid whose decoded image has at least DB dB of
                                           PSNR (or an MS-SSIM of at least M, sides >= 161) while the next coarser grid step
                                           does not: the coarsest step that meets the target where quality falls along the
                                           grid.  Prints the chosen step and the achieved value.  Not with --step,
                                           --target-bytes / --target-bpp, --roi, --near or --lossless
    encode --rdo R                         rate-distortion optimised quantisation with the Lagrangian R = m / 64 in (0, 4]
                                           (q^2 per bit; try 0.203125 = 13 / 64): fewer bytes for a little more error.  The
                                           encoder's choice alone: nothing in the container tells, decode needs no option

    encode --roi y0,x0,h,w:Q               region-of-interest coding: the blocks of 2^dwtlevels pixels that the rectangle touches
                                           are coded at the step Q, the rest at --step (default 1).  Repeatable, later ones
                                           override earlier ones; writes an LLDQ container around what the other options
                                           select.  Not with --target-bytes / --target-bpp.  decode needs no option; info
                                           prints the map's size, its steps and the share of blocks at each

    encode --aq S                          adaptive quantisation at the strength S = m / 16 in (0, 2] (try 1): a step map derived
                                           from the image -- flat blocks of 2^dwtlevels pixels get finer steps, busy ones coarser,
                                           around --step (default 1) -- in an LLDQ container, which decode and info read as any
                                           step map.  With --target-bytes / --target-bpp / --target-psnr / --target-msssim the
                                           search moves the base step of that map and prints it.  With --tile and --overlap.
                                           Not with --roi, --layers, --chroma other than 444 or --depth

    encode --layers M                      adds M quality layers (1..4) over the container of --step Q: layer j refines the levels
                                           below the coarsest to the step Q / 3^j (Q * 16 / 3^M >= 1), writing an LLDP container.
                                           Not with --near / --lossless, --roi, --overlap or a target
    decode --layers J                      decodes the base plus the first J layers (default: all the container holds); info
                                           prints the bytes each prefix reads

    encode --chroma {444,420,400}          the chroma format: 444 (default) codes three full-size planes; 420 codes Cb and Cr at
                                           half size (1.5 planes of coefficients); 400 loads the file as greyscale (PIL mode L)
                                           and codes one plane.  decode reads the format from the header and writes mode L for a
                                           400 container; info prints it.  Not with --near / --lossless, --layers, --roi,
                                           --overlap, --target-psnr / --target-msssim

    encode --depth D                       samples of D bits in 9..16: reads a .npy file of shape (H,W,3) or (H,W) (greyscale, with
                                           --chroma 400) or a binary PPM / PGM (P6 / P5) whose maxval is 2^D - 1 (16-bit samples
                                           big-endian, per Netpbm).  decode reads the depth from the header and writes .npy, .ppm
                                           or .pgm by the output's extension; info prints it.  compare --depth D takes two such
                                           files.  Not with --near / --lossless, --layers, --roi, --overlap, --target-psnr /
                                           --target-msssim

    decode --recon {centre,centroid}       centroid puts every coefficient of the levels that carry a step at the mean of its
                                           quantisation bin under the entropy model's Gaussian instead of the bin's centre: no
                                           bits, no container change, a little less error at large steps, behind --roi and under
                                           truncated --layers.  Not over a refined (LLDR) container without --base-only.  With
                                           --compare SRC the two reconstructions can be told apart by PSNR / MS-SSIM

The config is a JSON object of LiftingBasedDWTNetWrapper keys (utils/config.py DEFAULTS fill the rest).  The checkpoint is
read with the weights-only unpickler and must match the model's key set exactly (agents/base.py load_checkpoint).
Without a checkpoint the net gets seeded default-initialised weights -- for trying the tool out only: encoder and
decoder must then use the same config (and seed).
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import codec  # noqa: E402


def build_net(config_path, checkpoint=None, device="cuda:0"):
    import torch
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
        LiftingBasedDWTNetWrapper
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
    with open(config_path) as f:
        cfg = make_config(**json.load(f))
    torch.manual_seed(int(cfg.get("seed", 1337)))
    net = LiftingBasedDWTNetWrapper(cfg)
    if checkpoint:
        ckpt = torch.load(checkpoint, map_location="cpu", weights_only=True)
        sd = ckpt["state_dict"] if isinstance(ckpt, dict) and "state_dict" in ckpt else ckpt
        missing, unexpected = net.load_state_dict(sd, strict=False)
        if missing or unexpected:
            raise RuntimeError("checkpoint %s does not match the model: %d missing keys (e.g. %s), %d unexpected (e.g. %s)"
                               % (checkpoint, len(missing), missing[:3], len(unexpected), unexpected[:3]))
    return net.to(device).eval()


def print_quality(a_u8, b_u8, depth=None):
    """PSNR / MS-SSIM lines of two (H,W,3) uint8 tensors, or uint16 ones of ``depth`` bits (codec.quality)."""
    q = codec.quality(a_u8, b_u8, depth=depth)
    print("psnr     %.4f dB" % q["psnr"])
    if q["msssim"] is None:
        print("ms-ssim  n/a (a side is below 161)")
    else:
        print("ms-ssim  %.6f" % q["msssim"])
        print("ms-ssim  %.4f dB" % codec.msssim_db(q["msssim"]))


def _load_rgb(path):
    import numpy as np
    import torch
    from PIL import Image
    return torch.from_numpy(np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)))


def read_pnm(path):
    """A binary PPM (P6) or PGM (P5) file -> (numpy array (H,W,3) or (H,W), maxval): uint8 for maxval < 256, else uint16 read
    from big-endian 16-bit samples (Netpbm).  Comments (# to the end of the line) may stand between the header's tokens."""
    import numpy as np
    with open(path, "rb") as f:
        data = f.read()
    pos, tokens = 0, []
    while len(tokens) < 4:
        while pos < len(data) and data[pos:pos + 1].isspace():
            pos += 1
        if data[pos:pos + 1] == b"#":
            while pos < len(data) and data[pos:pos + 1] != b"\n":
                pos += 1
            continue
        start = pos
        while pos < len(data) and not data[pos:pos + 1].isspace():
            pos += 1
        if start == pos:
            raise ValueError("%s: truncated PNM header" % path)
        tokens.append(data[start:pos])
    pos += 1                                               # the single whitespace byte after maxval
    if tokens[0] not in (b"P5", b"P6"):
        raise ValueError("%s: not a binary PGM / PPM file (magic %r)" % (path, tokens[0]))
    try:
        W, H, maxval = (int(t) for t in tokens[1:])
    except ValueError:
        raise ValueError("%s: bad PNM header %r" % (path, tokens)) from None
    if W < 1 or H < 1 or not 1 <= maxval <= 65535:
        raise ValueError("%s: bad PNM header: %d x %d, maxval %d" % (path, W, H, maxval))
    ch = 3 if tokens[0] == b"P6" else 1
    dt = np.dtype(">u2") if maxval > 255 else np.dtype("u1")
    if len(data) - pos < H * W * ch * dt.itemsize:
        raise ValueError("%s: %d sample bytes, the header announces %d" % (path, len(data) - pos, H * W * ch * dt.itemsize))
    a = np.frombuffer(data, dtype=dt, count=H * W * ch, offset=pos).astype(np.uint16 if maxval > 255 else np.uint8)
    return (a.reshape(H, W, 3) if ch == 3 else a.reshape(H, W)), maxval


def write_pnm(path, a, maxval):
    """(H,W,3) -> binary PPM (P6), (H,W) -> binary PGM (P5), with the given maxval; samples above 255 as big-endian 16 bits."""
    import numpy as np
    a = np.asarray(a)
    if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or not 1 <= maxval <= 65535:
        raise ValueError("write_pnm: an (H,W,3) or (H,W) array and a maxval in [1, 65535]")
    with open(path, "wb") as f:
        f.write(b"%s\n%d %d\n%d\n" % (b"P6" if a.ndim == 3 else b"P5", a.shape[1], a.shape[0], maxval))
        f.write(np.ascontiguousarray(a.astype(">u2" if maxval > 255 else "u1")).tobytes())


def load_deep(path, depth, grey=False):
    """A .npy, .ppm or .pgm file of ``depth``-bit samples -> (H,W,3) (or (H,W,1) with grey) uint16 torch tensor.  A PNM file's
    maxval must be 2^depth - 1; the range of a .npy file is checked by the encoder."""
    import numpy as np
    import torch
    if path.lower().endswith(".npy"):
        a = np.load(path, allow_pickle=False)
        if a.dtype != np.uint16:
            raise ValueError("%s: --depth takes a uint16 array (got %s)" % (path, a.dtype))
    else:
        a, maxval = read_pnm(path)
        if maxval != (1 << depth) - 1:
            raise ValueError("%s: maxval %d, --depth %d needs %d" % (path, maxval, depth, (1 << depth) - 1))
        a = a.astype(np.uint16)
    if a.ndim != (2 if grey else 3) or (not grey and a.shape[2] != 3):
        raise ValueError("%s: expected %s, got shape %s" % (path, "(H,W) greyscale samples" if grey else "(H,W,3) RGB samples",
                                                           a.shape))
    x = torch.from_numpy(np.ascontiguousarray(a))
    return x[..., None] if grey else x


def save_deep(path, img, depth):
    """A decoded (H,W,3) / (H,W,1) uint16 tensor -> .npy, or .ppm / .pgm with maxval 2^depth - 1, by the extension."""
    import numpy as np
    a = img.numpy()
    a = a[..., 0] if a.shape[2] == 1 else a
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        with open(path, "wb") as f:
            np.save(f, a)
    elif ext == (".pgm" if a.ndim == 2 else ".ppm"):
        write_pnm(path, a, (1 << depth) - 1)
    else:
        raise ValueError("%s: a %d-bit %s image is written as .npy or %s" % (path, depth, "greyscale" if a.ndim == 2 else "RGB",
                                                                             ".pgm" if a.ndim == 2 else ".ppm"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("encode", "decode"):
        p = sub.add_parser(name)
        p.add_argument("--config", required=True)
        p.add_argument("--checkpoint")
        p.add_argument("--tiles-per-call", type=int, default=32)
        p.add_argument("src")
        p.add_argument("dst")
    sub.choices["encode"].add_argument("--tile", type=int, help="write a tiled container with this target tile side")
    sub.choices["encode"].add_argument("--overlap", type=int, default=0,
                                       help="with --tile: pixels neighbouring tiles share, cross-faded on decode (default 0)")
    sub.choices["encode"].add_argument("--coder", choices=("host", "gpu"), default="host",
                                       help="entropy coder: host (rans64, the default) or gpu (irans32 on the device)")
    sub.choices["encode"].add_argument("--near", type=int, metavar="D",
                                       help="add a residual layer that bounds every sample's error by D in 1..32 (0: lossless)")
    sub.choices["encode"].add_argument("--lossless", action="store_true", help="the same as --near 0")
    rate = sub.choices["encode"].add_mutually_exclusive_group()
    rate.add_argument("--step", type=float, metavar="Q", help="quantisation step n / 16 in [0.25, 64] (default 1)")
    rate.add_argument("--target-bytes", type=int, metavar="T", help="finest grid step whose container is at most T bytes")
    rate.add_argument("--target-bpp", type=float, metavar="R", help="the same for R bits per pixel")
    rate.add_argument("--target-psnr", type=float, metavar="DB",
                      help="a grid step whose decoded image has at least DB dB while the next coarser one does not")
    rate.add_argument("--target-msssim", type=float, metavar="M", help="the same for an MS-SSIM of at least M in (0, 1)")
    sub.choices["encode"].add_argument("--rdo", type=float, metavar="R",
                                       help="rate-distortion optimised quantisation, Lagrangian m / 64 in (0, 4] (default off)")
    sub.choices["encode"].add_argument("--roi", action="append", metavar="Y0,X0,H,W:Q",
                                       help="code this rectangle at the step Q, the rest at --step (repeatable; writes LLDQ)")
    sub.choices["encode"].add_argument("--aq", type=float, metavar="S",
                                       help="adaptive quantisation, strength m / 16 in (0, 2]: an activity-derived step map around "
                                            "the step, or around the base step a target chooses (writes LLDQ)")
    sub.choices["encode"].add_argument("--layers", type=int, metavar="M",
                                       help="add M quality layers (1..4) that refine the step by 3 each (writes LLDP)")
    sub.choices["encode"].add_argument("--chroma", choices=("444", "420", "400"), default="444",
                                       help="chroma format: 444 (default), 420 (half-size chroma) or 400 (greyscale, mode L)")
    sub.choices["encode"].add_argument("--depth", type=int, metavar="D",
                                       help="samples of D bits in 9..16 from a .npy, .ppm or .pgm file (default: 8-bit image files)")
    sub.choices["decode"].add_argument("--layers", type=int, metavar="J",
                                       help="decode the base plus the first J quality layers of an LLDP container (default: all)")
    sub.choices["decode"].add_argument("--recon", choices=("centre", "centroid"), default="centre",
                                       help="where a coefficient goes inside its quantisation bin: the centre (default) or the "
                                            "bin's mean under the entropy model's Gaussian")
    sub.choices["decode"].add_argument("--base-only", action="store_true",
                                       help="decode the base layer of a refined (LLDR) container only")
    sub.choices["decode"].add_argument("--region", help="y0,x0,h,w: decode only this region (tiled containers only)")
    sub.choices["decode"].add_argument("--reduce", type=int, default=0,
                                       help="decode at 1/2^k of each side from the coarse wavelet levels (default 0: full)")
    sub.choices["decode"].add_argument("--compare", metavar="SRC",
                                       help="print PSNR and MS-SSIM of the decoded image against this image file")
    p = sub.add_parser("info")
    p.add_argument("src")
    p = sub.add_parser("compare")
    p.add_argument("a")
    p.add_argument("b")
    p.add_argument("--depth", type=int, metavar="D", help="compare two .npy / .ppm files of D-bit samples (9..16)")
    a = ap.parse_args(argv)

    if a.cmd == "info":
        with open(a.src, "rb") as f:
            blob = f.read()
        hdr = codec.read_header(blob)
        if "inner" in hdr:                     # LLDQ: the map, then the inner container's
            import numpy as np
            m = codec.parse_mapped(blob)[1]
            print("%-15s %d x %d blocks of %d x %d pixels, CRC %08x" % ("step map", hdr["hb"], hdr["wb"], 1 << hdr["block"],
                                                                     1 << hdr["block"], hdr["map_crc"]))
            vals, counts = np.unique(m, return_counts=True)
            for v, c in zip(vals.tolist(), counts.tolist()):
                print("%-15s %g: %d blocks (%.1f %%)" % ("  step", v / codec.STEP_DENOM, c, 100.0 * c / m.size))
            hdr = hdr["inner"]
        if "layers" in hdr:                    # LLDP: the layer count and the bytes each prefix reads, then the base container's
            print("%-15s %d (bell positions 0 .. %d, table CRC %08x)" % ("layers", hdr["layers"], hdr["K"], hdr["table_crc"]))
            print("%-15s %d" % ("units", hdr["units"]))
            print("%-15s %d" % ("base_bytes", hdr["base_bytes"]))
            for j, n in enumerate(hdr["layer_bytes"]):
                print("%-15s step %g: %d bytes" % ("layers %d" % j, hdr["base"]["step"] / 3 ** j, n))
            hdr = hdr["base"]
        elif "base" in hdr:                    # LLDR: the layer's own fields and the byte split, then the base container's
            print("%-15s %s" % ("near", "0 (lossless)" if hdr["near"] == 0 else "%d (every sample within %d)" % (hdr["near"],
                                                                                                            hdr["near"])))
            print("%-15s %d" % ("units", hdr["units"]))
            print("%-15s %d" % ("base_bytes", hdr["base_bytes"]))
            print("%-15s %d" % ("residual_bytes", hdr["residual_bytes"]))
            hdr = hdr["base"]
        for k, v in hdr.items():
            print("%-15s %s" % (k, v.hex() if isinstance(v, bytes) else v))
        print("%-15s %d bits per sample" % ("sample depth", hdr.get("depth", 8)))
        fmt = hdr.get("chroma", "444")
        print("%-15s %s (%d planes coded%s)" % ("chroma format", fmt, codec.CHROMA_PLANES[fmt],
                                              ", Cb and Cr at half size" if fmt == "420" else ""))
        if "ny" in hdr:
            print("%-15s %d x %d tiles of %d x %d (rows x columns)" % ("grid", hdr["ny"], hdr["nx"], hdr["th"], hdr["tw"]))
            if hdr["overlap"]:
                print("%-15s neighbouring tiles share %d pixels (stride %d x %d)"
                      % ("lapped", hdr["overlap"], hdr["th"] - hdr["overlap"], hdr["tw"] - hdr["overlap"]))
        for k, n in enumerate(codec.reduce_bytes(hdr)):
            print("%-15s %d x %d: %d bytes" % ("reduce %d" % k, -(-hdr["W"] >> k), -(-hdr["H"] >> k), n))
        return 0

    if a.cmd == "compare":
        deep = a.depth is not None and codec.check_depth(a.depth) != 8
        xa, xb = (load_deep(a.a, a.depth), load_deep(a.b, a.depth)) if deep else (_load_rgb(a.a), _load_rgb(a.b))
        if xa.shape != xb.shape:
            print("compare: the images differ in size: %dx%d and %dx%d" % (xa.shape[1], xa.shape[0], xb.shape[1], xb.shape[0]),
                  file=sys.stderr)
            return 2
        print_quality(xa, xb, a.depth if deep else None)
        return 0

    import numpy as np
    import torch
    from PIL import Image
    net = build_net(a.config, a.checkpoint)
    if a.cmd == "encode":
        deep = a.depth is not None and codec.check_depth(a.depth) != 8
        if deep:
            x = load_deep(a.src, a.depth, a.chroma == "400")[None]
            img = x[0]
        else:
            img = np.asarray(Image.open(a.src).convert("L" if a.chroma == "400" else "RGB"), dtype=np.uint8)
            x = torch.from_numpy(np.ascontiguousarray(img))[None]
            if a.chroma == "400":
                x = x[..., None]                                # (1,H,W,1)
        if a.lossless and a.near not in (None, 0):
            print("--lossless is --near 0; give one of them", file=sys.stderr)
            return 2
        kw = {"near": 0 if a.lossless else a.near} if (a.lossless or a.near is not None) else {}
        if a.step is not None:
            kw["step"] = a.step
        elif a.target_bytes is not None:
            kw["target_bytes"] = a.target_bytes
        elif a.target_bpp is not None:
            kw["target_bytes"] = codec.target_bpp_bytes(a.target_bpp, img.shape[0], img.shape[1])
        elif a.target_psnr is not None:
            kw["target_psnr"] = a.target_psnr
        elif a.target_msssim is not None:
            kw["target_msssim"] = a.target_msssim
        if a.rdo is not None:
            kw["rdo"] = a.rdo
        if a.layers is not None:
            kw["layers"] = a.layers
        if a.chroma != "444":
            kw["chroma"] = a.chroma
        if deep:
            kw["depth"] = a.depth
        if a.aq is not None:
            for flag, given in (("--roi", bool(a.roi)), ("--layers", a.layers is not None), ("--chroma " + a.chroma, a.chroma != "444"),
                                ("--depth", a.depth is not None)):
                if given and codec.check_aq(a.aq):
                    print("--aq cannot be combined with %s (the activity map is defined for 8-bit 4:4:4 images and is the only "
                          "source of the step map)" % flag, file=sys.stderr)
                    return 2
            kw["aq"] = a.aq
        if a.roi:
            if a.target_bytes is not None or a.target_bpp is not None:
                print("--roi cannot be combined with --target-bytes / --target-bpp (a byte target over a step map is not defined)",
                      file=sys.stderr)
                return 2
            if a.target_psnr is not None or a.target_msssim is not None:
                print("--roi cannot be combined with --target-psnr / --target-msssim (a quality target over a step map is not "
                      "defined)", file=sys.stderr)
                return 2
            regions = []
            for r in a.roi:
                try:
                    rect, q = r.split(":")
                    regions.append(tuple(int(v) for v in rect.split(",")) + (float(q),))
                    assert len(regions[-1]) == 5
                except (ValueError, AssertionError):
                    print("--roi takes y0,x0,h,w:Q (got %r)" % r, file=sys.stderr)
                    return 2
            kw["step_map"] = codec.step_map_from_regions(img.shape[0], img.shape[1], codec.describe(net)[2], kw.pop("step", 1.0),
                                                         regions)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if a.tile is None:
            if a.overlap:
                print("--overlap needs --tile", file=sys.stderr)
                return 2
            blob = codec.encode_images(net, x, coder=a.coder, **kw)[0]
        elif a.overlap:
            blob = codec.encode_tiled(net, x, tile=a.tile, tiles_per_call=a.tiles_per_call, coder=a.coder,
                                      overlap=a.overlap, **kw)[0]
        else:
            blob = codec.encode_tiled(net, x, tile=a.tile, tiles_per_call=a.tiles_per_call, coder=a.coder, **kw)[0]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        with open(a.dst, "wb") as f:
            f.write(blob)
        H, W = img.shape[:2]
        print("encoded %dx%d: %d bytes, %.4f bpp, %.3f s" % (W, H, len(blob), len(blob) * 8 / (H * W), dt))
        hdr = codec.read_header(blob)
        if "inner" in hdr:
            print("step map: %d x %d blocks, steps %g .. %g" % (hdr["hb"], hdr["wb"], hdr["step_min"], hdr["step_max"]))
            hdr = hdr["inner"]
        if "layers" in hdr:
            print("layers %d: bytes read by each prefix %s" % (hdr["layers"], hdr["layer_bytes"]))
            hdr = hdr["base"]
        elif "base" in hdr:
            print("near %d: base %d bytes, residual %d bytes" % (hdr["near"], hdr["base_bytes"], hdr["residual_bytes"]))
            hdr = hdr["base"]
        if hdr["step"] != 1.0:
            print("step: %g" % hdr["step"])
        if a.aq and (a.target_bytes is not None or a.target_bpp is not None):
            print("aq %g: base step %g" % (a.aq, codec.SEARCH_STATS["step"]))
        if a.target_psnr is not None:
            st = codec.SEARCH_STATS
            print("target %g dB: step %g, %.4f dB (SSE %d), %d probes, %d encode"
                  % (a.target_psnr, st["step"], codec.sse_psnr(st["sse"], H, W), st["sse"], st["probes"], st["encodes"]))
        elif a.target_msssim is not None:
            st = codec.SEARCH_STATS
            print("target ms-ssim %g: step %g, %.6f (%.4f dB), %d probes, %d encode"
                  % (a.target_msssim, st["step"], st["msssim"], codec.msssim_db(st["msssim"]), st["probes"], st["encodes"]))
        if a.tile is not None:
            print("tiles: %d x %d of %dx%d" % (hdr["ny"], hdr["nx"], hdr["tw"], hdr["th"]))
            if hdr["overlap"]:
                print("overlap: %d" % hdr["overlap"])
    else:
        with open(a.src, "rb") as f:
            blob = f.read()
        kw = {"refine": False} if a.base_only else {}
        if a.layers is not None:
            kw["layers"] = a.layers
        if a.recon != "centre":
            kw["recon"] = a.recon
        inner = codec.read_header(blob)["inner"] if blob[:4] == codec.MAPPED_MAGIC else codec.read_header(blob)
        tiled = "ny" in inner.get("base", inner)
        region = None
        if a.region is not None:
            if not tiled:
                print("--region needs a tiled container (encode --tile)", file=sys.stderr)
                return 2
            region = tuple(int(v) for v in a.region.split(","))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if tiled:
            img = codec.decode_tiled(net, blob, region=region, tiles_per_call=a.tiles_per_call, reduce=a.reduce, **kw)
        else:
            img = codec.decode_images(net, [blob], reduce=a.reduce, **kw)[0]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        grey = img.shape[2] == 1                                # a chroma=400 container: mode L
        depth = inner.get("base", inner).get("depth", 8)
        if depth != 8:
            save_deep(a.dst, img, depth)
        else:
            Image.fromarray(img[..., 0].numpy() if grey else img.numpy()).save(a.dst)
        print("decoded %dx%d%s: %.3f s" % (img.shape[1], img.shape[0], " (greyscale)" if grey else "", dt))
        if a.compare is not None:
            if grey:
                print("--compare: PSNR / MS-SSIM of single-channel images are not defined here", file=sys.stderr)
                return 2
            src = load_deep(a.compare, depth) if depth != 8 else _load_rgb(a.compare)
            if src.shape != img.shape:
                print("--compare: %s is %dx%d, the decoded image %dx%d" % (a.compare, src.shape[1], src.shape[0], img.shape[1],
                                                                         img.shape[0]), file=sys.stderr)
                return 2
            print_quality(src, img.cpu(), depth if depth != 8 else None)
    return 0


if __name__ == "__main__":
    sys.exit(main())
