"""Wall time of coding one 3x512x512 image with each coded entropy layer: compress + decompress from the strings.

    python tools/time_coding.py [--step q] [--rdo R]

--step q (default 1, the trained operating point): the quantisation step of DESIGN.md 7.1.6.  At 1 the timed call is
net.compress(x), as this tool has always done; at any other step it is encode_strings_planes(step=q) followed by
decode_strings_planes(step=q), the same two halves with the step passed down.
--rdo R: the encoder half with rate-distortion optimised quantisation at the Lagrangian R = m / 64, through
the two halves as well; the decoder half is the same call as without it."""
import argparse
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import (  # noqa: E402
    LiftingBasedDWTNetWrapper, byte_extractor, decode_strings_planes, encode_strings_planes)
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--step", type=float, default=1.0)
ap.add_argument("--rdo", type=float, default=None)
a = ap.parse_args()


def code(net, x):
    if a.step == 1.0 and not a.rdo:
        return net.compress(x)
    B, _, H, W = x.shape
    x_pm = x.permute(1, 0, 2, 3).unsqueeze(2).contiguous()
    s_xe, s_xo = encode_strings_planes(net.nets(), x_pm, step=a.step, rdo=a.rdo)
    xhat = decode_strings_planes(net.nets(), s_xe, s_xo, H, W, B, step=a.step)
    len_xe = sum(byte_extractor(row) for row in s_xe)
    len_xo = sum(byte_extractor(row) for level in s_xo for row in level)
    return xhat, len_xe * 8 / (B * H * W), len_xo * 8 / (B * H * W)


for ent in ("conditioned2ZTsepSubbands", "onlyEZWT", "DWTConditioned2EntropyLayerZTBlock"):
    cfg = make_config(dwtlevels=4, mode="validate", entropy_layer=ent)
    torch.manual_seed(0)
    net = LiftingBasedDWTNetWrapper(cfg).to("cuda:0").eval()
    x = torch.rand(1, 3, 512, 512, device="cuda:0")
    with torch.no_grad():
        code(net, x[:, :, :64, :64])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        xhat, bxe, bxo = code(net, x)
        torch.cuda.synchronize()
        print(ent, "compress+decompress of one 3x512x512 image%s: %.2f s, %.3f bpp"
              % (("" if a.step == 1.0 else " at step %g" % a.step) + (" with rdo %g" % a.rdo if a.rdo else ""), time.perf_counter() - t0, float(bxe + bxo)))
