"""Times lldwt_ztblock_phase (the ZTBlock coder's fused phase kernel) per (level, phase) at the BASELINE batch (8x3x512x512,
4 levels: phase grids 32x32, 64x64, 128x128): HIP-event time per launch and achieved fp32 TF/s against the 155 TF fp32-MFMA
peak.  FLOPs counted from shapes: 2 x (9k*32 + 9*32*32 + 2*32*32 + 32) per head per phase pixel, two heads, every plane, image
and subband.
  python tools/bench_ztblock.py [batch] [size] [levels]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
S = int(sys.argv[2]) if len(sys.argv) > 2 else 512
L = int(sys.argv[3]) if len(sys.argv) > 3 else 4
P = 3
PEAK_TF = 155.0
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)


def rnd(*shape, scale=1.0):
    return ((torch.rand(*shape, generator=g) - 0.5) * scale).to(dev)


def packed_for(k):
    shapes = [(32, k, 3, 3), (32,), (32, 32, 3, 3), (32,), (32, 32, 1, 1), (32,), (32, 32, 1, 1), (32,), (1, 32, 1, 1), (1,)]
    return ops.ztblock_pack([rnd(P, 3, 2, *s, scale=0.3) for s in shapes])


def time_launch(fn, iters=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


rows = []
packs = {k: packed_for(k) for k in range(1, 5)}
for lev in range(L - 2, -1, -1):                       # coarse to fine, as the coder runs them
    H = S >> (lev + 1)
    h2 = H // 2
    parent = rnd(P, B, 3, h2, h2, scale=8.0)
    level = rnd(P, B, 3, H, H, scale=8.0)
    out = torch.empty(P, B, 6, h2, h2, device=dev)
    for k in range(1, 5):
        ms = time_launch(lambda: ops.ztblock_phase(parent, level, packs[k], k, out=out))
        flops = 2.0 * 2 * (9 * k * 32 + 9 * 32 * 32 + 2 * 32 * 32 + 32) * P * B * 3 * h2 * h2
        tf = flops / (ms * 1e-3) / 1e12
        rows.append({"level": lev, "phase": k, "grid": [h2, h2], "ms": round(ms, 4), "tflops": round(tf, 2),
                     "pct_of_155tf": round(100.0 * tf / PEAK_TF, 1)})
        print("level %d (phase grid %3dx%-3d) phase %d: %8.3f ms  %6.2f TF/s  %5.1f %% of %.0f TF" % (
            lev, h2, h2, k, ms, tf, 100.0 * tf / PEAK_TF, PEAK_TF))
total = sum(r["ms"] for r in rows)
print(json.dumps({"batch": B, "size": S, "levels": L, "total_ms_all_phases": round(total, 3), "rows": rows}))
