#!/usr/bin/env python
"""Diagnostic: in-kernel clock stamps of the cgp register-chain kernel (k_cgp16), persistent and streaming forms, at the
level-0 shape of BASELINE configs[2] (3 planes x 8 images x 3 subbands of 256 x 256).   python tools/cgp_stamps.py"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    dev = "cuda:0"
    P, B, G, S = 3, 8, 3, 256
    torch.manual_seed(0)
    c = [93, 162, 54, 18, 2]
    ws = [(torch.randn(P, G * c[i + 1], c[i], 1, 1, device=dev) / c[i] ** 0.5) for i in range(4)]
    bs = [torch.randn(P, G * c[i + 1], device=dev) * 0.1 for i in range(4)]
    packed16 = ops.cgp16_pack(ws, bs, G)
    plc = torch.randn(P, B, G * 81, S, S, device=dev)
    xq = torch.randn(P, B, G, S, S, device=dev).round_()
    tap_bits = 0b0000000000000_11_11111_11111          # the 12 causal taps of the 5x5 type-A mask

    def run():
        return ops.cgp16_params(plc, xq, packed16, 5, tap_bits)
    for _ in range(30):
        run()
    torch.cuda.synchronize()
    res = {}
    # ---- the persistent form (the default at this size): per wave [workgroup][wave][8], see CGP_PSTAMP in csrc/cgp_f16x3.hip
    for name, flags, nw in (("persistent", 2 << 2, 12),):
        st = torch.zeros(1024, nw, 8, dtype=torch.int64, device=dev)       # at least one workgroup per CU
        ops.set_diagnostics(2, st, flags)
        run()
        torch.cuda.synchronize()
        ops.set_diagnostics(2, None)
        s = st.cpu().numpy().astype(np.int64).reshape(-1, 8)
        s = s[s[:, 5] > 0]                                                 # waves that ran blocks
        blocks = s[:, 5].astype(np.float64)
        total = (s[:, 2] + s[:, 3] + s[:, 4]).astype(np.float64)
        real = (s[:, 7] - s[:, 6]).astype(np.float64)
        r = {"waves": int(s.shape[0]), "blocks": int(blocks.sum()), "blocks_per_wave_min_max": [int(blocks.min()), int(blocks.max())],
             "prologue_cycles_mean (weights of the pair into LDS, barrier)": float((s[:, 1] - s[:, 0]).mean()),
             "cycles_per_block": {"input wait + |max| + split": float(s[:, 2].sum() / blocks.sum()),
                                  "layers 0 + 1 (60 weight steps, 180 MFMAs)": float(s[:, 3].sum() / blocks.sum()),
                                  "layers 2 + 3 + store": float(s[:, 4].sum() / blocks.sum())},
             "cycles_per_block_total": float(total.sum() / blocks.sum()),
             "ideal_mfma_cycles_per_block": 66 * 3 * 32,
             "in_kernel_clock_GHz": float(np.median((total + s[:, 1] - s[:, 0]) / real) * 0.1),
             "launch_span_us": float((s[:, 7].max() - s[:, 6].min()) / 100.0)}
        res[name] = r
    # ---- the streaming form: [z][group][column][8]
    cols = S * S // 32
    st = torch.zeros(P * B, G, cols, 8, dtype=torch.int64, device=dev)
    ops.set_diagnostics(2, st, 1 << 2)
    run()
    torch.cuda.synchronize()
    ops.set_diagnostics(2, None)
    s = st.cpu().numpy().astype(np.int64)
    d = np.diff(s[..., :6], axis=-1)
    names = ["inputs (48 loads per lane per block) + |max|", "layers 0 + 1 (60 weight steps, 180 MFMAs)", "layer 2", "layer 3", "store"]
    rs = {"mean_cycles_per_wave": {n: float(d[..., i].mean()) for i, n in enumerate(names)}}
    tot = s[..., 5] - s[..., 0]
    real = (s[..., 7] - s[..., 6]).astype(np.float64)
    ok = real > 0
    rs["total_cycles_mean"] = float(tot.mean())
    rs["ideal_mfma_cycles"] = 66 * 3 * 32
    rs["in_kernel_clock_GHz"] = float(np.median(tot[ok] / real[ok]) * 0.1)
    t0, t1 = s[..., 6].min(), s[..., 7].max()
    rs["launch_span_us"] = float((t1 - t0) / 100.0)
    rs["waves"] = int(s[..., 0].size)
    rs["mean_wave_duration_us"] = float(real[ok].mean() / 100.0)
    rs["resident_waves_estimate"] = float(real[ok].sum() / (t1 - t0))
    res["streaming"] = rs
    print(json.dumps(res, indent=1))

if __name__ == "__main__":
    main()
