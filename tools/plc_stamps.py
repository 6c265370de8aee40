#!/usr/bin/env python
"""Diagnostic: in-kernel clock stamps (s_memtime) of the fused tree-context pair (k_conv3_f16x3<2>) at the level-0 shape of
BASELINE configs[2] (3 planes x 8 images, parent 128 x 128 -> 243 channels at 256 x 256).  The kernel writes stamps only
when a stamp buffer is registered through lldwt_set_diagnostics (this tool).  Three legs: the kernel as it is (one workgroup per
pixel tile that loops over the tile's channel blocks, where the host's rule folds the launch), k_plc_wino with one workgroup per
(tile, channel block) (diagnostics flag 2) and in its earlier form (flag 1); per leg the prologue (k_plc_wino: in four parts), the
cycles per 32 channels and per chunk and what of them is not matrix time, the epilogue, the in-kernel clock and the workgroup's
cycles.  A folded leg reports pass 0 and the later passes apart (a pass stamps into the slots of its channel block, so the buffer
has one layout in every leg), and their sum per tile.   python tools/plc_stamps.py"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    dev = "cuda:0"
    P, B, C, S = 3, 8, 243, 256
    torch.manual_seed(0)
    parent = torch.randn(P, B, 3, S // 2, S // 2, device=dev).round_()
    w1 = (torch.rand(P, C, 3, 3, 3, device=dev) - 0.5) * 0.4
    b1 = torch.rand(P, C, device=dev) - 0.5
    w2 = (torch.rand(P, C, C, 3, 3, device=dev) - 0.5) * 0.04
    b2 = torch.rand(P, C, device=dev) - 0.5
    pk1 = ops.plc_fused_pack1(w1, b1)
    pk2 = ops.conv_f16x3_pack(w2)

    def run():
        return ops.plc_fused(parent, pk1, pk2, b2, C, C)
    nwg = (S // 32) * (S // 8) * 2 * P * B
    wino = ops.plc_algo() == "winograd"
    # matrix cycles of 32 channels: the direct kernel's 36 x 12 MFMAs of 32 cycles + 18 of the first conv; k_plc_wino's two
    # 16-channel chunks of 144 x 32 + the first conv's 16x16x32 MFMAs of 16 cycles (21 per chunk, 36 in the earlier form)
    def matrix_cycles(flags):
        return 2 * (144 * 32 + (36 if flags & 1 else 21) * 16) if wino else 36 * 12 * 32 + 18 * 32

    def leg(flags):
        for _ in range(100):
            run()
        torch.cuda.synchronize()
        st = torch.zeros(nwg, 4, 16, dtype=torch.int64, device=dev)
        ops.set_diagnostics(1, st, flags=flags)
        try:
            run()
            torch.cuda.synchronize()
        finally:
            ops.set_diagnostics(1, None)
        s = st.cpu().numpy().astype(np.int64)
        matrix = matrix_cycles(flags)
        res = {"workgroups": nwg, "algo": ops.plc_algo(), "flags": flags}
        # [image][channel block][tile][wave][slot]; folded: channel block 1 of a tile is a later pass, with next to no prologue (its
        # start time says nothing: unfolded, a tile's second workgroup is dispatched a round later, as its first one ends)
        s5 = s.reshape(P * B, 2, nwg // (2 * P * B), 4, 16)
        folded = bool(wino and (s5[:, 1, ..., 1] - s5[:, 1, ..., 0]).mean() < 0.25 * (s5[:, 0, ..., 1] - s5[:, 0, ..., 0]).mean())
        res["folded"] = folded
        if folded:
            def part(x):
                pro = np.diff(x[..., [0, 12, 13, 2, 1]], axis=-1).mean(axis=tuple(range(x.ndim - 1)))
                ch = np.diff(x[..., [1, 3, 4, 5, 6, 7, 8, 9, 10]], axis=-1).mean(axis=tuple(range(x.ndim - 1)))
                return {"prologue": float((x[..., 1] - x[..., 0]).mean()),
                        "prologue_parts": {"parent patch + abs-max": float(pro[0]), "im2col": float(pro[1]),
                                           "wait at the im2col barrier": float(pro[2]), "chunk-0 rows / zeroing + barrier": float(pro[3])},
                        "per_16_channel_chunk": float(ch.mean()) / 2, "epilogue": float((x[..., 11] - x[..., 10]).mean()),
                        "pass_total": float((x[..., 11] - x[..., 0]).mean()),
                        "pass_us_median": float(np.median(x[..., 15] - x[..., 14]) / 100.0)}
            res["passes"] = {"pass 0": part(s5[:, 0]), "later passes": part(s5[:, 1:])}
            res["passes"]["between the passes (stamp 11 of a pass to stamp 0 of the next)"] = float((s5[:, 1, ..., 0] - s5[:, 0, ..., 11]).mean())
            res["passes"]["sum over a tile's passes (stamp 0 of pass 0 to stamp 11 of the last)"] = float((s5[:, 1, ..., 11] - s5[:, 0, ..., 0]).mean())
            res["tile_us_median"] = float(np.median(s5[:, 1, ..., 15] - s5[:, 0, ..., 14]) / 100.0)
        if wino:
            # k_plc_wino: slot 1 at the loop's entry, slots 3 .. 9 at its chunks 2, 4 .. 14, slot 10 behind the loop: eight spans of
            # two 16-channel chunks.  Slots 12, 13, 2 split the prologue (0 .. 1) into four parts
            t = s[..., [1, 3, 4, 5, 6, 7, 8, 9, 10]]
            chunks = [float(v) for v in np.diff(t, axis=-1).mean(axis=(0, 1))]
            pro = s[..., [0, 12, 13, 2, 1]]
            parts = np.diff(pro, axis=-1).mean(axis=(0, 1))
            res["mean_cycles_per_wave"] = {
                "prologue": float((s[..., 1] - s[..., 0]).mean()),
                "prologue_parts": {"parent patch + abs-max": float(parts[0]), "im2col": float(parts[1]),
                                   "wait at the im2col barrier": float(parts[2]), "chunk-0 rows + barrier": float(parts[3])},
                "chunks": chunks, "epilogue": float((s[..., 11] - s[..., 10]).mean())}
            res["cycles_per_16_channel_chunk"] = float(np.mean(chunks)) / 2
            res["cycles_per_chunk_outside_the_144_main_mfmas"] = float(np.mean(chunks)) / 2 - 144 * 32
            per32 = float(np.mean(chunks))
        else:
            # the direct kernel stamps each of its eight 32-channel chunks at its start (slot 2 right behind slot 1)
            d = np.diff(s[..., :12], axis=-1)
            chunks = [float(d[..., 1 + i].mean()) for i in range(8)]
            res["mean_cycles_per_wave"] = {"prologue": float(d[..., 0].mean()), "chunks": chunks,
                                           "last chunk -> loop end": float(d[..., 9].mean()), "epilogue": float(d[..., 10].mean())}
            per32 = float(np.mean(chunks[1:]))
        res["matrix_cycles_per_32_channels"] = matrix
        res["cycles_per_32_channels"] = per32
        res["non_matrix_cycles_per_32_channels"] = per32 - matrix
        tot = s[..., 11] - s[..., 0]
        real = (s[..., 15] - s[..., 14]).astype(np.float64)
        ok = real > 0
        res["total_cycles_mean"] = float(tot.mean())
        res["in_kernel_clock_GHz"] = float(np.median(tot[ok] / real[ok]) * 0.1)
        res["wg_duration_us_median"] = float(np.median(real[ok]) / 100.0)
        t0, t1 = s[..., 14].min(), s[..., 15].max()
        res["launch_span_us"] = float((t1 - t0) / 100.0)
        res["sum_wg_duration_over_span_per_cu"] = float(((s[:, 0, 15] - s[:, 0, 14]).sum() / 100.0) / ((t1 - t0) / 100.0) / 256)
        # the CU time of the launch that no workgroup's stamps 14 .. 15 cover, per workgroup started (per tile when folded): start, end
        # and the last, partly filled round together -- an upper bound on the gap between two workgroups on a CU
        started = nwg // 2 if folded else nwg
        res["uncovered_cu_us_per_workgroup_started"] = float((256 * (t1 - t0) - (s[:, 0, 15] - s[:, 0, 14]).sum()) / 100.0 / started)
        res["wave_skew_at_loop_end_cycles"] = float((s[..., 10].max(axis=-1) - s[..., 10].min(axis=-1)).mean())
        return res

    # the current form, then (diagnostics flag 1) k_plc_wino in its earlier form: the A/B leg.  The direct kernel has one form
    legs = {"current": leg(0)}
    if wino:
        legs["one workgroup per channel block (flag 2)"] = leg(2)
        legs["earlier (flag 1)"] = leg(1)
    for name, r in legs.items():
        if r.get("folded"):
            for pn in ("pass 0", "later passes"):
                q = r["passes"][pn]
                print("%-18s %-12s prologue %6.0f  per chunk %6.0f  epilogue %6.0f  pass %7.0f cycles" % (
                    name, pn, q["prologue"], q["per_16_channel_chunk"], q["epilogue"], q["pass_total"]), file=sys.stderr)
        if wino:
            pp = r["mean_cycles_per_wave"]["prologue_parts"]
            print("%-18s prologue parts: %s; per 16-channel chunk %.0f (outside the 144 main MFMAs %.0f)" % (
                name, ", ".join("%s %.0f" % kv for kv in pp.items()), r["cycles_per_16_channel_chunk"],
                r["cycles_per_chunk_outside_the_144_main_mfmas"]), file=sys.stderr)
        print("%-18s prologue %7.0f  per 32 channels %7.0f (non-matrix %6.0f)  epilogue %7.0f  workgroup %7.0f cycles  %.3f GHz" % (
            name, r["mean_cycles_per_wave"]["prologue"], r["cycles_per_32_channels"], r["non_matrix_cycles_per_32_channels"],
            r["mean_cycles_per_wave"]["epilogue"], r["total_cycles_mean"], r["in_kernel_clock_GHz"]), file=sys.stderr)
    print(json.dumps(legs, indent=1))

if __name__ == "__main__":
    main()
