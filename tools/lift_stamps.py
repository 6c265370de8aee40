#!/usr/bin/env python
"""Diagnostic: in-kernel clock stamps (s_memtime) of the fused lifting step at the level-0 row-pass shape of BASELINE
configs[2]: per-phase cycles of every wave, barrier waits, in-kernel clock.  The kernel writes stamps only when
a stamp buffer is registered through lldwt_set_diagnostics (this tool); a normal run executes none.   python tools/lift_stamps.py

python tools/lift_stamps.py --ab [FILE]: the tile classes (border, top edge, bottom edge, left edge, interior first / continuing)
at the level-0 row-pass shape (256 x 512) and at level 3's (32 x 64: four corner tiles per image, runs of one tile), once with
diagnostics flag 256 (conv2's weight fragments requested at the head of P2, the earlier form) and once without (requested in
six chunks during P1), in one process, two launches per form; written to FILE as JSON if given.

python tools/lift_stamps.py --p2 [FILE]: stamps INSIDE P2 (diagnostics flag 512: kernels of their own, no production launch holds
them) of the interior continuing tiles at the level-0 shape, for both forms: cycles of the first pair, the loop's pair, the
single tile and the tail per wave, the MFMA cycles a wave issues in them, the skew of the waves at P2's barrier and -- on every
second tile row, for the earlier form -- the cycles each k-step of the loop's pair waits for its LDS operands.

python tools/lift_stamps.py --classes [FILE]: the same tile classes and shapes for the library as built, no flag, two launches per
shape, with the launch's span in real time and the in-kernel clock: for comparing two BUILDS (a change that touches code all
diagnostics forms share has no flag to compare against), one process per build, run back to back on one box."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NSTAMP = 32                                    # LF_NSTAMP of csrc/lifting_f16.hip: stamp slots per wave and tile
P2_OLD, P2_STAMPS = 256, 512                   # diagnostics flags: the earlier form of P2; the kernels that stamp inside P2
MFMA_CYCLES = 16                               # v_mfma_f32_16x16x32_f16 on one SIMD
NAMES = ["P0 load+filter", "P0 barrier", "P1 conv1+tanh", "P1 barrier", "P2 conv2+tanh", "P2 barrier",
         "PC composite", "PC barrier", "PC finish+store"]


def stamp(h, w, dbg, P=3, B=8):
    """One stamped launch of a vertical step on P * B images of h x w -> stamps as (Z, tiles_y, tiles_x, 8 waves, 16)."""
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import _lib, ops
    lib = _lib.load()
    dev = "cuda:0"
    torch.manual_seed(0)
    x = torch.rand(P * B, 2 * h, w, device=dev) - 0.5
    ws = [(torch.randn(P, *s, device=dev) * sc) for s, sc in (((16, 1, 5, 5), 0.2), ((16,), 0.1), ((16, 16, 5, 5), 0.05), ((16,), 0.1),
                                                             ((16, 16, 5, 5), 0.05), ((16,), 0.1), ((1, 16, 5, 5), 0.05), ((1,), 0.1))]
    packed = ops.pack_pblock(*ws)
    taps = torch.tensor([0.0, -1.586, -1.586], device=dev).repeat(P, 1).contiguous()
    src = ops.view_of(x, P * B, h, w, offset=0, sz=2 * h * w, sy=2 * w, sx=1)
    din = ops.view_of(x, P * B, h, w, offset=w, sz=2 * h * w, sy=2 * w, sx=1)
    out = torch.empty(P * B, h, w, device=dev)
    dout = ops.view_of(out, P * B, h, w)
    lib.lldwt_set_lift_mode(1)
    gx, gy = (w + 31) // 32, (h + 15) // 16
    st = torch.zeros(gx * gy * P * B, 8, NSTAMP, dtype=torch.int64, device=dev)

    def run():
        ops.lift_step(src, din, dout, P * B, B, h, w, taps, packed, 16, 5, True, 1.0, 0.1)
    try:
        ops.set_diagnostics(0, None, dbg)
        for _ in range(200):                   # warm the clocks under load
            run()
        torch.cuda.synchronize()
        ops.set_diagnostics(0, st, dbg)
        run()
        torch.cuda.synchronize()
    finally:
        ops.set_diagnostics(0, None, 0)
    return st.cpu().numpy().astype(np.int64).reshape(P * B, gy, gx, 8, NSTAMP)


def classes(s, rl):
    """Mean cycles (stamp 0 to stamp 9, mean over waves and tiles) of each class of tile present; rl = the launch's run length."""
    gy, gx = s.shape[1:3]
    ty = np.arange(gy)[:, None] * np.ones((1, gx), int)
    tx = np.ones((gy, 1), int) * np.arange(gx)[None, :]
    inner_x = (tx > 0) & (tx < gx - 1)
    inner = inner_x & (ty > 0) & (ty < gy - 1)
    sel = {"all_tiles": np.ones((gy, gx), bool), "border": ~inner, "top_edge": (ty == 0) & inner_x,
           "bottom_edge": (ty == gy - 1) & inner_x, "left_edge": (tx == 0) & (ty > 0) & (ty < gy - 1),
           "corner": ((ty == 0) | (ty == gy - 1)) & ~inner_x,
           "interior_first_of_run": inner & (ty % rl == 0), "interior_continuing": inner & (ty % rl != 0)}
    out = {}
    for name, m in sel.items():
        if m.any():
            t = s[:, m]
            d = np.diff(t[..., :10], axis=-1)
            out[name] = {"tiles_per_image": int(m.sum()), "total_cycles_mean": float((t[..., 9] - t[..., 0]).mean()),
                         "phases": {n: round(float(d[..., i].mean()), 1) for i, n in enumerate(NAMES)}}
    return out


def ab(path):
    res = {"what": "k_lift_fused_f16<false, 0>, one vertical step on 24 images; cycles from the tile's first stamp to its last, mean "
                   "over the eight waves and the tiles of a class; 'parent_form' = diagnostics flag 256, 'change' = no flag; one process",
           "shapes": {}}
    for key, (h, w, rl) in (("level0_row_pass_256x512", (256, 512, int(os.environ.get("LLDWT_STAMPS_RL", "8")))),
                            ("level3_row_pass_32x64", (32, 64, 1))):
        old, new = classes(stamp(h, w, P2_OLD), rl), classes(stamp(h, w, 0), rl)
        old2, new2 = classes(stamp(h, w, P2_OLD), rl), classes(stamp(h, w, 0), rl)    # a second pair: what the stamps resolve
        res["shapes"][key] = {"run_length": rl, "parent_form": old, "change": new,
                              "total_cycles_mean": {c: {"parent_form": [old[c]["total_cycles_mean"], old2[c]["total_cycles_mean"]],
                                                        "change": [new[c]["total_cycles_mean"], new2[c]["total_cycles_mean"]]}
                                                    for c in old}}
    txt = json.dumps(res, indent=1)
    print(txt)
    if path:
        with open(path, "w") as f:
            f.write(txt + "\n")


def classes_of_build(path):
    res = {"what": "k_lift_fused_f16 as built (no diagnostics flag), one vertical step on 24 images; cycles from the tile's first stamp to "
                   "its last, mean over the eight waves and the tiles of a class; two launches per shape; launch_span_us = last end "
                   "stamp minus first start stamp of the launch (s_memrealtime, 100 MHz)",
           "shapes": {}}
    for key, (h, w, rl) in (("level0_row_pass_256x512", (256, 512, int(os.environ.get("LLDWT_STAMPS_RL", "8")))),
                            ("level3_row_pass_32x64", (32, 64, 1))):
        runs = []
        for _ in range(2):
            s = stamp(h, w, 0)
            c = classes(s, rl)
            real = (s[..., 15] - s[..., 14]).astype(np.float64)
            ok = real > 0
            runs.append({"launch_span_us": float((s[..., 15].max() - s[..., 14].min()) / 100.0),
                         "in_kernel_clock_GHz": float(np.median((s[..., 9] - s[..., 0])[ok] / real[ok]) * 0.1), "classes": c})
        res["shapes"][key] = {"run_length": rl, "launches": runs}
    txt = json.dumps(res, indent=1)
    print(txt)
    if path:
        with open(path, "w") as f:
            f.write(txt + "\n")


def p2_of(s, rl):
    """P2 of the interior continuing tiles of one stamped launch (flag 512), mean over tiles and waves unless named otherwise."""
    gy, gx = s.shape[1:3]
    ty = np.arange(gy)[:, None] * np.ones((1, gx), int)
    tx = np.ones((gy, 1), int) * np.arange(gx)[None, :]
    cont = (tx > 0) & (tx < gx - 1) & (ty > 0) & (ty < gy - 1) & (ty % rl != 0)
    # the earlier form's stamping kernel drains the LDS queue at every k-step head of the loop's pair on odd tile rows (the wait
    # stamps): those rows give the waits, the even rows everything else
    waits = bool((s[:, cont & (ty % 2 == 1)][..., 25] > 0).any())
    t = s[:, cont & (ty % 2 == 0)] if waits else s[:, cont]
    d = lambda i, j: (t[..., i] - t[..., j]).astype(np.float64)
    p2 = d(5, 4)
    out = {"tiles": int(t.shape[0] * t.shape[1]),
           "P2 (stamp 4 to 5)": round(float(p2.mean()), 1),
           "set-up: the wait for the weight fragments, biases (4 to 16)": round(float(d(16, 4).mean()), 1),
           "first pair, no epilogue beside it (16 to 17)": round(float(d(17, 16).mean()), 1),
           "loop pair with the first pair's ten slices (17 to 18)": round(float(d(18, 17).mean()), 1),
           "single tile with the loop pair's ten slices (21 to 22)": round(float(d(22, 21).mean()), 1),
           "tail: the single tile's tanh, split, store (22 to 5)": round(float(d(5, 22).mean()), 1),
           "single tile's share of P2": round(float((d(22, 21) / p2).mean()), 4),
           "MFMA cycles a wave issues in P2 (195 x 16)": 195 * MFMA_CYCLES,
           "MFMA cycles of both waves of a SIMD (the floor)": 2 * 195 * MFMA_CYCLES,
           "MFMA cycles of both waves: a pair / the single tile": [2 * 78 * MFMA_CYCLES, 2 * 39 * MFMA_CYCLES],
           "skew at P2's barrier: last wave minus first, mean over tiles": round(float((t[..., 5].max(-1) - t[..., 5].min(-1)).mean()), 1),
           "P2 barrier wait (5 to 6)": round(float(d(6, 5).mean()), 1),
           "per wave: P2": [round(float(p2[..., k].mean()), 1) for k in range(8)],
           "per wave: P2 barrier wait": [round(float(d(6, 5)[..., k].mean()), 1) for k in range(8)]}
    if not waits:
        return out
    o = s[:, cont & (ty % 2 == 1)]
    n = o[..., 25].astype(np.float64)
    ok = n > 0
    per_pair = o[..., 24][ok] / n[ok]                      # 13 wait stamps per pair
    base = float(np.median(o[..., 26][ok]))                # one wait stamp with nothing in flight
    out["operand waits of the loop pair (odd tile rows)"] = {
        "sum of the 13 wait stamps per pair": round(float(per_pair.mean()), 1),
        "one wait stamp with nothing in flight (median)": base,
        "waited beyond the stamp's own round trip, per pair": round(float(per_pair.mean()) - 13 * base, 1),
        "per wave: sum of the 13 wait stamps": [round(float((o[..., k, 24][ok[..., k]] / n[..., k][ok[..., k]]).mean()), 1) for k in range(8)],
        "loop pair on these rows, with its stamps (17 to 18)": round(float((o[..., 18] - o[..., 17]).mean()), 1)}
    return out


def p2(path):
    h, w, rl = 256, 512, int(os.environ.get("LLDWT_STAMPS_RL", "8"))
    res = {"what": "k_lift_fused_f16<false, 0>, stamps inside P2 (diagnostics flag 512), interior continuing tiles of one vertical step on "
                   "24 images of 256 x 512; cycles per wave; 'parent_form' = flag 256 (weight fragments requested at P2's head), 'change' = during P1; "
                   "two launches per form, one process.  A stamp is fenced and costs cycles: read shares and differences of like with like",
           "run_length": rl, "parent_form": [], "change": []}
    for _ in range(2):
        res["parent_form"].append(p2_of(stamp(h, w, P2_OLD | P2_STAMPS), rl))
        res["change"].append(p2_of(stamp(h, w, P2_STAMPS), rl))
    txt = json.dumps(res, indent=1)
    print(txt)
    if path:
        with open(path, "w") as f:
            f.write(txt + "\n")


def main():
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    if len(sys.argv) > 1 and sys.argv[1] == "--ab":
        return ab(sys.argv[2] if len(sys.argv) > 2 else "")
    if len(sys.argv) > 1 and sys.argv[1] == "--classes":
        return classes_of_build(sys.argv[2] if len(sys.argv) > 2 else "")
    if len(sys.argv) > 1 and sys.argv[1] == "--p2":
        return p2(sys.argv[2] if len(sys.argv) > 2 else "")
    P, B, h, w = 3, 8, 256, 512
    abl = None
    dbg = int(os.environ.get("LLDWT_LF_DBG", "0"))
    s = stamp(h, w, dbg, P, B)
    gx, gy = w // 32, h // 16
    interior = np.zeros((gy, gx), bool)
    interior[1:-1, 1:-1] = True                # y0 >= 2 and y0 + 18 <= h etc: every tile but the frame
    res = {"ablations_interior_mean_cycles": abl}
    si = s[:, interior]                        # (Z, n_int, 8, 16)
    names = NAMES
    d = np.diff(si[..., :10], axis=-1)
    res["interior_mean_cycles_per_wave"] = {n: float(d[..., i].mean()) for i, n in enumerate(names)}
    res["interior_max_over_waves_mean"] = {n: float(d[..., i].max(axis=-1).mean()) for i, n in enumerate(names)}
    tot = si[..., 9] - si[..., 0]
    res["interior_total_cycles_mean"] = float(tot.mean())
    # vertical reuse: with a run length of RL tiles (LLDWT_STAMPS_RL, default 8 at this shape) the tiles at ty % RL == 0 start a
    # run (all 28 / 24 rows of t1 / t2), the others continue one (16 new rows each)
    rl = int(os.environ.get("LLDWT_STAMPS_RL", "8"))
    ty = np.arange(gy)[:, None] * np.ones((1, gx), int)
    for name, sel in (("first_of_run", interior & (ty % rl == 0)), ("continuing", interior & (ty % rl != 0))):
        if sel.any():
            sx_ = s[:, sel]
            dd = np.diff(sx_[..., :10], axis=-1)
            res["interior_%s_mean_cycles_per_wave" % name] = {n: float(dd[..., i].mean()) for i, n in enumerate(names)}
            res["interior_%s_total" % name] = float((sx_[..., 9] - sx_[..., 0]).mean())
    real = (si[..., 15] - si[..., 14]).astype(np.float64)      # 100 MHz ticks
    ok = real > 0
    res["in_kernel_clock_GHz"] = float(np.median(tot[ok] / real[ok]) * 0.1)
    res["wg_duration_us_median"] = float(np.median(real[ok]) / 100.0)
    sb = s[:, ~interior]
    if os.environ.get("LLDWT_LF_DBG", "0") == "16":          # sequential path for every tile
        res["border_total_cycles_mean"] = float((sb[..., 12] - sb[..., 0]).mean())
    else:                                                     # composed path + strip correction: same stamps as interior tiles
        db = np.diff(sb[..., :10], axis=-1)
        res["border_mean_cycles_per_wave"] = {n: float(db[..., i].mean()) for i, n in enumerate(names)}
        res["border_total_cycles_mean"] = float((sb[..., 9] - sb[..., 0]).mean())
        edge = np.zeros((gy, gx), bool)
        edge[0, 1:-1] = True
        se = s[:, edge]
        res["top_edge_total_cycles_mean"] = float((se[..., 9] - se[..., 0]).mean())
        res["top_edge_finish"] = float((se[..., 9] - se[..., 8]).mean())
        edge[:] = False
        edge[1:-1, 0] = True
        se = s[:, edge]
        res["left_edge_total_cycles_mean"] = float((se[..., 9] - se[..., 0]).mean())
        res["left_edge_finish"] = float((se[..., 9] - se[..., 8]).mean())
        res["left_edge_PC+strips"] = float((se[..., 7] - se[..., 6]).mean())
    # the span of the launch in real time and the number of workgroups resident at once
    t0, t1 = s[..., 14].min(), s[..., 15].max()
    res["launch_span_us"] = float((t1 - t0) / 100.0)
    res["sum_wg_duration_over_span_per_cu"] = float(((s[..., 0, 15] - s[..., 0, 14]).sum() / 100.0) / ((t1 - t0) / 100.0) / 256)
    # per-CU timeline: gap between a workgroup's end and the next one's start on the same CU
    hw = s[..., 0, 13].reshape(-1)
    xcc, cu, se = (hw >> 32) & 0xF, (hw >> 8) & 0xF, (hw >> 13) & 0x7
    key = (xcc * 8 + se) * 16 + cu
    t_start, t_end = s[..., 0, 14].reshape(-1), s[..., :, 15].max(axis=-1).reshape(-1)
    gaps, per_cu = [], []
    for k in np.unique(key):
        m = key == k
        o = np.argsort(t_start[m])
        ts, te = t_start[m][o], t_end[m][o]
        gaps.extend(((ts[1:] - te[:-1]) / 100.0).tolist())
        per_cu.append(int(m.sum()))
    res["distinct_cus"] = int(len(np.unique(key)))
    res["wgs_per_cu_min_max"] = [min(per_cu), max(per_cu)]
    res["gap_us_between_wgs_on_a_cu"] = {"median": float(np.median(gaps)), "mean": float(np.mean(gaps)),
                                         "p90": float(np.percentile(gaps, 90))}
    res["first_start_spread_us"] = float((np.sort(t_start)[255] - t_start.min()) / 100.0)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
