"""Generates tests/golden/lift_step_digests.json: the bits of the fused lifting step (k_lift_fused_f16, eval path), pinned as one
sha256 over the output tensor's fp32 bytes per case.  The diagnostics forms of the kernel share its source, so none of them can
serve as the reference for a change to that source; this file is recorded at the commit BEFORE such a change and the test
recomputes it after.  Needs the GPU; run by hand:

    python tests/golden/make_lift_digests.py [--out FILE] [--commit HASH]

Step cases launch ops.lift_step with the weights and inputs of tests/test_gpu_lift_conv2_sched.py (P = 2 planes of seeded fills,
inputs in [-1, 1], one constant image at 48 x 64):
  shapes 16x32, 32x64, 48x64, 48x96 (a tile that is interior AND continues a run), 41x70 (the image ends inside the last tiles);
  both orientations; the three precision modes; diagnostics flags 0 and 32 (no hand-down: runs of one tile);
  batch 2 (fewer tiles than CUs: every tile starts a run) and the smallest batch at which the dispatch's cost rule takes the whole
  column as one run, computed from the device's CU count as the scheduling test computes it (one batch where the two coincide).
Level cases launch ops.lifting_forward, one level on 2 x 1 x 64 x 64 per plane: the row pass and the paired L / H column launch;
the digest runs over ll and then yh.
The batch of the one-run cases, and with it the case names, depend on the CU count: the file records it and the test asserts it.
``cases()`` and ``run()`` are what tests/test_gpu_lift_issue_bits.py recomputes, so the inputs are defined once, here.  The file
also names the commit it was generated at and the git blob id of csrc/lifting_f16.hip at that commit (--commit: for a run in a
copy of the tree without its .git)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for _p in (REPO, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PKG = "imagecompressionlearnedliftingandlearnedtreebasedmodels_amd"
OUT = os.path.join(HERE, "lift_step_digests.json")
PINNED = PKG + "/csrc/lifting_f16.hip"
P, C = 2, 16
NO_REUSE = 32
PRECISIONS = ("f16x3", "fp16", "bf16")
STEP_OF = {1: (1, (0, 1)), 0: (2, (1, 0))}          # by `vertical`: tap index, (block, pack index)
SHAPES = [(16, 32), (32, 64), (48, 64), (48, 96), (41, 70)]
CONSTANT_SHAPE = (48, 64)
LEVEL_SHAPE = (2, 64, 64)                            # B, H, W per plane
_cache = {}


def cu_count():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def dispatch_run_length(Z, h, w, ncu):
    """The cost rule of lift_f16_launch (composed path): the longest run that still fills whole rounds."""
    cdiv = lambda a, b: -(-a // b)
    tiles_x, tiles_y = cdiv(w, 32), cdiv(h, 16)
    best, best_rl = 1e30, 1
    for rl in range(1, tiles_y + 1):
        cost = cdiv(Z * tiles_x * cdiv(tiles_y, rl), ncu) * (1.0 + 0.8 * (rl - 1))
        if cost < best - 1e-9:
            best, best_rl = cost, rl
    return best_rl


def batch_for_whole_column_runs(h, w, ncu):
    tiles_y = -(-h // 16)
    for batch in range(2, 1025):
        if dispatch_run_length(P * batch, h, w, ncu) == tiles_y:
            return batch
    raise AssertionError("no batch up to 1024 makes the dispatch take runs of %d tiles at %dx%d on %d CUs" % (tiles_y, h, w, ncu))


def cases(ncu=None):
    """-> list of (name, kind, h, w, vertical, batch, flags, precision, constant); kind 'step' or 'level'."""
    ncu = ncu or cu_count()
    out = []
    for (h, w), constant in [(s, False) for s in SHAPES] + [(CONSTANT_SHAPE, True)]:
        for vertical in (1, 0):
            for batch in sorted({2, batch_for_whole_column_runs(h, w, ncu)}):
                for flags in (0, NO_REUSE):
                    for prec in PRECISIONS:
                        name = "step%s/%dx%d/v%d/b%d/f%d/%s" % ("_const" if constant else "", h, w, vertical, batch, flags, prec)
                        out.append((name, "step", h, w, vertical, batch, flags, prec, constant))
    B, H, W = LEVEL_SHAPE
    out += [("level/%dx%dx%d/%s" % (B, H, W, prec), "level", H, W, 1, B, 0, prec, False) for prec in PRECISIONS]
    return out


def _weights():
    if "w" not in _cache:
        import gpu_util
        from helpers import filled
        from oracle import model, weights
        cfg = dict(model.DEFAULT_CFG, filtersize=5, dwtlevels=1)
        sds = [filled(weights.autoencoder_template(cfg), "c2s%d." % p) for p in range(P)]
        _cache["w"] = gpu_util.lifting_params(sds)
    return _cache["w"]


def inputs(kind, h, w, vertical, batch, constant):
    """Host tensors of a case, built once and never modified: (src, dst) of a step, (x,) of a level."""
    key = (kind, h, w, vertical, batch, constant)
    if key not in _cache:
        if kind == "level":
            g = torch.Generator().manual_seed(4100 + h + w)
            _cache[key] = (2.0 * torch.rand(P, batch, 1, h, w, generator=g) - 1.0,)
        elif constant:
            _cache[key] = (torch.full((P, batch, 1, h, w), 1.0), torch.full((P, batch, 1, h, w), -1.0))
        else:
            g = torch.Generator().manual_seed(9000 + 131 * h + w + 7 * vertical + batch)
            src = 2.0 * torch.rand(P, batch, 1, h, w, generator=g) - 1.0
            dst = 2.0 * torch.rand(P, batch, 1, h, w, generator=g) - 1.0
            _cache[key] = (src, dst)
    return _cache[key]


def run(case):
    """-> (outputs, given): host tensors the case computed, in the order of the digest, and the host tensor each one is to differ
    from (the step's dst_in; the level's input at the outputs' sampling)."""
    import gpu_util as gu
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    name, kind, h, w, vertical, batch, flags, prec, constant = case
    taps, packed = _weights()
    before = ops.get_precision()
    try:
        ops.set_precision(prec)
        ops.set_diagnostics(0, None, flags)
        if kind == "level":
            x, = inputs(kind, h, w, vertical, batch, constant)
            ll, yh = ops.lifting_forward(gu.dev(x), taps, packed, 1, C, 5, 0.1)
            torch.cuda.synchronize()
            sub = x[..., 0::2, 0::2]
            return [ll.cpu(), yh[0].cpu()], [sub, sub.expand(-1, -1, 3, -1, -1)]
        src, dst = inputs(kind, h, w, vertical, batch, constant)
        j, (blk, u) = STEP_OF[vertical]
        src_d, dst_d = gu.dev(src), gu.dev(dst)
        out_d = torch.empty_like(dst_d)
        Z = P * batch
        v = lambda t: ops.view_of(t, Z, h, w)
        ops.lift_step(v(src_d), v(dst_d), v(out_d), Z, batch, h, w, taps[j].contiguous(), packed[:, blk, u].contiguous(), C, 5,
                      vertical, 1.0, 0.1)
        torch.cuda.synchronize()
        return [out_d.cpu()], [dst]
    finally:
        ops.set_diagnostics(0, None, 0)
        ops.set_precision(before)


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        assert t.dtype == torch.float32
        h.update(t.contiguous().numpy().tobytes())
    return h.hexdigest()


def _blob_id(path):
    """git hash-object of a file."""
    with open(path, "rb") as f:
        data = f.read()
    return hashlib.sha1(b"blob %d\0" % len(data) + data).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--commit", default=None, help="git rev-parse HEAD, for a run in a copy of the tree without its .git")
    a = ap.parse_args()
    commit = a.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=REPO).decode().strip()
    out = dict(provenance=dict(commit=commit, blobs={PINNED: _blob_id(os.path.join(REPO, PINNED))}, cu_count=cu_count()), cases={})
    for case in cases():
        outs, given = run(case)
        assert all(bool(torch.isfinite(t).all()) for t in outs), case[0]
        assert all(not torch.equal(t, g) for t, g in zip(outs, given)), case[0]
        out["cases"][case[0]] = digest(outs)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("ok", len(out["cases"]), "cases, CUs:", out["provenance"]["cu_count"])


if __name__ == "__main__":
    main()
