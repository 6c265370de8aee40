"""Generates tests/golden/streams_n1.json: the bytes the three coded entropy layers write from the filled weights, pinned as
digests (n1: codec.CODING_NUMERICS_VERSION; a change that bumps it regenerates the file).  Needs the GPU; run by hand:

    python tests/golden/make_streams.py [--out FILE] [--commit HASH]

Inputs: helpers.filled(weights.wrapper_template(cfg)) as tests/test_gpu_coding.py builds its layers, coefficients drawn on the
CPU from a seeded torch.Generator and fed straight to compress_planes (no transform), the default precision mode.
  shape A: L=3, B=2, 64x48 -- not square, two images, two tree levels above the coarsest;
  shape B: L=3, B=1, 32x8  -- tree levels 16x4 and 8x2 and a 4x1 coarsest level: wavefront steps without a pixel at slope 3
           (the 8x2 level) and at slope 2 (the crop stacks).
Recorded per case: the sha256 over all streams, each prefixed by its length as 4 bytes little endian, xe[p][b] and then the
levels finest first, each [p][b]; and the sha256 over the fp32 bytes of xe_q and every xo_q, finest first.  A case of the
estimating sink records its list of byte counts in place of the first digest.  ``cases()`` and ``run()`` are what
tests/test_gpu_stream_digests.py recomputes, so the inputs are defined once, here.
The file also names the commit it was generated at and the git blob ids of the two modules whose output it pins (--commit: for a
run in a copy of the tree without its .git)."""
import argparse
import hashlib
import json
import os
import struct
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for _p in (REPO, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PKG = "imagecompressionlearnedliftingandlearnedtreebasedmodels_amd"
OUT = os.path.join(HERE, "streams_n1.json")
PINNED = (PKG + "/graphs/models/entropy_coding.py", PKG + "/graphs/models/LiftingBasedDWT_net.py")
DEV = "cuda:0"
L = 3
SHAPES = {"A": (2, 64, 48), "B": (1, 32, 8)}                       # B, H, W
LAYERS = {"cond2": "conditioned2ZTsepSubbands", "ezwt": "onlyEZWT", "ztblock": "DWTConditioned2EntropyLayerZTBlock"}
STEP, RDO = 23 / 16, 13 / 64
MAP_VALUES = (8, 16, 23, 40)
GAIN = 12.0
VARIANTS = {"plain": {}, "step": dict(step=STEP), "step_rdo": dict(step=STEP, rdo=RDO), "map": dict(step="map"),
            "map_rdo": dict(step="map", rdo=RDO)}
GENERIC_LEVEL = 1                                                   # the level of shape A that the generic cases code
_NETS = {}


def cases():
    """-> list of (name, layer key, shape key, coder, variant key); layer "generic": one level on code_tree_level_generic."""
    out = []
    for layer in LAYERS:
        for coder in ("host", "gpu"):
            out += [("A/%s/%s/%s" % (layer, coder, v), layer, "A", coder, v) for v in VARIANTS]
    for coder in ("host", "gpu"):
        out += [("B/cond2/%s/%s" % (coder, v), "cond2", "B", coder, v) for v in ("plain", "map")]
    out += [("A/generic/host/%s" % v, "generic", "A", "host", v) for v in ("step_rdo", "map")]
    out += [("A/%s/estimate/step_rdo" % layer, layer, "A", "estimate", "step_rdo") for layer in LAYERS]
    return out


def _entropy_models(layer):
    """The entropy layer of every plane, from the filled weights (tests/test_gpu_coding.py::_layers)."""
    if layer not in _NETS:
        from helpers import filled
        from oracle import weights
        from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
            LiftingBasedDWTNetWrapper
        from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
        cfg = make_config(dwtlevels=L, mode="validate", entropy_layer=LAYERS[layer])
        net = LiftingBasedDWTNetWrapper(cfg)
        net.load_state_dict(filled(weights.wrapper_template(dict(cfg))), strict=False)
        _NETS[layer] = net.to(DEV).eval()
    return [n.entropymodel for n in _NETS[layer].nets()]


def coefficients(shape):
    """tests/test_gpu_coding.py::_coefs_hw -> (xe, [xo] finest first) on the device."""
    B, H, W = SHAPES[shape]
    g = torch.Generator().manual_seed(1000 + H + W)
    xe = (torch.rand(3, B, 1, H >> L, W >> L, generator=g) - 0.5) * GAIN
    xo = [(torch.rand(3, B, 3, H >> (i + 1), W >> (i + 1), generator=g) - 0.5) * GAIN for i in range(L)]
    return xe.to(DEV), [t.to(DEV) for t in xo]


def step_map(shape):
    """(B, H >> L, W >> L) int32 drawn from MAP_VALUES."""
    B, H, W = SHAPES[shape]
    g = torch.Generator().manual_seed(77 + H)
    return torch.tensor(MAP_VALUES, dtype=torch.int32)[torch.randint(0, len(MAP_VALUES), (B, H >> L, W >> L), generator=g)]


def run(case):
    """-> (streams, tensors, decode): the flat stream list in the recorded order, [xe_q] + [xo_q] finest first, and
    decode(first_level) -> the decoder's tensors in the same order (None where the case has no such decode)."""
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models import entropy_coding as ec
    name, layer, shape, coder, variant = case
    kw = dict(VARIANTS[variant])
    if kw.get("step") == "map":
        kw["step"] = step_map(shape)
    xe, xo = coefficients(shape)
    flat = lambda rows: [s for row in rows for s in row]
    if layer == "generic":
        em = _entropy_models("cond2")
        Layer = type(em[0])
        tabs, _ = Layer._coding_setup(em)
        i = GENERIC_LEVEL
        if isinstance(kw.get("step"), torch.Tensor):
            kw["step"] = ops.StepMap(ops.step_map_pairs(kw["step"], DEV), L - 1 - i)
        with torch.no_grad():
            plc, packed, dims, K, bits = Layer._tree_context(em, i, xo[i + 1], 3)
            em_i = [l.ent_out_xo_list[i] for l in em]
            gen = lambda y, strings, **k: ec.code_tree_level_generic(em_i, plc, packed[0], dims, K, bits, y, xo[i].shape, tabs,
                                                                     strings, coder=coder, **k)
            s, q = gen(xo[i], None, **kw)
            return flat(s), [q], lambda first_level: [gen(None, s, step=kw["step"])[1]] if first_level == 0 else None
    em = _entropy_models(layer)
    Layer = type(em[0])
    s_xe, s_xo, xe_q, xo_q = Layer.compress_planes(em, xe, xo, coder=ec.ESTIMATE if coder == "estimate" else coder, **kw)

    def decode(first_level):
        if coder == "estimate":
            return None
        d_xe, d_xo = Layer.decompress_planes(em, s_xe, s_xo, xe.shape, [t.shape for t in xo], coder=coder,
                                             first_level=first_level, step=kw.get("step", 1.0))
        return [d_xe] + d_xo
    return flat(s_xe) + [s for lv in s_xo for s in flat(lv)], [xe_q] + xo_q, decode


def record(streams, tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().float().cpu().contiguous().numpy().tobytes())
    out = dict(values=h.hexdigest())
    if streams and isinstance(streams[0], int):
        out["estimate"] = [int(v) for v in streams]
        return out
    h = hashlib.sha256()
    for s in streams:
        h.update(struct.pack("<I", len(s)) + bytes(s))
    return dict(out, streams=h.hexdigest(), bytes=sum(len(s) for s in streams))


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
    out = dict(provenance=dict(commit=commit, blobs={p: _blob_id(os.path.join(REPO, p)) for p in PINNED}), cases={})
    for case in cases():
        streams, tensors, _ = run(case)
        out["cases"][case[0]] = record(streams, tensors)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("ok", len(out["cases"]), "cases")


if __name__ == "__main__":
    main()
