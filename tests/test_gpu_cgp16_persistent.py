"""GPU: the persistent form of the context MLP's eval chain (k_cgp16 with the weights of a (plane, group) held in LDS by one
workgroup per CU) against the streaming form (LLDWT_CGP16=stream), through ops.cgp16_params.

Bound: none -- equality.  A block is the same 32 consecutive pixels of one (image, plane, group) in both forms, so the input
maximum, the scales and the bounds are the same numbers, and every accumulator sees its MFMAs in the same order; only where
the weight fragments are read from (LDS or L2) and which wave computes a block differ.  torch.equal on the whole
(sigma, mu) tensor.

The switch is read when the library loads, so the two legs run in fresh child processes (this file, run as a script) on the
same seeded weights and inputs.  The dispatch keeps the streaming form below a block count (the small cases here), so the
persistent kernel is also forced in-process through ops.set_diagnostics at every case and compared with the streaming leg.

Weights are random per (plane, group): a workgroup that loaded another pair's weights fails.
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPS = 0b0000000000000_11_11111_11111          # the 12 causal taps of the 5x5 type-A mask
# name -> (planes, batch, groups, h, w, precision)
CASES = {
    "bench_level0": (3, 8, 3, 256, 256, "f16x3"),
    "bench_level1": (3, 8, 3, 128, 128, "f16x3"),
    "bench_level2": (3, 8, 3, 64, 64, "f16x3"),
    "hw_not_multiple_of_32": (2, 2, 3, 37, 53, "f16x3"),       # 1961 pixels: the last block has 9
    "fewer_blocks_than_waves": (3, 1, 3, 8, 8, "f16x3"),       # 2 blocks per pair, 18 in all
    "one_plane_one_image": (1, 1, 3, 64, 48, "f16x3"),
    "one_plane_one_group": (1, 2, 1, 40, 40, "f16x3"),
    "fp16": (3, 2, 3, 64, 64, "fp16"),
    "bf16": (3, 2, 3, 64, 64, "bf16"),
}
FORCE_STREAM, FORCE_PERSISTENT = 1 << 2, 2 << 2     # ops.set_diagnostics(2, None, flags)


def _inputs(name):
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    P, B, G, h, w, _ = CASES[name]
    gen = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    c = [93, 162, 54, 18, 2]
    ws = [(torch.randn(P, G * c[i + 1], c[i], 1, 1, generator=gen) / c[i] ** 0.5).to(DEV) for i in range(4)]
    bs = [(torch.randn(P, G * c[i + 1], generator=gen) * 0.1).to(DEV) for i in range(4)]
    plc = torch.randn(P, B, G * 81, h, w, generator=gen).to(DEV)
    xq = (torch.randn(P, B, G, h, w, generator=gen) * 4.0).round_().to(DEV)
    return ops.cgp16_pack(ws, bs, G), plc, xq


def _params(name, flags=0):
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    packed, plc, xq = _inputs(name)
    ops.set_precision(CASES[name][5])
    ops.set_diagnostics(2, None, flags)
    try:
        out = ops.cgp16_params(plc, xq, packed, 5, TAPS)
        torch.cuda.synchronize()
    finally:
        ops.set_diagnostics(2, None, 0)
        ops.set_precision("f16x3")
    return out.cpu()


def _leg(out_path):
    sys.path.insert(0, REPO)
    torch.save({name: _params(name) for name in CASES}, out_path)


@pytest.fixture(scope="module")
def legs(tmp_path_factory):
    d = tmp_path_factory.mktemp("cgp16")
    out = {}
    for leg in ("default", "stream"):
        env = dict(os.environ)
        env.pop("LLDWT_CGP16", None)
        if leg == "stream":
            env["LLDWT_CGP16"] = "stream"
        path = str(d / ("%s.pt" % leg))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=REPO, capture_output=True, text=True,
                           timeout=900)
        assert r.returncode == 0, "leg %s failed (rc=%d):\n%s" % (leg, r.returncode, r.stderr[-3000:])
        out[leg] = torch.load(path)
    return out


def _report(name, what, a, b):
    diff = (a - b).abs()
    print("%s %s: max |diff| = %.3g, differing = %d of %d, sum |stream| = %.6f" % (
        name, what, float(diff.max()), int((a != b).sum()), a.numel(), float(b.abs().double().sum())))


@pytest.mark.parametrize("name", sorted(CASES))
def test_default_dispatch_equals_streaming(legs, name):
    a, b = legs["default"][name], legs["stream"][name]
    _report(name, "default vs stream", a, b)
    assert torch.isfinite(b).all() and float(b.abs().sum()) > 0
    assert torch.equal(a, b)


@pytest.mark.parametrize("flags,form", [(FORCE_PERSISTENT, "forced persistent"), (FORCE_STREAM, "forced stream")])
@pytest.mark.parametrize("name", sorted(CASES))
def test_forced_form_equals_streaming(legs, name, flags, form):
    a, b = _params(name, flags), legs["stream"][name]
    _report(name, "%s vs stream" % form, a, b)
    assert torch.equal(a, b)


def test_other_pairs_weights_give_other_results(legs):
    """The guard of the guard: the pairs' results really depend on the pair's weights (planes and groups see the SAME inputs
    here, so equal outputs across pairs would mean the weights do not matter and a wrong-pair load could not be seen)."""
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    P, B, G, h, w, _ = CASES["bench_level2"]
    packed, plc, xq = _inputs("bench_level2")
    plc = plc[:1, :, :81].repeat(P, 1, G, 1, 1).contiguous()
    xq = xq[:1, :, :1].repeat(P, 1, G, 1, 1).contiguous()
    try:
        ops.set_diagnostics(2, None, FORCE_PERSISTENT)
        out = ops.cgp16_params(plc, xq, packed, 5, TAPS).view(P, B, G, 2, h, w)
        ops.set_diagnostics(2, None, FORCE_STREAM)
        ref = ops.cgp16_params(plc, xq, packed, 5, TAPS).view(P, B, G, 2, h, w)
    finally:
        ops.set_diagnostics(2, None, 0)
    assert torch.equal(out, ref)
    flat = out.permute(0, 2, 1, 3, 4, 5).reshape(P * G, -1)
    for i in range(P * G):
        for j in range(i + 1, P * G):
            assert not torch.equal(flat[i], flat[j]), (i, j)


if __name__ == "__main__":
    _leg(sys.argv[1])
