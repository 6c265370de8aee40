"""GPU: the row-wise Winograd F(2,3) form of the fused tree-context pair (k_plc_wino, the default of lldwt_plc_fused at
precision 0) against the direct kernel (LLDWT_PLC_ALGO=direct, read when the library loads: child processes), against a
float64 reference, repeat determinism, and an entropy-coding round trip that runs through it."""
import os
import subprocess
import sys
import tempfile

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (P, B, cmid, cout, hp, wp, act): ragged parents (1x1, odd sizes, tiles overhanging both ways), partial 16-channel chunks and
# partial 128-channel output blocks, and one slice of the level-0 shape of the benchmark (parent 128 x 128, 243 channels)
SHAPES = [(1, 1, 17, 5, 1, 1, 0), (2, 1, 100, 129, 7, 35, 2), (1, 3, 243, 243, 9, 16, 1), (2, 2, 256, 40, 40, 70, 2),
          (1, 1, 64, 243, 4, 17, 0), (1, 2, 243, 243, 128, 128, 0)]


def _ops():
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    return ops


def _case(i):
    P, B, cmid, cout, hp, wp, act = SHAPES[i]
    g = torch.Generator().manual_seed(40 + i)
    parent = (torch.rand(P, B, 3, hp, wp, generator=g) - 0.5) * 4.0
    w1 = (torch.rand(P, cmid, 3, 3, 3, generator=g) - 0.5) * 0.6
    b1 = torch.rand(P, cmid, generator=g) - 0.5
    w2 = (torch.rand(P, cout, cmid, 3, 3, generator=g) - 0.5) * (2.0 / (cmid * 9) ** 0.5)
    b2 = torch.rand(P, cout, generator=g) - 0.5
    return parent, w1, b1, w2, b2, cmid, cout, act


def _run(ops, parent, w1, b1, w2, b2, cmid, cout, act):
    return ops.plc_fused(parent.to(DEV), ops.plc_fused_pack1(w1.to(DEV), b1.to(DEV)), ops.conv_f16x3_pack(w2.to(DEV)),
                         b2.to(DEV), cmid, cout, act=act)


def test_default_is_winograd():
    ops = _ops()
    expect = "direct" if os.environ.get("LLDWT_PLC_ALGO") == "direct" or os.environ.get("LLDWT_PLC_SHAPE") == "16" else "winograd"
    assert ops.plc_algo() == expect


def test_winograd_and_direct_agree():
    """Both algorithms in child processes (the switch is read once per process) on every shape of SHAPES: a few 1e-6 of the
    output scale apart, as two fp32-accurate paths are."""
    code = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import torch, test_gpu_plc_winograd as t\n"
        "ops = t._ops(); assert ops.plc_algo() == sys.argv[2], ops.plc_algo()\n"
        "torch.save([t._run(ops, *t._case(i)).cpu() for i in range(len(t.SHAPES))], sys.argv[1])\n" % (REPO, os.path.join(REPO, "tests")))
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for algo in ("direct", "winograd"):
            env = dict(os.environ, LLDWT_PLC_ALGO=algo)
            env.pop("LLDWT_PLC_SHAPE", None)
            f = os.path.join(td, algo + ".pt")
            subprocess.run([sys.executable, "-c", code, f, algo], check=True, env=env, timeout=600)
            out[algo] = torch.load(f, weights_only=True)
    worst = 0.0
    for i, (a, b) in enumerate(zip(out["direct"], out["winograd"])):
        assert a.shape == b.shape
        d = float((a - b).abs().max()) / max(float(a.abs().max()), 1e-6)
        worst = max(worst, d)
        assert d < 6e-6, (SHAPES[i], d)
    print("\n[plc winograd] vs direct over %d shapes: worst relative difference %.3g" % (len(SHAPES), worst))


@pytest.mark.parametrize("i", [0, 1, 2, 3, 4])
def test_winograd_against_float64(i):
    """The pair against a float64 evaluation of the same maths (nearest 2x upsample, LeakyReLU 0.01 between the convs)."""
    ops = _ops()
    parent, w1, b1, w2, b2, cmid, cout, act = _case(i)
    y = _run(ops, parent, w1, b1, w2, b2, cmid, cout, act).cpu().double()
    for p in range(parent.shape[0]):
        up = F.interpolate(parent[p].double(), scale_factor=2, mode="nearest")
        t = F.leaky_relu(F.conv2d(up, w1[p].double(), b1[p].double(), padding=1), 0.01)
        r = F.conv2d(t, w2[p].double(), b2[p].double(), padding=1)
        r = F.leaky_relu(r, 0.01) if act == 2 else (F.relu(r) if act == 3 else r)
        if act == 1:
            r = torch.tanh(r)
        e = float((y[p] - r).abs().max()) / max(float(r.abs().max()), 1e-6)
        assert e < (2e-6 if act != 1 else 2e-5), (SHAPES[i], p, e)


def test_winograd_is_deterministic():
    """Encoder and decoder evaluate the pair separately and need the same bits: repeated calls are bit-identical."""
    ops = _ops()
    args = _case(3)
    a = _run(ops, *args)
    for _ in range(2):
        assert torch.equal(_run(ops, *args), a)


def test_coding_round_trip_through_winograd():
    """decode(encode(x)) is bit-exact with the Winograd pair computing the tree contexts on both sides."""
    from test_gpu_coding import _coefs, _layers
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
        DWTConditioned2EntropyLayerZTsepSubbands as Layer
    ops = _ops()
    if ops.plc_algo() != "winograd":
        pytest.skip("LLDWT_PLC_ALGO / LLDWT_PLC_SHAPE select the direct kernel in this process")
    calls = []
    orig = ops.plc_fused

    def spy(*a, **k):
        calls.append(1)
        return orig(*a, **k)
    net, sd, cfg = _layers(3)
    xe, xo = _coefs(3, 2, 64, 11, gain=1.5)
    em = [n.entropymodel for n in net.nets()]
    ops.plc_fused = spy
    try:
        s_xe, s_xo, xe_q, xo_q = Layer.compress_planes(em, xe.to(DEV), [t.to(DEV) for t in xo])
        xe_d, xo_d = Layer.decompress_planes(em, s_xe, s_xo, xe.shape, [t.shape for t in xo])
    finally:
        ops.plc_fused = orig
    assert calls, "the coder did not run the fused pair"
    assert torch.equal(xe_d, xe_q)
    for a, b in zip(xo_d, xo_q):
        assert torch.equal(a, b)
