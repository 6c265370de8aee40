"""GPU: the irans32 device coder (csrc/rans_gpu.hip, irans.py) -- its bytes and symbols pinned to the
Python definition tools/irans_ref.py, round trips of every coded layer against the host coder, tiles and regions, a fresh
process, no host coder on the device path, stream size, and corrupt-stream refusal.  The pins here stop at 8 lanes, the
Gaussian tables and sparse escapes; the coder's lane (16, 32), table and escape domain is pinned in
tests/test_gpu_irans_domain.py on the cases of tests/irans_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import _lib, ans, codec, irans

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import irans_ref as R  # noqa: E402

from test_irans_host import gaussian_symbols  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = ("conditioned2ZTsepSubbands", "onlyEZWT", "DWTConditioned2EntropyLayerZTBlock")
_NETS = {}


def _net(layer, L=3):
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
        LiftingBasedDWTNetWrapper
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
    key = (layer, L)
    if key not in _NETS:
        cfg = make_config(dwtlevels=L, mode="validate", entropy_layer=layer)
        torch.manual_seed(0)
        _NETS[key] = LiftingBasedDWTNetWrapper(cfg).to(DEV).eval()
    return _NETS[key]


def _images(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(B, 3, max(2, H // 16), max(2, W // 16), generator=g)
    x = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
    x = x * 200 + torch.rand(B, 3, H, W, generator=g) * 40
    return x.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


class _Tabs:
    def __init__(self, cdf, sizes, offs):
        w = max(len(r) for r in cdf)
        self.cdf = np.array([r + [0] * (w - len(r)) for r in cdf], dtype=np.int32)
        self.sizes = np.asarray(sizes, dtype=np.int32)
        self.offsets = np.asarray(offs, dtype=np.int32)


def _streams(n, Z, seed):
    sym, idx = [], []
    for z in range(Z):
        s, i, tabs = gaussian_symbols(n, seed + z)
        sym.append(s)
        idx.append(i)
    return sym, idx, tabs


# ------------------------------------------------------------------------------------------------ 1. spec pins
@pytest.mark.parametrize("n", [1, 300, 8191, 8192, 16384, 40000])
def test_encoder_bytes_equal_the_reference(n):
    sym, idx, tabs = _streams(n, 3, 100 + n)
    T = _Tabs(*tabs)
    dt = irans.DeviceTables(T.cdf, T.sizes, T.offsets, DEV)
    got = irans.encode(torch.tensor(sym, dtype=torch.int32, device=DEV), torch.tensor(idx, dtype=torch.int32, device=DEV), dt)
    for z in range(3):
        assert got[z] == R.encode(sym[z], idx[z], *tabs), z


@pytest.mark.parametrize("n", [300, 8192, 40000])
def test_decoder_pops_reference_streams_whole_and_in_pieces(n):
    sym, idx, tabs = _streams(n, 3, 200 + n)
    T = _Tabs(*tabs)
    dt = irans.DeviceTables(T.cdf, T.sizes, T.offsets, DEV)
    streams = [R.encode(sym[z], idx[z], *tabs) for z in range(3)]
    idx_d = torch.tensor(idx, dtype=torch.int32, device=DEV)
    d = irans.Decoder(streams, n, dt, DEV)
    whole = d.pop(idx_d)
    d.finish()
    assert whole.cpu().tolist() == sym
    g = np.random.default_rng(n)
    d = irans.Decoder(streams, n, dt, DEV)
    parts, a = [], 0
    while a < n:
        b = min(n, a + int(g.integers(1, 700)))                        # uneven, step-sized pieces, mid-round ends
        parts.append(d.pop(idx_d[:, a:b].contiguous()))
        a = b
    d.finish()
    assert torch.cat(parts, 1).cpu().tolist() == sym


def test_stream_size_against_the_host_coder():
    for n in (8192, 60000):
        sym, idx, tabs = _streams(n, 2, 300 + n)
        T = _Tabs(*tabs)
        dt = irans.DeviceTables(T.cdf, T.sizes, T.offsets, DEV)
        gpu = irans.encode(torch.tensor(sym, dtype=torch.int32, device=DEV), torch.tensor(idx, dtype=torch.int32, device=DEV), dt)
        host = ans.encode_streams(np.asarray(sym, dtype=np.int32), np.asarray(idx, dtype=np.int32), T.cdf, T.sizes, T.offsets)
        K = irans.lanes(n)
        for z in range(2):
            assert len(gpu[z]) <= len(host[z]) * 1.01 + 4 * K + 16, (n, len(gpu[z]), len(host[z]))


# ------------------------------------------------------------------------------------------------ 2. round trips
@pytest.mark.parametrize("layer", LAYERS)
@pytest.mark.parametrize("L", [3, 4])
@pytest.mark.parametrize("B", [1, 3])
def test_gpu_coder_decodes_to_the_host_coders_image(layer, L, B):
    net = _net(layer, L)
    x = _images(B, 40, 52, 7 * L + B)
    host = codec.decode_images(net, codec.encode_images(net, x))
    blobs = codec.encode_images(net, x, coder="gpu")
    assert all(codec.read_header(b)["coder"] == "gpu" for b in blobs)
    gpu = codec.decode_images(net, blobs)
    for b in range(B):
        assert torch.equal(gpu[b], host[b]), b


def test_tiles_and_regions_with_the_gpu_coder():
    net = _net("conditioned2ZTsepSubbands", 3)
    x = _images(1, 150, 200, 14)
    hblob = codec.encode_tiled(net, x, tile=64)[0]
    gblob = codec.encode_tiled(net, x, tile=64, coder="gpu")[0]
    assert codec.read_header(gblob)["coder"] == "gpu" and codec.read_header(hblob)["coder"] == "host"
    full = codec.decode_tiled(net, hblob)
    assert torch.equal(codec.decode_tiled(net, gblob), full)
    for region in [(10, 20, 60, 70), (149, 199, 1, 1)]:
        y0, x0, h, w = region
        assert torch.equal(codec.decode_tiled(net, gblob, region=region, tiles_per_call=2), full[y0:y0 + h, x0:x0 + w])


_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import codec
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import LiftingBasedDWTNetWrapper
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
d = sys.argv[2]
cfg = make_config(dwtlevels=3, mode="validate", entropy_layer="conditioned2ZTsepSubbands")
torch.manual_seed(0)
net = LiftingBasedDWTNetWrapper(cfg).to("cuda:0").eval()
torch.save(codec.decode_images(net, [open(d + "/g.lld", "rb").read()])[0], d + "/child.pt")
"""


def test_gpu_container_decodes_in_a_fresh_process(tmp_path):
    net = _net("conditioned2ZTsepSubbands", 3)
    x = _images(1, 72, 90, 4)
    want = codec.decode_images(net, codec.encode_images(net, x))[0]
    (tmp_path / "g.lld").write_bytes(codec.encode_images(net, x, coder="gpu")[0])
    r = subprocess.run([sys.executable, "-c", _CHILD, REPO, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert torch.equal(torch.load(tmp_path / "child.pt"), want)


# ------------------------------------------------------------------------------------------------ 3. no host coder
def test_no_host_coder_on_the_device_path(monkeypatch):
    lib = _lib.load()

    def refuse(*a, **k):
        raise AssertionError("host rANS entry point called on the gpu coder path")
    for name in ("lldwt_rans_decoder_new", "lldwt_rans_decode", "lldwt_rans_decode_multi", "lldwt_rans_encode",
                 "lldwt_rans_encode_multi"):
        monkeypatch.setattr(lib, name, refuse)
    x = _images(2, 40, 52, 21)
    for layer in LAYERS:
        net = _net(layer, 3)
        out = codec.decode_images(net, codec.encode_images(net, x, coder="gpu"))
        assert len(out) == 2 and out[0].shape == (40, 52, 3)
    with pytest.raises(AssertionError, match="host rANS"):
        codec.encode_images(_net("onlyEZWT", 3), x)


# ------------------------------------------------------------------------------------------------ 4. corrupt stream
def test_flipped_bytes_in_a_gpu_container_raise_corrupt_stream():
    net = _net("conditioned2ZTsepSubbands", 3)
    blob = codec.encode_images(net, _images(1, 40, 52, 31), coder="gpu")[0]
    hdr, streams = codec.parse_container(blob)
    g = np.random.default_rng(5)
    for k in (0, 1, len(streams) - 1):
        s = bytearray(streams[k])
        for p in g.integers(0, len(s), 3):
            s[p] ^= 0x5A
        bad = codec.pack_container(hdr, streams[:k] + [bytes(s)] + streams[k + 1:])
        with pytest.raises(ValueError, match="corrupt stream"):
            codec.decode_images(net, [bad])
