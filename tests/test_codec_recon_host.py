"""Host (CPU) tests of the decoders' ``recon`` argument: what is refused and what is let through, on the host,
with the GPU library made unreachable.  Nothing here touches the GPU."""
import importlib.util
import os

import pytest
import torch

from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import _lib, codec, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = "cgp=f16,plc_algo=direct,plc_fuse=1,plc_mode=f16x3,plc_shape=16,precision=f16x3,storage=fp32"
DIGEST = bytes(range(16))
L = 3


class LibraryLoaded(Exception):
    pass


@pytest.fixture
def net(monkeypatch):
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
        LiftingBasedDWTNetWrapper
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config

    def no_library():
        raise LibraryLoaded("the GPU library was loaded")
    monkeypatch.setattr(_lib, "load", no_library)
    return LiftingBasedDWTNetWrapper(make_config(dwtlevels=L, mode="validate")).eval()


def _hdr(H=64, W=96, **kw):
    return dict(layer="conditioned2ZTsepSubbands", netType="LiftingBasedNeuralWaveletv4", dwtlevels=L, H=H, W=W,
                numerics=codec.CODING_NUMERICS_VERSION, arithmetic=codec._with_step(BASE, 48), digest=DIGEST, **kw)


def _streams(count, seed=0):
    return [bytes((seed + 7 * i + j) & 0xFF for j in range(3 + i)) for i in range(count)]


def _unit():
    return dict(cs_xh=0, cs_x=0, scales=bytes(24), streams=[b""] * 3)


def _containers():
    plain = codec.pack_container(_hdr(), _streams(12))
    tiled = codec.pack_tiled(_hdr(H=100, W=64, th=64, tw=64, ny=2, nx=1), [_streams(12, 1), _streams(12, 2)])
    return plain, tiled, codec.pack_refined(0, 0, plain, [_unit()]), codec.pack_refined(0, 0, tiled, [_unit(), _unit()])


def test_check_recon():
    assert ops.check_recon(None) == "centre" == ops.check_recon("centre") and ops.check_recon("centroid") == "centroid"
    assert codec._recon_arg(None) is None and codec._recon_arg("centre") is None and codec._recon_arg("centroid") == "centroid"
    for bad in ("center", "Centroid", "", 1, True, 0.5, b"centroid", ("centroid",)):
        with pytest.raises(ValueError, match="recon"):
            ops.check_recon(bad)
        with pytest.raises(ValueError, match="recon"):
            codec._recon_arg(bad)


def test_a_bad_recon_is_refused_before_anything_else(net):
    """Before the container is even looked at, and before the library loads."""
    plain, tiled, _, _ = _containers()
    for bad in ("center", "mean", 1, True):
        with pytest.raises(ValueError, match="recon"):
            codec.decode_images(net, [plain], recon=bad)
        with pytest.raises(ValueError, match="recon"):
            codec.decode_images(net, [b"not a container"], recon=bad)
        with pytest.raises(ValueError, match="recon"):
            codec.decode_tiled(net, tiled, recon=bad)
        with pytest.raises(ValueError, match="recon"):
            codec.decode_tiled(net, b"not a container", recon=bad)


def test_a_refined_container_refuses_the_centroid_under_its_residual(net):
    _, _, rplain, rtiled = _containers()
    with pytest.raises(ValueError, match="recon and near"):
        codec.decode_images(net, [rplain], recon="centroid")
    with pytest.raises(ValueError, match="recon and near"):
        codec.decode_images(net, [rplain], recon="centroid", refine=True)
    with pytest.raises(ValueError, match="recon and near"):
        codec.decode_tiled(net, rtiled, recon="centroid")
    with pytest.raises(ValueError, match="recon and near"):
        codec.decode_tiled(net, rtiled, recon="centroid", region=(0, 0, 8, 8))


def _passes_the_argument_checks(call):
    """The call gets past every check of ``recon``: what stops it is the identity check of these made-up containers (their
    weights digest is not the net's) or the unreachable library, and says nothing of recon."""
    with pytest.raises((ValueError, LibraryLoaded)) as e:
        call()
    assert "recon" not in str(e.value), str(e.value)


def test_the_other_values_and_pairs_are_let_through(net):
    plain, tiled, rplain, rtiled = _containers()
    for rc in (None, "centre", "centroid"):
        _passes_the_argument_checks(lambda: codec.decode_images(net, [plain], recon=rc))
        _passes_the_argument_checks(lambda: codec.decode_tiled(net, tiled, recon=rc))
        # over LLDR: without its residual -- refine=False, or a reduced decode, which never applies it
        _passes_the_argument_checks(lambda: codec.decode_images(net, [rplain], recon=rc, refine=False))
        _passes_the_argument_checks(lambda: codec.decode_tiled(net, rtiled, recon=rc, refine=False))
        _passes_the_argument_checks(lambda: codec.decode_images(net, [rplain], recon=rc, reduce=1))
        _passes_the_argument_checks(lambda: codec.decode_tiled(net, rtiled, recon=rc, reduce=1))
    for rc in (None, "centre"):                                                 # the centre decode under the residual, as ever
        _passes_the_argument_checks(lambda: codec.decode_images(net, [rplain], recon=rc))
        _passes_the_argument_checks(lambda: codec.decode_tiled(net, rtiled, recon=rc))


def test_the_hooks_take_recon_only_for_a_centroid_decode(monkeypatch):
    """_decode_groups hands ``recon`` to the _decode_tiles hook only when it is set, so wrappers of the hook written before the
    argument existed see the calls they always saw."""
    seen = []
    result = torch.zeros(1)
    monkeypatch.setattr(codec, "_decode_tiles", lambda nets, s_xe, s_xo, th, tw, n, **kw: seen.append(kw) or result)
    hdr = dict(_hdr(), coder="host", step=3.0)
    units = [_streams(12, 1), _streams(12, 2)]
    for rc, want in ((None, False), ("centroid", True)):
        seen.clear()
        got = list(codec._decode_groups([None] * 3, units, 64, 96, 2, hdr, 0, recon=rc))
        assert len(got) == 1 and got[0][:2] == (0, 2) and got[0][2] is result and len(seen) == 1
        assert ("recon" in seen[0]) == want and seen[0].get("recon") == rc
    for ch in ("420", "400"):                                                  # the chroma planes' calls carry it too
        seen.clear()
        list(codec._decode_groups([None] * 3, [u[:4 * codec.CHROMA_PLANES[ch]] for u in units], 64, 96, 2, dict(hdr, chroma=ch), 0,
                                  recon="centroid"))
        assert len(seen) == (2 if ch == "420" else 1) and all(kw["recon"] == "centroid" for kw in seen)


def test_the_tool_knows_the_option():
    spec = importlib.util.spec_from_file_location("codec_cli_recon", os.path.join(REPO, "tools", "codec.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    assert "--recon {centre,centroid}" in cli.__doc__
