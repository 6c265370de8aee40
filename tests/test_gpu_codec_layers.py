"""GPU: the quality layers of the codec -- the three kernels of csrc/layers.hip against ONE fp32 restatement on
the host with `torch.equal`, the round trip of every coded layer with both coders (the embedded base, the level tensors of
encoder and decoder, the error bound of every refined coefficient), truncated containers, batch invariance, a decode in a fresh
process, tiles with regions and reduced decodes, and the code length of every refinement stream.

The restatement (normative, all fp32, every product rounded before it is added):
    idx  = #(table[:63] < max(sigma * inv_q_prev, 0.11f))
    m    = rint((v_prev - mu) * inv_q_prev),  a = min(|m|, K),  row = idx * (K + 1) + a,  sign = m < 0 ? -1 : +1
    t    = clamp(rint((y - v_prev) * inv_q_j), -1, 1),  v_j = v_prev + t * q_j,  coded symbol = sign * t
with (q_j, inv_q_j) = ops.layer_pair(n, j)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from helpers import filled
from oracle import weights

from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import codec, irans, ops
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import quality_layers as ql

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = ("conditioned2ZTsepSubbands", "onlyEZWT", "DWTConditioned2EntropyLayerZTBlock")
CODERS = ("host", "gpu")
AE_GAIN = 100.0
STEP, STEP_N, M = 3.0, 48, 2
_CACHE = {}


def _table63():
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import get_scale_table
    return torch.as_tensor(get_scale_table()).float()[:63].contiguous()


# ------------------------------------------------------------------------------------------------ 1. the kernels
def _restate(y, v, sigma, mu, table63, prev, cur, K):
    """Host fp32 tensors -> (sym, row, sign, v_j, m, t before the clamp)."""
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    sb = torch.maximum(sigma * f(prev[1]), f(0.11))
    idx = (table63.reshape(*([1] * sigma.dim()), 63) < sb[..., None]).sum(-1).int()
    m = torch.round((v - mu) * f(prev[1]))
    a = torch.minimum(m.abs(), f(float(K))).int()
    sign = torch.where(m < 0, -1, 1).int()
    raw = torch.round((y - v) * f(cur[1]))
    t = torch.clamp(raw, -1.0, 1.0)
    prod = t * f(cur[0])                                           # rounded on its own, then added: no fused multiply-add
    return t.int() * sign, idx * (K + 1) + a, sign, v + prod, m, raw


def _kernel_case(H, W, n, j, seed):
    """(y, v_prev, sigma, mu) of shape (3,2,3,H,W).  sigma / q_prev runs from below the 0.11 bound to above 256; v_prev sits
    k steps of q_prev from mu with k in [-12, 12], so the bell positions fall below, at and beyond K on both sides; the
    residual y - v_prev is a few q_j (beyond the clamp for most), and on a quarter of the positions v_prev is 0 and y is
    exactly +-q_j / 2 or +-fl(3 q_j / 2), or the fp32 neighbour of one of them, so that the rounded product falls on either side
    of a tie of rint and on the tie itself."""
    g = torch.Generator().manual_seed(seed)
    P, B, G = 3, 2, 3
    shape = (P, B, G, H, W)
    (qp, _), (q, _) = ops.layer_pair(n, j - 1), ops.layer_pair(n, j)
    sigma = qp * torch.exp(torch.rand(shape, generator=g) * (np.log(600.0) - np.log(0.01)) + np.log(0.01))
    sigma[0, 0, 0, 0, :3] = qp * torch.tensor([0.05, 0.11, 300.0])
    mu = (torch.rand(shape, generator=g) - 0.5) * 20 * qp
    mu = torch.where(torch.rand(shape, generator=g) < 0.5, torch.round(mu * 16) / 16, mu)
    k = torch.randint(-12, 13, shape, generator=g).float()
    k[0, 0, 1, 0, :5] = torch.tensor([-9.0, -8.0, 0.0, 8.0, 9.0])
    v = mu + k * qp
    y = v + (torch.rand(shape, generator=g) - 0.5) * 10 * q
    edge = torch.rand(shape, generator=g) < 0.25
    edge[0, 0, 1, 0, :5] = False
    h = torch.tensor(q, dtype=torch.float32) * 0.5                 # exact
    base = torch.stack([h, -h, 3 * h, -3 * h])
    inf = torch.tensor(float("inf"))
    cands = torch.cat([base, torch.nextafter(base, inf), torch.nextafter(base, -inf)])     # 12 values
    pick = cands[torch.randint(0, 12, shape, generator=g)]
    v = torch.where(edge, torch.zeros(()), v)
    y = torch.where(edge, pick, y)
    return y, v, sigma, mu, edge


@pytest.mark.parametrize("H,W", [(10, 6), (8, 16)])
@pytest.mark.parametrize("j", [1, 3])
@pytest.mark.parametrize("n", [4, 48, 1024])
def test_layer_kernels_equal_the_fp32_restatement(H, W, n, j):
    """(10, 6): the element form; (8, 16): the 4-wide form (row length a multiple of 4).  Symbol, row and value of the encoder,
    row and sign of the decoder's first half and the value of its second are `torch.equal` to the restatement; the decoder pair
    reproduces v_j from the encoder's symbols, and no input is written to."""
    K = ql.K
    prev, cur = ops.layer_pair(n, j - 1), ops.layer_pair(n, j)
    y, v, sigma, mu, edge = _kernel_case(H, W, n, j, 1000 * n + 10 * j + W)
    table = _table63()
    rsym, rrow, rsign, rv, m, raw = _restate(y, v, sigma, mu, table, prev, cur, K)
    # the inputs hold what the issue asks for
    sc = sigma * prev[1]
    assert float(sc.min()) < 0.11 and float(sc.max()) > 256 and int((rrow // (K + 1)).min()) <= 1 and int((rrow // (K + 1)).max()) == 63
    for side in (m < 0, m > 0):
        assert bool((side & (m.abs() < K)).any()) and bool((side & (m.abs() == K)).any()) and bool((side & (m.abs() > K)).any())
    assert bool((m == 0).any()) and int((rrow % (K + 1)).max()) == K
    h = torch.tensor(cur[0], dtype=torch.float32) * 0.5
    for r in (h, -h, 3 * h, -3 * h):
        assert bool(((y - v) == r)[edge].any())
    assert bool((raw.abs() > 1).any()) and set(rsym.unique().tolist()) == {-1, 0, 1}
    prod = ((y - v) * torch.tensor(cur[1]))[edge].abs()
    print("n %d j %d %dx%d: %d of %d edge products exactly on a tie of rint" % (n, j, H, W, int(((prod == 0.5) | (prod == 1.5)).sum()),
                                                                                  int(edge.sum())))
    P, B, G = sigma.shape[:3]
    params = torch.empty(P, B, 2 * G, H, W)
    params[:, :, 0::2], params[:, :, 1::2] = sigma, mu
    yd, vd, pd, td = y.to(DEV), v.to(DEV), params.to(DEV), table.to(DEV)
    sym, row, vj = ops.layer_encode(yd, vd, pd, td, prev, cur, K)
    assert sym.dtype == row.dtype == torch.int32 and vj.dtype == torch.float32
    assert torch.equal(sym.cpu(), rsym) and torch.equal(row.cpu(), rrow) and torch.equal(vj.cpu(), rv)
    row2, sign = ops.layer_rows(vd, pd, td, prev, K)
    assert torch.equal(row2.cpu(), rrow) and torch.equal(sign.cpu(), rsign)
    out = ops.layer_apply(vd, sym, sign, cur)
    assert torch.equal(out, vj)
    # no input was written to; in place gives the same values
    assert torch.equal(yd.cpu(), y) and torch.equal(vd.cpu(), v) and torch.equal(pd.cpu(), params) and torch.equal(td.cpu(), table)
    same = vd.clone()
    assert ops.layer_apply(same, sym, sign, cur, out=same) is same and torch.equal(same, vj)


def test_layer_kernels_refuse_bad_arguments():
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import _lib
    t = _table63().to(DEV)
    v = torch.zeros(1, 1, 1, 4, 4, device=DEV)
    p = torch.ones(1, 1, 2, 4, 4, device=DEV)
    prev, cur = ops.layer_pair(48, 0), ops.layer_pair(48, 1)
    with pytest.raises(_lib.LLDWTError, match="pair"):
        ops.layer_encode(v, v, p, t, prev, (cur[0], cur[1] * 1.5), ql.K)
    with pytest.raises(_lib.LLDWTError, match="finer"):
        ops.layer_encode(v, v, p, t, cur, prev, ql.K)
    with pytest.raises(_lib.LLDWTError, match="K"):
        ops.layer_rows(v, p, t, prev, 0)
    with pytest.raises(_lib.LLDWTError, match="belong together"):
        ops.layer_rows(v, p[:, :, :1].contiguous(), t, prev, ql.K)
    with pytest.raises(_lib.LLDWTError, match="int32"):
        ops.layer_apply(v, v, v.int(), cur)


# ------------------------------------------------------------------------------------------------ 2. the codec
def _layer_net(layer, L):
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
        LiftingBasedDWTNetWrapper
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
    cfg = make_config(dwtlevels=L, mode="validate", entropy_layer=layer)
    net = LiftingBasedDWTNetWrapper(cfg)
    net.load_state_dict(filled(weights.wrapper_template(dict(cfg))), strict=False)
    return net.to(DEV).eval()


def _net(layer):
    """The layer's net with the deterministic filled weights, L = 3, and the last (linear) layer of the subband auto-encoders of
    the levels 0 and 1 scaled by AE_GAIN, as tests/test_gpu_codec_step.py builds it: the gain brings the levels a step reaches
    to the amplitude a trained codec has them at (std about 15), so that the symbols of the base and of the layers are busy."""
    if ("net", layer) not in _CACHE:
        net = _layer_net(layer, 3)
        with torch.no_grad():
            for n in net.nets():
                for lev in range(2):
                    last = n.autoencoder.Yh_ae[lev].ae_down[6]
                    last.weight.mul_(AE_GAIN)
                    last.bias.mul_(AE_GAIN)
        _CACHE[("net", layer)] = net
    return _CACHE[("net", layer)]


def _images(B, H, W, seed):
    """Smooth colour fields plus noise, as uint8 (B,H,W,3) on the host."""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(B, 3, max(2, H // 16), max(2, W // 16), generator=g)
    x = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
    x = x * 200 + torch.rand(B, 3, H, W, generator=g) * 40
    return x.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _case(layer, coder):
    """One 72 x 90 image through the codec with step=3, layers=2 and through the strings API beside it, computed once per
    (layer, coder) and left unchanged: the containers, the decodes, and the level tensors of encoder and decoder."""
    key = ("case", layer, coder)
    if key in _CACHE:
        return _CACHE[key]
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.layers.lifting_dwt_nets import (encode_planes,
                                                                                                          encode_shapes, padded_size)
    net = _net(layer)
    img = _images(1, 72, 90, 5)
    c = dict(net=net, img=img)
    c["blob"] = codec.encode_images(net, img, coder=coder, step=STEP, layers=M)[0]
    c["base"] = codec.encode_images(net, img, coder=coder, step=STEP)[0]
    c["dec_base"] = codec.decode_images(net, [c["base"]])[0]
    c["dec"] = [codec.decode_images(net, [c["blob"]], layers=j)[0] for j in range(M + 1)]
    # the strings API: the tensors the codec's walk has inside
    nets = net.nets()
    aes, em = [n.autoencoder for n in nets], [n.entropymodel for n in nets]
    Hp, Wp = padded_size(aes, 72, 90)
    with torch.no_grad():
        x = ops.u8hwc_to_ycc_pad(img.to(DEV).contiguous(), Hp, Wp)
        y_xe, y = encode_planes(aes, x)
        s_xe, s_xo, _, v0 = type(em[0]).compress_planes(em, y_xe, y, coder=coder, step=STEP)
        streams, vs = ql.encode_units(em, y, v0, STEP_N, M, coder)
        shape_xe, shapes = encode_shapes(aes, 1, Hp, Wp)
        _, d0 = type(em[0]).decompress_planes(em, s_xe, s_xo, shape_xe, shapes, coder=coder, step=STEP)
        c["decoded_levels"] = [ql.decode_units(em, d0, streams, STEP_N, j, coder) for j in range(M + 1)]
    c.update(em=em, y=y, v0=v0, d0=d0, streams=streams, vs=vs)
    _CACHE[key] = c
    return c


def _tolerance(y, v0):
    """What fp32 rounding may add to |y - v_j| beyond q_j / 2.  Every operand of the chain -- y, mu, v -- is at most a few A in
    magnitude, A = max(|y|, |v_0|, 1) over the level (the test asserts |mu| <= 4 A on the layers' parameter pass).  The base
    symbol is rint of (y - mu) * inv_q, two roundings and the rounding of inv_q itself: its decision boundary moves by at most
    3 * 2^-24 * |y - mu| <= 15 * 2^-24 * A in the domain of y; its value sym * q + mu rounds once more, 2^-24 * 5 A.  A layer
    moves its boundaries by 3 * 2^-24 * 1.5 q_j and rounds its update t * q_j and the sum, 2 * 2^-24 * 2 A.  Over the base and
    two layers that is below 32 * 2^-24 * A; the bound used is 64 * 2^-24 * A = 2^-18 A (4e-4 at A = 100, against q_2 / 2 = 0.17)."""
    return 2.0 ** -18 * max(float(y.abs().max()), float(v0.abs().max()), 1.0)


@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("layer", LAYERS)
def test_layered_round_trip(layer, coder):
    c = _case(layer, coder)
    # the embedded base is the single-rate container, byte for byte; the header reports the layers
    hdr, base, lay = codec.parse_layered(c["blob"])
    assert base == c["base"] and c["blob"][:4] == b"LLDP"
    rh = codec.read_header(c["blob"])
    assert rh["layers"] == M and rh["base"]["step"] == STEP and rh["base"]["coder"] == coder
    sizes = codec.layer_bytes(c["blob"])
    assert len(c["base"]) < sizes[0] < sizes[1] < sizes[2] == len(c["blob"]) - 4
    # layers=0 is the base decode; the default is every layer
    assert torch.equal(c["dec"][0], c["dec_base"])
    assert torch.equal(codec.decode_images(c["net"], [c["blob"]])[0], c["dec"][M])
    # the codec's streams are those of the strings API beside it
    for jj in range(M):
        assert lay[jj][0] == [c["streams"][jj][i][p][0] for p in range(3) for i in range(2)]
    # the decoder's level tensors are the encoder's, at every prefix
    for i in range(3):
        assert torch.equal(c["d0"][i], c["v0"][i])
    for j in range(M + 1):
        got = c["decoded_levels"][j]
        assert got[2] is c["d0"][2]                                             # the coarsest level is not refined
        for i in range(2):
            assert torch.equal(got[i], c["v0"][i] if j == 0 else c["vs"][j - 1][i]), (j, i)
    # the error of every coefficient of the levels 0 and 1: within q_j / 2, and never growing with j
    for i in range(2):
        y, v0 = c["y"][i], c["v0"][i]
        tol = _tolerance(y, v0)
        mu = ql.level_params(c["em"], i, c["v0"])[:, :, 1::2]
        assert float(mu.abs().max()) <= 4 * max(float(y.abs().max()), float(v0.abs().max()), 1.0)
        err = [(y - v0).abs()] + [(y - c["vs"][j][i]).abs() for j in range(M)]
        for j, e in enumerate(err):
            q = ops.layer_pair(STEP_N, j)[0]
            print("%s %s level %d layer %d: max |y - v| = %.6f (q / 2 = %.6f, tolerance %.2g), %.0f %% outside the next layer's zero bin"
                  % (layer, coder, i, j, float(e.max()), q / 2, tol, 100 * float((e > ops.layer_pair(STEP_N, j + 1)[0] / 2).float().mean())))
            assert float(e.max()) <= q / 2 + tol, (i, j, float(e.max()))
            if j:
                assert bool((e <= err[j - 1] + tol).all()), (i, j)
    for j in range(M + 1):                                                      # printed, not asserted: the learned inverse is nonlinear
        p = codec.quality(c["img"][0], c["dec"][j])["psnr"]
        print("%s %s: %d layers: %d bytes, PSNR %.2f dB" % (layer, coder, j, sizes[j], p))


def test_layers_keep_closing_in_after_rdo_moved_the_base():
    """rdo moves base symbols toward zero, so y may lie outside the base bin; the clamp then takes the full step toward y and the
    later layers keep closing in: the error never grows with j, and the decoder still reproduces the encoder's tensors."""
    net = _net(LAYERS[1])
    em = [n.entropymodel for n in net.nets()]
    c = _case(LAYERS[1], "gpu")
    with torch.no_grad():
        y_xe = torch.zeros_like(c["y"][2][:, :, :1])
        _, s_xo, _, v0 = type(em[0]).compress_planes(em, y_xe, c["y"], coder="gpu", step=STEP, rdo=2.0)
        streams, vs = ql.encode_units(em, c["y"], v0, STEP_N, M, "gpu")
        got = ql.decode_units(em, v0, streams, STEP_N, M, "gpu")
    moved = 0
    for i in range(2):
        y = c["y"][i]
        tol = _tolerance(y, v0[i])
        err = [(y - v0[i]).abs()] + [(y - vs[j][i]).abs() for j in range(M)]
        moved += int((err[0] > STEP / 2 + tol).sum())
        for j in range(1, M + 1):
            assert bool((err[j] <= err[j - 1] + tol).all())
        assert torch.equal(got[i], vs[M - 1][i])
        # outside the base bin the first layer takes a whole step toward y
        out = err[0] > STEP / 2 + tol
        assert bool((err[1][out] <= err[0][out] - ops.layer_pair(STEP_N, 1)[0] + tol).all())
    print("rdo 2.0 moved %d coefficients out of their base bin" % moved)
    assert moved > 0


# ------------------------------------------------------------------------------------------------ 3. truncation
@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("layer", LAYERS)
def test_truncated_containers_decode_as_their_prefix(layer, coder):
    c = _case(layer, coder)
    assert codec.truncate_layers(c["blob"], 0) == c["base"] and codec.truncate_layers(c["blob"], M) == c["blob"]
    cut = codec.truncate_layers(c["blob"], 1)
    assert codec.read_header(cut)["layers"] == 1 and len(cut) < len(c["blob"])
    assert torch.equal(codec.decode_images(c["net"], [cut])[0], c["dec"][1])
    assert not torch.equal(c["dec"][1], c["dec"][0]) and not torch.equal(c["dec"][2], c["dec"][1])
    with pytest.raises(ValueError, match="layers"):
        codec.decode_images(c["net"], [cut], layers=2)
    with pytest.raises(ValueError, match="layers"):
        codec.decode_images(c["net"], [c["base"]], layers=1)
    # containers of different prefixes, and a plain one, in one call
    mixed = codec.decode_images(c["net"], [c["blob"], cut, c["base"]])
    assert torch.equal(mixed[0], c["dec"][2]) and torch.equal(mixed[1], c["dec"][1]) and torch.equal(mixed[2], c["dec_base"])


# ------------------------------------------------------------------------------------------------ 4. batches
@pytest.mark.parametrize("layer", LAYERS)
def test_a_batch_of_two_gives_the_bytes_of_each_alone(layer):
    net = _net(layer)
    img = _images(2, 40, 56, 17)
    both = codec.encode_images(net, img, coder="gpu", step=STEP, layers=M)
    for b in range(2):
        assert both[b] == codec.encode_images(net, img[b:b + 1], coder="gpu", step=STEP, layers=M)[0]
    dec = codec.decode_images(net, both)
    for b in range(2):
        assert torch.equal(dec[b], codec.decode_images(net, both[b:b + 1])[0])


# ------------------------------------------------------------------------------------------------ 5. another process
def _child(path_in, path_out):
    blob = open(path_in, "rb").read()
    net = _net(LAYERS[1])
    torch.save([codec.decode_images(net, [blob], layers=j)[0] for j in (1, None)], path_out)


def test_a_fresh_process_decodes_the_same_images():
    c = _case(LAYERS[1], "gpu")
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_codec_layers as t\n"
            "t._child(sys.argv[1], sys.argv[2])\n" % (REPO, os.path.join(REPO, "tests")))
    with tempfile.TemporaryDirectory() as td:
        fin, fout = os.path.join(td, "in.lldp"), os.path.join(td, "out.pt")
        with open(fin, "wb") as f:
            f.write(c["blob"])
        r = subprocess.run([sys.executable, "-c", code, fin, fout], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        got = torch.load(fout, weights_only=True)
    assert torch.equal(got[0], c["dec"][1]) and torch.equal(got[1], c["dec"][M])


# ------------------------------------------------------------------------------------------------ 6. tiles
def test_tiled_layers_decode_regions_and_reduced_sizes(monkeypatch):
    net = _net(LAYERS[2])
    img = _images(1, 128, 128, 23)
    blob = codec.encode_tiled(net, img, tile=64, step=STEP, layers=1)[0]
    base = codec.encode_tiled(net, img, tile=64, step=STEP)[0]
    hdr, got_base, lay = codec.parse_layered(blob)
    assert got_base == base and hdr["units"] == 4 and (hdr["base"]["ny"], hdr["base"]["nx"]) == (2, 2) and hdr["layers"] == 1
    assert blob == codec.encode_tiled(net, img, tile=64, step=STEP, layers=1, tiles_per_call=3)[0]
    full = codec.decode_tiled(net, blob)
    assert torch.equal(codec.decode_tiled(net, blob, layers=0), codec.decode_tiled(net, base))
    assert not torch.equal(full, codec.decode_tiled(net, base))
    # a tile is the image encode_images codes with the same arguments
    tile3 = codec.encode_images(net, img[:, 64:, 64:].contiguous(), step=STEP, layers=1)[0]
    assert torch.equal(codec.decode_images(net, [tile3])[0], full[64:, 64:])
    # a region inside tile 2 = (1, 0): the crop of the full decode, from that tile's base and layer streams alone
    seen, orig = [], codec._decode_tiles

    def spy(nets, s_xe, s_xo, th, tw, n, **kw):
        seen.append((n, kw.get("layers")))
        return orig(nets, s_xe, s_xo, th, tw, n, **kw)
    monkeypatch.setattr(codec, "_decode_tiles", spy)
    assert torch.equal(codec.decode_tiled(net, blob, region=(70, 5, 20, 30)), full[70:90, 5:35])
    assert len(seen) == 1 and seen[0][0] == 1
    streams, n, j = seen[0][1]
    assert (n, j) == (STEP_N, 1) and [streams[0][i][p] for p in range(3) for i in range(2)] == [[s] for s in lay[0][2]]
    assert torch.equal(codec.decode_tiled(net, blob, region=(60, 60, 10, 10)), full[60:70, 60:70])
    assert seen[1][0] == 4
    # reduce=1 refines level 1 alone: the level-0 streams are not even handed over, so emptying them changes nothing ...
    seen.clear()
    half = codec.decode_tiled(net, blob, reduce=1)
    assert half.shape == (64, 64, 3) and all(s[1][0][0][0] is None and s[1][0][0][1] is not None for s in seen)
    gutted = codec.pack_layered(hdr["table_crc"], base, [[[b"" if k % 2 == 0 else s for k, s in enumerate(u)] for u in lay[0]]])
    assert torch.equal(codec.decode_tiled(net, gutted, reduce=1), half)
    # ... and it differs from the reduced base decode, which reduce=2 (no refined level left) equals
    assert not torch.equal(half, codec.decode_tiled(net, base, reduce=1))
    assert torch.equal(codec.decode_tiled(net, blob, reduce=2), codec.decode_tiled(net, base, reduce=2))
    assert torch.equal(codec.decode_tiled(net, blob, reduce=1, region=(3, 40, 20, 24)), half[3:23, 40:64])


def test_refused_pairs_through_the_public_entry_points():
    net = _net(LAYERS[1])
    img = _images(1, 40, 56, 3)
    for kw, word in ((dict(near=0), "near"), (dict(step_map=np.full((5, 7), 2.0)), "step_map"), (dict(target_bytes=4000), "target_bytes"),
                     (dict(target_psnr=30.0), "target_psnr"), (dict(target_msssim=0.9), "target_msssim")):
        with pytest.raises(ValueError, match="layers and %s" % word):
            codec.encode_images(net, img, layers=1, **kw)
    with pytest.raises(ValueError, match="layers and overlap"):
        codec.encode_tiled(net, _images(1, 128, 128, 4), tile=64, overlap=16, layers=1)
    with pytest.raises(ValueError, match=r"n / 3\^m >= 1"):
        codec.encode_images(net, img, step=1.0, layers=3)
    plain = codec.encode_images(net, img, step=STEP)
    assert codec.encode_images(net, img, step=STEP, layers=None) == plain and codec.encode_images(net, img, step=STEP, layers=0) == plain


# ------------------------------------------------------------------------------------------------ 7. code length
@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("layer", LAYERS)
def test_refinement_streams_are_near_their_ideal_length(layer, coder):
    """Every refinement stream against the ideal code length of its symbols under the LLDP tables, within the bound the other
    code-length tests apply: ideal <= bits <= 1.01 ideal + 64 for the host coder, and for irans32 that bound times 1.01 plus
    its K lanes' final states and header, 8 (4 K + 16) bits."""
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models import entropy_coding as ec
    c = _case(layer, coder)
    tab, t63 = ql.tables(), _table63().to(DEV)
    total_ideal = total_bits = 0.0
    for i in range(2):
        params = ql.level_params(c["em"], i, c["v0"])
        v = c["v0"][i].contiguous()
        for j in range(1, M + 1):
            sym, row, v = ops.layer_encode(c["y"][i].contiguous(), v, params, t63, ops.layer_pair(STEP_N, j - 1),
                                           ops.layer_pair(STEP_N, j), ql.K)
            assert torch.equal(v, c["vs"][j - 1][i])
            sh, rh = sym.cpu().numpy(), row.cpu().numpy()
            lanes = irans.lanes(sh[0, 0].size)
            for p in range(3):
                ideal, escapes = ec.ideal_bits(sh[p, 0].reshape(-1), rh[p, 0].reshape(-1), tab)
                bits = 8 * len(c["streams"][j - 1][i][p][0])
                bound = ideal * 1.01 + 64
                if coder == "gpu":
                    bound = bound * 1.01 + 8 * (4 * lanes + 16)
                assert escapes == 0 and ideal <= bits <= bound, (i, j, p, ideal, bits, bound)
                total_ideal += ideal
                total_bits += bits
    n = sum(c["y"][i].numel() for i in range(2)) * M
    print("%s %s: %.0f bits ideal, %.0f written, %.3f bits per refinement symbol (log2 3 = 1.585)"
          % (layer, coder, total_ideal, total_bits, total_bits / n))
