"""GPU: variable-rate coding -- the quantiser with a step in its three forms (lldwt_gauss_quantise, the
wavefront step's epilogue, the tensor-op restatement) against ONE fp32 restatement on the host with `torch.equal`, the round
trip of every coded layer with both coders, the code-length kernel against integer numpy, and the codec: the header key, the
decode, tiles, the residual layer over a stepped base, and the byte target.

The restatement (the normative quantiser, all fp32):
    idx = #(table[:63] < max(sigma * inv_q, 0.11f));  sym = rint((y - mu) * inv_q);  value = (float)sym * q + mu
with q = n / 16 and inv_q = fp32(1 / q).  sym * q is exact (|sym| < 2^12, n <= 1024), so a device that fuses the
multiply-add and a host that does not agree bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import filled
from oracle import weights

from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import _lib, codec, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYERS = ("conditioned2ZTsepSubbands", "onlyEZWT", "DWTConditioned2EntropyLayerZTBlock")
GAIN = 60.0
_CACHE = {}


def _table63():
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import get_scale_table
    return torch.as_tensor(get_scale_table()).float()[:63].contiguous()


def _restate(sigma, mu, y, table63, n):
    """Host tensors -> (idx, sym, value); sym / value are None without y."""
    q, inv_q = ops.step_pair(n / 16.0)
    sb = torch.maximum(sigma * inv_q, torch.tensor(0.11, dtype=torch.float32))
    idx = (table63.reshape(*([1] * sigma.dim()), 63) < sb[..., None]).sum(-1).int()
    if y is None:
        return idx, None, None
    sym = torch.round((y - mu) * inv_q).int()
    return idx, sym, sym.float() * q + mu


def _nonzero_share(sym):
    return float((sym != 0).float().mean())


# ------------------------------------------------------------------------------------------------ 1. lldwt_gauss_quantise
def _quant_case(H, W, seed):
    """params of a full (H, W) grid, (3,2,6,H,W), and coefficients (3,2,3,H,W): sigma from below the 0.11 bound to above 256,
    half of the means on the 1/16 grid with the coefficient EXACTLY on a rounding boundary mu + (k + 1/2) q for q = 1."""
    g = torch.Generator().manual_seed(seed)
    P, B, G = 3, 2, 3
    sigma = torch.exp(torch.rand(P, B, G, H, W, generator=g) * (np.log(600.0) - np.log(0.01)) + np.log(0.01))
    sigma[0, 0, 0, 0, :3] = torch.tensor([0.05, 0.11, 300.0])
    mu = (torch.rand(P, B, G, H, W, generator=g) - 0.5) * 20
    grid = torch.rand(P, B, G, H, W, generator=g) < 0.5
    mu = torch.where(grid, torch.round(mu * 16) / 16, mu)
    y = (torch.rand(P, B, G, H, W, generator=g) - 0.5) * GAIN
    return sigma, mu, y, grid


@pytest.mark.parametrize("H,W", [(10, 6), (8, 16)])
@pytest.mark.parametrize("n", [4, 16, 24, 1024])
def test_quantiser_kernel_equals_the_fp32_restatement(H, W, n):
    """(10, 6): the element-wise form; (8, 16): the 4-wide form (grid width a multiple of 4), with whole-vector level accesses
    on the contiguous grid and element accesses on the phases."""
    sigma, mu, y, grid = _quant_case(H, W, 7 * H + W)
    q = n / 16.0
    k = torch.round((y - mu) / q)
    y = torch.where(grid, mu + (k + 0.5) * q, y)               # exact: mu on the 1/16 grid, (k + 1/2) q on the 1/32 grid
    assert torch.equal((y - mu)[grid], ((k + 0.5) * q)[grid])
    table = _table63()
    P, B, G = sigma.shape[:3]
    assert float(sigma.min()) < 0.11 and float(sigma.max()) > 256
    for r0, c0, s in ((0, 0, 2), (0, 1, 2), (1, 0, 2), (1, 1, 2), (0, 0, 1)):
        sel = (slice(None),) * 3 + (slice(r0, None, s), slice(c0, None, s))
        sg, m, yy = sigma[sel], mu[sel], y[sel]
        params = torch.empty(P, B, 2 * G, *sg.shape[3:])
        params[:, :, 0::2], params[:, :, 1::2] = sg, m
        ridx, rsym, rval = _restate(sg, m, yy, table, n)
        level = torch.full((P, B, G, H, W), 777.0, device=DEV)
        idx, sym = ops.gauss_quantise(params.to(DEV), table.to(DEV), level, r0, c0, s, q, y=y.to(DEV))
        assert torch.equal(idx.cpu(), ridx) and torch.equal(sym.cpu(), rsym)
        want = torch.full((P, B, G, H, W), 777.0)
        want[sel] = rval
        assert torch.equal(level.cpu(), want)                                    # the phase's values, nothing else touched
        # decoder: indexes alone, then the values from the encoder's symbols
        idx0, none = ops.gauss_quantise(params.to(DEV), table.to(DEV), None, r0, c0, s, q)
        assert none is None and torch.equal(idx0.cpu(), ridx)
        lev2 = torch.full((P, B, G, H, W), 777.0, device=DEV)
        idx2, _ = ops.gauss_quantise(params.to(DEV), table.to(DEV), lev2, r0, c0, s, q, sym=sym)
        assert torch.equal(idx2.cpu(), ridx) and torch.equal(lev2, level)


def test_quantiser_refuses_bad_arguments():
    table = _table63().to(DEV)
    params = torch.ones(1, 1, 2, 4, 4, device=DEV)
    level = torch.zeros(1, 1, 1, 8, 8, device=DEV)
    with pytest.raises(ValueError, match="step"):
        ops.gauss_quantise(params, table, level, 0, 0, 2, 0.3, y=level)
    with pytest.raises(_lib.LLDWTError, match="does not fit"):
        ops.gauss_quantise(params, table, level, 2, 0, 2, 1.0, y=level)          # row 2 + 2 * 3 = 8 is outside
    with pytest.raises(_lib.LLDWTError):
        ops.gauss_quantise(params, table, None, 0, 0, 2, 1.0, y=level)


# ------------------------------------------------------------------------------------------------ 2. the wavefront step
def _cond2(L=3):
    if ("cond2", L) not in _CACHE:
        _CACHE[("cond2", L)] = _layer_net(LAYERS[0], L)
    return _CACHE[("cond2", L)]


def _layer_net(layer, L):
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
        LiftingBasedDWTNetWrapper
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
    cfg = make_config(dwtlevels=L, mode="validate", entropy_layer=layer)
    net = LiftingBasedDWTNetWrapper(cfg)
    net.load_state_dict(filled(weights.wrapper_template(dict(cfg))), strict=False)
    return net.to(DEV).eval()


class _Wavefront:
    """One tree level of conditioned2ZTsepSubbands driven step by step through the C entry points."""

    def __init__(self, H, W, B, seed):
        from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models import entropy_coding as ec
        from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
            DWTConditioned2EntropyLayerZTsepSubbands as Layer
        self.lib = _lib.load()
        em = [n.entropymodel for n in _cond2().nets()]
        Layer._coding_setup(em)
        g = torch.Generator().manual_seed(seed)
        self.P, self.B, self.G, self.H, self.W = 3, B, 3, H, W
        parent = ((torch.rand(3, B, 3, H // 2, W // 2, generator=g) - 0.5) * GAIN).to(DEV)
        self.y = ((torch.rand(3, B, 3, H, W, generator=g) - 0.5) * GAIN).to(DEV)
        with torch.no_grad():
            self.plc, packed, _, self.K, self.bits = Layer._tree_context(em, 0, parent, 3)
        self.packed16 = packed[1]
        assert self.packed16 is not None and self.K == 5
        self.table = em[0].ent_out_xo_list[0].scale_table.to(DEV).float()[:63].contiguous()
        self.starts = ec._step_offsets(H, W, self.K // 2 + 1)
        self.nsteps, self.ntot = len(self.starts) - 1, H * W
        self.st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def pixels(self, t):
        """rows, columns of step t in the kernel's order (rows ascending)."""
        slope = self.K // 2 + 1
        rows = [r for r in range(self.H) if 0 <= t - slope * r < self.W]
        return torch.tensor(rows, dtype=torch.long), torch.tensor([t - slope * r for r in rows], dtype=torch.long)

    def encode_step(self, yhat, idx, sym, t, n=None):
        p = lambda a: C.c_void_p(a.data_ptr())
        head = (p(self.plc), p(yhat), p(self.y), p(self.packed16), p(self.table), p(idx), p(sym), None)
        tail = (self.P, self.B, self.H, self.W, self.G, self.K, int(self.bits), t, self.ntot, self.starts[t])
        if n is None:
            ops.check(self.lib.lldwt_cgp16_wavefront_step(*head, *tail, self.st), "step")
        else:
            ops.check(self.lib.lldwt_cgp16_wavefront_step_q(*head, None, *tail, *ops.step_pair(n / 16.0), self.st), "step_q")

    def decode_step(self, yhat, t, n=None, want_sigma=False):
        """-> (idx (Z, cnt, G), mu (Z, G, cnt), sigma or None) of step t on the state yhat, which is not changed."""
        cnt = self.starts[t + 1] - self.starts[t]
        Z = self.P * self.B
        idx = torch.zeros(Z, cnt, self.G, device=DEV, dtype=torch.int32)
        mu = torch.zeros(Z, self.G, cnt, device=DEV)
        sg = torch.zeros(Z, self.G, cnt, device=DEV) if want_sigma else None
        p = lambda a: None if a is None else C.c_void_p(a.data_ptr())
        head = (p(self.plc), p(yhat), None, p(self.packed16), p(self.table), p(idx), None, p(mu))
        tail = (self.P, self.B, self.H, self.W, self.G, self.K, int(self.bits), t, cnt, 0)
        if n is None:
            ops.check(self.lib.lldwt_cgp16_wavefront_step(*head, *tail, self.st), "step")
        else:
            ops.check(self.lib.lldwt_cgp16_wavefront_step_q(*head, p(sg), *tail, *ops.step_pair(n / 16.0), self.st), "step_q")
        return idx, mu, sg

    def apply(self, sym, mu, yhat, t, n=None):
        cnt = self.starts[t + 1] - self.starts[t]
        p = lambda a: C.c_void_p(a.data_ptr())
        args = (p(sym), p(mu), p(yhat), self.P, self.B, self.H, self.W, self.G, self.K, t, cnt, 0)
        if n is None:
            ops.check(self.lib.lldwt_wavefront_apply(*args, self.st), "apply")
        else:
            ops.check(self.lib.lldwt_wavefront_apply_q(*args, *ops.step_pair(n / 16.0), self.st), "apply_q")

    def buffers(self):
        Z = self.P * self.B
        return (torch.zeros(self.P, self.B, self.G, self.H, self.W, device=DEV),
                torch.zeros(Z, self.ntot, self.G, device=DEV, dtype=torch.int32),
                torch.zeros(Z, self.ntot, self.G, device=DEV, dtype=torch.int32))


def _probe_steps(wf):
    """The first step, the last, and the longest diagonals (a full 32-pixel block where the level has 32 rows)."""
    lens = [wf.starts[t + 1] - wf.starts[t] for t in range(wf.nsteps)]
    longest = max(lens)
    mid = [t for t in range(wf.nsteps) if lens[t] == longest]
    return sorted({0, mid[0], mid[len(mid) // 2], wf.nsteps // 3, wf.nsteps - 1})


@pytest.mark.parametrize("H,W", [(32, 32), (24, 40)])
def test_wavefront_step_q_at_the_unit_step_equals_the_entry_point_without_a_step(H, W):
    wf = _Wavefront(H, W, 2, 11)
    ya, ia, sa = wf.buffers()
    yb, ib, sb = wf.buffers()
    probe = _probe_steps(wf)
    for t in range(wf.nsteps):
        if t in probe:                                                             # decoder mode on the same state
            i0, m0, _ = wf.decode_step(ya, t)
            i1, m1, _ = wf.decode_step(yb, t, n=16)
            assert torch.equal(i0, i1) and torch.equal(m0, m1)
            cnt = wf.starts[t + 1] - wf.starts[t]
            sym = torch.randint(-40, 41, (wf.P * wf.B, cnt, wf.G), device=DEV, dtype=torch.int32)
            o0, o1 = ya.clone(), yb.clone()
            wf.apply(sym, m0, o0, t)
            wf.apply(sym, m1, o1, t, n=16)
            assert torch.equal(o0, o1)
        wf.encode_step(ya, ia, sa, t)
        wf.encode_step(yb, ib, sb, t, n=16)
    assert torch.equal(ia, ib) and torch.equal(sa, sb) and torch.equal(ya, yb)
    assert _nonzero_share(sa) > 0.2


@pytest.mark.parametrize("H,W", [(32, 32), (24, 40)])
@pytest.mark.parametrize("n", [40, 4])
def test_wavefront_step_q_equals_the_fp32_restatement(H, W, n):
    """A step t in decoder mode with sigma_out, then in encoder mode on the same state: idx, sym and yhat are the restatement
    of (sigma, mu, y); the decoder's apply writes the same values from the encoder's symbols."""
    wf = _Wavefront(H, W, 2, 12)
    yhat, idx_all, sym_all = wf.buffers()
    table = wf.table.cpu()
    Z, G = wf.P * wf.B, wf.G
    for t in range(wf.nsteps):
        check = t in _probe_steps(wf)
        if check:
            before = yhat.clone()
            idx_d, mu, sigma = wf.decode_step(yhat, t, n=n, want_sigma=True)
            assert torch.equal(yhat, before)
        wf.encode_step(yhat, idx_all, sym_all, t, n=n)
        if check:
            rows, cols = wf.pixels(t)
            a, b = wf.starts[t], wf.starts[t + 1]
            assert b - a == len(rows)
            yv = wf.y.cpu().reshape(Z, G, wf.H, wf.W)[:, :, rows, cols]                    # (Z, G, cnt)
            ridx, rsym, rval = _restate(sigma.cpu(), mu.cpu(), yv, table, n)
            assert torch.equal(idx_d.cpu(), ridx.permute(0, 2, 1))
            assert torch.equal(idx_all[:, a:b].cpu(), ridx.permute(0, 2, 1))
            assert torch.equal(sym_all[:, a:b].cpu(), rsym.permute(0, 2, 1))
            assert torch.equal(yhat.cpu().reshape(Z, G, wf.H, wf.W)[:, :, rows, cols], rval)
            dec = before.clone()
            wf.apply(sym_all[:, a:b].contiguous(), mu, dec, t, n=n)
            assert torch.equal(dec, yhat)
    if n == 40:
        assert _nonzero_share(sym_all) > 0.2


def test_wavefront_step_q_refuses_a_step_off_the_grid():
    wf = _Wavefront(32, 32, 2, 13)
    yhat, idx, sym = wf.buffers()
    p = lambda a: C.c_void_p(a.data_ptr())
    rc = wf.lib.lldwt_cgp16_wavefront_step_q(p(wf.plc), p(yhat), p(wf.y), p(wf.packed16), p(wf.table), p(idx), p(sym), None, None,
                                             wf.P, wf.B, wf.H, wf.W, wf.G, wf.K, int(wf.bits), 0, wf.ntot, 0, 0.3, 1 / 0.3, wf.st)
    assert rc != 0 and b"step" in wf.lib.lldwt_last_error()


# ------------------------------------------------------------------------------------------------ 3. the three layers
def _layer_case(layer):
    """-> (entropy models, layer class, xe, [xo]) for L = 3, 64 x 64 planes, B = 2."""
    if layer not in _CACHE:
        net = _cond2() if layer == LAYERS[0] else _layer_net(layer, 3)
        em = [n.entropymodel for n in net.nets()]
        g = torch.Generator().manual_seed(5)
        S, L, B = 64, 3, 2
        xe = ((torch.rand(3, B, 1, S >> L, S >> L, generator=g) - 0.5) * GAIN).to(DEV)
        xo = [((torch.rand(3, B, 3, S >> (i + 1), S >> (i + 1), generator=g) - 0.5) * GAIN).to(DEV) for i in range(L)]
        _CACHE[layer] = (em, type(em[0]), xe, xo)
    return _CACHE[layer]


def _unit_step(layer, coder):
    key = ("unit", layer, coder)
    if key not in _CACHE:
        em, cls, xe, xo = _layer_case(layer)
        _CACHE[key] = cls.compress_planes(em, xe, xo, coder=coder)
    return _CACHE[key]


def _level0_share(layer, q):
    """The share of non-zero symbols of level 0 (the largest tensor a layer codes) at step q, read from the device sink."""
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models import entropy_coding as ec
    key = ("share", layer, q)
    if key not in _CACHE:
        em, cls, xe, xo = _layer_case(layer)
        seen, orig = [], ec._DeviceSink.flush

        def spy(self):
            seen.append(torch.cat([t.reshape(-1) for t in self.sym]))
            return orig(self)
        ec._DeviceSink.flush = spy
        try:
            cls.compress_planes(em, xe, xo, coder="gpu", step=q)
        finally:
            ec._DeviceSink.flush = orig
        level0 = max(seen, key=lambda t: t.numel())
        assert level0.numel() == xo[0].numel()
        _CACHE[key] = _nonzero_share(level0)
    return _CACHE[key]


@pytest.mark.parametrize("n", [4, 40, 256])
@pytest.mark.parametrize("coder", ["host", "gpu"])
@pytest.mark.parametrize("layer", LAYERS)
def test_layer_round_trip_with_a_step(layer, coder, n):
    em, cls, xe, xo = _layer_case(layer)
    L, q = len(xo), n / 16.0
    s_xe, s_xo, xe_q, xo_q = cls.compress_planes(em, xe, xo, coder=coder, step=q)
    d_xe, d_xo = cls.decompress_planes(em, s_xe, s_xo, xe.shape, [t.shape for t in xo], coder=coder, step=q)
    assert torch.equal(d_xe, xe_q) and len(d_xo) == L and all(torch.equal(a, b) for a, b in zip(d_xo, xo_q))
    for i in range(L - 1):
        err = float((xo_q[i] - xo[i]).abs().max())
        print("%s %s n=%d level %d: max|xo_q - xo| = %.6f (bound %.6f)" % (layer, coder, n, i, err, q / 2 * (1 + 2.0 ** -20)))
        assert err <= q / 2 * (1 + 2.0 ** -20), (i, err)
    if n == 256:                                                                   # the coarsest step used here
        share = _level0_share(layer, q)
        print("%s: %.0f %% of the level-0 symbols are non-zero at step %g" % (layer, 100 * share, q))
        assert share > 0.2, share
    u_xe, u_xo, uxe_q, uxo_q = _unit_step(layer, coder)
    assert torch.equal(xe_q, uxe_q) and torch.equal(xo_q[L - 1], uxo_q[L - 1])     # xe and the coarsest level: step 1
    assert s_xe == u_xe and s_xo[L - 1] == u_xo[L - 1]
    size = lambda rows: sum(len(s) for lev in rows for pl in lev for s in pl)
    assert (size(s_xo[:L - 1]) < size(u_xo[:L - 1])) == (n > 16)                   # coarser: fewer bytes, finer: more


def test_layers_refuse_a_step_with_one_level():
    em, cls, xe, xo = _layer_case(LAYERS[1])
    with pytest.raises(ValueError, match="step"):
        cls.compress_planes(em, xe, xo[-1:], step=2.0)
    with pytest.raises(ValueError, match="step"):
        cls.compress_planes(em, xe, xo, step=0.3)


# ------------------------------------------------------------------------------------------------ 4. lldwt_code_cost
def test_code_cost_equals_the_integer_reference():
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models import entropy_coding as ec
    em = [n.entropymodel for n in _cond2().nets()]
    type(em[0])._coding_setup(em)
    tabs = em[0].__dict__["_rans_tables"]
    rng = np.random.default_rng(3)
    Z, n = 6, 1000
    idx = rng.integers(0, tabs.cdf.shape[0], size=(Z, n)).astype(np.int32)
    width = tabs.sizes[idx] - 2
    sym = (tabs.offsets[idx] + (rng.random((Z, n)) * width).astype(np.int32)).astype(np.int32)
    esc = rng.random((Z, n)) < 0.01                                                # ~1 % escapes, below and above the table
    sym = np.where(esc, np.where(rng.random((Z, n)) < 0.5, tabs.offsets[idx] - 1 - rng.integers(0, 50, (Z, n)),
                                 tabs.offsets[idx] + width + rng.integers(0, 50, (Z, n))), sym).astype(np.int32)
    cost = ops.cost_table(tabs.cdf, tabs.sizes)
    v = sym - tabs.offsets[idx]
    inside = (v >= 0) & (v < width)
    ref = np.where(inside, cost[idx, np.where(inside, v, 0)].astype(np.int64), ops.COST_ESCAPE).sum(1)
    assert 1 <= int((~inside).sum()) and np.array_equal(~inside, esc)
    ct = ec.device_cost_tables(tabs, torch.device(DEV))
    sums, escapes = ops.code_cost(torch.from_numpy(sym).to(DEV), torch.from_numpy(idx).to(DEV), *ct)
    assert np.array_equal(sums.cpu().numpy(), ref) and np.array_equal(escapes.cpu().numpy(), (~inside).sum(1))
    for z in range(Z):
        bits, e = ec.ideal_bits(sym[z], idx[z], tabs)
        got = (int(sums[z]) - e * ops.COST_ESCAPE) / ops.COST_ONE_BIT
        assert e == int(escapes[z]) and abs(got - bits) <= n * 2.0 ** -10, (z, got, bits)


# ------------------------------------------------------------------------------------------------ 5. the codec
AE_GAIN = 100.0


def _net(layer):
    """The layer's net with the deterministic filled weights, L = 3, and the last (linear) layer of the subband auto-encoders
    of the levels 0 .. L-2 scaled by AE_GAIN.  With the filled weights alone the coefficients of these images stay below 1
    (std 0.15 at level 0): every symbol is 0 from step 1 on and the containers sit on the floor that xe and the coarsest
    level set, so no step could be told from another.  The gain brings the levels a step reaches to the amplitude of the
    layer-level tests (std 15 to 17, as GAIN = 60 gives), where a trained codec at its operating point has them."""
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


def _codec_level0_share(net, img, q):
    """The share of non-zero level-0 symbols when the codec codes img at step q (read from the device sink)."""
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models import entropy_coding as ec
    seen, orig = [], ec._DeviceSink.flush

    def spy(self):
        seen.append(torch.cat([t.reshape(-1) for t in self.sym]))
        return orig(self)
    ec._DeviceSink.flush = spy
    try:
        codec.encode_images(net, img, coder="gpu", step=q)
    finally:
        ec._DeviceSink.flush = orig
    return _nonzero_share(max(seen, key=lambda t: t.numel()))


def _encoder_recon(net, img, q):
    """What the encoder itself reconstructs at step q: the strings API with recon=True, through the codec's I/O kernels."""
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.layers.lifting_dwt_nets import padded_size
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models.LiftingBasedDWT_net import \
        encode_strings_planes
    B, H, W, _ = img.shape
    nets = net.nets()
    Hp, Wp = padded_size([n.autoencoder for n in nets], H, W)
    with torch.no_grad():
        x = ops.u8hwc_to_ycc_pad(img.to(DEV).contiguous(), Hp, Wp)
        _, _, xhat = encode_strings_planes(nets, x, recon=True, step=q)
        return ops.ycc_to_u8hwc_crop(xhat.contiguous(), H, W).cpu()


@pytest.mark.parametrize("H,W", [(64, 64), (72, 88)])
@pytest.mark.parametrize("layer", LAYERS)
def test_codec_step_containers(layer, H, W):
    net = _net(layer)
    img = _images(2, H, W, H + W)
    plain = codec.encode_images(net, img)
    assert codec.encode_images(net, img, step=None) == plain and codec.encode_images(net, img, step=1) == plain
    assert codec.encode_images(net, img, step=1.0) == plain
    hdr = codec.read_header(plain[0])
    assert hdr["step"] == 1.0 and "step" not in hdr["arithmetic"]
    share = _codec_level0_share(net, img, 8.0)
    print("%s %dx%d: %.0f %% of the level-0 symbols are non-zero at step 8" % (layer, H, W, 100 * share))
    assert share > 0.2, share
    sizes = [[len(b) for b in plain]]
    for q in (2.0, 4.0, 8.0):
        blobs = codec.encode_images(net, img, step=q)
        sizes.append([len(b) for b in blobs])
        for b in blobs:
            h = codec.read_header(b)
            assert h["step"] == q and codec._split_step(h["arithmetic"]) == (int(q * 16), hdr["arithmetic"])
        dec = codec.decode_images(net, blobs)
        assert torch.equal(torch.stack(dec), _encoder_recon(net, img, q))
    print("%s %dx%d: bytes at steps 1, 2, 4, 8: %s" % (layer, H, W, sizes))
    for b in range(2):
        col = [s[b] for s in sizes]
        assert all(x > y for x, y in zip(col, col[1:])), col
    # containers of different steps in one call
    mixed = codec.decode_images(net, [plain[0], blobs[1], plain[1], blobs[0]])
    assert torch.equal(mixed[1], dec[1]) and torch.equal(mixed[3], dec[0])
    assert torch.equal(torch.stack([mixed[0], mixed[2]]), torch.stack(codec.decode_images(net, plain)))


@pytest.mark.parametrize("layer", LAYERS)
def test_an_edited_step_is_refused_or_decodes_differently(layer):
    net = _net(layer)
    img = _images(1, 64, 64, 3)
    blob = codec.encode_images(net, img, step=4.0)[0]
    good = codec.decode_images(net, [blob])[0]
    hdr, streams = codec.parse_container(blob)
    assert "step=64" in hdr["arithmetic"]
    assert codec.pack_container(hdr, streams) == blob
    edited = codec.pack_container(dict(hdr, arithmetic=hdr["arithmetic"].replace("step=64", "step=32")), streams)   # re-sealed
    assert codec.read_header(edited)["step"] == 2.0
    try:
        other = codec.decode_images(net, [edited])[0]
    except (ValueError, _lib.LLDWTError):              # a coder that runs out of stream, or one whose final state is wrong
        other = None
    assert other is None or not torch.equal(other, good)
    for bad in ("step=2048", "step=3", "step=abc", "step=64,step=64"):
        broken = codec.pack_container(dict(hdr, arithmetic=hdr["arithmetic"].replace("step=64", bad)), streams)
        with pytest.raises(ValueError, match="step"):
            codec.decode_images(net, [broken])


@pytest.mark.parametrize("overlap", [0, 16])
def test_tiled_with_a_step_decodes_regions(overlap):
    net = _net(LAYERS[2])
    img = _images(1, 128, 192, 9)
    blob = codec.encode_tiled(net, img, tile=64, overlap=overlap, step=2.5)[0]
    hdr = codec.read_header(blob)
    assert hdr["step"] == 2.5 and hdr["overlap"] == overlap and hdr["ny"] * hdr["nx"] >= 6
    assert len(blob) < len(codec.encode_tiled(net, img, tile=64, overlap=overlap)[0])
    full = codec.decode_tiled(net, blob)
    assert full.shape == (128, 192, 3)
    for y0, x0, h, w in ((0, 0, 128, 192), (40, 50, 60, 100), (64, 128, 64, 64), (127, 191, 1, 1)):
        assert torch.equal(codec.decode_tiled(net, blob, region=(y0, x0, h, w)), full[y0:y0 + h, x0:x0 + w])
    if not overlap:                                # every tile is the image encode_images codes at the same step
        tile0 = codec.encode_images(net, img[:, :64, :64].contiguous(), step=2.5)[0]
        assert torch.equal(codec.decode_images(net, [tile0])[0], full[:64, :64])


@pytest.mark.parametrize("layer", LAYERS)
def test_lossless_over_a_stepped_base_and_reduced_decodes(layer):
    net = _net(layer)
    img = _images(1, 72, 88, 21)
    blob = codec.encode_images(net, img, near=0, step=4.0)[0]
    hdr = codec.read_header(blob)
    assert hdr["near"] == 0 and hdr["base"]["step"] == 4.0
    assert torch.equal(codec.decode_images(net, [blob])[0], img[0])                        # bit for bit
    base = codec.encode_images(net, img, step=4.0)[0]
    assert torch.equal(codec.decode_images(net, [blob], refine=False)[0], codec.decode_images(net, [base])[0])
    half = codec.decode_images(net, [base], reduce=1)[0]
    assert half.shape == (36, 44, 3)
    # xe and the coarsest level keep the unit step: from reduce = L - 1 on, the decode is that of the unit-step container
    plain = codec.encode_images(net, img)[0]
    for k in (2, 3):
        assert torch.equal(codec.decode_images(net, [base], reduce=k)[0], codec.decode_images(net, [plain], reduce=k)[0])
    tiled = codec.encode_tiled(net, _images(1, 128, 128, 22), tile=64, near=2, step=4.0)[0]
    assert codec.read_header(tiled)["base"]["step"] == 4.0
    err = (codec.decode_tiled(net, tiled).int() - _images(1, 128, 128, 22)[0].int()).abs().max()
    assert int(err) <= 2


# ------------------------------------------------------------------------------------------------ 6. the byte target
@pytest.mark.parametrize("layer", LAYERS)
def test_target_bytes_finds_the_finest_grid_step_that_fits(layer):
    net = _net(layer)
    img = _images(1, 64, 64, 31)
    k0 = codec.STEP_GRID_K[0]
    n8, n9 = codec.STEP_GRID[8 - k0], codec.STEP_GRID[9 - k0]
    b8, b9 = (codec.encode_images(net, img, step=n / 16)[0] for n in (n8, n9))
    S8, S9 = len(b8), len(b9)
    print("%s: S8 = %d, S9 = %d bytes" % (layer, S8, S9))
    got = codec.encode_images(net, img, target_bytes=(S8 + S9) // 2)
    print("%s: T = %d -> %s" % (layer, (S8 + S9) // 2, codec.SEARCH_STATS))
    assert got == [b9]
    assert codec.encode_images(net, img, target_bytes=S9) == [b9]
    with pytest.raises(ValueError, match=r"target_bytes.*smallest achievable is \d+"):
        codec.encode_images(net, img, target_bytes=10)
    with pytest.raises(ValueError, match="step and target_bytes"):
        codec.encode_images(net, img, step=2.0, target_bytes=S9)
    with pytest.raises(ValueError, match="target_bytes"):
        codec.encode_images(net, img, near=0, target_bytes=S9)
    # a batch is searched image by image
    two = _images(2, 64, 64, 32)
    T = len(codec.encode_images(net, two[:1], step=2.0)[0])
    for b, blob in enumerate(codec.encode_images(net, two, target_bytes=T)):
        assert len(blob) <= T
        n = int(codec.read_header(blob)["step"] * 16)
        assert blob == codec.encode_images(net, two[b:b + 1], step=n / 16)[0]
        i = codec.STEP_GRID.index(n)
        assert i == 0 or len(codec.encode_images(net, two[b:b + 1], step=codec.STEP_GRID[i - 1] / 16)[0]) > T


def test_target_bytes_on_a_tiled_frame():
    net = _net(LAYERS[2])
    img = _images(1, 128, 192, 41)
    ref = codec.encode_tiled(net, img, tile=64, step=4.0)[0]
    T = len(ref) + 3
    blob = codec.encode_tiled(net, img, tile=64, target_bytes=T)[0]
    hdr = codec.read_header(blob)
    print("tiled: T = %d -> %s" % (T, codec.SEARCH_STATS))
    assert len(blob) <= T and hdr["step"] <= 4.0 and hdr["ny"] * hdr["nx"] == 6
    n = int(hdr["step"] * 16)
    i = codec.STEP_GRID.index(n)
    assert blob == codec.encode_tiled(net, img, tile=64, step=n / 16)[0]
    assert i == 0 or len(codec.encode_tiled(net, img, tile=64, step=codec.STEP_GRID[i - 1] / 16)[0]) > T
    assert codec.decode_tiled(net, blob).shape == (128, 192, 3)
    with pytest.raises(ValueError, match=r"target_bytes.*smallest achievable"):
        codec.encode_tiled(net, img, tile=64, target_bytes=50)
