"""CPU (no GPU): rate-distortion optimised quantisation on the host -- the checks of the `rdo` argument and
the tensor-op restatement of the rule (entropy_coding._finish_step with rdo, which code_tree_level_generic runs and the GPU
tests hold both kernels against) on CPU tensors against a float64 evaluation of the Lagrangian over the two candidates.

The rule (all fp32): v = (y - mu) * inv_q, s0 = rint(v), s1 = s0 - sign(s0), t = 1 + 2 sign(s0) (v - s0),
dc = cost[idx][s0] - cost[idx][s1], sym = s1 where (float)dc * k > t with k = rho * 2^-16, s0 elsewhere and where s0 == 0.
In exact arithmetic that is J(s1) < J(s0) for J(s) = (v - s)^2 + rho * bits(s) (in units of q^2): the squared error grows by
(v - s1)^2 - (v - s0)^2 = t.  The fp32 rule rounds dc * k and t once each (relative error 2^-24 each, |t| <= 2, rho * bits <=
4 * 32), so the two can disagree only where |rho dc / 2^16 - t| is below ~1e-5; the band asked for is 1e-4."""
import numpy as np
import pytest
import torch

from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import codec, ops
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.entropy_models import GaussianConditional
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models import entropy_coding as ec
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models import LiftingBasedDWT_net as net_mod

SIGMAS = (0.3, 0.6, 1.0, 2.0, 5.0, 15.0)
DRAWS = 200000
_CACHE = {}


# ------------------------------------------------------------------------------------------------ the argument
@pytest.mark.parametrize("rdo,m", [(1 / 64, 1), (13 / 64, 13), (1, 64), (4, 256), (4.0, 256)])
def test_rdo_values_on_the_grid_are_accepted(rdo, m):
    assert codec.check_rdo(rdo) == m
    k = ops.rdo_scale(rdo)
    assert k == m / 64 / 65536 and float(torch.tensor(k, dtype=torch.float32)) == k           # exact in fp32
    assert k * 2.0 ** 22 == m


def test_rdo_off():
    assert codec.check_rdo(None) == 0 and codec.check_rdo(0) == 0 and codec.check_rdo(0.0) == 0
    with pytest.raises(ValueError, match="rdo"):            # the kernels' scale has no "off": the callers do not get there
        ops.rdo_scale(0)


@pytest.mark.parametrize("bad", [0.1, 4.5, -1, float("nan"), "fast", 1 / 128, 4 + 1 / 64])
def test_rdo_values_off_the_grid_are_refused(bad):
    with pytest.raises(ValueError, match="rdo"):
        codec.check_rdo(bad)
    with pytest.raises(ValueError, match="rdo"):
        ops.rdo_scale(bad)
    with pytest.raises(ValueError, match="rdo"):
        net_mod._check_rdo(bad, 3)


def test_rdo_with_one_level_is_refused_before_any_device_call():
    """With dwtlevels = 1 there is no level below the coarsest: ValueError naming rdo from the codec's argument check and from
    each layer's compress_planes, which gets no tensor here (a device call would fail on None, not with this message)."""
    with pytest.raises(ValueError, match="rdo.*dwtlevels"):
        codec._rdo_arg(13 / 64, 1)
    assert codec._rdo_arg(13 / 64, 2) == 13 / 64 and codec._rdo_arg(0, 1) is None and codec._rdo_arg(None, 1) is None
    with pytest.raises(ValueError, match="rdo.*dwtlevels"):
        net_mod.onlyEZWT.compress_planes([], None, [None], rdo=13 / 64)
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
    net = net_mod.LiftingBasedDWTNetWrapper(make_config(dwtlevels=1, mode="validate", entropy_layer="onlyEZWT")).eval()   # CPU
    img = torch.zeros(1, 32, 32, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="rdo.*dwtlevels"):
        codec.encode_images(net, img, rdo=13 / 64)
    with pytest.raises(ValueError, match="rdo.*dwtlevels"):
        codec.encode_tiled(net, img, tile=32, rdo=13 / 64)
    with pytest.raises(ValueError, match="rdo"):
        codec.encode_images(net, img, rdo=0.1)
    with pytest.raises(ValueError, match="rdo.*dwtlevels"):
        net_mod._check_rdo(13 / 64, 1)
    assert net_mod._check_rdo(None, 1) is None and net_mod._check_rdo(0, 1) is None and net_mod._check_rdo(0.25, 2) == 0.25


# ------------------------------------------------------------------------------------------------ the rule
class _Keep:
    """The encoder side of a sink: keeps what one step hands it."""
    decoding = False

    def step(self, idx, sym=None):
        self.idx, self.sym = idx, sym
        return sym


def _model():
    if "em" not in _CACHE:
        em = GaussianConditional(None)
        tabs = ec._Tables(em, net_mod.get_scale_table())
        cost = ops.cost_table(tabs.cdf, tabs.sizes)
        _CACHE["em"] = (em, tabs, tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))
                                        for a in (cost, tabs.sizes, tabs.offsets)))
    return _CACHE["em"]


def _draws(n16):
    """Per sigma / q in SIGMAS DRAWS coefficients: (sigma, mu, y) fp32 of shape (1, 1, len(SIGMAS), DRAWS), at the step n16 / 16."""
    key = ("draws", n16)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(100 + n16)
        q = n16 / 16.0
        sigma = (torch.tensor(SIGMAS, dtype=torch.float32) * q).reshape(1, 1, -1, 1).expand(1, 1, len(SIGMAS), DRAWS).contiguous()
        mu = (torch.rand(1, 1, len(SIGMAS), DRAWS, generator=g) - 0.5) * 8
        y = mu + sigma * torch.randn(1, 1, len(SIGMAS), DRAWS, generator=g)
        _CACHE[key] = (sigma, mu, y)
    return _CACHE[key]


@pytest.mark.parametrize("n16", [16, 24])
@pytest.mark.parametrize("m", [4, 8, 13, 64, 256])
def test_restatement_equals_the_float64_lagrangian(m, n16):
    em, tabs, (cost, sizes, offsets) = _model()
    sigma, mu, y = _draws(n16)
    q, inv_q = ops.step_pair(n16 / 16.0)
    rho = m / 64.0
    sink = _Keep()
    val = ec._finish_step(em, sink, sigma, mu, y, n16 / 16.0, (ops.rdo_scale(rho), cost, sizes, offsets))
    sym = sink.sym.permute(0, 1, 3, 2)
    idx = sink.idx.permute(0, 1, 3, 2)
    plain = _Keep()
    ec._finish_step(em, plain, sigma, mu, y, n16 / 16.0)
    assert torch.equal(plain.idx, sink.idx)                                     # the index does not depend on the choice
    s0 = plain.sym.permute(0, 1, 3, 2)
    assert torch.equal(val, sym.float() * q + mu)
    v = (y - mu) * inv_q                                                        # the rounded fp32 product the rule is stated on
    assert torch.equal(s0, torch.round(v).int())
    # float64 over the two candidates, costs looked up in numpy
    c = cost.numpy().astype(np.int64)
    ix, o, sz = idx.numpy(), offsets.numpy().astype(np.int64), sizes.numpy().astype(np.int64)

    def bits(s):
        col = s - o[ix]
        ok = (col >= 0) & (col < sz[ix] - 2) & (col < c.shape[1])
        return np.where(ok, c[ix, np.where(ok, col, 0)], ops.COST_ESCAPE)
    s0n = s0.numpy().astype(np.int64)
    s1n = s0n - np.sign(s0n)
    v64 = v.numpy().astype(np.float64)
    b0, b1 = bits(s0n), bits(s1n)
    j0 = (v64 - s0n) ** 2 + rho * b0 / 65536.0
    j1 = (v64 - s1n) ** 2 + rho * b1 / 65536.0
    want = np.where((j1 < j0) & (s0n != 0), s1n, s0n)
    got = sym.numpy().astype(np.int64)
    t = 1.0 + 2.0 * np.sign(s0n) * (v64 - s0n)
    band = (np.abs(rho * (b0 - b1) / 65536.0 - t) < 1e-4) & (s0n != 0)
    decided = int((s0n != 0).sum())
    differ = got != want
    print("m=%d n=%d: %.2f %% of the decided coefficients moved, %d in the tie band (%.4f %%), %d disagree"
          % (m, n16, 100.0 * (got != s0n).sum() / decided, int(band.sum()), 100.0 * band.sum() / decided, int(differ.sum())))
    assert not (differ & ~band).any()
    assert band.sum() <= 0.001 * decided
    assert (bits(got) <= b0).all()                                              # never a longer code than the plain symbol's
    assert float(np.abs(v64 - got).max()) <= 1.5
    assert (got != s0n).any() and all((s0n[0, 0, j] != 0).any() for j in range(len(SIGMAS)))     # every sigma takes part


def test_unit_step_is_the_literal_quantiser():
    """At step 1 the one body of _finish_step gives what compressai's contract states without a step: build_indexes(sigma),
    round(y - mu), symbol + mu -- no product with 1 is needed for that (it would be exact anyway)."""
    em = _model()[0]
    sigma, mu, y = (t[..., :5000] for t in _draws(16))
    sink = _Keep()
    val = ec._finish_step(em, sink, sigma, mu, y)
    sym = torch.round(y - mu)
    assert torch.equal(sink.idx, em.build_indexes(sigma).permute(0, 1, 3, 2))
    assert sink.sym.dtype == torch.int32 and torch.equal(sink.sym, sym.int().permute(0, 1, 3, 2))
    assert torch.equal(val, sym + mu)
    again = _Keep()
    assert torch.equal(ec._finish_step(em, again, sigma, mu, y, 1.0), val) and torch.equal(again.sym, sink.sym)


@pytest.mark.parametrize("n16", [16, 23, 40])
@pytest.mark.parametrize("rdo", [False, True])
def test_scalar_step_equals_the_same_step_as_constant_pairs(n16, rdo):
    """A number and the pair of constant tensors holding ops.step_pair of it go through the same arithmetic: equal indexes,
    symbols and values, with the rule of 7.1.7 and without."""
    em, _, (cost, sizes, offsets) = _model()
    sigma, mu, y = (t[..., :20000] for t in _draws(n16))
    ra = (ops.rdo_scale(13 / 64), cost, sizes, offsets) if rdo else None
    q, inv_q = ops.step_pair(n16 / 16.0)
    pair = (torch.full((1, 1, 1, y.shape[3]), q), torch.full((1, 1, 1, y.shape[3]), inv_q))
    a, b = _Keep(), _Keep()
    va = ec._finish_step(em, a, sigma, mu, y, n16 / 16.0, ra)
    vb = ec._finish_step(em, b, sigma, mu, y, pair, ra)
    assert torch.equal(a.idx, b.idx) and torch.equal(a.sym, b.sym) and torch.equal(va, vb)
    assert bool((a.sym != 0).any())
    if rdo:
        plain = _Keep()
        ec._finish_step(em, plain, sigma, mu, y, n16 / 16.0)
        assert not torch.equal(plain.sym, a.sym)                                 # the rule took part


def test_lookup_and_choice_on_a_small_table():
    """The lookup's four exits and the choice's sign handling, by hand: table 0 holds symbols -1 .. 2, table 1 symbol 5 only."""
    cost = torch.tensor([[3 << 16, 1 << 16, 2 << 16, 6 << 16, 0], [1 << 16, 0, 0, 0, 0]], dtype=torch.int32)
    sizes = torch.tensor([6, 3], dtype=torch.int32)
    offsets = torch.tensor([-1, 5], dtype=torch.int32)
    idx = torch.tensor([0, 0, 0, 0, 0, 1, 1, 2, -1])
    sym = torch.tensor([-1, 0, 2, 3, -2, 5, 6, 0, 0])
    E = ops.COST_ESCAPE
    assert ops.rdo_lookup(cost, sizes, offsets, idx, sym).tolist() == [3 << 16, 1 << 16, 6 << 16, E, E, 1 << 16, E, E, E]
    k = ops.rdo_scale(0.25)
    v = torch.tensor([1.6, 1.6, -0.9, -0.9, 0.3, 3.0])
    s0 = torch.round(v)
    c0 = torch.tensor([6 << 16, 2 << 16, 3 << 16, 2 << 16, 9 << 16, E], dtype=torch.int32)
    c1 = torch.tensor([2 << 16, 2 << 16, 1 << 16, 1 << 16, 0, E], dtype=torch.int32)
    # t = 0.2, 0.2, 0.8, 0.8, -, 1;  rho * bits saved = 1, 0, 0.5, 0.25, -, 0
    assert ops.rdo_choose(v, s0, c0, c1, k).tolist() == [1.0, 2.0, -1.0, -1.0, 0.0, 3.0]
    assert ops.rdo_choose(v, s0, c0, c1, ops.rdo_scale(0.5)).tolist() == [1.0, 2.0, 0.0, -1.0, 0.0, 3.0]
