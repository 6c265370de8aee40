"""float64 references for the rate kernels (Gaussian conditional, factorized EntropyBottleneck) and the GDN: the yardstick of
tests/test_rate_ref_host.py and tests/test_gpu_rate_domain.py.  No device code.

The formulas are the oracle's (oracle/entropy.py, oracle/subband_ae.py are dtype-agnostic); this file only feeds them:
  * quantisation is done in fp32 (round(x - mu) + mu, x + noise are exact IEEE operations that the host and the device do
    alike; a float64 subtraction would resolve ties differently), then v, mu, sigma and the parameters are cast;
  * the bounds are the fp32 constants the kernels compile in (double(float32(0.11)) < 0.11): an element set exactly at a bound
    lands on the same side of the LowerBound gradient rule in both;
  * evaluated in float32 the same functions are the fp32 oracle: its distance from the float64 result on the same inputs is
    what fp32 costs the formula, and sets the bars (4 x that, never tighter than the project's parity bars)."""
import contextlib
import functools

import numpy as np
import torch

from oracle import entropy, subband_ae, weights


def f32(v):
    """The double that holds float32(v)."""
    return float(np.float32(v))


SCALE_BOUND = f32(0.11)
LIK_BOUND = f32(1e-9)
PEDESTAL = 2.0 ** -36                                        # (2^-18)^2, exact in fp32
F64, F32 = torch.float64, torch.float32


def nonneg_bound(minimum=0.0):
    """The NonNegativeParametrizer's (bound, pedestal) as the fp32 numbers the library passes to its kernels."""
    return f32(np.sqrt(np.float64(np.float32(minimum)) + PEDESTAL)), PEDESTAL


@contextlib.contextmanager
def fp32_bounds(lik_bound=LIK_BOUND):
    """The oracle's constants replaced by their fp32 values for the duration (lik_bound=0: the unbounded likelihood)."""
    saved = (entropy.SCALE_BOUND, entropy.LIKELIHOOD_BOUND, subband_ae.nonneg_bound)
    entropy.SCALE_BOUND, entropy.LIKELIHOOD_BOUND, subband_ae.nonneg_bound = SCALE_BOUND, lik_bound, nonneg_bound
    try:
        yield
    finally:
        entropy.SCALE_BOUND, entropy.LIKELIHOOD_BOUND, subband_ae.nonneg_bound = saved


# ------------------------------------------------------------------------------------------------ bars
def bits_bar(err32):
    """|kernel - float64| in bits: 4 x the fp32 oracle's error on the same inputs, floor 1e-4 (the parity bar of the rates)."""
    return max(4.0 * err32, 1e-4)


def grad_bar(err32_rel):
    """Relative to the largest |reference| of the compared group: 4 x the fp32 oracle's, floor 2e-4 (rate-gradient parity bar)."""
    return max(4.0 * err32_rel, 2e-4)


def gdn_bar(err32):
    return max(4.0 * err32, 2e-6)


def kink(lik_raw):
    """Elements whose float64 likelihood is within 1e-3 relative of the 1e-9 floor: fp32 and float64 may sit on different sides
    of the floor's gradient rule there, so the gradient comparisons leave them out (forward bits are continuous: no exclusion)."""
    return (lik_raw - LIK_BOUND).abs() <= 1e-3 * LIK_BOUND


def rel_err(a, ref, mask=None):
    """max |a - ref| over the (masked) group, relative to the group's own max |ref| (0 if the reference is 0 and a matches)."""
    a, ref = a.double(), ref.double()
    if mask is not None:
        a, ref = a[mask], ref[mask]
    if ref.numel() == 0:
        return 0.0
    d, m = (a - ref).abs().max().item(), ref.abs().max().item()
    return d / m if m > 0 else (0.0 if d == 0 else float("inf"))


# ------------------------------------------------------------------------------------------------ Gaussian conditional
BUCKET_NAMES = ("< 0.11", "[0.11, 1)", "[1, 16)", "[16, 256)", "[256, 4096]")
_EDGES = (SCALE_BOUND, 1.0, 16.0, 256.0)


def bucket_index(sigma):
    """Index into BUCKET_NAMES for every fp32 sigma."""
    return torch.bucketize(sigma, torch.tensor(_EDGES, dtype=F32), right=True)


def gauss_quant(x, mu, noise=None):
    """compressai quantize in fp32: training x + noise, eval round(x - mu) + mu."""
    return x + noise if noise is not None else torch.round(x - mu) + mu


def gauss_eval(v, sigma, mu, dtype=F64, gbits=None, train=True):
    """bits (and, given gbits, dx / dsigma / dmu by autograd under the pass-through LowerBound rule) of quantised fp32 v.
    eval: v = round(x - mu) + mu, so dv/dx = 0 and dv/dmu = 1 (the two mu paths cancel)."""
    grad = gbits is not None
    v_, s_, m_ = (t.to(dtype).clone().requires_grad_(grad) for t in (v, sigma, mu))
    with fp32_bounds():
        bits = -torch.log2(entropy.gaussian_likelihood(v_, s_, m_))
    out = {"bits": bits.detach()}
    if grad:
        bits.backward(gbits.to(dtype))
        out["dx"] = v_.grad if train else torch.zeros_like(v_.grad)
        out["dsigma"] = s_.grad
        out["dmu"] = m_.grad if train else m_.grad + v_.grad
    return out


def gauss_lik_raw(v, sigma, mu):
    """float64 likelihood before its 1e-9 floor."""
    with fp32_bounds(0.0), torch.no_grad():
        return entropy.gaussian_likelihood(v.double(), sigma.double(), mu.double())


def pack_params(sigma, mu):
    """(P,B,C,h,w) x 2 -> (P,B,2C,h,w): sigma on the even, mu on the odd channels."""
    P, B, C, h, w = sigma.shape
    return torch.stack([sigma, mu], 3).reshape(P, B, 2 * C, h, w).contiguous()


@functools.lru_cache(maxsize=None)
def gauss_inputs(shape, mu_scale, seed, sigma_lo=None, sigma_hi=None, nsig=12.0):
    """fp32 (x, sigma, mu, noise) over the argument domain.  Default: sigma log-uniform within each of the five buckets (the first
    holds sigma <= 0 and (0, 0.11)), elements exactly at 0.11f and at its two fp32 neighbours, |mu| <= mu_scale, |x - mu| up
    to nsig * max(sigma, 0.11) (denser near 0) and 256 exact ties x - mu = k + 0.5.  With sigma_lo / sigma_hi: one log-uniform
    range and no planted elements.  Read-only: shared between tests."""
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))
    u = torch.rand(shape, generator=g, dtype=F64)
    if sigma_lo is None:
        bk = torch.randint(0, 5, shape, generator=g)
        lo = torch.tensor([1e-4, SCALE_BOUND, 1.0, 16.0, 256.0], dtype=F64)[bk].log()
        hi = torch.tensor([SCALE_BOUND, 1.0, 16.0, 256.0, 4096.0], dtype=F64)[bk].log()
        sigma = torch.exp(lo + u * (hi - lo)).float().clamp_(max=4096.0)
        nonpos = (bk == 0) & (torch.rand(shape, generator=g) < 0.4)
        sigma = torch.where(nonpos, -3.0 * torch.rand(shape, generator=g), sigma)
        flat, idx = sigma.view(-1), torch.randperm(n, generator=g)[:128]
        sb = torch.tensor(SCALE_BOUND, dtype=F32)
        flat[idx[:32]] = sb
        flat[idx[32:64]] = torch.nextafter(sb, torch.tensor(0.0))
        flat[idx[64:96]] = torch.nextafter(sb, torch.tensor(1.0))
        flat[idx[96:]] = 0.0
    else:
        sigma = torch.exp(np.log(sigma_lo) + u * (np.log(sigma_hi) - np.log(sigma_lo))).float()
    mu = (torch.rand(shape, generator=g) * 2 - 1) * mu_scale
    t = nsig * torch.rand(shape, generator=g) ** 2
    sgn = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    x = mu + sgn * t * sigma.clamp(min=SCALE_BOUND)
    if sigma_lo is None:
        idx = torch.randperm(n, generator=g)[:256]
        mf, xf = mu.view(-1), x.view(-1)
        mf[idx] = torch.round(mf[idx] * 8) / 8                       # mu + k + 0.5 is then exact in fp32
        xf[idx] = mf[idx] + (torch.randint(-20, 21, (256,), generator=g).float() + 0.5)
    noise = torch.rand(shape, generator=g) - 0.5
    return x.contiguous(), sigma.contiguous(), mu.contiguous(), noise.contiguous()


def per_bucket(err, sigma):
    """{bucket name: max of err over the bucket} for the buckets that have elements."""
    bi = bucket_index(sigma)
    return {BUCKET_NAMES[b]: err[bi == b].max().item() for b in range(5) if bool((bi == b).any())}


@functools.lru_cache(maxsize=None)
def gauss_case(shape, mu_scale, seed, train, grad=False, sigma_lo=None, sigma_hi=None, nsig=12.0):
    """One Gaussian case, computed once and shared: inputs, the quantised v, the float64 reference and, per sigma bucket, the fp32
    oracle's distance from it ("err32": bits; with grad also "gerr32": {dx, dsigma, dmu} relative to the bucket's max |ref|
    outside the kink mask "excl").  Read-only."""
    x, sigma, mu, noise = gauss_inputs(shape, mu_scale, seed, sigma_lo, sigma_hi, nsig)
    v = gauss_quant(x, mu, noise if train else None)
    gb = None
    if grad:
        gb = torch.randn(shape, generator=torch.Generator().manual_seed(seed + 7))      # both signs: both sides of the floor rule
    r64, r32 = gauss_eval(v, sigma, mu, F64, gb, train), gauss_eval(v, sigma, mu, F32, gb, train)
    out = dict(x=x, sigma=sigma, mu=mu, noise=noise if train else None, v=v, gbits=gb, ref=r64, bucket=bucket_index(sigma),
               err32=per_bucket((r32["bits"].double() - r64["bits"]).abs(), sigma))
    if grad:
        out["excl"] = kink(gauss_lik_raw(v, sigma, mu))
        out["gerr32"] = {k: {BUCKET_NAMES[b]: rel_err(r32[k], r64[k], (out["bucket"] == b) & ~out["excl"]) for b in range(5)}
                         for k in ("dx", "dsigma", "dmu")}
    return out


# ------------------------------------------------------------------------------------------------ factorized (EntropyBottleneck)
EB_FLOATS = 59
_F = entropy.EB_FILTERS


def eb_pack(sd, prefix=""):
    """(C,59): m0(3) b0(3) f0(3) | m1(9) b1(3) f1(3) | m2 .. | m3 .. | m4(3) b4(1) median(1), matrices row-major."""
    C = sd[prefix + "_matrix0"].shape[0]
    parts = []
    for i in range(5):
        parts += [sd[prefix + "_matrix%d" % i].reshape(C, -1), sd[prefix + "_bias%d" % i].reshape(C, -1)]
        if i < 4:
            parts.append(sd[prefix + "_factor%d" % i].reshape(C, -1))
    parts.append(sd[prefix + "quantiles"][:, :, 1].reshape(C, 1))
    return torch.cat(parts, 1).contiguous()


def eb_unpack(packed):
    """Views of a (C,59) tensor under the oracle's state-dict names (autograd flows back into ``packed``)."""
    C, o, sd = packed.shape[0], 0, {}
    for i in range(5):
        n = _F[i + 1] * _F[i]
        sd["_matrix%d" % i] = packed[:, o:o + n].reshape(C, _F[i + 1], _F[i])
        o += n
        sd["_bias%d" % i] = packed[:, o:o + _F[i + 1]].reshape(C, _F[i + 1], 1)
        o += _F[i + 1]
        if i < 4:
            sd["_factor%d" % i] = packed[:, o:o + _F[i + 1]].reshape(C, _F[i + 1], 1)
            o += _F[i + 1]
    assert o == EB_FLOATS - 1
    return sd


EB_SLOT_NAMES = tuple(n for i in range(5) for n in (["m%d" % i] * (_F[i + 1] * _F[i]) + ["b%d" % i] * _F[i + 1] +
                                                      (["f%d" % i] * _F[i + 1] if i < 4 else []))) + ("median",)


@functools.lru_cache(maxsize=None)
def eb_params(kind, P=2, C=3):
    """(P,C,59) raw fp32 parameters.  "init": the initialisation with the deterministic perturbation of the parity tests.
    "stress": on top of it one matrix entry above softplus' threshold of 20, four near -10 (softplus ~ 4e-5), factors +-3
    (tanh saturated at +-0.995), biases +-5 behind the first layer, medians +-37.25; the first layer's biases place the density
    around the median so that the +-15 span sees likelihoods on both sides of the floor."""
    out = []
    for p in range(P):
        sd = weights.fill_by_name({"p%d.e." % p + a: b for a, b in entropy.eb_init_state(C).items()})
        sd = {k.split(".e.")[1]: v.clone() for k, v in sd.items()}
        if kind == "stress":
            for c in range(C):
                s = 1.0 if (c + p) % 2 == 0 else -1.0
                med = 37.25 * s
                sd["quantiles"][c, 0, 1] = med
                sd["_matrix1"][c, 0, 0] = 20.5 + c
                sd["_matrix2"][c, 1, :] = torch.tensor([-10.25, -10.0, -9.75])
                sd["_matrix3"][c, 2, 0] = -10.5
                for i in range(4):
                    for j in range(3):
                        sd["_factor%d" % i][c, j, 0] = 3.0 if (i + j + c) % 2 == 0 else -3.0
                for i in range(1, 5):
                    for j in range(_F[i + 1]):
                        sd["_bias%d" % i][c, j, 0] = 5.0 if (i + j + c + p) % 2 == 0 else -5.0
                m0 = torch.nn.functional.softplus(sd["_matrix0"][c, :, 0])
                sd["_bias0"][c, :, 0] = -m0 * med + torch.tensor([0.75, -0.5, 0.25]) * s
        else:
            assert kind == "init"
        out.append(eb_pack(sd))
    return torch.stack(out, 0).contiguous()


def eb_quant(x, eb, noise=None):
    """x (P,B,C,h,w), eb (P,C,59): training x + noise, eval round(x - median) + median, in fp32."""
    med = eb[:, :, 58][:, None, :, None, None]
    return x + noise if noise is not None else torch.round(x - med) + med


def _eb_lik(v, packed, lik_bound=LIK_BOUND):
    P, B, C, h, w = v.shape
    vv = v.permute(0, 2, 1, 3, 4).reshape(P * C, 1, B * h * w)
    with fp32_bounds(lik_bound):
        lik = entropy.eb_likelihood(vv, eb_unpack(packed.reshape(P * C, EB_FLOATS)), "")
    return lik.reshape(P, C, B, h, w).permute(0, 2, 1, 3, 4)


def eb_eval(v, eb, dtype=F64, gbits=None, train=True):
    """bits (and, given gbits, dx and the gradient of the RAW packed parameters -- softplus and tanh inside the tape; the median
    only enters the quantisation and is detached there: its slot is 0) of quantised fp32 v (P,B,C,h,w); eb (P,C,59)."""
    grad = gbits is not None
    v_, e_ = v.to(dtype).clone().requires_grad_(grad), eb.to(dtype).clone().requires_grad_(grad)
    bits = -torch.log2(_eb_lik(v_, e_))
    out = {"bits": bits.detach()}
    if grad:
        bits.backward(gbits.to(dtype))
        out["dx"] = v_.grad if train else torch.zeros_like(v_.grad)
        out["deb"] = e_.grad if e_.grad is not None else torch.zeros_like(e_)
    return out


def eb_lik_raw(v, eb):
    with torch.no_grad():
        return _eb_lik(v.double(), eb.double(), 0.0)


@functools.lru_cache(maxsize=None)
def eb_inputs(kind, hw, span, seed):
    """x (2,2,3,1,hw) = median + span * U(-1, 1), its first four elements of every row at the offsets -128, -127, 127, 128 from the
    median (the two ends of the eval table and the first integers beyond it), and noise.  Read-only."""
    eb = eb_params(kind)
    P, C = eb.shape[:2]
    g = torch.Generator().manual_seed(seed)
    med = eb[:, :, 58][:, None, :, None, None]
    x = med + span * (torch.rand(P, 2, C, 1, hw, generator=g) * 2 - 1)
    x[..., :4] = med + torch.tensor([-128.0, -127.0, 127.0, 128.0])
    noise = torch.rand(x.shape, generator=g) - 0.5
    return x.contiguous(), noise.contiguous()


@functools.lru_cache(maxsize=None)
def eb_case(kind, hw, span, seed, train, grad=False):
    """One factorized case: inputs, the float64 reference and the fp32 oracle's distance from it.  With grad the incoming gradient is
    zero on the kink elements ("excl"), so that they drop out of the parameter sums as well; "gerr32": dx relative to the tensor's
    max |ref|, deb per slot relative to the slot's max |ref| over (plane, channel)."""
    eb = eb_params(kind)
    x, noise = eb_inputs(kind, hw, span, seed)
    v = eb_quant(x, eb, noise if train else None)
    gb = excl = None
    if grad:
        excl = kink(eb_lik_raw(v, eb))
        gb = torch.randn(x.shape, generator=torch.Generator().manual_seed(seed + 7)) + 0.5
        gb = torch.where(excl, torch.zeros(()), gb).contiguous()
    r64, r32 = eb_eval(v, eb, F64, gb, train), eb_eval(v, eb, F32, gb, train)
    out = dict(eb=eb, x=x, noise=noise if train else None, v=v, gbits=gb, excl=excl, ref=r64,
               err32=(r32["bits"].double() - r64["bits"]).abs().max().item())
    if grad:
        out["gerr32"] = {"dx": rel_err(r32["dx"], r64["dx"]),
                         "deb": [rel_err(r32["deb"][:, :, i], r64["deb"][:, :, i]) for i in range(EB_FLOATS)]}
    return out


# ------------------------------------------------------------------------------------------------ GDN
def gdn_eval(x, beta, gamma, inverse, dtype=F64, gy=None, beta_min=1e-6):
    """graphs/layers/gdn.py through the oracle, plane by plane: x (P,B,C,h,w), beta (P,C), gamma (P,C,C) raw (reparametrised
    inside, pass-through rule below the bounds) -> y and, given gy, dx / dbeta / dgamma."""
    grad = gy is not None
    x_, b_, g_ = (t.to(dtype).clone().requires_grad_(grad) for t in (x, beta, gamma))
    with fp32_bounds():
        y = torch.stack([subband_ae.gdn(x_[p], b_[p], g_[p], inverse, beta_min) for p in range(x.shape[0])], 0)
    out = {"y": y.detach()}
    if grad:
        y.backward(gy.to(dtype))
        out.update(dx=x_.grad, dbeta=b_.grad, dgamma=g_.grad)
    return out


@functools.lru_cache(maxsize=None)
def gdn_inputs(P, B, C, h, w, seed, beta_min=1e-6, edges=True):
    """x and raw beta / gamma, with ``edges`` some entries below their bounds, below zero and exactly at the bounds.  Read-only."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(P, B, C, h, w, generator=g) - 0.5) * 4
    beta = 0.3 + torch.rand(P, C, generator=g) * 1.2
    gamma = torch.rand(P, C, C, generator=g) * (0.6 / C ** 0.5)
    if not edges:
        return x.contiguous(), beta.contiguous(), gamma.contiguous()
    bb, gb = nonneg_bound(beta_min)[0], nonneg_bound(0.0)[0]
    bf, gf = beta.view(-1), gamma.view(-1)
    for k, val in enumerate((-0.7, 0.5 * bb, bb)):                  # below zero, below the bound, at the bound
        bf[k::7] = val
    for k, val in enumerate((-0.2, 0.5 * gb, gb, 0.0)):
        gf[k::11] = val
    if C == 1:                                                      # one entry each: plane 0 below the bounds, the last ordinary
        beta[0, 0], gamma[0, 0, 0] = 0.5 * bb, -0.2
        beta[-1, 0], gamma[-1, 0, 0] = 0.9, 0.3
    elif C == 2:
        beta[:] = torch.tensor([0.8, 0.5 * bb])
        gamma[:] = torch.tensor([[0.3, -0.2], [gb, 0.25]])
    return x.contiguous(), beta.contiguous(), gamma.contiguous()


@functools.lru_cache(maxsize=None)
def gdn_case(P, B, C, h, w, inverse, seed, grad=False):
    x, beta, gamma = gdn_inputs(P, B, C, h, w, seed)
    gy = torch.randn(x.shape, generator=torch.Generator().manual_seed(seed + 7)) if grad else None
    r64, r32 = gdn_eval(x, beta, gamma, inverse, F64, gy), gdn_eval(x, beta, gamma, inverse, F32, gy)
    out = dict(x=x, beta=beta, gamma=gamma, gy=gy, ref=r64, err32=(r32["y"].double() - r64["y"]).abs().max().item())
    if grad:
        out["gerr32"] = {k: rel_err(r32[k], r64[k]) for k in ("dx", "dbeta", "dgamma")}
    return out


# ------------------------------------------------------------------------------------------------ the cases both test files use
SWEEP_FWD, SWEEP_BWD = (2, 2, 3, 64, 64), (2, 2, 3, 32, 32)
MU_SCALES = (1.0, 1000.0)
SEED_GAUSS_FWD, SEED_GAUSS_BWD, SEED_EB_FWD, SEED_EB_BWD, SEED_GDN, SEED_GDN_TRAIN = 11, 12, 21, 22, 31, 33
EB_KINDS, EB_SPANS = ("init", "stress"), (15.0, 200.0, 4000.0)
EB_HW_FWD, EB_HW_BWD, EB_SPAN_BWD = (5, 117, 8196), (5, 300, 2125), 15.0
GDN_FWD = tuple((2, 2, C, 1, hw) for C in (1, 6, 192) for hw in (5, 300)) + ((1, 1, 2, 1, 262144 + 300),)
GDN_TRAIN = ((2, 2, 6, 9, 21), (2, 2, 192, 4, 6))
