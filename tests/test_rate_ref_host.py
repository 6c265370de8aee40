"""CPU: the float64 reference of the rate and GDN kernels (tests/rate_ref.py) checked against the fp32 oracle, and the yardsticks of
tests/test_gpu_rate_domain.py: per sigma bucket / parameter set, the fp32 oracle's distance from float64 on the very inputs the
GPU tests use.  The GPU bars are 4 x these (never below the project's parity bars); they are printed here (pytest -s)."""
import torch

import rate_ref as R
from oracle import entropy, subband_ae


def test_bounds_are_the_fp32_constants():
    assert R.SCALE_BOUND < 0.11 and R.SCALE_BOUND == float(torch.tensor(0.11, dtype=torch.float32))
    assert R.LIK_BOUND == float(torch.tensor(1e-9, dtype=torch.float32)) and R.LIK_BOUND != 1e-9
    bb, ped = R.nonneg_bound(1e-6)
    assert ped == 2.0 ** -36 and bb == float(torch.tensor(bb, dtype=torch.float32)) and R.nonneg_bound(0.0)[0] == 2.0 ** -18
    with R.fp32_bounds():
        assert entropy.SCALE_BOUND == R.SCALE_BOUND and subband_ae.nonneg_bound is R.nonneg_bound
    assert entropy.SCALE_BOUND == 0.11 and entropy.LIKELIHOOD_BOUND == 1e-9 and subband_ae.nonneg_bound is not R.nonneg_bound


def test_packing_is_the_package_layout():
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.entropy_models import pack_entropy_bottleneck
    sd = entropy.eb_init_state(3, torch.Generator().manual_seed(1))
    sd = {k: v + 0.01 * torch.arange(v.numel(), dtype=torch.float32).reshape(v.shape) for k, v in sd.items()}
    packed = R.eb_pack(sd)
    assert torch.equal(packed, pack_entropy_bottleneck(sd)) and packed.shape == (3, R.EB_FLOATS)
    back = R.eb_unpack(packed)
    for k, v in back.items():
        assert torch.equal(v, sd[k])
    assert len(R.EB_SLOT_NAMES) == R.EB_FLOATS and R.EB_SLOT_NAMES[58] == "median" and R.EB_SLOT_NAMES[9] == "m1"


# 4 x the measured distance of the fp32 oracle from the float64 helpers at ordinary arguments
AGREE_GAUSS = {"[0.11, 1)": 2.8e-5, "[1, 16)": 7.2e-5}
AGREE_EB = 1.3e-4
AGREE_GDN = 2.6e-6


def test_helpers_agree_with_the_fp32_oracle_at_ordinary_arguments():
    """sigma log-uniform in [0.11, 16], |x - mu| <= 6 sigma, |mu| <= 1; the factorized model with the init-like parameters and
    x within +-15 of the median; GDN with beta in [0.3, 1.5] and positive gamma.  The float64 helpers against the UNPATCHED fp32
    oracle (gaussian_conditional_forward / entropy_bottleneck_forward / gdn).  Measured (one seed each, 49 152 / 98 352 / 14 400
    elements): Gaussian bits 6.9e-6 on [0.11, 1) and 1.8e-5 on [1, 16) in both modes; factorized bits 3.1e-5; GDN 6.3e-7.  The
    quantised values are identical.  The bars are 4 x these."""
    for train in (False, True):
        c = R.gauss_case(R.SWEEP_FWD, 1.0, 13, train, False, 0.11, 16.0, 6.0)
        q, lik = entropy.gaussian_conditional_forward(c["x"], c["sigma"], c["mu"], train, c["noise"])
        assert torch.equal(q, c["v"])
        err = R.per_bucket((-torch.log2(lik).double() - c["ref"]["bits"]).abs(), c["sigma"])
        print("gauss ordinary, %s: %s" % ("noise" if train else "eval", {k: "%.2e" % v for k, v in err.items()}))
        assert set(err) == set(AGREE_GAUSS)
        for k, v in err.items():
            assert v <= AGREE_GAUSS[k], (k, v)
    worst = 0.0
    for train in (False, True):
        c = R.eb_case("init", 8196, 15.0, R.SEED_EB_FWD, train)
        for p in range(2):
            sd = {"e." + k: v for k, v in R.eb_unpack(c["eb"][p]).items()}
            sd["e.quantiles"] = torch.stack([c["eb"][p, :, 58]] * 3, 1)[:, None, :]
            q, lik = entropy.entropy_bottleneck_forward(c["x"][p], sd, "e.", train, None if c["noise"] is None else c["noise"][p])
            assert torch.equal(q, c["v"][p])
            worst = max(worst, (-torch.log2(lik).double() - c["ref"]["bits"][p]).abs().max().item())
    print("factorized ordinary: %.2e" % worst)
    assert worst <= AGREE_EB
    worst = 0.0
    for inverse in (False, True):
        x, beta, gamma = R.gdn_inputs(2, 2, 6, 1, 300, R.SEED_GDN, edges=False)
        ref = R.gdn_eval(x, beta, gamma, inverse)["y"]
        for p in range(2):
            worst = max(worst, (subband_ae.gdn(x[p], beta[p], gamma[p], inverse).double() - ref[p]).abs().max().item())
    print("gdn ordinary: %.2e" % worst)
    assert worst <= AGREE_GDN


def test_gradient_helpers_against_central_differences():
    """The float64 gradients the GPU tests compare against, checked by central differences of the float64 forward at a handful of
    elements away from the kinks (the autograd tape includes the LowerBound rule: pass-through wherever the bound is inactive)."""
    x, sigma, mu, noise = R.gauss_inputs((1, 1, 1, 4, 8), 1.0, 5, 0.2, 40.0, 3.0)
    v = R.gauss_quant(x, mu, noise)
    gb = torch.ones_like(x)
    r = R.gauss_eval(v, sigma, mu, R.F64, gb, True)
    h = 1e-6
    for name, k in (("dx", 0), ("dsigma", 1), ("dmu", 2)):
        args = [v.double(), sigma.double(), mu.double()]
        hi, lo = list(args), list(args)
        hi[k], lo[k] = args[k] + h, args[k] - h
        with R.fp32_bounds():
            fd = (-torch.log2(entropy.gaussian_likelihood(*hi)) + torch.log2(entropy.gaussian_likelihood(*lo))) / (2 * h)
        assert (fd - r[name]).abs().max().item() <= 1e-6 * max(1.0, r[name].abs().max().item()), name
    eb = R.eb_params("stress")
    xe, ne = R.eb_inputs("stress", 5, 15.0, R.SEED_EB_BWD)
    ve = R.eb_quant(xe, eb, ne)
    re_ = R.eb_eval(ve, eb, R.F64, torch.ones_like(xe), True)
    assert re_["deb"][:, :, 58].abs().max().item() == 0.0
    for slot in (0, 9, 25, 33, 54, 57):                       # m0, the entry above 20, an entry near -10, a factor, m4, b4
        d = torch.zeros_like(eb, dtype=R.F64)
        d[:, :, slot] = h
        fd = (R.eb_eval(ve, eb.double() + d)["bits"] - R.eb_eval(ve, eb.double() - d)["bits"]).sum((1, 3, 4)) / (2 * h)
        ref = re_["deb"][:, :, slot]
        assert (fd - ref).abs().max().item() <= 1e-5 * max(1e-3, ref.abs().max().item()), (slot, fd, ref)


def test_sweep_covers_the_domain():
    """What the generators promise: every bucket populated, sigma <= 0, the bound and its two fp32 neighbours, exact ties, both sides
    of the 1e-9 floor and of the fast erfc's 10.05 cut-off; the stress parameters reach softplus' threshold and saturated tanh and
    still leave a fifth of the +-15 span above the floor."""
    for ms in R.MU_SCALES:
        for shape, seed in ((R.SWEEP_FWD, R.SEED_GAUSS_FWD), (R.SWEEP_BWD, R.SEED_GAUSS_BWD)):
            x, sigma, mu, noise = R.gauss_inputs(shape, ms, seed)
            bi = R.bucket_index(sigma)
            assert all(int((bi == b).sum()) > 0.1 * sigma.numel() for b in range(5))
            sb = torch.tensor(R.SCALE_BOUND, dtype=torch.float32)
            for val in (sb, torch.nextafter(sb, torch.tensor(0.0)), torch.nextafter(sb, torch.tensor(1.0)), torch.tensor(0.0)):
                assert int((sigma == val).sum()) >= 32
            assert bool((sigma < 0).any()) and float(sigma.max()) > 3000 and float(mu.abs().max()) > 0.9 * ms
            d = x - mu
            assert int(((d - torch.floor(d)) == 0.5).sum()) >= 256
            raw = R.gauss_lik_raw(R.gauss_quant(x, mu, noise), sigma, mu)
            assert 0.1 < float((raw < R.LIK_BOUND).float().mean()) < 0.5
            arg = ((x + noise - mu).abs() + 0.5) / (sigma.clamp(min=R.SCALE_BOUND) * 2 ** 0.5)
            assert bool((arg > 10.06).any()) and bool((arg < 10.0).any())
    eb = R.eb_params("stress")
    assert int((eb[:, :, :58] > 20).sum()) == 6 and int((eb[:, :, :58] < -9).sum()) == 24 and float(eb[:, :, 58].abs().min()) == 37.25
    for kind in R.EB_KINDS:
        x, _ = R.eb_inputs(kind, 117, 15.0, R.SEED_EB_FWD)
        med = R.eb_params(kind)[:, :, 58][:, None, :, None, None]
        assert torch.equal(torch.round(x - med)[..., :4], torch.tensor([-128.0, -127.0, 127.0, 128.0]).expand(2, 2, 3, 1, 4))
        raw = R.eb_lik_raw(R.eb_quant(x, R.eb_params(kind)), R.eb_params(kind))
        assert float((raw > R.LIK_BOUND).float().mean()) > 0.2
    x, _ = R.eb_inputs("init", 8196, 4000.0, R.SEED_EB_FWD)
    raw = R.eb_lik_raw(R.eb_quant(x, R.eb_params("init")), R.eb_params("init"))
    assert float((raw < R.LIK_BOUND).float().mean()) > 0.5


def test_bar_sources_gauss():
    """The per-bucket error of the fp32 oracle against float64 on the inputs of the GPU sweeps (same generators, same seeds)."""
    for ms in R.MU_SCALES:
        for train in (False, True):
            c = R.gauss_case(R.SWEEP_FWD, ms, R.SEED_GAUSS_FWD, train)
            print("gauss bits  |mu|<=%-6g %-5s %s" % (ms, "noise" if train else "eval",
                                                      "  ".join("%s %.1e -> bar %.1e" % (k, v, R.bits_bar(v)) for k, v in c["err32"].items())))
            assert len(c["err32"]) == 5 and all(0 <= v < 2e-2 for v in c["err32"].values())
            assert max(c["err32"][k] for k in R.BUCKET_NAMES[:3]) < 1e-4       # ordinary sigma: the floor of 1e-4 is the bar
            c = R.gauss_case(R.SWEEP_BWD, ms, R.SEED_GAUSS_BWD, train, True)
            for k, d in c["gerr32"].items():
                print("gauss %-6s |mu|<=%-6g %-5s %s" % (k, ms, "noise" if train else "eval",
                                                         "  ".join("%s %.1e -> %.1e" % (a, b, R.grad_bar(b)) for a, b in d.items())))
                assert all(0 <= v < 1e-2 for v in d.values())


def test_bar_sources_factorized_and_gdn():
    for kind in R.EB_KINDS:
        for span in R.EB_SPANS:
            for hw in R.EB_HW_FWD:
                for train in (False, True):
                    e = R.eb_case(kind, hw, span, R.SEED_EB_FWD, train)["err32"]
                    print("factorized bits %-6s +-%-6g hw %-5d %-5s %.1e -> bar %.1e" % (kind, span, hw, "noise" if train else "eval",
                                                                                        e, R.bits_bar(e)))
                    assert 0 <= e < 1e-3
        for hw in R.EB_HW_BWD:
            for train in (False, True):
                c = R.eb_case(kind, hw, R.EB_SPAN_BWD, R.SEED_EB_BWD, train, True)
                g = c["gerr32"]
                print("factorized grad %-6s hw %-5d %-5s dx %.1e  deb (worst slot) %.1e" % (kind, hw, "noise" if train else "eval",
                                                                                         g["dx"], max(g["deb"])))
                assert g["dx"] < 2e-4 / 4 and max(g["deb"]) < 2e-4 / 4       # the 2e-4 floor is the bar for every slot
                assert c["ref"]["deb"][:, :, 58].abs().max().item() == 0.0
                if not train:
                    assert c["ref"]["dx"].abs().max().item() == 0.0
    for shape in R.GDN_FWD:
        for inverse in (False, True):
            c = R.gdn_case(*shape, inverse, R.SEED_GDN)
            print("gdn y %s inverse %d: %.1e -> bar %.1e (max |y| %.1e)" % (shape, inverse, c["err32"], R.gdn_bar(c["err32"]),
                                                                        c["ref"]["y"].abs().max().item()))
            assert 0 <= c["err32"] < 1e-3
    for shape in R.GDN_TRAIN:
        for inverse in (False, True):
            c = R.gdn_case(*shape, inverse, R.SEED_GDN_TRAIN, True)
            print("gdn train %s inverse %d: y %.1e  %s" % (shape, inverse, c["err32"],
                                                          "  ".join("%s %.1e" % kv for kv in c["gerr32"].items())))
            assert all(v < 2e-4 / 4 for v in c["gerr32"].values())
            assert float(c["ref"]["dbeta"].abs().min()) == 0.0 and float(c["ref"]["dgamma"].abs().min()) == 0.0   # blocked entries


def test_exclusion_caps():
    """The gradient comparisons leave out the elements within 1e-3 relative of the likelihood floor: at most 1 % of a tensor."""
    for ms in R.MU_SCALES:
        for train in (False, True):
            share = R.gauss_case(R.SWEEP_BWD, ms, R.SEED_GAUSS_BWD, train, True)["excl"].float().mean().item()
            print("gauss bwd |mu|<=%g %s: excluded %.4f %%" % (ms, "noise" if train else "eval", 100 * share))
            assert share <= 0.01
    for kind in R.EB_KINDS:
        for hw in R.EB_HW_BWD:
            for train in (False, True):
                share = R.eb_case(kind, hw, R.EB_SPAN_BWD, R.SEED_EB_BWD, train, True)["excl"].float().mean().item()
                print("factorized bwd %s hw %d %s: excluded %.4f %%" % (kind, hw, "noise" if train else "eval", 100 * share))
                assert share <= 0.01
