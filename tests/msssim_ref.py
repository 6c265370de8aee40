"""Restatement of MS-SSIM (pytorch-msssim 0.2.1, data_range 1, win 11, sigma 1.5, K = (0.01, 0.03)) in plain torch on the CPU:
the yardstick of tests/test_msssim_host.py and tests/test_gpu_msssim.py.  Evaluated in float64 it is the reference; evaluated in
float32 its distance from the float64 result is what fp32 costs this formula, which sets the tolerance of the kernels."""
import functools

import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
C1, C2 = 1e-4, 9e-4


def window(dtype):
    g = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5) ** 2 / (2 * 1.5 ** 2))
    return (g / g.sum()).to(dtype)


def _filt(t, g):
    c = t.shape[1]
    t = F.conv2d(t, g.view(1, 1, 11, 1).expand(c, 1, 11, 1), groups=c)
    return F.conv2d(t, g.view(1, 1, 1, 11).expand(c, 1, 1, 11), groups=c)


def ms_ssim_ref(x, y, offset=0.5, scales=5, dtype=torch.float64):
    """-> (v (S,B,C), m (B,C)) in ``dtype``; differentiable in y."""
    g = window(dtype)
    X, Y = x.to(dtype) + offset, y.to(dtype) + offset
    vs = []
    for s in range(scales):
        mx, my = _filt(X, g), _filt(Y, g)
        sxx, syy, sxy = _filt(X * X, g) - mx * mx, _filt(Y * Y, g) - my * my, _filt(X * Y, g) - mx * my
        cs = (2 * sxy + C2) / (sxx + syy + C2)
        if s < scales - 1:
            vs.append(torch.relu(cs.mean((2, 3))))
            pad = (X.shape[2] % 2, X.shape[3] % 2)
            X, Y = F.avg_pool2d(X, 2, padding=pad), F.avg_pool2d(Y, 2, padding=pad)
        else:
            l = (2 * mx * my + C1) / (mx * mx + my * my + C1)
            vs.append(torch.relu((l * cs).mean((2, 3))))
    v = torch.stack(vs, 0)
    w = torch.tensor(WEIGHTS[:scales], dtype=dtype).view(-1, 1, 1)
    return v, torch.prod(v ** w, 0)


def images(B, H, W, seed):
    """The smooth colour fields plus noise of tests/test_gpu_codec.py::_images, as uint8 (B,H,W,3) on the host."""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(B, 3, max(2, H // 16), max(2, W // 16), generator=g)
    x = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
    x = x * 200 + torch.rand(B, 3, H, W, generator=g) * 40
    return x.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def pair(B, C, H, W, noise, seed=0):
    """x in [-0.5, 0.5] from ``images`` (its first C channels), y = clamp(x + noise * randn); fp32 (B,C,H,W) on the host."""
    x = images(B, H, W, seed).permute(0, 3, 1, 2)[:, :C].float().div(255.0).sub(0.5).contiguous()
    g = torch.Generator().manual_seed(seed + 1000)
    y = (x + noise * torch.randn(x.shape, generator=g)).clamp(-0.5, 0.5).contiguous()
    return x, y


@functools.lru_cache(maxsize=None)
def case(B, C, H, W, noise, scales=5, grad=False):
    """One parity case, computed once per session and shared: x, y, the float64 reference (v, m[, gradient of mean(m) in y])
    and the float32 evaluation's distance from it (the yardstick of the tolerances).  Treat the result as read-only."""
    x, y = pair(B, C, H, W, noise)
    out = {"x": x, "y": y}
    y64 = y.double().requires_grad_(grad)
    v64, m64 = ms_ssim_ref(x, y64, scales=scales, dtype=torch.float64)
    y32 = y.clone().requires_grad_(grad)
    v32, m32 = ms_ssim_ref(x, y32, scales=scales, dtype=torch.float32)
    out.update(v=v64.detach(), m=m64.detach(), v_err32=(v32.detach().double() - v64.detach()).abs().max().item(),
               m_err32=(m32.detach().double() - m64.detach()).abs().max().item())
    if grad:
        m64.mean().backward()
        m32.mean().backward()
        out.update(g=y64.grad, g_err32=(y32.grad.double() - y64.grad).abs().max().item())
    return out


def value_bar(err32):
    """Bound on |kernel - float64| for v and m: 4 x the float32 evaluation's error, floor 2e-6 (16 ulp of fp32 at 1)."""
    return max(4 * err32, 2e-6)


def grad_bar(err32, gref):
    """Bound on the gradient's max abs error: 4 x the float32 evaluation's, floor 1e-5 of the reference's largest magnitude."""
    return max(4 * err32, 1e-5 * gref.abs().max().item())
