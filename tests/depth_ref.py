"""Samples of 9 to 16 bits in the codec stated once in plain fp32 torch ops on the CPU, in the normative
order.  The kernels of csrc/depth.hip are held torch.equal to these functions (tests/test_gpu_codec_depth.py); the 4:2:0
resampling and the affine map of a reduced decode are those of tests/chroma_ref.py.

Every function works on CPU tensors; every quotient, product and sum is one separately rounded fp32 operation (eager torch ops
never contract).  uint16 tensors come in and go out as torch.uint16; the arithmetic runs on their values as float32, which holds
every integer up to 2^24 exactly."""
import torch

from chroma_ref import affine, downsample, upsample  # noqa: F401  (re-exported: one place for the tests to import from)

KR, KG, KB = 0.2126, 0.7152, 0.0722                   # BT.709, the constants of csrc/ops.hip


def _f(v):
    """A Python float rounded to fp32, as a 0-d tensor (so that it enters every op as the fp32 constant of the kernels)."""
    return torch.tensor(v, dtype=torch.float32)


def maxval(d):
    """M = 2^d - 1 as the fp32 constant of the kernels (exact: at most 16 bits)."""
    assert 8 <= d <= 16
    return _f(float((1 << d) - 1))


def rgb_in(v, d):
    """(..., 3) uint16 (or uint8 at d = 8) RGB samples of depth d -> (Y - 0.5, Cb, Cr), three float32 tensors of shape (...):
    x = v / M, a true division, then the expressions of k_u8hwc_to_ycc_tiles in their order."""
    x = v.to(torch.float32) / maxval(d)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    yy = _f(KR) * r + _f(KG) * g + _f(KB) * b         # ((KR r + KG g) + KB b): left to right, as the kernel's expression
    cb = _f(0.5) * (b - yy) / (_f(1.0) - _f(KB)) + _f(0.5)
    cr = _f(0.5) * (r - yy) / (_f(1.0) - _f(KR)) + _f(0.5)
    return yy - _f(0.5), cb, cr


def _sample(c, d):
    """clamp(c, -0.5, 0.5) -> floor((c + 0.5) * M + 0.5) as uint16."""
    q = torch.floor((c.clamp(-0.5, 0.5) + _f(0.5)) * maxval(d) + _f(0.5))
    return q.to(torch.int32).to(torch.uint16)


def rgb_out(ycc, d):
    """(Y - 0.5, Cb, Cr), three float32 tensors of one shape -> (..., 3) uint16 RGB samples of depth d: the expressions of
    ycc_vals_u8 with M in place of 255."""
    s0, cb, cr = ycc
    y = s0 + _f(0.5)
    r = y + (_f(2.0) - _f(2.0) * _f(KR)) * (cr - _f(0.5))
    b = y + (_f(2.0) - _f(2.0) * _f(KB)) * (cb - _f(0.5))
    g = (y - _f(KR) * r - _f(KB) * b) / _f(KG)
    return torch.stack([_sample(r - _f(0.5), d), _sample(g - _f(0.5), d), _sample(b - _f(0.5), d)], -1)


def grey_in(v, d):
    """4:0:0 forward: v / M - 0.5."""
    return v.to(torch.float32) / maxval(d) - _f(0.5)


def grey_out(s, d):
    """4:0:0 inverse: floor((clamp(s, -0.5, 0.5) + 0.5) * M + 0.5) as uint16."""
    return _sample(s, d)
