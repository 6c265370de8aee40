"""The chroma formats of the codec stated once in plain fp32 torch ops on the CPU, in the normative order.
The kernels of csrc/chroma.hip are held torch.equal to these functions (tests/test_gpu_codec_chroma.py).

Every function takes and returns float32 CPU tensors; every product and sum is one separately rounded fp32 operation (eager
torch ops never contract)."""
import torch


def downsample(c):
    """4:2:0 forward: (..., h, w) with even h, w -> (..., h / 2, w / 2).  Sample (i, j) is ((c00 + c01) + (c10 + c11)) * 0.25
    over the pixels (2i..2i+1, 2j..2j+1)."""
    assert c.dtype == torch.float32 and c.shape[-1] % 2 == 0 and c.shape[-2] % 2 == 0
    c00, c01 = c[..., 0::2, 0::2], c[..., 0::2, 1::2]
    c10, c11 = c[..., 1::2, 0::2], c[..., 1::2, 1::2]
    return ((c00 + c01) + (c10 + c11)) * 0.25


def _near_far(n):
    """For the 2 n positions along an axis over n samples: (index of the nearer sample, index of the farther one, clamped to
    the plane): cy = y >> 1, ny = cy + 1 if y is odd else cy - 1."""
    y = torch.arange(2 * n)
    cy = y >> 1
    ny = torch.where((y & 1) == 1, cy + 1, cy - 1).clamp(0, n - 1)
    return cy, ny


def upsample(c):
    """4:2:0 inverse: (..., hc, wc) -> (..., 2 hc, 2 wc).  t(r) = 0.75 c[r][cx] + 0.25 c[r][nx], v = 0.75 t(cy) + 0.25 t(ny):
    the centred phase (a chroma sample sits in the middle of its 2 x 2 pixels), clamped at the plane's own border."""
    assert c.dtype == torch.float32
    cy, ny = _near_far(c.shape[-2])
    cx, nx = _near_far(c.shape[-1])
    t = 0.75 * c[..., :, cx] + 0.25 * c[..., :, nx]
    return 0.75 * t[..., cy, :] + 0.25 * t[..., ny, :]


def affine(s, inv_a, b):
    """The per-plane map of a reduced-resolution decode on one plane's samples: (s - b) * inv_a (inv_a, b: fp32-rounded floats)."""
    return (s - float(b)) * float(inv_a)


def grey_in(g_u8):
    """4:0:0 forward: uint8 -> g / 255 - 0.5."""
    return g_u8.to(torch.float32) / 255.0 - 0.5


def grey_out(s):
    """4:0:0 inverse: floor((clamp(s, -0.5, 0.5) + 0.5) * 255 + 0.5) as uint8."""
    return torch.floor((s.clamp(-0.5, 0.5) + 0.5) * 255.0 + 0.5).to(torch.uint8)
