"""CPU: the sample-depth rules of the codec on the reference alone, tests/depth_ref.py -- fp32 is enough for
an exact round trip up to 16 bits, depth 8 on uint16 data is the uint8 formulas, and the v8 * 257 identity at depth 16."""
import pytest
import torch

import chroma_ref
import depth_ref

DEPTHS = (9, 10, 12, 14, 16)
CORNERS = [[r, g, b] for r in (0, 1) for g in (0, 1) for b in (0, 1)]


def _triples(d, n, seed):
    """n seeded random RGB triples of depth d plus the eight cube corners, as (n + 8, 3) uint16."""
    M = (1 << d) - 1
    v = torch.randint(0, M + 1, (n, 3), dtype=torch.int32, generator=torch.Generator().manual_seed(seed))
    return torch.cat([v, torch.tensor(CORNERS, dtype=torch.int32) * M]).to(torch.uint16)


@pytest.mark.parametrize("d", DEPTHS)
def test_rgb_round_trip_is_exact(d):
    v = _triples(d, 1 << 20, d)
    back = depth_ref.rgb_out(depth_ref.rgb_in(v, d), d)
    assert back.dtype == torch.uint16 and torch.equal(back, v)


@pytest.mark.parametrize("d", DEPTHS)
def test_grey_round_trip_is_exact_for_every_value(d):
    v = torch.arange(1 << d, dtype=torch.int32).to(torch.uint16)
    s = depth_ref.grey_in(v, d)
    assert s.dtype == torch.float32 and float(s.min()) == -0.5 and float(s.max()) == 0.5
    assert torch.equal(depth_ref.grey_out(s, d), v)


def test_output_rule_clamps_and_rounds_half_up():
    d, M = 10, 1023.0
    s = torch.tensor([-0.7, -0.5, 0.5, 0.7, (0.5 / M) - 0.5, (1.5 / M) - 0.5], dtype=torch.float32)
    got = depth_ref.grey_out(s, d).to(torch.int32).tolist()
    assert got[:4] == [0, 0, 1023, 1023]
    want = torch.floor((s[4:].double() + 0.5).float() * torch.tensor(M) + 0.5).to(torch.int32).tolist()
    assert got[4:] == want


def test_depth_8_on_uint16_is_the_uint8_path():
    """Depth 8 on uint16 storage: the greyscale rules of chroma_ref and the 4:4:4 expressions written with 255."""
    g = torch.arange(256, dtype=torch.int32)
    assert torch.equal(depth_ref.grey_in(g.to(torch.uint16), 8), chroma_ref.grey_in(g.to(torch.uint8)))
    s = torch.linspace(-0.7, 0.7, 100001, dtype=torch.float32)
    assert torch.equal(depth_ref.grey_out(s, 8).to(torch.int32), chroma_ref.grey_out(s).to(torch.int32))
    v = torch.randint(0, 256, (1 << 16, 3), dtype=torch.int32, generator=torch.Generator().manual_seed(8))
    x = v.to(torch.uint8).to(torch.float32) / 255.0
    r, gg, b = x[:, 0], x[:, 1], x[:, 2]
    f = lambda c: torch.tensor(c, dtype=torch.float32)
    yy = f(0.2126) * r + f(0.7152) * gg + f(0.0722) * b
    cb = 0.5 * (b - yy) / (1.0 - f(0.0722)) + 0.5
    cr = 0.5 * (r - yy) / (1.0 - f(0.2126)) + 0.5
    got = depth_ref.rgb_in(v.to(torch.uint16), 8)
    assert torch.equal(got[0], yy - 0.5) and torch.equal(got[1], cb) and torch.equal(got[2], cr)
    back = depth_ref.rgb_out(got, 8)
    assert torch.equal(back.to(torch.int32), v)


def test_the_257_identity_is_bitwise():
    """65535 = 255 * 257: (v8 * 257) / 65535 and v8 / 255 are one real number, so one fp32 -- the nets see the same tensors."""
    v8 = torch.cat([torch.randint(0, 256, (1 << 16, 3), dtype=torch.int32, generator=torch.Generator().manual_seed(257)),
                    torch.tensor(CORNERS, dtype=torch.int32) * 255])
    a = depth_ref.rgb_in((v8 * 257).to(torch.uint16), 16)
    b = depth_ref.rgb_in(v8.to(torch.uint16), 8)
    for p in range(3):
        assert torch.equal(a[p].view(torch.int32), b[p].view(torch.int32)), p
    g = torch.arange(256, dtype=torch.int32)
    assert torch.equal(depth_ref.grey_in((g * 257).to(torch.uint16), 16).view(torch.int32),
                       depth_ref.grey_in(g.to(torch.uint16), 8).view(torch.int32))
