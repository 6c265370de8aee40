"""GPU: the irans32 device coder (csrc/rans_gpu.hip, irans.py) pinned to its definition tools/irans_ref.py
over its lane, table and escape domain -- the cases of tests/irans_cases.py (checked on the host by test_irans_cases_host.py):
encoder bytes at K = 1..32 on four table sets and six escape patterns, decoder symbols from the reference's streams under
four piece plans at K = 16 and 32, strides with padding, the defined refusals, the format's dearest stream, and one image
through the codec at 32 lanes.  Every comparison is exact."""
import ctypes as C
import os
import sys

import pytest
import torch

from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import _lib, codec, irans

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import irans_cases as IC  # noqa: E402
from irans_cases import R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Z = 3
SEEDS = (1, 2, 3)                                                       # one per stream: different byte lengths
ALL_N = (1, 4095, 8192, 16387, 32799, 65537, 131071, 131072, 131109, 196608)      # K = 1 1 2 4 8 16 16 32 32 32
K32_N = (131072, 131109, 196608)
N16, N32 = 65537, IC.N32
_DT = {}


def _dt(tset):
    if tset not in _DT:
        _DT[tset] = irans.DeviceTables(*IC.arrays(IC.tables(tset)), DEV)
    return _DT[tset]


def _cases(tset, pattern, n):
    """-> (sym (Z, n) list, idx (Z, n) list, the reference's Z streams)."""
    cs = [IC.case(tset, pattern, n, s) for s in SEEDS]
    return [c[0] for c in cs], [c[1] for c in cs], [c[2] for c in cs]


def _dev(rows):
    return torch.tensor(rows, dtype=torch.int32, device=DEV)


def _encode_direct(sym, idx, n, stride, dt):
    """lldwt_irans_encode on (Z, stride) int32 device tensors -> (lengths, flag, per stream the bytes or None)."""
    z = int(sym.shape[0])
    assert sym.is_contiguous() and idx.is_contiguous() and sym.shape == idx.shape == (z, stride)
    cap = irans.capacity(n)
    out = torch.zeros(z * cap, device=DEV, dtype=torch.uint8)
    meta = torch.zeros(z + 1, device=DEV, dtype=torch.int64)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(_lib.load().lldwt_irans_encode(p(sym), p(idx), z, n, stride, *dt.args(), p(irans._rcp(DEV)), p(out), cap, p(meta),
                                              C.c_void_p(meta.data_ptr() + 8 * z), irans._stream()), "irans_encode")
    torch.cuda.synchronize()
    m, o = meta.cpu().tolist(), out.cpu().numpy()
    return m[:z], m[z], [o[(k + 1) * cap - m[k]:(k + 1) * cap].tobytes() if m[k] >= 0 else None for k in range(z)]


# ------------------------------------------------------------------------------------------------ 1. encoder bytes
ENC = [("edge", "dense", n) for n in ALL_N]
ENC += [(t, p, n) for n in K32_N for t in IC.TABLE_SETS for p in ("none", "dense", "all", "lanes", "magnitudes")
        if (t, p) != ("edge", "dense")]


@pytest.mark.parametrize("tset,pattern,n", ENC)
def test_encoder_bytes_equal_the_reference(tset, pattern, n):
    sym, idx, want = _cases(tset, pattern, n)
    got = irans.encode(_dev(sym), _dev(idx), _dt(tset))
    assert len({len(w) for w in want}) == Z or n == 1
    for z in range(Z):
        assert got[z] == want[z], z


# ------------------------------------------------------------------------------------------------ 2. decoder symbols
DEC = [("edge", "lanes"), ("edge", "dense"), ("gaussian", "sparse"), ("ladder0", "all")]


@pytest.mark.parametrize("plan", IC.PLANS)
@pytest.mark.parametrize("tset,pattern", DEC)
@pytest.mark.parametrize("n", [N16, N32])
def test_decoder_pops_the_references_streams(n, tset, pattern, plan):
    sym, idx, streams = _cases(tset, pattern, n)
    K = irans.lanes(n)
    assert K == R.lanes(n) == (16 if n == N16 else 32)
    cuts = IC.pieces(n, K, plan, 7, IC.escapes(IC.tables(tset), sym[0], idx[0]))
    idx_d = _dev(idx)
    d = irans.Decoder(streams, n, _dt(tset), DEV)
    parts = [d.pop(idx_d[:, a:b].contiguous()) for a, b in zip(cuts, cuts[1:])]
    d.finish()
    assert torch.equal(torch.cat(parts, 1), _dev(sym))


# ------------------------------------------------------------------------------------------------ 3. strides and padding
def test_decoder_strides_leave_the_padding_alone():
    n, tset = N32, "edge"
    sym, idx, streams = _cases(tset, "dense", n)
    cuts = IC.pieces(n, 32, "round_edges", 8)
    idx_d, sym_d = _dev(idx), _dev(sym)
    d = irans.Decoder(streams, n, _dt(tset), DEV)
    for a, b in zip(cuts, cuts[1:]):
        cnt = b - a
        pi = torch.full((Z, cnt + 5), -7, dtype=torch.int32, device=DEV)       # an index the kernel would refuse
        pi[:, :cnt] = idx_d[:, a:b]
        out = torch.full((Z, cnt + 5), -12345, dtype=torch.int32, device=DEV)
        assert d.pop(pi, cnt, cnt + 5, out) is out
        assert torch.equal(out[:, :cnt], sym_d[:, a:b]) and bool((out[:, cnt:] == -12345).all()), (a, b)
    d.finish()


def test_encoder_stride_and_padded_indexes():
    n, tset = N32, "edge"
    sym, idx, want = _cases(tset, "dense", n)
    ps = torch.full((Z, n + 3), 1 << 30, dtype=torch.int32, device=DEV)
    pi = torch.full((Z, n + 3), -7, dtype=torch.int32, device=DEV)
    ps[:, :n], pi[:, :n] = _dev(sym), _dev(idx)
    lens, flag, got = _encode_direct(ps, pi, n, n + 3, _dt(tset))
    assert flag == 0 and lens == [len(w) for w in want]
    assert got == want
    assert _encode_direct(_dev(sym), _dev(idx), n, n, _dt(tset))[2] == want


# ------------------------------------------------------------------------------------------------ 4. defined refusals
# Both kernels were read for this: k_irans_encode reads sizes / cdf / rcp only after 0 <= ci < ncdf, 0 <= maxv and
# maxv + 1 < stride, and refuses freq == 0 or > 65536 before any state moves; k_irans_decode replaces a bad index by row 0
# (flag set) before its table reads, and every stream byte comes through rd(), which returns 0 past the end.
def _zero_freq_tables():
    """The edge set plus one row with a slot of frequency 0 (slot 1 of [10, 0, 65525, 1])."""
    cdf, sizes, offs = IC.tables("edge")
    row = [0, 10, 10, 65535, 65536]
    return cdf + [row + [0] * (len(cdf[0]) - len(row))], sizes + [5], offs + [0]


@pytest.mark.parametrize("bad", ["ncdf", "minus_one", "zero_freq"])
def test_encoder_refuses_a_bad_stream_and_codes_its_neighbours(bad):
    n = N32
    sym, idx, want = _cases("edge", "dense", n)
    tabs = _zero_freq_tables() if bad == "zero_freq" else IC.tables("edge")
    dt = irans.DeviceTables(*IC.arrays(tabs), DEV)
    sym, idx = [list(s) for s in sym], [list(i) for i in idx]
    at = n // 2 + 5
    if bad == "zero_freq":
        idx[1][at], sym[1][at] = len(tabs[1]) - 1, 1                    # value 1 of the new row: frequency 0
        idx[0][at], sym[0][at] = len(tabs[1]) - 1, 0                    # its good slots code as ever
        idx[2][at], sym[2][at] = len(tabs[1]) - 1, 2
        want = [R.encode(sym[0], idx[0], *tabs), None, R.encode(sym[2], idx[2], *tabs)]
    else:
        idx[1][at] = len(tabs[1]) if bad == "ncdf" else -1
    with pytest.raises(_lib.LLDWTError, match="irans_encode"):
        irans.encode(_dev(sym), _dev(idx), dt)
    lens, flag, got = _encode_direct(_dev(sym), _dev(idx), n, n, dt)
    assert flag != 0 and lens[1] == -1
    assert got[0] == want[0] and got[2] == want[2]


def test_decoder_refuses_truncated_and_overlong_streams():
    n = N32
    sym, idx, streams = _cases("edge", "dense", n)
    st, idx_d = streams[0], _dev(idx[:1])
    for cut in (0, 3, 4 * 32 - 1, len(st) // 2, len(st) - 1):
        d = irans.Decoder([st[:cut]], n, _dt("edge"), DEV)
        d.pop(idx_d)
        with pytest.raises(ValueError, match="corrupt stream"):
            d.finish()
    d = irans.Decoder([st + b"\0"], n, _dt("edge"), DEV)                # a trailing byte: the cursor check
    d.pop(idx_d)
    with pytest.raises(ValueError, match="corrupt stream"):
        d.finish()
    d = irans.Decoder([st], n, _dt("edge"), DEV)                        # and the stream itself passes
    assert d.pop(idx_d).cpu().tolist() == sym[:1]
    d.finish()


# ------------------------------------------------------------------------------------------------ 5. the dearest stream
def test_worst_case_stream_has_room_and_the_references_bytes():
    n = 8192
    sym, idx = IC.worst_case(n)
    want = R.encode(sym, idx, *IC.tables("edge"))
    got = irans.encode(_dev([sym]), _dev([idx]), _dt("edge"))          # raises on "no room"
    assert got == [want] and len(want) <= irans.capacity(n)


# ------------------------------------------------------------------------------------------------ 6. through the codec
def test_lossless_image_through_the_codec_at_32_lanes(monkeypatch):
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.models import entropy_coding as ec
    from test_gpu_irans import _images, _net
    H, W = 384, 464
    net = _net("conditioned2ZTsepSubbands", 3)
    x = _images(1, H, W, 41)
    base_n, coded_n = [], []
    flush, encode = ec._DeviceSink.flush, irans.encode

    def spy_flush(self):
        base_n.append(sum(t.numel() for t in self.idx) // (self.P * self.B))
        return flush(self)

    def spy_encode(sym, idx, dt):
        coded_n.append(int(sym.shape[1]))
        return encode(sym, idx, dt)
    monkeypatch.setattr(ec._DeviceSink, "flush", spy_flush)
    monkeypatch.setattr(irans, "encode", spy_encode)
    gblob = codec.encode_images(net, x, coder="gpu", near=0)
    monkeypatch.undo()
    assert max(base_n) == 3 * (H // 2) * (W // 2) == 133632 and irans.lanes(max(base_n)) == 32
    resid_n = [m for m in coded_n if m not in base_n]
    assert resid_n and set(resid_n) == {H * W} and irans.lanes(H * W) == 32
    got = codec.decode_images(net, gblob)[0]
    assert torch.equal(got, x[0])                                       # the layer is lossless
    host = codec.decode_images(net, codec.encode_images(net, x, near=0))[0]
    assert torch.equal(got, host)
