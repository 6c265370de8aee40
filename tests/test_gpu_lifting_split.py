"""GPU: the forked lifting transform (lldwt_lifting_forward_split: levels < k on the caller's stream, the rest on a second one)
against the unsplit call.  The two run the same program of the same launches, so the bound is equality: torch.equal on ll and
every yh.  64 x 128 with L = 4 puts two levels on each side of a fork at 2, so the LL ping-pong changes parity across it; k = 0
and k = L are the unsplit call.  Block property "same" and "different", the gains of config.scale on and off (their ops, and
the final ll, belong to the level they write)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P, B = 3, 2
CASES = [(64, 64, 3, (0, 1, 2, 3)), (64, 128, 4, (0, 1, 2, 3, 4))]


def _nets(L, blockprop, scale):
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.layers.lifting_dwt_nets import \
        LiftingBasedNeuralWaveletv4
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.utils.config import make_config
    cfg = make_config(dwtlevels=L, block_property=blockprop, scale=scale, mode="validate")
    torch.manual_seed(11)
    nets = [LiftingBasedNeuralWaveletv4(cfg).to(DEV).eval() for _ in range(P)]
    with torch.no_grad():
        for p, n in enumerate(nets):                 # gains away from their initial value, different per plane
            n.nh.fill_(0.3 + 0.1 * p)
            n.nl.fill_(-0.2 - 0.1 * p)
    return nets


@pytest.mark.parametrize("scale", [0, 1])
@pytest.mark.parametrize("blockprop", ["same", "different"])
@pytest.mark.parametrize("H,W,L,ks", CASES)
def test_split_equals_unsplit(H, W, L, ks, blockprop, scale):
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.layers.lifting_dwt_nets import lifting_forward_planes
    nets = _nets(L, blockprop, scale)
    x = (torch.rand(P, B, 1, H, W, generator=torch.Generator().manual_seed(5)) - 0.5).to(DEV)
    with torch.no_grad():
        ll0, yh0 = lifting_forward_planes(nets, x)
        torch.cuda.synchronize()
        for k in ks:
            with ops.eval_overlap(k, x.device) as ov:
                ll, yh = lifting_forward_planes(nets, x)
                assert ov.lent == (0 < k < L)            # k = 0 and k = L: the unsplit call, nothing lent
                if ov.lent:
                    with pytest.raises(Exception):       # the workspace is with the tail until the join
                        ops.workspace(16, x.device)
                ov.join()
                assert not ov.lent
                # consumed on the caller's stream at once, no synchronise in between
                same = [torch.equal(ll, ll0)] + [torch.equal(a, b) for a, b in zip(yh, yh0)]
            assert all(same), (k, same)


def test_program_levels_and_bad_arguments():
    """Every op of the forward program carries the level whose buffers it writes, in level order; a split needs its event."""
    import ctypes as C
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import _lib, ops
    for scale in (False, True):
        prog, _ = ops.lifting_program(6, 64, 128, 4, False, 0, False, 16, scale)
        per = 12 + (6 if scale else 0)
        assert [o.level for o in prog] == [i // per for i in range(4 * per)]
        for o in prog:
            if o.buf_dout >= 8:                          # a yh buffer: the level's own
                assert o.buf_dout - 8 == o.level
    nets = _nets(3, "same", 0)
    x = torch.zeros(P, B, 1, 64, 64, device=DEV)
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.layers.lifting_dwt_nets import _lifting_params
    taps, packed, _, _ = _lifting_params(nets)
    lib = _lib.load()
    ll = torch.empty(P, B, 1, 8, 8, device=DEV)
    yh = [torch.empty(P, B, 3, 64 >> (i + 1), 64 >> (i + 1), device=DEV) for i in range(3)]
    nb = lib.lldwt_lifting_ws_bytes(P * B, 64, 64, 16)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    r = lib.lldwt_lifting_forward_split(x.data_ptr(), ll.data_ptr(), ops._ptr_array(yh), P, B, 64, 64, 3, taps.data_ptr(),
                                        packed.data_ptr(), int(packed.shape[1]), 0, 0, 16, 5, 0.1, 0, None, None, ws.data_ptr(), nb,
                                        2, st, st, None)
    assert r == -1 and b"split" in lib.lldwt_last_error()
    torch.cuda.synchronize()


def test_native_unsplit_levels():
    """split_level <= 0 and >= levels through lldwt_lifting_forward_split itself (ops.lifting_forward never passes them on): the
    unsplit call on `stream`, with no second stream and no event to touch."""
    import ctypes as C
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import _lib, ops
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd.graphs.layers.lifting_dwt_nets import (_lifting_params,
                                                                                                              lifting_forward_planes)
    L, H, W = 3, 64, 64
    nets = _nets(L, "different", 1)
    x = (torch.rand(P, B, 1, H, W, generator=torch.Generator().manual_seed(6)) - 0.5).to(DEV)
    taps, packed, nh, nl = _lifting_params(nets)
    lib = _lib.load()
    nb = lib.lldwt_lifting_ws_bytes(P * B, H, W, 16)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    with torch.no_grad():
        ll0, yh0 = lifting_forward_planes(nets, x)
        for k in (-1, 0, L, L + 5):
            ll = torch.zeros_like(ll0)
            yh = [torch.zeros_like(t) for t in yh0]
            r = lib.lldwt_lifting_forward_split(x.data_ptr(), ll.data_ptr(), ops._ptr_array(yh), P, B, H, W, L, taps.data_ptr(),
                                                packed.data_ptr(), int(packed.shape[1]), 0, 1, 16, 5, 0.1, 0, nh.data_ptr(),
                                                nl.data_ptr(), ws.data_ptr(), nb, k, st, None, None)
            assert r == 0, (k, lib.lldwt_last_error())
            assert torch.equal(ll, ll0) and all(torch.equal(a, b) for a, b in zip(yh, yh0)), k
