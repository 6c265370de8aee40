"""Tensor-level wrappers over the C-ABI (include/lldwt.h).  PyTorch supplies device memory and the stream only.

Tensor convention: "plane-major" (P, B, C, h, w) fp32 contiguous CUDA(HIP) tensors; P = number of per-plane networks
(3 for clrch == 1), parameters stacked on a leading P axis.
"""
import collections
import ctypes as C
import os
import threading

import torch

from . import _lib
from ._lib import (ACT_LRELU, ACT_NONE, ACT_RELU, ACT_TANH, EPI_LRELU_BWD, EPI_NONE, EPI_TANH_BWD, ConvDesc, View,  # noqa: F401
                   check)

_ws = {}


def _env_choice(name, default, allowed):
    """One of the `allowed` strings from the environment variable `name`; read on every call so tests can switch it."""
    v = os.environ.get(name, default)
    if v not in allowed:
        names = " or ".join(a if a.isdigit() else repr(a) for a in allowed)      # 0 or 1; 'f32' or 'f16x3'
        raise _lib.LLDWTError("%s must be %s (got %r)" % (name, names, v))
    return v


def plc_mode():
    """Arithmetic of the dense 243 -> 243 3x3 tree-context conv (LiftingBasedDWT_net.py:271-272): 'f32' = fp32 MFMA
    (reference arithmetic), 'f16x3' = split-fp16 (power-of-two scaled hi*hi + hi*lo + lo*hi on the fp16 matrix cores, fp32
    accumulate; ~2^-21 relative per product, csrc/conv_f16x3.hip).
    Default 'f16x3' (parity-gated by tests/test_gpu_fullsize_oracle.py at the same bars as 'f32'); the fp32 kernel
    stays available as the exact-arithmetic fallback.  Environment variable LLDWT_PLC_MODE."""
    return _env_choice("LLDWT_PLC_MODE", "f16x3", ("f32", "f16x3"))


def train_lift_f16():
    """True when the training forward of the lifting steps runs on the fused f16x3 kernel (lldwt_train_lift_f16: lift mode f16x3
    and LLDWT_TRAIN_LIFT != f32); the packed P/U blocks must then carry their split-fp16 section."""
    return bool(_lib.load().lldwt_train_lift_f16())


def set_precision(name):
    """Arithmetic of the eval path's matrix kernels (fused lifting step, tree-context pair, cgp chain): 'f16x3' (default: three
    fp16 MFMA products per fp32 MAC, fp32-level accuracy), 'fp16' or 'bf16' (ONE product per MAC on operands rounded to that
    type, fp32 accumulate; BASELINE configs[4] / configs[1], tolerance class 1e-2 -- never the headline).  Also settable with
    the environment variable LLDWT_PRECISION before the library is loaded.  Training is not affected."""
    if name not in _lib.PRECISIONS:
        raise _lib.LLDWTError("precision must be one of %s (got %r)" % (sorted(_lib.PRECISIONS), name))
    check(_lib.load().lldwt_set_precision(_lib.PRECISIONS[name]), "lldwt_set_precision")


def get_precision():
    code = _lib.load().lldwt_get_precision()
    return [k for k, v in _lib.PRECISIONS.items() if v == code][0]


_diag_keep = {}


def set_diagnostics(kind, stamps=None, flags=0):
    """Diagnostics hook of the split-fp16 kernels (lldwt_set_diagnostics; tools/*_stamps.py and the composed-vs-sequential
    tests only): kind 0 = fused lifting step (flags = its debug mask), 1 = tree-pair conv (flags: 1 = k_plc_wino in its
    earlier form, 2 = one workgroup per (tile, channel block), 4 = one workgroup per tile at any size), 2 = cgp chain (flags: bound-only variant /
    forced form of cgp16_params, include/lldwt.h).  ``stamps``: an
    int64 device tensor the kernels write s_memtime stamps into (kept alive here until it is replaced), None = off."""
    _diag_keep[kind] = stamps
    ptr = C.c_void_p(stamps.data_ptr()) if stamps is not None else C.c_void_p(0)
    nbytes = stamps.numel() * stamps.element_size() if stamps is not None else 0
    check(_lib.load().lldwt_set_diagnostics(int(kind), ptr, nbytes, int(flags)), "lldwt_set_diagnostics")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t, name="tensor"):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise _lib.LLDWTError("%s must be a contiguous fp32 device tensor (got %s)" % (
            name, None if t is None else (t.device, t.dtype, t.is_contiguous())))
    return C.c_void_p(t.data_ptr())


def _opt(t, name="tensor"):
    return C.c_void_p(0) if t is None else _chk(t, name)


def workspace(nbytes, device):
    """Grow-only scratch buffer per device (the library never allocates: include/lldwt.h conventions).  While a forked
    lifting_forward has it in use on the tail stream (eval_overlap), nobody else gets it: asking is an error."""
    key = (device.type, device.index)
    ov = current_overlap()
    if ov is not None and ov.lent and ov.ws_key == key:
        raise _lib.LLDWTError("workspace: lent to the tail stream of a forked lifting transform until the join")
    buf = _ws.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _ws[key] = buf
    return buf


# ---- the forked eval step: the coarse end of the transform on a second stream ---------------------------
class _Overlap:
    """State of one eval_overlap context: the level the next lifting_forward forks at, the tail stream and the fork / join
    events; ``lent``: the workspace is with the tail stream, from the forked call until join()."""

    def __init__(self, split, device, tail, fork, done):
        self.split, self.tail, self.fork, self.done, self.lent = int(split), tail, fork, done, False
        self.ws_key = (device.type, device.index)       # the workspace() this context lends

    def join(self):
        """The current stream waits for everything enqueued on the tail so far; the workspace comes back."""
        if self.lent:
            self.done.record(self.tail)
            torch.cuda.current_stream().wait_event(self.done)
            self.lent = False


# One context per host thread (a thread drives one device at a time); the streams and events are per (thread, device), so two
# threads that run eval steps on two devices share nothing here.  workspace() itself is one buffer per device, as ever: two
# host threads on ONE device were never served by it (ownership and threading).
_tls = threading.local()
_tail_priority = [-1]           # -1: the highest priority the device offers, 0: the default (DESIGN.md 9 item 7 has both measured)


def current_overlap():
    """The eval_overlap context the calling thread is inside, or None."""
    return getattr(_tls, "ov", None)


def lift_split_level(Z, H, W, levels, cus=0):
    """The rule of the forked eval step (csrc/lift_split.h through lldwt_lift_split_level): the level to fork at, or 0."""
    r = _lib.load().lldwt_lift_split_level(int(Z), int(H), int(W), int(levels), int(cus))
    check(min(r, 0), "lift_split_level")
    return r


def set_tail_priority(priority):
    """Priority of the tail stream (torch.cuda.Stream's: -1 high, 0 default) for the streams created from now on; the
    calling thread's existing ones are dropped.  Diagnostics: tools/bench_tail_priority.py, the priority comparison of
    DESIGN.md 9 item 7."""
    if current_overlap() is not None:
        raise _lib.LLDWTError("set_tail_priority: inside an eval_overlap context")
    _tail_priority[0] = int(priority)
    _tls.tail = {}


def tail_stream(device):
    """The second stream of the forked eval step and its two events, created once per device (and host thread)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    tails = _tls.__dict__.setdefault("tail", {})
    ent = tails.get(idx)
    if ent is None:
        with torch.cuda.device(idx):
            st = torch.cuda.Stream(priority=_tail_priority[0])
            fork, done = torch.cuda.Event(), torch.cuda.Event()
            fork.record()           # torch creates the HIP event at its first record; the library is handed the handle
        ent = tails[idx] = (st, fork, done)
    return ent


class eval_overlap:
    """``with ops.eval_overlap(k, device) as ov:`` -- a lifting_forward inside forks at level k (lldwt_lifting_forward_split):
    levels < k on the current stream, the rest on ov.tail, where the caller continues their work under
    torch.cuda.stream(ov.tail).  ov.join() makes the current stream wait for the tail; leaving the context joins if the caller
    has not.  Not for a stream under capture, and not re-entrant."""

    def __init__(self, split_level, device):
        self.args = (split_level, device)

    def __enter__(self):
        if current_overlap() is not None:
            raise _lib.LLDWTError("eval_overlap: already inside one")
        if torch.cuda.is_current_stream_capturing():
            raise _lib.LLDWTError("eval_overlap: the current stream is under capture")
        _tls.ov = _Overlap(self.args[0], self.args[1], *tail_stream(self.args[1]))
        return _tls.ov

    def __exit__(self, *exc):
        try:
            _tls.ov.join()
        finally:
            _tls.ov = None
        return False


def rgb_to_ycc(x):
    """(B,3,H,W) RGB in [0,1] -> plane-major (3,B,1,H,W) YCbCr with Y-0.5 (agents/liftingDWT_agent.py:86-87)."""
    lib = _lib.load()
    B, c, H, W = x.shape
    assert c == 3
    y = torch.empty(3, B, 1, H, W, device=x.device, dtype=torch.float32)
    check(lib.lldwt_rgb_to_ycc(_chk(x, "x"), _chk(y), B, H, W, _stream()), "rgb_to_ycc")
    return y


def _u8hwc(src, who):
    """The input check of the uint8 image kernels -> (B, H, W)."""
    if not (isinstance(src, torch.Tensor) and src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous()
            and src.dim() == 4 and src.shape[3] == 3):
        raise _lib.LLDWTError("%s: expected a contiguous (B,H,W,3) uint8 device tensor" % who)
    return tuple(src.shape[:3])


def u8hwc_to_f32chw(src):
    """(B,H,W,3) uint8 device tensor -> (B,3,H,W) fp32 in [0,1] (ToTensor semantics, dataloaders/image_dl.py:81)."""
    B, H, W = _u8hwc(src, "u8hwc_to_f32chw")
    dst = torch.empty(B, 3, H, W, device=src.device, dtype=torch.float32)
    check(_lib.load().lldwt_u8hwc_to_f32chw(C.c_void_p(src.data_ptr()), _chk(dst), B, H, W, _stream()), "u8hwc_to_f32chw")
    return dst


def ycc_to_rgb(y, clamp=False):
    """plane-major (3,B,1,H,W) -> (B,3,H,W) RGB-0.5 (agents/liftingDWT_agent.py:90-94, clamp :181)."""
    lib = _lib.load()
    _, B, _, H, W = y.shape
    x = torch.empty(B, 3, H, W, device=y.device, dtype=torch.float32)
    check(lib.lldwt_ycc_to_rgb(_chk(y, "y"), _chk(x), B, H, W, int(bool(clamp)), _stream()), "ycc_to_rgb")
    return x


def u8hwc_to_ycc_pad(src, Hp, Wp):
    """(B,H,W,3) uint8 RGB device tensor -> plane-major (3,B,1,Hp,Wp) YCbCr with Y-0.5, replicate-edge padded
    (lldwt_u8hwc_to_ycc_pad; inside the image bitwise equal to rgb_to_ycc(u8hwc_to_f32chw(src)))."""
    B, H, W = _u8hwc(src, "u8hwc_to_ycc_pad")
    y = torch.empty(3, B, 1, Hp, Wp, device=src.device, dtype=torch.float32)
    check(_lib.load().lldwt_u8hwc_to_ycc_pad(C.c_void_p(src.data_ptr()), _chk(y), B, H, W, Hp, Wp, _stream()),
          "u8hwc_to_ycc_pad")
    return y


def u8hwc_to_ycc_tiles(src, th, tw, ny, nx, first, n):
    """(B,H,W,3) uint8 RGB device tensor -> plane-major (3,n,1,th,tw) YCbCr with Y-0.5 of the tiles first .. first+n-1 of a
    ny x nx grid of th x tw tiles per image (index (b * ny + ty) * nx + tx), replicate-edge padded past the image
    (lldwt_u8hwc_to_ycc_tiles; bitwise u8hwc_to_ycc_pad of the cropped tile)."""
    B, H, W = _u8hwc(src, "u8hwc_to_ycc_tiles")
    y = torch.empty(3, n, 1, th, tw, device=src.device, dtype=torch.float32)
    check(_lib.load().lldwt_u8hwc_to_ycc_tiles(C.c_void_p(src.data_ptr()), _chk(y), B, H, W, th, tw, ny, nx, first, n,
                                               _stream()), "u8hwc_to_ycc_tiles")
    return y


def _tiles_to_u8hwc(who, y, grid, region, affine, tiles, first, B, out):
    """The body of ycc_tiles_to_u8hwc (affine = None) and ll_tiles_to_u8hwc (affine = (inv_a, b)); who: the name in messages."""
    H, W, th, tw, ny, nx = grid
    y0, x0, h, w = region
    _, n, _, yh, yw = y.shape
    if (yh, yw) != (th, tw):
        raise _lib.LLDWTError("%s: tiles are %d x %d, the grid says %d x %d" % (who, yh, yw, th, tw))
    if affine is not None and (len(affine[0]) != 3 or len(affine[1]) != 3):
        raise _lib.LLDWTError("%s: inv_a and b need 3 values each" % who)
    tptr = C.c_void_p(0)
    if tiles is not None:
        if len(tiles) != n or any(t < 0 or t >= B * ny * nx for t in tiles):
            raise _lib.LLDWTError("%s: need %d tile indexes in [0, %d)" % (who, n, B * ny * nx))
        tiles = torch.tensor(list(tiles), dtype=torch.int32).to(y.device)
        tptr = C.c_void_p(tiles.data_ptr())
    if out is None:
        out = torch.empty(B, h, w, 3, device=y.device, dtype=torch.uint8)
    if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (B, h, w, 3)):
        raise _lib.LLDWTError("%s: out must be a contiguous (%d,%d,%d,3) uint8 device tensor" % (who, B, h, w))
    args = (_chk(y, "y"), tptr, first, n, B, H, W, th, tw, ny, nx, y0, x0, h, w)
    if affine is None:
        check(_lib.load().lldwt_ycc_tiles_to_u8hwc(*args, C.c_void_p(out.data_ptr()), _stream()), who)
    else:
        ia = (C.c_float * 3)(*[float(v) for v in affine[0]])
        bb = (C.c_float * 3)(*[float(v) for v in affine[1]])
        check(_lib.load().lldwt_ll_tiles_to_u8hwc(*args, C.cast(ia, C.c_void_p), C.cast(bb, C.c_void_p),
                                                  C.c_void_p(out.data_ptr()), _stream()), who)
    return out


def ycc_tiles_to_u8hwc(y, grid, region, tiles=None, first=0, B=1, out=None):
    """plane-major (3,n,1,th,tw) decoded tiles -> the uint8 RGB pixels of those tiles inside the image and the region,
    written into out (B,h,w,3) (allocated when None; pixels no tile covers are left as they are) and returned.
    grid = (H, W, th, tw, ny, nx); region = (y0, x0, h, w) inside the image; tiles: the n tile indexes (list), or None for
    first .. first+n-1 (lldwt_ycc_tiles_to_u8hwc: bytes as ycc_to_u8hwc_crop)."""
    return _tiles_to_u8hwc("ycc_tiles_to_u8hwc", y, grid, region, None, tiles, first, B, out)


def ll_tiles_to_u8hwc(y, grid, region, inv_a, b, tiles=None, first=0, B=1, out=None):
    """ycc_tiles_to_u8hwc for a reduced-resolution decode: y (3,n,1,th,tw) holds each tile's decoded LL band at level k, grid
    and region are in reduced coordinates, and plane p's samples become (s - b[p]) * inv_a[p] before the colour and u8 rule
    (lldwt_ll_tiles_to_u8hwc; inv_a, b: 3 floats each, lifting_dwt_nets.ll_affine).  The untiled decode is the 1 x 1 grid."""
    return _tiles_to_u8hwc("ll_tiles_to_u8hwc", y, grid, region, (inv_a, b), tiles, first, B, out)


def ycc_tiles_sq_err(y, grid, src, tiles=None, first=0, B=1, out=None):
    """The exact squared error of the bytes ycc_tiles_to_u8hwc(y, grid, (0, 0, H, W), ...) would write against the original
    src (B,H,W,3) uint8, per image, without writing them (lldwt_ycc_tiles_sq_err) -> the (B,) int64 device
    tensor of sums.  y: plane-major (3,n,1,th,tw) decoded tiles; grid = (H, W, th, tw, ny, nx); tiles: the n tile indexes
    (list; an index outside [0, B * ny * nx) adds nothing), or None for first .. first+n-1.  out: a (B,) int64 device tensor
    that is added to (several calls may feed one sum); None: a zeroed one.  Integer sums: exact and reproducible."""
    who = "ycc_tiles_sq_err"
    H, W, th, tw, ny, nx = grid
    if not (isinstance(y, torch.Tensor) and y.dim() == 5 and y.shape[0] == 3 and y.shape[2] == 1):
        raise _lib.LLDWTError("%s: y must be (3,n,1,th,tw)" % who)
    _, n, _, yh, yw = y.shape
    if (yh, yw) != (th, tw):
        raise _lib.LLDWTError("%s: tiles are %d x %d, the grid says %d x %d" % (who, yh, yw, th, tw))
    if _u8hwc(src, who) != (B, H, W):
        raise _lib.LLDWTError("%s: src is %s, the grid says (%d,%d,%d,3)" % (who, tuple(src.shape), B, H, W))
    tptr = C.c_void_p(0)
    if tiles is not None:
        if len(tiles) != n or any(not -(1 << 31) <= t < 1 << 31 for t in tiles):
            raise _lib.LLDWTError("%s: need %d tile indexes that fit 32 bits" % (who, n))
        tiles = torch.tensor(list(tiles), dtype=torch.int32).to(y.device)
        tptr = C.c_void_p(tiles.data_ptr())
    if out is None:
        out = torch.zeros(B, device=y.device, dtype=torch.int64)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.int64 and out.is_contiguous()
            and tuple(out.shape) == (B,)):
        raise _lib.LLDWTError("%s: out must be a contiguous (%d,) int64 device tensor" % (who, B))
    check(_lib.load().lldwt_ycc_tiles_sq_err(_chk(y, "y"), tptr, first, n, B, H, W, th, tw, ny, nx, C.c_void_p(src.data_ptr()),
                                             C.c_void_p(out.data_ptr()), _stream()), who)
    return out


def u8hwc_to_ycc_tiles_lapped(src, th, tw, ov, ny, nx, first, n):
    """u8hwc_to_ycc_tiles on a lapped grid: tile (ty, tx) starts at (ty * (th - ov), tx * (tw - ov)), so neighbours share ov
    pixels (lldwt_u8hwc_to_ycc_tiles_lapped; bitwise u8hwc_to_ycc_pad of the replicate-padded crop)."""
    B, H, W = _u8hwc(src, "u8hwc_to_ycc_tiles_lapped")
    if n < 1 or th < 1 or tw < 1:
        raise _lib.LLDWTError("u8hwc_to_ycc_tiles_lapped: n, th, tw must be positive")
    y = torch.empty(3, n, 1, th, tw, device=src.device, dtype=torch.float32)
    check(_lib.load().lldwt_u8hwc_to_ycc_tiles_lapped(C.c_void_p(src.data_ptr()), _chk(y), B, H, W, th, tw, ov, ny, nx,
                                                      first, n, _stream()), "u8hwc_to_ycc_tiles_lapped")
    return y


def ycc_tiles_blend(y, grid, region, tiles, acc):
    """Accumulates the decoded lapped tiles y (3,n,1,th,tw), whose tile indexes (ty * nx + tx, one image) are ``tiles``, into
    the fp32 region buffer acc (3,1,1,h,w) with the cross-fade weights of codec.lap_weights, and returns acc.
    grid = (H, W, th, tw, ov, ny, nx); region = (y0, x0, h, w) inside the image.  acc must be zero before the first group
    of a decode and the groups must come in ascending tile index (lldwt_ycc_tiles_blend)."""
    H, W, th, tw, ov, ny, nx = grid
    y0, x0, h, w = region
    if not (isinstance(y, torch.Tensor) and y.dim() == 5 and y.shape[0] == 3 and y.shape[2] == 1):
        raise _lib.LLDWTError("ycc_tiles_blend: y must be (3,n,1,th,tw)")
    _, n, _, yh, yw = y.shape
    if (yh, yw) != (th, tw):
        raise _lib.LLDWTError("ycc_tiles_blend: tiles are %d x %d, the grid says %d x %d" % (yh, yw, th, tw))
    tiles = list(tiles)
    if len(tiles) != n or len(set(tiles)) != n or any(t < 0 or t >= ny * nx for t in tiles):
        raise _lib.LLDWTError("ycc_tiles_blend: need %d distinct tile indexes in [0, %d)" % (n, ny * nx))
    if not (isinstance(acc, torch.Tensor) and acc.is_cuda and acc.dtype == torch.float32 and acc.is_contiguous()
            and tuple(acc.shape) == (3, 1, 1, h, w)):
        raise _lib.LLDWTError("ycc_tiles_blend: acc must be a contiguous (3,1,1,%d,%d) fp32 device tensor" % (h, w))
    slots = torch.full((ny * nx,), -1, dtype=torch.int32)
    slots[torch.tensor(tiles, dtype=torch.int64)] = torch.arange(n, dtype=torch.int32)
    slots = slots.to(y.device)
    check(_lib.load().lldwt_ycc_tiles_blend(_chk(y, "y"), C.c_void_p(slots.data_ptr()), ny * nx, n, H, W, th, tw, ov, ny, nx,
                                            y0, x0, h, w, _chk(acc, "acc"), _stream()), "ycc_tiles_blend")
    return acc


def ycc_to_u8hwc_crop(y, H, W):
    """plane-major (3,B,1,Hp,Wp) YCbCr with Y-0.5 -> (B,H,W,3) uint8 RGB of the top-left H x W
    (lldwt_ycc_to_u8hwc_crop: floor((v + 0.5) * 255 + 0.5) of v = ycc_to_rgb(y, clamp=True))."""
    _, B, _, Hp, Wp = y.shape
    dst = torch.empty(B, H, W, 3, device=y.device, dtype=torch.uint8)
    check(_lib.load().lldwt_ycc_to_u8hwc_crop(_chk(y, "y"), C.c_void_p(dst.data_ptr()), B, H, W, Hp, Wp, _stream()),
          "ycc_to_u8hwc_crop")
    return dst


def u8hwc_to_ycc420_tiles(src, th, tw, ny, nx, first, n):
    """u8hwc_to_ycc_tiles for 4:2:0: (B,H,W,3) uint8 RGB device tensor -> (luma (1,n,1,th,tw) with Y-0.5,
    chroma (2,n,1,th/2,tw/2)) of the tiles first .. first+n-1; luma is bitwise plane 0 of u8hwc_to_ycc_tiles, a chroma sample
    ((c00 + c01) + (c10 + c11)) * 0.25f over its 2 x 2 tile pixels (lldwt_u8hwc_to_ycc420_tiles).  th, tw even."""
    who = "u8hwc_to_ycc420_tiles"
    B, H, W = _u8hwc(src, who)
    if n < 1 or th < 2 or tw < 2 or th % 2 or tw % 2:
        raise _lib.LLDWTError("%s: n must be positive and th, tw even (got %r, %r, %r)" % (who, n, th, tw))
    luma = torch.empty(1, n, 1, th, tw, device=src.device, dtype=torch.float32)
    chroma = torch.empty(2, n, 1, th // 2, tw // 2, device=src.device, dtype=torch.float32)
    check(_lib.load().lldwt_u8hwc_to_ycc420_tiles(C.c_void_p(src.data_ptr()), _chk(luma), _chk(chroma), B, H, W, th, tw, ny, nx,
                                                  first, n, _stream()), who)
    return luma, chroma


def _tile_list(who, tiles, n, count, dev):
    """The tile list argument of the chroma output wrappers -> (pointer, the device tensor that must outlive the call)."""
    if tiles is None:
        return C.c_void_p(0), None
    if len(tiles) != n or any(t < 0 or t >= count for t in tiles):
        raise _lib.LLDWTError("%s: need %d tile indexes in [0, %d)" % (who, n, count))
    t = torch.tensor(list(tiles), dtype=torch.int32).to(dev)
    return C.c_void_p(t.data_ptr()), t


def _affine_arg(who, affine, count):
    """affine = None or (inv_a, b) of ``count`` floats each -> two pointers (NULL, NULL for None) and their owners."""
    if affine is None:
        return C.c_void_p(0), C.c_void_p(0), None
    if len(affine) != 2 or len(affine[0]) != count or len(affine[1]) != count:
        raise _lib.LLDWTError("%s: inv_a and b need %d value(s) each" % (who, count))
    ia = (C.c_float * count)(*[float(v) for v in affine[0]])
    bb = (C.c_float * count)(*[float(v) for v in affine[1]])
    return C.cast(ia, C.c_void_p), C.cast(bb, C.c_void_p), (ia, bb)


def ycc420_tiles_to_u8hwc(luma, chroma, grid, region, affine=None, tiles=None, first=0, B=1, out=None):
    """ycc_tiles_to_u8hwc for 4:2:0: luma (1,n,1,th,tw) and chroma (2,n,1,th/2,tw/2) decoded tiles -> the
    uint8 RGB pixels of those tiles inside the image and the region, written into out (B,h,w,3) (allocated when None) and
    returned; the chroma is upsampled in registers with the weights 3/4, 1/4 clamped at the tile's own plane.  grid, region,
    tiles, first as ycc_tiles_to_u8hwc.  affine = (inv_a, b), 3 floats each: a reduced-resolution decode, every luma and chroma
    sample of plane p becomes (s - b[p]) * inv_a[p] before the upsampling (lldwt_ycc420_tiles_to_u8hwc)."""
    who = "ycc420_tiles_to_u8hwc"
    H, W, th, tw, ny, nx = grid
    y0, x0, h, w = region
    if not (isinstance(luma, torch.Tensor) and luma.dim() == 5 and luma.shape[0] == 1 and luma.shape[2] == 1):
        raise _lib.LLDWTError("%s: luma must be (1,n,1,th,tw)" % who)
    n = luma.shape[1]
    if tuple(luma.shape[3:]) != (th, tw) or th % 2 or tw % 2:
        raise _lib.LLDWTError("%s: luma tiles are %d x %d, the grid says %d x %d (even sides)" % (who, luma.shape[3], luma.shape[4],
                                                                                                  th, tw))
    if not (isinstance(chroma, torch.Tensor) and tuple(chroma.shape) == (2, n, 1, th // 2, tw // 2)):
        raise _lib.LLDWTError("%s: chroma must be (2,%d,1,%d,%d)" % (who, n, th // 2, tw // 2))
    tptr, keep = _tile_list(who, tiles, n, B * ny * nx, luma.device)
    ia, bb, keep_af = _affine_arg(who, affine, 3)
    if out is None:
        out = torch.empty(B, h, w, 3, device=luma.device, dtype=torch.uint8)
    if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (B, h, w, 3)):
        raise _lib.LLDWTError("%s: out must be a contiguous (%d,%d,%d,3) uint8 device tensor" % (who, B, h, w))
    check(_lib.load().lldwt_ycc420_tiles_to_u8hwc(_chk(luma, "luma"), _chk(chroma, "chroma"), tptr, first, n, B, H, W, th, tw, ny,
                                                  nx, y0, x0, h, w, ia, bb, C.c_void_p(out.data_ptr()), _stream()), who)
    return out


def u8hw_to_y_tiles(src, th, tw, ny, nx, first, n):
    """u8hwc_to_ycc_tiles for greyscale (4:0:0): (B,H,W,1) uint8 device tensor -> (1,n,1,th,tw),
    g / 255.0f - 0.5f, of the tiles first .. first+n-1, replicate-edge padded (lldwt_u8hw_to_y_tiles)."""
    who = "u8hw_to_y_tiles"
    if not (isinstance(src, torch.Tensor) and src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous()
            and src.dim() == 4 and src.shape[3] == 1):
        raise _lib.LLDWTError("%s: expected a contiguous (B,H,W,1) uint8 device tensor" % who)
    if n < 1 or th < 1 or tw < 1:
        raise _lib.LLDWTError("%s: n, th, tw must be positive" % who)
    B, H, W = src.shape[:3]
    y = torch.empty(1, n, 1, th, tw, device=src.device, dtype=torch.float32)
    check(_lib.load().lldwt_u8hw_to_y_tiles(C.c_void_p(src.data_ptr()), _chk(y), B, H, W, th, tw, ny, nx, first, n, _stream()),
          who)
    return y


def y_tiles_to_u8hw(y, grid, region, affine=None, tiles=None, first=0, B=1, out=None):
    """ycc_tiles_to_u8hwc for greyscale (4:0:0): y (1,n,1,th,tw) decoded tiles -> the uint8 pixels of those
    tiles inside the image and the region, floor((clamp(s, -0.5, 0.5) + 0.5) * 255 + 0.5), written into out (B,h,w,1)
    (allocated when None) and returned.  affine = (inv_a, b), 1 float each: s -> (s - b[0]) * inv_a[0] first, a reduced-resolution
    decode (lldwt_y_tiles_to_u8hw)."""
    who = "y_tiles_to_u8hw"
    H, W, th, tw, ny, nx = grid
    y0, x0, h, w = region
    if not (isinstance(y, torch.Tensor) and y.dim() == 5 and y.shape[0] == 1 and y.shape[2] == 1):
        raise _lib.LLDWTError("%s: y must be (1,n,1,th,tw)" % who)
    n = y.shape[1]
    if tuple(y.shape[3:]) != (th, tw):
        raise _lib.LLDWTError("%s: tiles are %d x %d, the grid says %d x %d" % (who, y.shape[3], y.shape[4], th, tw))
    tptr, keep = _tile_list(who, tiles, n, B * ny * nx, y.device)
    ia, bb, keep_af = _affine_arg(who, affine, 1)
    if out is None:
        out = torch.empty(B, h, w, 1, device=y.device, dtype=torch.uint8)
    if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (B, h, w, 1)):
        raise _lib.LLDWTError("%s: out must be a contiguous (%d,%d,%d,1) uint8 device tensor" % (who, B, h, w))
    check(_lib.load().lldwt_y_tiles_to_u8hw(_chk(y, "y"), tptr, first, n, B, H, W, th, tw, ny, nx, y0, x0, h, w, ia, bb,
                                            C.c_void_p(out.data_ptr()), _stream()), who)
    return out


# ---- samples of 9 to 16 bits (csrc/depth.hip): the uint16 siblings of the wrappers above, same argument checks
def _u16(src, ch, depth, who):
    """The input check of the uint16 image kernels -> (B, H, W).  depth: 8 .. 16 at this level, always on uint16 storage."""
    if not (isinstance(src, torch.Tensor) and src.is_cuda and src.dtype == torch.uint16 and src.is_contiguous()
            and src.dim() == 4 and src.shape[3] == ch):
        raise _lib.LLDWTError("%s: expected a contiguous (B,H,W,%d) uint16 device tensor" % (who, ch))
    _depth(depth, who)
    return tuple(src.shape[:3])


def _depth(depth, who):
    if isinstance(depth, bool) or not isinstance(depth, int) or not 8 <= depth <= 16:
        raise _lib.LLDWTError("%s: depth must be an integer in [8, 16] (got %r)" % (who, depth))


def depth_flag(device):
    """A zeroed int32 device scalar for the range flag of the uint16 input kernels: they store 1 there when they meet a sample
    above 2^depth - 1 and never write it otherwise, so one flag may serve every call of an encode."""
    return torch.zeros(1, device=device, dtype=torch.int32)


def _flag(flag, src, who):
    if flag is None:
        return depth_flag(src.device)
    if not (isinstance(flag, torch.Tensor) and flag.is_cuda and flag.dtype == torch.int32 and flag.numel() == 1):
        raise _lib.LLDWTError("%s: flag must be an int32 device scalar" % who)
    return flag


def _out_u16(who, out, shape, dev):
    if out is None:
        out = torch.empty(*shape, device=dev, dtype=torch.uint16)
    if not (out.is_cuda and out.dtype == torch.uint16 and out.is_contiguous() and tuple(out.shape) == tuple(shape)):
        raise _lib.LLDWTError("%s: out must be a contiguous (%d,%d,%d,%d) uint16 device tensor" % ((who,) + tuple(shape)))
    return out


def u16hwc_to_f32chw(src, depth, flag=None):
    """u8hwc_to_f32chw on uint16: (B,H,W,3) uint16 device tensor -> (B,3,H,W) fp32, v / (2^depth - 1).  flag: as
    u16hwc_to_ycc_tiles (lldwt_u16hwc_to_f32chw)."""
    who = "u16hwc_to_f32chw"
    B, H, W = _u16(src, 3, depth, who)
    flag = _flag(flag, src, who)
    dst = torch.empty(B, 3, H, W, device=src.device, dtype=torch.float32)
    check(_lib.load().lldwt_u16hwc_to_f32chw(C.c_void_p(src.data_ptr()), _chk(dst), B, H, W, depth, C.c_void_p(flag.data_ptr()),
                                             _stream()), who)
    return dst


def u16hwc_to_ycc_tiles(src, th, tw, ny, nx, first, n, depth, flag=None):
    """u8hwc_to_ycc_tiles on (B,H,W,3) uint16 samples of ``depth`` bits: v / (2^depth - 1), then the same expressions, so depth 8
    gives the uint8 wrapper's floats bit for bit.  flag: an int32 device scalar (depth_flag) that receives 1 when a sample exceeds
    2^depth - 1; None: a private one nobody reads (lldwt_u16hwc_to_ycc_tiles)."""
    who = "u16hwc_to_ycc_tiles"
    B, H, W = _u16(src, 3, depth, who)
    flag = _flag(flag, src, who)
    y = torch.empty(3, n, 1, th, tw, device=src.device, dtype=torch.float32)
    check(_lib.load().lldwt_u16hwc_to_ycc_tiles(C.c_void_p(src.data_ptr()), _chk(y), B, H, W, th, tw, ny, nx, first, n, depth,
                                                C.c_void_p(flag.data_ptr()), _stream()), who)
    return y


def ycc_tiles_to_u16hwc(y, grid, region, depth, affine=None, tiles=None, first=0, B=1, out=None):
    """ycc_tiles_to_u8hwc (affine=None) and ll_tiles_to_u8hwc (affine = (inv_a, b), 3 floats each) for samples of ``depth`` bits:
    floor((c + 0.5) * (2^depth - 1) + 0.5) stored as uint16 into out (B,h,w,3) (lldwt_ycc_tiles_to_u16hwc)."""
    who = "ycc_tiles_to_u16hwc"
    H, W, th, tw, ny, nx = grid
    y0, x0, h, w = region
    _depth(depth, who)
    if not (isinstance(y, torch.Tensor) and y.dim() == 5 and y.shape[0] == 3 and y.shape[2] == 1):
        raise _lib.LLDWTError("%s: y must be (3,n,1,th,tw)" % who)
    n = y.shape[1]
    if tuple(y.shape[3:]) != (th, tw):
        raise _lib.LLDWTError("%s: tiles are %d x %d, the grid says %d x %d" % (who, y.shape[3], y.shape[4], th, tw))
    tptr, keep = _tile_list(who, tiles, n, B * ny * nx, y.device)
    ia, bb, keep_af = _affine_arg(who, affine, 3)
    out = _out_u16(who, out, (B, h, w, 3), y.device)
    check(_lib.load().lldwt_ycc_tiles_to_u16hwc(_chk(y, "y"), tptr, first, n, B, H, W, th, tw, ny, nx, y0, x0, h, w, ia, bb, depth,
                                                C.c_void_p(out.data_ptr()), _stream()), who)
    return out


def u16hwc_to_ycc420_tiles(src, th, tw, ny, nx, first, n, depth, flag=None):
    """u8hwc_to_ycc420_tiles on (B,H,W,3) uint16 samples of ``depth`` bits -> (luma, chroma); flag as u16hwc_to_ycc_tiles
    (lldwt_u16hwc_to_ycc420_tiles).  th, tw even."""
    who = "u16hwc_to_ycc420_tiles"
    B, H, W = _u16(src, 3, depth, who)
    if n < 1 or th < 2 or tw < 2 or th % 2 or tw % 2:
        raise _lib.LLDWTError("%s: n must be positive and th, tw even (got %r, %r, %r)" % (who, n, th, tw))
    flag = _flag(flag, src, who)
    luma = torch.empty(1, n, 1, th, tw, device=src.device, dtype=torch.float32)
    chroma = torch.empty(2, n, 1, th // 2, tw // 2, device=src.device, dtype=torch.float32)
    check(_lib.load().lldwt_u16hwc_to_ycc420_tiles(C.c_void_p(src.data_ptr()), _chk(luma), _chk(chroma), B, H, W, th, tw, ny, nx,
                                                   first, n, depth, C.c_void_p(flag.data_ptr()), _stream()), who)
    return luma, chroma


def ycc420_tiles_to_u16hwc(luma, chroma, grid, region, depth, affine=None, tiles=None, first=0, B=1, out=None):
    """ycc420_tiles_to_u8hwc for samples of ``depth`` bits, stored as uint16 into out (B,h,w,3) (lldwt_ycc420_tiles_to_u16hwc)."""
    who = "ycc420_tiles_to_u16hwc"
    H, W, th, tw, ny, nx = grid
    y0, x0, h, w = region
    _depth(depth, who)
    if not (isinstance(luma, torch.Tensor) and luma.dim() == 5 and luma.shape[0] == 1 and luma.shape[2] == 1):
        raise _lib.LLDWTError("%s: luma must be (1,n,1,th,tw)" % who)
    n = luma.shape[1]
    if tuple(luma.shape[3:]) != (th, tw) or th % 2 or tw % 2:
        raise _lib.LLDWTError("%s: luma tiles are %d x %d, the grid says %d x %d (even sides)" % (who, luma.shape[3], luma.shape[4],
                                                                                                  th, tw))
    if not (isinstance(chroma, torch.Tensor) and tuple(chroma.shape) == (2, n, 1, th // 2, tw // 2)):
        raise _lib.LLDWTError("%s: chroma must be (2,%d,1,%d,%d)" % (who, n, th // 2, tw // 2))
    tptr, keep = _tile_list(who, tiles, n, B * ny * nx, luma.device)
    ia, bb, keep_af = _affine_arg(who, affine, 3)
    out = _out_u16(who, out, (B, h, w, 3), luma.device)
    check(_lib.load().lldwt_ycc420_tiles_to_u16hwc(_chk(luma, "luma"), _chk(chroma, "chroma"), tptr, first, n, B, H, W, th, tw, ny,
                                                   nx, y0, x0, h, w, ia, bb, depth, C.c_void_p(out.data_ptr()), _stream()), who)
    return out


def u16hw_to_y_tiles(src, th, tw, ny, nx, first, n, depth, flag=None):
    """u8hw_to_y_tiles on (B,H,W,1) uint16 samples of ``depth`` bits: v / (2^depth - 1) - 0.5f; flag as u16hwc_to_ycc_tiles
    (lldwt_u16hw_to_y_tiles)."""
    who = "u16hw_to_y_tiles"
    B, H, W = _u16(src, 1, depth, who)
    if n < 1 or th < 1 or tw < 1:
        raise _lib.LLDWTError("%s: n, th, tw must be positive" % who)
    flag = _flag(flag, src, who)
    y = torch.empty(1, n, 1, th, tw, device=src.device, dtype=torch.float32)
    check(_lib.load().lldwt_u16hw_to_y_tiles(C.c_void_p(src.data_ptr()), _chk(y), B, H, W, th, tw, ny, nx, first, n, depth,
                                             C.c_void_p(flag.data_ptr()), _stream()), who)
    return y


def y_tiles_to_u16hw(y, grid, region, depth, affine=None, tiles=None, first=0, B=1, out=None):
    """y_tiles_to_u8hw for samples of ``depth`` bits, stored as uint16 into out (B,h,w,1) (lldwt_y_tiles_to_u16hw)."""
    who = "y_tiles_to_u16hw"
    H, W, th, tw, ny, nx = grid
    y0, x0, h, w = region
    _depth(depth, who)
    if not (isinstance(y, torch.Tensor) and y.dim() == 5 and y.shape[0] == 1 and y.shape[2] == 1):
        raise _lib.LLDWTError("%s: y must be (1,n,1,th,tw)" % who)
    n = y.shape[1]
    if tuple(y.shape[3:]) != (th, tw):
        raise _lib.LLDWTError("%s: tiles are %d x %d, the grid says %d x %d" % (who, y.shape[3], y.shape[4], th, tw))
    tptr, keep = _tile_list(who, tiles, n, B * ny * nx, y.device)
    ia, bb, keep_af = _affine_arg(who, affine, 1)
    out = _out_u16(who, out, (B, h, w, 1), y.device)
    check(_lib.load().lldwt_y_tiles_to_u16hw(_chk(y, "y"), tptr, first, n, B, H, W, th, tw, ny, nx, y0, x0, h, w, ia, bb, depth,
                                             C.c_void_p(out.data_ptr()), _stream()), who)
    return out


RESID_MAX_NEAR = 32          # LLDWT_RESID_MAX_NEAR
RESID_CONTEXTS = 24          # 3 channels x 8 activity classes


def resid_unit_size(grid, t):
    """The in-image rectangle size (uh, uw) of tile t of grid = (H, W, th, tw, ny, nx) (any image of the batch)."""
    H, W, th, tw, ny, nx = grid
    ty, tx = divmod(int(t) % (ny * nx), nx)
    return min(th, H - ty * th), min(tw, W - tx * tw)


def _resid_args(who, bufs, grid, region, tiles, B):
    """The shared checks of the residual kernels -> (tile tensor on the device, n, uh, uw, geometry arguments)."""
    H, W, th, tw, ny, nx = (int(v) for v in grid)
    y0, x0, h, w = (int(v) for v in region)
    for t in bufs:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
                and tuple(t.shape) == (B, h, w, 3)):
            raise _lib.LLDWTError("%s: image buffers must be contiguous (%d,%d,%d,3) uint8 device tensors" % (who, B, h, w))
    tiles = [int(t) for t in tiles]
    if not tiles or any(t < 0 or t >= B * ny * nx for t in tiles):
        raise _lib.LLDWTError("%s: need at least one tile index in [0, %d)" % (who, B * ny * nx))
    sizes = {resid_unit_size((H, W, th, tw, ny, nx), t) for t in tiles}
    if len(sizes) != 1:
        raise _lib.LLDWTError("%s: the units of one call must have one rectangle size (got %s)" % (who, sorted(sizes)))
    uh, uw = sizes.pop()
    for t in tiles:
        ty, tx = divmod(t % (ny * nx), nx)
        if ty * th < y0 or tx * tw < x0 or ty * th + uh > y0 + h or tx * tw + uw > x0 + w:
            raise _lib.LLDWTError("%s: tile %d is not inside the region %s" % (who, t, (y0, x0, h, w)))
    tdev = torch.tensor(tiles, dtype=torch.int32).to(bufs[0].device)
    return tdev, len(tiles), uh, uw, (0, len(tiles), B, H, W, th, tw, ny, nx, y0, x0, h, w, uh, uw)


def resid_analyse(x, xh, grid, region, tiles, d):
    """Encoder kernel of the residual layer (lldwt_resid_analyse).  x, xh: (B,h,w,3) uint8 device buffers
    of the region (y0, x0, h, w) of the originals and the base reconstructions; grid = (H, W, th, tw, ny, nx); tiles: the
    units (tile indexes (b * ny + ty) * nx + tx, one rectangle size, inside the region); d: the bound, 0 = lossless.
    -> (sym (3n, uh*uw) int32, ctx (3n, uh*uw) int32, hist (n,3,8,2Q+1) int32, cs_xh (n) int64, cs_x (n) int64); the
    checksums are the uint64 sums reinterpreted as int64."""
    d = int(d)
    if not 0 <= d <= RESID_MAX_NEAR:
        raise _lib.LLDWTError("resid_analyse: near-lossless bound %d outside [0, %d]" % (d, RESID_MAX_NEAR))
    tdev, n, uh, uw, geo = _resid_args("resid_analyse", (x, xh), grid, region, tiles, int(x.shape[0]))
    Q = (255 + d) // (2 * d + 1)
    dev = x.device
    sym = torch.empty(3 * n, uh * uw, device=dev, dtype=torch.int32)
    ctx = torch.empty(3 * n, uh * uw, device=dev, dtype=torch.int32)
    hist = torch.zeros(n, 3, 8, 2 * Q + 1, device=dev, dtype=torch.int32)
    cs = torch.zeros(2, n, device=dev, dtype=torch.int64)
    p = lambda t: C.c_void_p(t.data_ptr())
    check(_lib.load().lldwt_resid_analyse(p(x), p(xh), p(tdev), *geo, d, p(sym), p(ctx), p(hist), p(cs[0]), p(cs[1]),
                                          _stream()), "resid_analyse")
    return sym, ctx, hist, cs[0], cs[1]


def resid_contexts(xh, grid, region, tiles, scales):
    """Decoder kernel (lldwt_resid_contexts): xh as resid_analyse; scales: (n, 24) uint8 device tensor, the table index of
    each context c * 8 + a of each unit -> (idx (3n, uh*uw) int32, cs_xh (n) int64)."""
    tdev, n, uh, uw, geo = _resid_args("resid_contexts", (xh,), grid, region, tiles, int(xh.shape[0]))
    if not (isinstance(scales, torch.Tensor) and scales.is_cuda and scales.dtype == torch.uint8 and scales.is_contiguous()
            and tuple(scales.shape) == (n, RESID_CONTEXTS)):
        raise _lib.LLDWTError("resid_contexts: scales must be a contiguous (%d,%d) uint8 device tensor" % (n, RESID_CONTEXTS))
    idx = torch.empty(3 * n, uh * uw, device=xh.device, dtype=torch.int32)
    cs = torch.zeros(n, device=xh.device, dtype=torch.int64)
    p = lambda t: C.c_void_p(t.data_ptr())
    check(_lib.load().lldwt_resid_contexts(p(xh), p(tdev), *geo, p(scales), p(idx), p(cs), _stream()), "resid_contexts")
    return idx, cs


def resid_apply(xh, grid, region, tiles, d, sym, out=None):
    """Decoder kernel (lldwt_resid_apply): out = clamp(xh + sym * (2d + 1), 0, 255) on the units' pixels, written into out
    (a buffer like xh; None: xh itself, in place) -> (out, cs_out (n) int64).  sym: (3n, uh*uw) int32 device tensor."""
    d = int(d)
    if not 0 <= d <= RESID_MAX_NEAR:
        raise _lib.LLDWTError("resid_apply: near-lossless bound %d outside [0, %d]" % (d, RESID_MAX_NEAR))
    out = xh if out is None else out
    tdev, n, uh, uw, geo = _resid_args("resid_apply", (xh, out), grid, region, tiles, int(xh.shape[0]))
    if not (isinstance(sym, torch.Tensor) and sym.is_cuda and sym.dtype == torch.int32 and sym.is_contiguous()
            and tuple(sym.shape) == (3 * n, uh * uw)):
        raise _lib.LLDWTError("resid_apply: sym must be a contiguous (%d,%d) int32 device tensor" % (3 * n, uh * uw))
    cs = torch.zeros(n, device=xh.device, dtype=torch.int64)
    p = lambda t: C.c_void_p(t.data_ptr())
    check(_lib.load().lldwt_resid_apply(p(xh), p(tdev), *geo, d, p(sym), p(out), p(cs), _stream()), "resid_apply")
    return out, cs


def pblock_packed_floats(Cc, K):
    return int(_lib.load().lldwt_pblock_packed_floats(Cc, K))


def pack_pblock(w1, b1, w2, b2, w3, b3, w4, b4, train=False, compose=True):
    """Stacked P_block_v2 parameters (planes, ...) in PyTorch layout -> packed (planes, total) buffer.  train=True: for the
    fp32 training kernels only (the split-fp16 section of the buffer is not written).  compose=False: the split-fp16 section
    without the composed 9x9 kernels of the eval path (lldwt_pack_pblock_seq: the fused training forward's pack)."""
    lib = _lib.load()
    planes, Cc, _, K, _ = w1.shape
    out = torch.empty(planes, pblock_packed_floats(Cc, K), device=w1.device, dtype=torch.float32)
    fn = lib.lldwt_pack_pblock_train if train else (lib.lldwt_pack_pblock if compose else lib.lldwt_pack_pblock_seq)
    check(fn(_chk(w1), _chk(b1), _chk(w2), _chk(b2), _chk(w3), _chk(b3), _chk(w4), _chk(b4), _chk(out), planes, Cc, K,
             _stream()), "pack_pblock")
    return out


def bwd_lift_f16():
    """True when lift_step_bwd with a backward pack runs the fused split-fp16 backward-data launch (include/lldwt.h)."""
    return bool(_lib.load().lldwt_bwd_lift_f16())


def pack_pblock_bwd(w1, w2, w3, w4):
    """Backward pack of a tanh P_block_v2 (planes, 16, ., 5, 5): transposed, mirrored weights in the forward pack's layout."""
    lib = _lib.load()
    planes, Cc, _, K, _ = w1.shape
    out = torch.empty(planes, pblock_packed_floats(Cc, K), device=w1.device, dtype=torch.float32)
    nb = lib.lldwt_pack_pblock_bwd_ws_bytes(planes)
    ws = workspace(nb, w1.device)
    check(lib.lldwt_pack_pblock_bwd(_chk(w1), _chk(w2), _chk(w3), _chk(w4), _chk(out), C.c_void_p(ws.data_ptr()), nb, planes,
                                    Cc, K, _stream()), "pack_pblock_bwd")
    return out


def view_of(t, z, h, w, offset=0, sz=None, sy=None, sx=1):
    """lldwt_view over the storage of ``t`` (element offsets/strides)."""
    return View(C.c_void_p(t.data_ptr() + 4 * offset), sz if sz is not None else h * w, sy if sy is not None else w, sx)


def lift_step(src, dst_in, dst_out, Z, batch, h, w, taps, packed, Cc, K, vertical, sign, res_weight, linear=False):
    """One lifting step on lldwt_view arguments (see include/lldwt.h)."""
    lib = _lib.load()
    nb = lib.lldwt_lift_step_ws_bytes(Z, h, w, Cc)
    ws = workspace(nb, taps.device)
    check(lib.lldwt_lift_step(src, dst_in, dst_out, Z, batch, h, w, _chk(taps), _chk(packed), Cc, K, int(vertical),
                              float(sign), float(res_weight), int(bool(linear)), C.c_void_p(ws.data_ptr()), nb,
                              _stream()), "lift_step")


def _ptr_array(tensors):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


def lifting_forward(x, taps, packed, levels, Cc, K, res_weight, linear=False, different=False, scale_nh=None,
                    scale_nl=None, block_offset=0):
    """x: (P,B,1,H,W) -> (ll (P,B,1,H>>L,W>>L), [yh_i (P,B,3,H>>(i+1),W>>(i+1))])  (lifting_dwt_nets.py:728-732)."""
    lib = _lib.load()
    P, B, _, H, W = x.shape
    dev = x.device
    ll = torch.empty(P, B, 1, H >> levels, W >> levels, device=dev, dtype=torch.float32)
    yh = [torch.empty(P, B, 3, H >> (i + 1), W >> (i + 1), device=dev, dtype=torch.float32) for i in range(levels)]
    nb = lib.lldwt_lifting_ws_bytes(P * B, H, W, Cc)
    ws = workspace(nb, dev)
    ov = current_overlap()
    if ov is not None and 0 < ov.split < levels:
        # forked (eval_overlap): yh[:split] are ordered on the current stream, yh[split:] and ll on ov.tail; the workspace
        # stays with the tail until ov.join()
        fork = ov.fork.cuda_event
        if not fork or ov.tail.cuda_stream == torch.cuda.current_stream().cuda_stream:
            raise _lib.LLDWTError("lifting_forward: the overlap context has no event handle or no second stream")
        ov.lent = True          # before the call: if it fails behind the fork, leaving the context still joins the tail
        check(lib.lldwt_lifting_forward_split(_chk(x, "x"), _chk(ll), _ptr_array(yh), P, B, H, W, levels, _chk(taps, "taps"),
                                              _chk(packed, "packed"), int(packed.shape[1]), int(block_offset),
                                              int(bool(different)), Cc, K, float(res_weight), int(bool(linear)),
                                              _opt(scale_nh), _opt(scale_nl), C.c_void_p(ws.data_ptr()), nb, ov.split,
                                              _stream(), C.c_void_p(ov.tail.cuda_stream), C.c_void_p(fork)),
              "lifting_forward_split")
        return ll, yh
    check(lib.lldwt_lifting_forward(_chk(x, "x"), _chk(ll), _ptr_array(yh), P, B, H, W, levels, _chk(taps, "taps"),
                                    _chk(packed, "packed"), int(packed.shape[1]), int(block_offset),
                                    int(bool(different)), Cc, K, float(res_weight), int(bool(linear)), _opt(scale_nh),
                                    _opt(scale_nl), C.c_void_p(ws.data_ptr()), nb, _stream()), "lifting_forward")
    return ll, yh


def lifting_inverse(ll, yh, taps, packed, Cc, K, res_weight, linear=False, scale_nh=None, scale_nl=None,
                    block_offset=0):
    lib = _lib.load()
    levels = len(yh)
    P, B, _, hl, wl = ll.shape
    H, W = hl << levels, wl << levels
    dev = ll.device
    x = torch.empty(P, B, 1, H, W, device=dev, dtype=torch.float32)
    for t in yh:
        _chk(t, "yh")
    nb = lib.lldwt_lifting_ws_bytes(P * B, H, W, Cc)
    ws = workspace(nb, dev)
    check(lib.lldwt_lifting_inverse(_chk(ll, "ll"), _ptr_array(yh), _chk(x), P, B, H, W, levels, _chk(taps, "taps"),
                                    _chk(packed, "packed"), int(packed.shape[1]), int(block_offset), Cc, K,
                                    float(res_weight), int(bool(linear)), _opt(scale_nh), _opt(scale_nl),
                                    C.c_void_p(ws.data_ptr()), nb, _stream()), "lifting_inverse")
    return x


def set_cdf97_short_levels(periodic):
    """Policy for CDF 9/7 level inputs shorter than the 10-tap filter (lldwt_set_cdf97_short_levels): False (default) =
    such a call raises LLDWTError (the reference's single-fold form and the exact periodic transform differ there),
    True = compute the periodic form (= PyWavelets)."""
    check(_lib.load().lldwt_set_cdf97_short_levels(1 if periodic else 0), "lldwt_set_cdf97_short_levels")


def cdf97_forward(x, levels, adj=False):
    """x: (Z..., H, W) as (P,B,C,H,W) -> (ll, [yh_i (P,B,C*3? no: (P,B*C,3,h,w))]).  Channels are folded into batch."""
    lib = _lib.load()
    P, B, Cc, H, W = x.shape
    Z = P * B * Cc
    dev = x.device
    ll = torch.empty(P, B, Cc, H >> levels, W >> levels, device=dev, dtype=torch.float32)
    yh = [torch.empty(P, B, Cc, 3, H >> (i + 1), W >> (i + 1), device=dev, dtype=torch.float32) for i in range(levels)]
    nb = lib.lldwt_cdf97_ws_bytes(Z, H, W)
    ws = workspace(nb, dev)
    check(lib.lldwt_cdf97_forward(_chk(x, "x"), _chk(ll), _ptr_array(yh), Z, H, W, levels, int(bool(adj)),
                                     C.c_void_p(ws.data_ptr()), nb, _stream()), "cdf97_forward")
    return ll, yh


def cdf97_inverse(ll, yh, adj=False):
    lib = _lib.load()
    levels = len(yh)
    P, B, Cc, hl, wl = ll.shape
    H, W = hl << levels, wl << levels
    Z = P * B * Cc
    x = torch.empty(P, B, Cc, H, W, device=ll.device, dtype=torch.float32)
    for t in yh:
        _chk(t, "yh")
    nb = lib.lldwt_cdf97_ws_bytes(Z, H, W)
    ws = workspace(nb, ll.device)
    check(lib.lldwt_cdf97_inverse(_chk(ll, "ll"), _ptr_array(yh), _chk(x), Z, H, W, levels, int(bool(adj)),
                                     C.c_void_p(ws.data_ptr()), nb, _stream()), "cdf97_inverse")
    return x


def subband_mlp_pack(w0, b0, w1, b1, w2, b2, w3, b3, transposed=False, hidden=32):
    """The operand pack of subband_mlp (lldwt_subband_mlp_pack): weights stacked (P,...) in Conv2d layout, or in
    ConvTranspose2d layout with transposed=True -> uint8 device tensor, valid until a weight changes."""
    lib = _lib.load()
    P, Cc = b3.shape
    nb = lib.lldwt_subband_mlp_packed_bytes(P, Cc)
    pack = torch.empty(nb, dtype=torch.uint8, device=w0.device)
    check(lib.lldwt_subband_mlp_pack(_chk(w0), _chk(b0), _chk(w1), _chk(b1), _chk(w2), _chk(b2), _chk(w3), _chk(b3), P, Cc,
                                     hidden, int(bool(transposed)), C.c_void_p(pack.data_ptr()), nb, _stream()),
          "subband_mlp_pack")
    return pack


def subband_mlp(x, w0, b0, w1, b1, w2, b2, w3, b3, transposed=False, hidden=32, pack=None):
    """SubbandAutoEncoder encode/decode (lifting_dwt_nets.py:99-110); x: (P,B,C,h,w), weights stacked (P,...).  ``pack``: the
    subband_mlp_pack of these weights when the caller keeps one (ae_planes does); built here otherwise."""
    lib = _lib.load()
    P, B, Cc, h, w = x.shape
    if pack is None:
        pack = subband_mlp_pack(w0, b0, w1, b1, w2, b2, w3, b3, transposed=transposed, hidden=hidden)
    y = torch.empty_like(x)
    check(lib.lldwt_subband_mlp(_chk(x, "x"), _chk(y), P, B, Cc, h * w, hidden, C.c_void_p(pack.data_ptr()), pack.numel(),
                                _stream()), "subband_mlp")
    return y


def subband_mlp_bwd(x, gy, w0, b0, w1, b1, w2, b2, w3, hidden=32):
    """Backward-data of the encode-layout subband MLP: -> (gx, [h0,h1,h2], [d0,d1,d2]); hidden tensors (P,B,C*hidden,h,w)."""
    P, B, Cc, h, w = x.shape
    gx = torch.empty_like(x)
    hs = [torch.empty(P, B, Cc * hidden, h, w, device=x.device, dtype=torch.float32) for _ in range(6)]
    check(_lib.load().lldwt_subband_mlp_bwd(_chk(x, "x"), _chk(gy, "gy"), _chk(gx), *[_chk(t) for t in hs], P, B, Cc, h * w,
                                            hidden, _chk(w0), _chk(b0), _chk(w1), _chk(b1), _chk(w2), _chk(b2), _chk(w3),
                                            _stream()), "subband_mlp_bwd")
    return gx, hs[:3], hs[3:]


def subband_mlp_bwd_w(x, gy, w0, b0, w1, b1, w2, b2, w3, hidden=32):
    """Backward of the encode-layout subband MLP with the parameter gradients formed in the kernel (lldwt_subband_mlp_bwd_w):
    -> (gx, [dw0, db0, dw1, db1, dw2, db2, dw3, db3]) in the shapes of the parameters."""
    lib = _lib.load()
    P, B, Cc, h, w = x.shape
    gx = torch.empty_like(x)
    shapes = [(P, Cc * hidden, 1, 1, 1), (P, Cc * hidden), (P, Cc * hidden, hidden, 1, 1), (P, Cc * hidden),
              (P, Cc * hidden, hidden, 1, 1), (P, Cc * hidden), (P, Cc, hidden, 1, 1), (P, Cc)]
    g = [torch.empty(s, device=x.device, dtype=torch.float32) for s in shapes]
    nb = lib.lldwt_subband_mlp_bwd_w_ws_bytes(P, Cc, h * w)
    ws = workspace(nb, x.device)
    check(lib.lldwt_subband_mlp_bwd_w(_chk(x, "x"), _chk(gy, "gy"), _chk(gx), P, B, Cc, h * w, hidden, _chk(w0), _chk(b0),
                                      _chk(w1), _chk(b1), _chk(w2), _chk(b2), _chk(w3), *[_chk(t) for t in g],
                                      C.c_void_p(ws.data_ptr()), nb, _stream()), "subband_mlp_bwd_w")
    return gx, g


def conv_desc(cin, cout, K, groups=1, act=ACT_NONE, upsample2=False, transposed=False, tap_mask=None, oc_block=None,
              oc_stride=0, oc_off=0, ytot=None, ic_block=0, ic_stride=0, ic_off=0, xtot=0, epi=0):
    return ConvDesc(cin, cout, K, groups, act, int(bool(upsample2)), int(bool(transposed)),
                    (1 << (K * K)) - 1 if tap_mask is None else int(tap_mask), cout if oc_block is None else oc_block,
                    oc_stride, oc_off, cout if ytot is None else ytot, ic_block, ic_stride, ic_off, xtot, epi)


def flip_mask(mask, K):
    """Tap mask of the 180-degree rotated kernel (backward-data of a masked conv)."""
    if mask is None:
        return None
    KK = K * K
    return sum(1 << (KK - 1 - t) for t in range(KK) if (mask >> t) & 1)


def conv_pack(w, K, groups=1, transposed=False, tap_mask=None, swap_hw=False):
    """(P,cout,cin/groups,K,K) -> packed (P, floats) in MFMA A-operand order.  transposed: the weight is in
    ConvTranspose2d layout (P,cin,cout/groups,K,K) (or a forward Conv2d weight used for its backward-data pass:
    then `cin` is the forward cout) and the taps are flipped; tap_mask refers to the effective (flipped) taps."""
    lib = _lib.load()
    P = w.shape[0]
    if transposed:
        cin, cout = w.shape[1], w.shape[2] * groups
    else:
        cout, cin = w.shape[1], w.shape[2] * groups
    d = conv_desc(cin, cout, K, groups, transposed=transposed, tap_mask=tap_mask)
    n = lib.lldwt_conv_packed_floats(C.byref(d))
    packed = torch.empty(P, n, device=w.device, dtype=torch.float32)
    check(lib.lldwt_conv_pack(_chk(w, "w"), _chk(packed), C.byref(d), P, int(bool(swap_hw)), _stream()), "conv_pack")
    return packed


def conv2d(x, w, bias, K, groups=1, act=ACT_NONE, upsample2=False, transposed=False, tap_mask=None, out=None,
           oc_block=None, oc_stride=0, oc_off=0, direct=False, packed=None, residual=None, aux=None, epi=0,
           ic_block=0, ic_stride=0, ic_off=0, cin=None, absmax=None):
    """General conv layer (include/lldwt.h lldwt_conv2d).  x: (P,B,xtot,h,w); w: (P,cout,cin/groups,K,K)
    (transposed: (P,cin,cout/groups,K,K)).  ``out``: optional pre-allocated (P,B,ytot,h,w) tensor for channel placement.
    ``packed``: result of conv_pack(w, ...) to skip re-packing; ``direct``: reference-order VALU kernel;
    ``absmax``: optional (P,64) fp32 tensor that receives max|y| per plane (lldwt_conv2d_absmax)."""
    lib = _lib.load()
    P, B, xtot, hi, wi = x.shape
    if transposed:
        cin_w, cout = w.shape[1], w.shape[2] * groups
    else:
        cout, cin_w = w.shape[1], w.shape[2] * groups
    cin = cin_w if cin is None else cin
    h, wd = (hi * 2, wi * 2) if upsample2 else (hi, wi)
    if out is None:
        out = torch.empty(P, B, cout, h, wd, device=x.device, dtype=torch.float32)
    d = conv_desc(cin, cout, K, groups, act, upsample2, transposed, tap_mask, oc_block, oc_stride, oc_off, out.shape[2],
                  ic_block, ic_stride, ic_off, xtot if ic_block else 0, epi)
    if not ic_block and xtot != cin:
        raise _lib.LLDWTError("conv2d: input has %d channels, weight expects %d" % (xtot, cin))
    if direct:
        assert residual is None and aux is None and not ic_block
        check(lib.lldwt_conv2d_direct(_chk(x, "x"), _chk(out, "out"), _chk(w, "w"), _opt(bias, "bias"), C.byref(d), P, B,
                                      h, wd, _stream()), "conv2d_direct")
        return out
    if packed is None:
        packed = conv_pack(w, K, groups, transposed, tap_mask)
    if absmax is not None:
        check(lib.lldwt_conv2d_absmax(_chk(x, "x"), _chk(out, "out"), _chk(packed, "packed"), _opt(bias, "bias"),
                                      _opt(residual, "residual"), _opt(aux, "aux"), _chk(absmax, "absmax"), C.byref(d), P, B,
                                      h, wd, _stream()), "conv2d_absmax")
        return out
    check(lib.lldwt_conv2d(_chk(x, "x"), _chk(out, "out"), _chk(packed, "packed"), _opt(bias, "bias"),
                           _opt(residual, "residual"), _opt(aux, "aux"), C.byref(d), P, B, h, wd, _stream()), "conv2d")
    return out


def tail_mode():
    """'fused' (default) or 'legacy' (LLDWT_TAIL=legacy, read when the library loads): the earlier launches of the small
    end-of-step work -- one launch per layer and per stack of the coarsest level's context stacks, the scalar sum kernel."""
    return "legacy" if _lib.load().lldwt_tail_legacy() else "fused"


def conv_stack_pair(xa, xb, layers, groups_a, groups_b):
    """Two independent grouped masked-conv stacks with the same per-group shapes as one grouped problem per layer
    (include/lldwt.h lldwt_conv_stack_pair).  xa: (P,B,groups_a*c,h,w), xb: (P,B,groups_b*c,h,w); layers: one
    (packed, bias, cin, cout, K, act, tap_mask) per layer of the MERGED problem (stack A's groups first).  -> (ya, yb), each
    bit-identical to conv2d run layer by layer on its stack alone."""
    lib = _lib.load()
    P, B, _, h, w = xa.shape
    if xb.shape[:2] != (P, B) or xb.shape[3:] != (h, w):
        raise _lib.LLDWTError("conv_stack_pair: inputs of different planes / batch / size")
    groups, n = groups_a + groups_b, len(layers)
    descs = (ConvDesc * n)(*[conv_desc(cin, cout, K, groups, act, tap_mask=mask) for _, _, cin, cout, K, act, mask in layers])
    if xa.shape[2] * groups != layers[0][2] * groups_a or xb.shape[2] * groups != layers[0][2] * groups_b:
        raise _lib.LLDWTError("conv_stack_pair: input channels do not match the first layer")
    packed = (C.c_void_p * n)(*[_chk(l[0], "packed").value for l in layers])
    bias = (C.c_void_p * n)(*[_opt(l[1], "bias").value for l in layers])
    cout = layers[-1][3] // groups
    ya = torch.empty(P, B, cout * groups_a, h, w, device=xa.device, dtype=torch.float32)
    yb = torch.empty(P, B, cout * groups_b, h, w, device=xa.device, dtype=torch.float32)
    mid = [l[3] for l in layers[:-1]]                      # even layers write ws0, odd layers ws1
    n0, n1 = P * B * h * w * max(mid[0::2]), P * B * h * w * max(mid[1::2] or [1])
    ws0 = torch.empty(n0, device=xa.device, dtype=torch.float32)
    ws1 = torch.empty(n1, device=xa.device, dtype=torch.float32)
    check(lib.lldwt_conv_stack_pair(_chk(xa, "xa"), _chk(xb, "xb"), _chk(ya), _chk(yb), packed, bias, descs, n, groups_a,
                                    _chk(ws0), _chk(ws1), n0, n1, P, B, h, w, _stream()), "conv_stack_pair")
    return ya, yb


def storage_dtype():
    """Storage type of the tree-context tensor between the two tree convs: 'fp32' (default, the reference's) or 'fp16'
    (BASELINE configs[4]: half the bytes, two MFMA products instead of three, 1e-2 tolerance class).  LLDWT_STORAGE."""
    return _env_choice("LLDWT_STORAGE", "fp32", ("fp32", "fp16"))


def conv2d_f16out(x, w, bias, K, oscale, act=ACT_NONE, upsample2=False, packed=None):
    """conv2d whose output is STORED as fp16 x oscale[plane] (include/lldwt.h lldwt_conv2d_f16out) -> (P,B,cout,h,w) half."""
    lib = _lib.load()
    P, B, cin, hi, wi = x.shape
    cout = w.shape[1]
    h, wd = (hi * 2, wi * 2) if upsample2 else (hi, wi)
    y = torch.empty(P, B, cout, h, wd, device=x.device, dtype=torch.float16)
    d = conv_desc(cin, cout, K, 1, act, upsample2, False, None, None, 0, 0, cout, 0, 0, 0, 0, 0)
    if packed is None:
        packed = conv_pack(w, K)
    check(lib.lldwt_conv2d_f16out(_chk(x, "x"), C.c_void_p(y.data_ptr()), _chk(packed, "packed"), _opt(bias, "bias"),
                                  _chk(oscale, "oscale"), C.byref(d), P, B, h, wd, _stream()), "conv2d_f16out")
    return y


def conv3x3_f16in(x16, packed, bias, cout, xscale, act=ACT_NONE):
    """Dense 3x3 conv reading an fp16-stored input (lldwt_conv3x3_f16in); packed = conv_f16x3_pack(w)."""
    if not (x16.is_cuda and x16.dtype == torch.float16 and x16.is_contiguous()):
        raise _lib.LLDWTError("conv3x3_f16in: x16 must be a contiguous fp16 device tensor")
    P, B, cin, h, w = x16.shape
    y = torch.empty(P, B, cout, h, w, device=x16.device, dtype=torch.float32)
    check(_lib.load().lldwt_conv3x3_f16in(C.c_void_p(x16.data_ptr()), _chk(y), C.c_void_p(packed.data_ptr()), _opt(bias, "bias"),
                                         _chk(xscale, "xscale"), cin, cout, act, P, B, h, w, _stream()), "conv3x3_f16in")
    return y


def plc_fuse():
    """Whether the eval path computes the tree-context PAIR in one launch (lldwt_plc_fused: the first conv on the fly
    inside the second's staging, no 243-channel tensor in HBM).  Only with plc_mode() == 'f16x3' and fp32 storage.
    Environment variable LLDWT_PLC_FUSE (default 1)."""
    return _env_choice("LLDWT_PLC_FUSE", "1", ("0", "1")) == "1"


def plc_fused_pack1(w1, b1):
    """(P,cmid,3,3,3), (P,cmid) fp32 -> packed split-fp16 first tree conv for plc_fused (uint8 (P, bytes))."""
    lib = _lib.load()
    P, cmid, cin, K, K2 = w1.shape
    if cin != 3 or K != 3 or K2 != 3:
        raise _lib.LLDWTError("plc_fused_pack1: a (P,cmid,3,3,3) weight")
    nb = int(lib.lldwt_plc_fused_pack1_bytes(cmid))
    if nb <= 0:
        raise _lib.LLDWTError("plc_fused_pack1: cmid must be in 1..256")
    packed = torch.empty(P, nb, device=w1.device, dtype=torch.uint8)
    check(lib.lldwt_plc_fused_pack1(_chk(w1, "w1"), _chk(b1, "b1"), C.c_void_p(packed.data_ptr()), cmid, P, _stream()),
          "plc_fused_pack1")
    return packed


def plc_fused(parent, packed1, packed2, bias2, cmid, cout, act=ACT_NONE):
    """y = act(conv3x3(LeakyReLU(conv3x3(up2(parent)) + b1)) + b2) in one launch (include/lldwt.h lldwt_plc_fused)."""
    P, B, cin, hp, wp = parent.shape
    if cin != 3:
        raise _lib.LLDWTError("plc_fused: the parent has 3 channels")
    y = torch.empty(P, B, cout, 2 * hp, 2 * wp, device=parent.device, dtype=torch.float32)
    check(_lib.load().lldwt_plc_fused(_chk(parent, "parent"), _chk(y), C.c_void_p(packed1.data_ptr()),
                                     C.c_void_p(packed2.data_ptr()), _opt(bias2, "bias2"), cmid, cout, act, P, B,
                                     2 * hp, 2 * wp, _stream()), "plc_fused")
    return y


def cgp_mode():
    """Arithmetic of the fused cgp stack on the eval path: 'f16x3' (default; split-fp16 register chain, csrc/cgp_f16x3.hip)
    or 'f32' (fp32 MFMA kernel k_cgp_rate).  Environment variable LLDWT_CGP_MODE."""
    return _env_choice("LLDWT_CGP_MODE", "f16x3", ("f32", "f16x3"))


# The split chain takes every hidden layer's operand scale from a bound (bound_l = bound_{l-1} * max row L1 norm + max |bias|) and
# fp16 keeps the full 22-bit split over 18 binades below it.  The bounds compound from layer to layer, so an even network (rows of
# similar L1 norm) already sits well below them and has about 6 of the 18 binades to spare at layer 3; a unit (or bias) far louder
# than its layer's typical row pushes the bound up and every other unit down by as much, and spends them.  Measured on MI355X
# (DESIGN.md 2.3): every form holds the fp32 bars up to 6.8 binades of this measure and leaves them from 7.6; the limit keeps two
# binades of margin.
CGP16_HEADROOM_LIMIT = 4.8


def cgp16_headroom(ws, bs, groups):
    """Binades of the chain's range that the bounds of layers 0 .. 2 spend beyond an even network: the largest over (plane, group)
    of sum_l log2(max(max row L1 norm, max |bias|) / median row L1 norm).  ws, bs as cgp16_pack takes them.  An fp32 reduction
    on the tensors' device and one host read (a stream synchronisation: not capturable in a HIP graph)."""
    tot = None
    for l in range(3):
        w = ws[l].detach()
        P = w.shape[0]
        rows = w.abs().reshape(P, groups, w.shape[1] // groups, -1).sum(dim=3).double()
        top = rows.amax(dim=2)
        top = torch.maximum(top, bs[l].detach().abs().reshape(P, groups, -1).amax(dim=2).double())
        t = torch.log2(top / rows.median(dim=2).values)
        t = torch.where(top > 0, t, torch.zeros_like(t)).clamp_min(0.0)          # an all-zero layer spends nothing
        tot = t if tot is None else tot + t
    return float(tot.max())


def cgp16_supported(ws, groups, bs):
    """Whether the split-fp16 register chain serves this stack: the reference's widths, and weights AND biases inside what its
    bound-derived scales represent (cgp16_headroom <= CGP16_HEADROOM_LIMIT).  Otherwise the callers take the fp32 kernels.
    The two paths give different bits and the coder follows this answer, so the answer is part of what encoder and decoder must
    share: the measure is an fp32 sum in the device's order, and weights within rounding of the limit (the two binades of margin
    lie below it, not around it) could be judged differently by another build or device -- as with every other kernel of the coder,
    a stream is decoded by the build that wrote it.  In training the answer is taken anew at every call and can change from one
    step to the next while the weights sit near the limit; either path meets the fp32 bars there."""
    c = [ws[0].shape[2]] + [w.shape[1] // groups for w in ws]
    if not (_lib.load().lldwt_cgp16_packed_bytes(c[0], c[1], c[2], c[3], groups) > 0 and c[4] == 2):
        return False
    return cgp16_headroom(ws, bs, groups) <= CGP16_HEADROOM_LIMIT


def cgp16_pack(ws, bs, groups):
    """The four (folded) 1x1 weights (P, groups*c_{l+1}, c_l, 1, 1) + biases -> packed split-fp16 fragments (uint8 (P, bytes))."""
    lib = _lib.load()
    P = ws[0].shape[0]
    c = [ws[0].shape[2]] + [w.shape[1] // groups for w in ws]
    nb = int(lib.lldwt_cgp16_packed_bytes(c[0], c[1], c[2], c[3], groups))
    if nb <= 0:
        raise _lib.LLDWTError("cgp16_pack: dimensions %s not built (93 -> 162 -> 54 -> 18 -> 2 only)" % (c,))
    packed = torch.empty(P, nb, device=ws[0].device, dtype=torch.uint8)
    args = []
    for w, b in zip(ws, bs):
        args += [_chk(w, "w"), _chk(b, "b")]
    check(lib.lldwt_cgp16_pack(*args, C.c_void_p(packed.data_ptr()), P, c[0], c[1], c[2], c[3], groups, _stream()), "cgp16_pack")
    return packed


def cgp16_params(plc, xq, packed16, K, tap_mask):
    """(sigma, mu) of every coefficient from the tree-context features plc (P,B,G*81,h,w) and the quantised subbands xq
    (P,B,G,h,w): -> params (P,B,2G,h,w) (include/lldwt.h lldwt_cgp16_params)."""
    P, B, G, h, w = xq.shape
    params = torch.empty(P, B, 2 * G, h, w, device=xq.device, dtype=torch.float32)
    check(_lib.load().lldwt_cgp16_params(_chk(plc, "plc"), _chk(xq, "xq"), C.c_void_p(packed16.data_ptr()), _chk(params), P, B,
                                        h, w, G, K, int(tap_mask), _stream()), "cgp16_params")
    return params


def cgp16_params_train(plc, xq, packed16, K, tap_mask):
    """Training forward of the cgp stack on the split-fp16 register chain (lldwt_cgp16_params_train):
    -> (params (P,B,2G,h,w), h1 (P,B,G*162,h,w), h2 (P,B,G*54,h,w), h3 (P,B,G*18,h,w))."""
    P, B, G, h, w = xq.shape
    params = torch.empty(P, B, 2 * G, h, w, device=xq.device, dtype=torch.float32)
    hs = [torch.empty(P, B, G * c, h, w, device=xq.device, dtype=torch.float32) for c in (162, 54, 18)]
    check(_lib.load().lldwt_cgp16_params_train(_chk(plc, "plc"), _chk(xq, "xq"), C.c_void_p(packed16.data_ptr()), _chk(params),
                                              _chk(hs[0]), _chk(hs[1]), _chk(hs[2]), P, B, h, w, G, K, int(tap_mask), _stream()),
          "cgp16_params_train")
    return params, hs[0], hs[1], hs[2]


def cgp16_pack_bwd(ws, groups):
    """The four forward 1x1 weights (P, groups*c_{l+1}, c_l, 1, 1) -> the transposed split-fp16 pack of cgp16_bwd (uint8 (P, bytes))."""
    lib = _lib.load()
    P = ws[0].shape[0]
    c = [ws[0].shape[2]] + [w.shape[1] // groups for w in ws]
    nb = int(lib.lldwt_cgp16_bwd_packed_bytes(c[0], c[1], c[2], c[3], groups))
    if nb <= 0:
        raise _lib.LLDWTError("cgp16_pack_bwd: dimensions %s not built (93 -> 162 -> 54 -> 18 -> 2 only)" % (c,))
    packed = torch.empty(P, nb, device=ws[0].device, dtype=torch.uint8)
    check(lib.lldwt_cgp16_pack_bwd(*[_chk(w, "w") for w in ws], C.c_void_p(packed.data_ptr()), P, c[0], c[1], c[2], c[3], groups,
                                   _stream()), "cgp16_pack_bwd")
    return packed


def cgp16_bwd(dparams, h1, h2, h3, packed_bwd16, groups):
    """Backward-data of the cgp stack on the split-fp16 register chain (lldwt_cgp16_bwd)
    -> (dplc (P,B,G*81,h,w), dtaps (P,B,G*12,h,w), d1, d2, d3)."""
    P, B, _, h, w = dparams.shape
    d1, d2, d3 = torch.empty_like(h1), torch.empty_like(h2), torch.empty_like(h3)
    dplc = torch.empty(P, B, groups * 81, h, w, device=dparams.device, dtype=torch.float32)
    dtaps = torch.empty(P, B, groups * 12, h, w, device=dparams.device, dtype=torch.float32)
    check(_lib.load().lldwt_cgp16_bwd(_chk(dparams), _chk(h1), _chk(h2), _chk(h3), C.c_void_p(packed_bwd16.data_ptr()), _chk(d1),
                                      _chk(d2), _chk(d3), _chk(dplc), _chk(dtaps), P, B, h * w, groups, _stream()), "cgp16_bwd")
    return dplc, dtaps, d1, d2, d3


def plc_shape():
    """MFMA shape of the split-fp16 3x3 conv kernels in this process: 32 (32x32x16, default) or 16 (LLDWT_PLC_SHAPE=16)."""
    return 16 if _lib.load().lldwt_plc_shape16() else 32


def plc_algo():
    """Algorithm of plc_fused's split-fp16 32x32x16 path in this process: 'winograd' (row-wise F(2,3), default) or 'direct'
    (LLDWT_PLC_ALGO=direct, or the 16x16x32 shape)."""
    return "winograd" if _lib.load().lldwt_plc_winograd() else "direct"


def conv_f16x3_pack(w):
    """(P,cout,cin,3,3) fp32 -> packed split-fp16 weights (uint8 tensor (P, bytes)) for conv3x3_f16x3."""
    lib = _lib.load()
    P, cout, cin, K, K2 = w.shape
    if K != 3 or K2 != 3:
        raise _lib.LLDWTError("conv_f16x3_pack: 3x3 kernels only")
    nb = int(lib.lldwt_conv_f16x3_packed_bytes(cin, cout))
    packed = torch.empty(P, nb, device=w.device, dtype=torch.uint8)
    check(lib.lldwt_conv_f16x3_pack(_chk(w, "w"), C.c_void_p(packed.data_ptr()), cin, cout, P, _stream()), "conv_f16x3_pack")
    return packed


def absmax_slots(x):
    """x (P, ...) -> slots (P,64) fp32 whose maximum per plane is max|x[p]| (device-side; feeds conv3x3_f16x3)."""
    P = x.shape[0]
    slots = torch.empty(P, 64, device=x.device, dtype=torch.float32)
    check(_lib.load().lldwt_absmax_slots(_chk(x, "x"), P, x.numel() // P, _chk(slots), _stream()), "absmax_slots")
    return slots


def conv3x3_f16x3(x, packed, bias, cout, act=ACT_NONE, slots=None):
    """Dense 3x3 conv on the fp16 matrix cores with split-fp16 operands (include/lldwt.h lldwt_conv3x3_f16x3)."""
    P, B, cin, h, w = x.shape
    if slots is None:
        slots = absmax_slots(x)
    y = torch.empty(P, B, cout, h, w, device=x.device, dtype=torch.float32)
    check(_lib.load().lldwt_conv3x3_f16x3(_chk(x, "x"), _chk(y), C.c_void_p(packed.data_ptr()), _opt(bias, "bias"),
                                         _chk(slots, "slots"), cin, cout, act, P, B, h, w, _stream()), "conv3x3_f16x3")
    return y


def conv2d_wgrad(x, dy, wshape, K, groups=1, upsample2=False, tap_mask=None, want_bias=True, oc_block=None, oc_stride=0,
                 oc_off=0, ic_block=0, ic_stride=0, ic_off=0, dw=None, db=None, alpha=1.0, swap_hw=False):
    """-> (dw (P,cout,cin/groups,K,K), dbias (P,cout) or None); dy: (P,B,ytot,h,w) read through the output placement."""
    lib = _lib.load()
    P, B, ytot, h, wd = dy.shape
    cout, cin = wshape[1], wshape[2] * groups
    if dw is None:
        dw = torch.zeros(wshape, device=x.device, dtype=torch.float32)
    if db is None and want_bias:
        db = torch.zeros(P, cout, device=x.device, dtype=torch.float32)
    d = conv_desc(cin, cout, K, groups, 0, upsample2, False, tap_mask, oc_block, oc_stride, oc_off, ytot, ic_block,
                  ic_stride, ic_off, x.shape[2] if ic_block else 0, 0)
    check(lib.lldwt_conv2d_wgrad(_chk(x, "x"), _chk(dy, "dy"), _chk(dw), _opt(db), C.byref(d), P, B, h, wd,
                                    float(alpha), int(bool(swap_hw)), _stream()), "conv2d_wgrad")
    return dw, db


def wgrad16_f16x3(x, dy, dw=None, db=None, alpha=1.0, swap_hw=False):
    """Backward-weights of a 16 -> 16 5x5 conv whose input is bounded by 1 (tanh outputs) on the fp16 matrix cores, split-fp16
    operands (lldwt_wgrad16_f16x3).  x, dy (P,B,16,h,w) -> (dw (P,16,16,5,5), db (P,16)), accumulated into dw / db if given."""
    P, B, Cc, h, wd = x.shape
    if Cc != 16 or dy.shape != x.shape:
        raise _lib.LLDWTError("wgrad16_f16x3: shapes %r %r" % (tuple(x.shape), tuple(dy.shape)))
    if dw is None:
        dw = torch.zeros(P, 16, 16, 5, 5, device=x.device, dtype=torch.float32)
    if db is None:
        db = torch.zeros(P, 16, device=x.device, dtype=torch.float32)
    slots = workspace(P * 64 * 4, x.device)
    check(_lib.load().lldwt_wgrad16_f16x3(_chk(x, "x"), _chk(dy, "dy"), _chk(dw), _chk(db), C.c_void_p(slots.data_ptr()), P, B, h, wd,
                                          float(alpha), int(bool(swap_hw)), _stream()), "wgrad16_f16x3")
    return dw, db


def conv3x3_wgrad_f16x3(x, dy, wshape, want_bias=True, alpha=1.0, x_slots=None, dy_slots=None):
    """Backward-weights of a dense 3x3 conv on the fp16 matrix cores, split-fp16 operands (lldwt_conv3x3_wgrad_f16x3).
    x (P,B,cin,h,w), dy (P,B,cout,h,w) -> (dw (P,cout,cin,3,3), dbias (P,cout) or None).  x_slots / dy_slots: the (P,64)
    |max| slots of x / dy (absmax_slots) if the caller has them already -- that pass is then skipped."""
    P, B, cin, h, wd = x.shape
    cout = dy.shape[2]
    if tuple(wshape) != (P, cout, cin, 3, 3) or dy.shape != (P, B, cout, h, wd):
        raise _lib.LLDWTError("conv3x3_wgrad_f16x3: shapes %r %r %r" % (tuple(x.shape), tuple(dy.shape), tuple(wshape)))
    dw = torch.zeros(wshape, device=x.device, dtype=torch.float32)
    db = torch.zeros(P, cout, device=x.device, dtype=torch.float32) if want_bias else None
    slots = torch.empty(P * 128, device=x.device, dtype=torch.float32) if x_slots is None or dy_slots is None else None
    for nm, t in (("x_slots", x_slots), ("dy_slots", dy_slots)):
        if t is not None and (t.numel() != P * 64 or t.dtype != torch.float32):
            raise _lib.LLDWTError("conv3x3_wgrad_f16x3: %s must hold (P, 64) floats" % nm)
    check(_lib.load().lldwt_conv3x3_wgrad_f16x3(_chk(x, "x"), _chk(dy, "dy"), _chk(dw), _opt(db), _opt(slots), _opt(x_slots, "x_slots"),
                                                  _opt(dy_slots, "dy_slots"), cin, cout, P, B, h, wd, float(alpha), _stream()),
          "conv3x3_wgrad_f16x3")
    return dw, db


def act_bwd(dy, y, act):
    dx = torch.empty_like(dy)
    check(_lib.load().lldwt_act_bwd(_chk(dy), _chk(y), _chk(dx), dy.numel(), act, _stream()), "act_bwd")
    return dx


def downsum2(g):
    P, B, Cc, h, w = g.shape
    out = torch.empty(P, B, Cc, h // 2, w // 2, device=g.device, dtype=torch.float32)
    check(_lib.load().lldwt_downsum2(_chk(g), _chk(out), P * B * Cc, h, w, _stream()), "downsum2")
    return out


def gdn(x, beta, gamma, inverse=False, beta_min=1e-6):
    lib = _lib.load()
    P, B, Cc, h, w = x.shape
    y = torch.empty_like(x)
    check(lib.lldwt_gdn(_chk(x, "x"), _chk(y), _chk(beta), _chk(gamma), P, B, Cc, h * w, int(bool(inverse)),
                        float(beta_min), _stream()), "gdn")
    return y


def lower_bound_fwd(x, bound):
    y = torch.empty_like(x)
    check(_lib.load().lldwt_lower_bound_fwd(_chk(x), _chk(y), x.numel(), float(bound), _stream()), "lower_bound_fwd")
    return y


def lower_bound_bwd(x, gy, bound):
    gx = torch.empty_like(x)
    check(_lib.load().lldwt_lower_bound_bwd(_chk(x), _chk(gy), _chk(gx), x.numel(), float(bound), _stream()),
          "lower_bound_bwd")
    return gx


def nonneg_param_fwd(x, minimum):
    y = torch.empty_like(x)
    check(_lib.load().lldwt_nonneg_param_fwd(_chk(x), _chk(y), x.numel(), float(minimum), _stream()), "nonneg_param_fwd")
    return y


def nonneg_param_bwd(x, gy, minimum):
    gx = torch.empty_like(x)
    check(_lib.load().lldwt_nonneg_param_bwd(_chk(x), _chk(gy), _chk(gx), x.numel(), float(minimum), _stream()),
          "nonneg_param_bwd")
    return gx


def quantize(x, noise=None):
    q = torch.empty_like(x)
    check(_lib.load().lldwt_quantize(_chk(x), _opt(noise), _chk(q), x.numel(), _stream()), "quantize")
    return q


def gauss_rate(x, params, noise=None, want_q=False, bit_sum=None):
    """x: (P,B,C,h,w); params: (P,B,2C,h,w) (sigma even, mu odd channels) -> (bits, q or None)."""
    P, B, Cc, h, w = x.shape
    assert params.shape == (P, B, 2 * Cc, h, w)
    bits = torch.empty_like(x)
    q = torch.empty_like(x) if want_q else None
    bs = C.c_void_p(0) if bit_sum is None else C.c_void_p(bit_sum.data_ptr())
    check(_lib.load().lldwt_gauss_rate(_chk(x), _chk(params), _opt(noise), _chk(bits), _opt(q), bs, P * B, Cc, h * w,
                                       _stream()), "gauss_rate")
    return bits, q


def ztblock_pack(ws):
    """Pack the phase nets of DWTConditioned2EntropyLayerZTBlock for lldwt_ztblock_phase.  ws: the 10 tensors w1, b1, ..., w5,
    b5 of the 5-layer net, each with leading dims (P, 3, 2) = (plane, subband, head 0 sigma / 1 mu): w1 (.., 32, k, 3, 3),
    w2 (.., 32, 32, 3, 3), w3 / w4 (.., 32, 32, 1, 1), w5 (.., 1, 32, 1, 1), biases (.., 32) / (.., 1).
    -> flat fp32 device tensor of P*3*2 records (csrc/ztblock.hip): MFMA B fragments of conv2 and the two 32 -> 32 1x1 layers
    (lane l of k-step s holds W[16 nb + (l & 15)][4 s + (l >> 4)], K ordered tap-major / channel-minor), conv1 as rows
    ci*9 + tap, then the biases and the last layer."""
    w1, b1, w2, b2, w3, b3, w4, b4, w5, b5 = [t.detach().float() for t in ws]
    lead = w1.shape[:3]
    if lead[1:] != (3, 2) or w1.shape[3:] not in [(32, k, 3, 3) for k in range(1, 5)] or w2.shape[3:] != (32, 32, 3, 3) or \
            w3.shape[3:] != (32, 32, 1, 1) or w4.shape[3:] != (32, 32, 1, 1) or w5.shape[3:] != (1, 32, 1, 1):
        raise _lib.LLDWTError("ztblock_pack: expected the (P,3,2)-stacked 3x3 k->32, 3x3 32->32, 1x1 32->32 x2, 1x1 32->1 "
                              "nets (got %s)" % [tuple(t.shape) for t in ws])
    R = int(lead[0]) * 6
    k = w1.shape[4]

    def frag(wk, nks):                                   # (R, K, 32) [k][n] -> (R, nks, 2, 64)
        return wk.reshape(R, nks, 4, 2, 16).permute(0, 1, 3, 2, 4).reshape(R, nks * 128)
    w1r = torch.zeros(R, 36, 32, device=w1.device)
    w1r[:, :9 * k] = w1.reshape(R, 32, k, 3, 3).permute(0, 2, 3, 4, 1).reshape(R, 9 * k, 32)
    parts = [frag(w2.reshape(R, 32, 32, 3, 3).permute(0, 3, 4, 2, 1).reshape(R, 288, 32), 72),
             frag(w3.reshape(R, 32, 32).transpose(1, 2), 8), frag(w4.reshape(R, 32, 32).transpose(1, 2), 8),
             w1r.reshape(R, 36 * 32), b1.reshape(R, 32), b2.reshape(R, 32), b3.reshape(R, 32), b4.reshape(R, 32),
             w5.reshape(R, 32), torch.nn.functional.pad(b5.reshape(R, 1), (0, 31))]
    packed = torch.cat(parts, 1).contiguous()
    assert packed.shape[1] == _lib.load().lldwt_ztblock_packed_floats()
    return packed.reshape(-1)


def ztblock_phase(parent, level, packed, k, out=None):
    """(sigma, mu) of polyphase phase k (1 ee, 2 eo, 3 oe, 4 oo) of a ZTBlock level: parent (P,B,3,h2,w2) decoded coarser
    level, level (P,B,3,2h2,2w2) the finer level (phases < k decoded; unused for k == 1), packed = ztblock_pack of the phase-k
    nets.  -> params (P,B,6,h2,w2): sigma of subband j on channel 2j, mu on 2j+1."""
    P, B, G, h2, w2 = parent.shape
    H, W = (level.shape[3], level.shape[4]) if level is not None else (2 * h2, 2 * w2)
    if G != 3 or (level is not None and tuple(level.shape[:3]) != (P, B, 3)):
        raise _lib.LLDWTError("ztblock_phase: parent / level must be (P,B,3,.,.) (got %s, %s)" % (
            tuple(parent.shape), None if level is None else tuple(level.shape)))
    if packed.numel() != P * 6 * _lib.load().lldwt_ztblock_packed_floats():
        raise _lib.LLDWTError("ztblock_phase: packed holds %d floats, %d planes need %d" % (
            packed.numel(), P, P * 6 * _lib.load().lldwt_ztblock_packed_floats()))
    params = torch.empty(P, B, 6, h2, w2, device=parent.device, dtype=torch.float32) if out is None else out
    check(_lib.load().lldwt_ztblock_phase(_chk(parent, "parent"), _opt(level, "level"), _chk(packed, "packed"),
                                          _chk(params, "params"), P, B, h2, w2, H, W, int(k), _stream()), "ztblock_phase")
    return params


STEP_DENOM = 16                      # a quantisation step is n / STEP_DENOM with an integer n in [STEP_N_MIN, STEP_N_MAX]
STEP_N_MIN, STEP_N_MAX = 4, 1024
COST_ONE_BIT = 1 << 16               # lldwt_code_cost counts in units of 2^-16 bit
COST_ESCAPE = 32 * COST_ONE_BIT      # the fixed cost of a symbol outside its table


def step_pair(step):
    """A quantisation step -> (q, inv_q) as Python floats holding fp32 values: q = n / 16 with an integer n
    in [4, 1024] (exact in fp32) and inv_q = fp32(1 / q), formed here once.  ValueError naming step otherwise."""
    try:
        q = float(step)
    except (TypeError, ValueError):
        raise ValueError("step must be a number n / 16 with an integer n in [%d, %d] (got %r)"
                         % (STEP_N_MIN, STEP_N_MAX, step)) from None
    n = q * STEP_DENOM
    if not (n == n and STEP_N_MIN <= n <= STEP_N_MAX and n == int(n)):
        raise ValueError("step must be n / 16 with an integer n in [%d, %d], i.e. a multiple of 0.0625 in [0.25, 64] (got %r)"
                         % (STEP_N_MIN, STEP_N_MAX, step))
    return q, float(torch.tensor(1.0 / q, dtype=torch.float32))


class StepMap(collections.namedtuple("StepMap", "pairs shift")):
    """A step map as a level sees it: pairs (units, mh, mw, 2) fp32 device tensor of step_map_pairs, one map
    per unit (image or tile), and shift: position (y, x) of the level takes the pair at (y >> shift, x >> shift).  The coding
    functions take one wherever they take a step."""
    __slots__ = ()


def step_map_pairs(n_u16, device=None):
    """The integer step map n (any shape, integers in [4, 1024]; step = n / 16) -> a float32 tensor of that shape + (2,) holding
    (q, inv_q) per entry, by the rule of step_pair: q = n / 16 (exact) and inv_q = fp32(1 / q), the division in float64 on the
    host.  The ONE place where the pairs of a map are formed: the kernels cannot check device data, and encoder and decoder
    must use the same pairs.  ValueError naming step_map for any other value."""
    import numpy as np
    n = n_u16.cpu().numpy() if isinstance(n_u16, torch.Tensor) else np.asarray(n_u16)
    if n.dtype.kind not in "iu":
        raise ValueError("step_map: the map holds integers n with step = n / %d (got dtype %s)" % (STEP_DENOM, n.dtype))
    n = n.astype(np.int64)
    if n.size == 0 or int(n.min()) < STEP_N_MIN or int(n.max()) > STEP_N_MAX:
        raise ValueError("step_map: every entry must be an integer n in [%d, %d] (step = n / %d)" % (STEP_N_MIN, STEP_N_MAX, STEP_DENOM))
    q = n.astype(np.float64) / STEP_DENOM
    pairs = np.stack((q.astype(np.float32), (1.0 / q).astype(np.float32)), -1)
    t = torch.from_numpy(np.ascontiguousarray(pairs))
    return t if device is None else t.to(device)


def _map_args(step, units, h, w):
    """The (qpairs, mh, mw, shift) arguments of the map entry points from a StepMap, checked against the units and the h x w level
    it is to cover (the entry points check the cover again)."""
    pairs, shift = step
    if not (isinstance(pairs, torch.Tensor) and pairs.is_cuda and pairs.dtype == torch.float32 and pairs.is_contiguous()
            and pairs.dim() == 4 and pairs.shape[0] == units and pairs.shape[3] == 2):
        raise _lib.LLDWTError("step map: the pairs must be a contiguous (%d, mh, mw, 2) float32 device tensor (ops.step_map_pairs)"
                              % units)
    shift = int(shift)
    if shift < 0 or (pairs.shape[1] << shift) < h or (pairs.shape[2] << shift) < w:
        raise _lib.LLDWTError("step map: %d x %d blocks at shift %d do not cover the %d x %d level"
                              % (pairs.shape[1], pairs.shape[2], shift, h, w))
    return C.c_void_p(pairs.data_ptr()), pairs.shape[1], pairs.shape[2], shift


RDO_DENOM = 64                       # a Lagrangian of rate-distortion optimised quantisation is m / RDO_DENOM, m in [1, RDO_M_MAX]
RDO_M_MAX = 256


def rdo_scale(rdo):
    """The Lagrangian rho of rate-distortion optimised quantisation, in units of q^2 per bit -> k, the Python
    float holding fp32(rho) * 2^-16 that the kernels multiply a code-length difference (units of 2^-16 bit) with.  rho = m / 64
    with an integer m in [1, 256] (exact in fp32, and so is k).  ValueError naming rdo otherwise."""
    try:
        rho = float(rdo)
    except (TypeError, ValueError):
        raise ValueError("rdo must be a number m / %d with an integer m in [1, %d] (got %r)" % (RDO_DENOM, RDO_M_MAX, rdo)) from None
    m = rho * RDO_DENOM
    if not (m == m and 1 <= m <= RDO_M_MAX and m == int(m)):
        raise ValueError("rdo must be m / %d with an integer m in [1, %d], i.e. a multiple of %g in [%g, %g] (got %r)"
                         % (RDO_DENOM, RDO_M_MAX, 1 / RDO_DENOM, 1 / RDO_DENOM, RDO_M_MAX / RDO_DENOM, rdo))
    return rho / COST_ONE_BIT


def rdo_choose(v, s0, cost0, cost1, k):
    """The decision of DESIGN.md 7.1.7 in fp32 tensor ops (any device).  v: the rounded product (y - mu) * inv_q, s0 = round(v)
    (float), cost0 / cost1: int32 code lengths of s0 and of s1 = s0 - sign(s0) in units of 2^-16 bit -> the chosen symbol
    (float): s1 where (float)(cost0 - cost1) * k > 1 + 2 sign(s0) (v - s0), s0 elsewhere and wherever s0 == 0."""
    g = torch.sign(s0)
    t = 1.0 + 2.0 * g * (v - s0)                                   # v - s0 and 2 g r are exact
    move = ((cost0 - cost1).float() * torch.tensor(k, dtype=torch.float32, device=v.device) > t) & (s0 != 0)
    return torch.where(move, s0 - g, s0)


def rdo_lookup(cost, sizes, offsets, idx, sym):
    """cost[idx][sym - offsets[idx]] as lldwt_code_cost looks it up (COST_ESCAPE outside the table); int tensors of one device,
    cost (T, width), idx / sym of one shape -> int32."""
    T, width = cost.shape
    idx = idx.long()
    ok = (idx >= 0) & (idx < T)
    ti = torch.where(ok, idx, torch.zeros_like(idx))
    v = sym.long() - offsets.long()[ti]
    ok &= (v >= 0) & (v < sizes.long()[ti] - 2) & (v < width)
    got = cost[ti, torch.where(ok, v, torch.zeros_like(v))]
    return torch.where(ok, got, torch.full_like(got, COST_ESCAPE)).int()


def gauss_quantise(params, table63, level, r0, c0, stride, step, y=None, sym=None, rdo=None):
    """The Gaussian quantiser with a step on a whole grid in one launch (lldwt_gauss_quantise).  params (P,B,2C,h,w): sigma on
    the even, mu on the odd channels; level (P,B,C,H,W): the positions (r0 + stride i, c0 + stride j) receive symbol * q + mu,
    the others are left alone.  Encoder: y (P,B,C,H,W) coefficients read at the same positions (may be level) -> (idx, sym),
    (P,B,C,h,w) int32.  Decoder: sym (P,B,C,h,w) int32 -> (idx, sym).  Neither (level None too): -> (idx, None), what the
    decoder needs before it can pop the symbols.  table63: the scale table's first 63 entries.
    rdo: encoder only, (k, cost, sizes, offsets) -- k of rdo_scale and the int32 device tensors of cost_table /
    entropy_coding.device_cost_tables: the symbols are chosen by the rule of DESIGN.md 7.1.7 (lldwt_gauss_quantise_rdo).
    step: a number, or a StepMap over the level (one map per image b of B): every position then takes the pair
    of its block, in all three modes and with rdo (lldwt_gauss_quantise_map)."""
    P, B, C2, h, w = params.shape
    Cc = C2 // 2
    smap = step if isinstance(step, StepMap) else None
    q, inv_q = (1.0, 1.0) if smap is not None else step_pair(step)
    if rdo is not None and y is None:
        raise _lib.LLDWTError("gauss_quantise: rdo is a choice of the encoder (give y)")
    if (y is not None and sym is not None) or (level is None) != (y is None and sym is None):
        raise _lib.LLDWTError("gauss_quantise: give y (encoder) or sym (decoder) with level, or none of the three")
    if C2 != 2 * Cc or (level is not None and (level.dim() != 5 or tuple(level.shape[:3]) != (P, B, Cc))) or \
            (y is not None and y.shape != level.shape):
        raise _lib.LLDWTError("gauss_quantise: params %s, level %s, y %s do not belong together" % (
            tuple(params.shape), None if level is None else tuple(level.shape), None if y is None else tuple(y.shape)))
    if table63.numel() != 63:
        raise _lib.LLDWTError("gauss_quantise: the table must hold 63 entries (got %d)" % table63.numel())
    if sym is not None and not (sym.is_cuda and sym.dtype == torch.int32 and sym.is_contiguous() and sym.numel() == P * B * Cc * h * w):
        raise _lib.LLDWTError("gauss_quantise: sym must be a contiguous int32 device tensor of %d values" % (P * B * Cc * h * w))
    H, W = (level.shape[3], level.shape[4]) if level is not None else (r0 + stride * (h - 1) + 1, c0 + stride * (w - 1) + 1)
    idx = torch.empty(P, B, Cc, h, w, device=params.device, dtype=torch.int32)
    out = torch.empty_like(idx) if y is not None else None
    p = lambda t: C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())
    if rdo is not None:
        k, cost, sizes, offsets = rdo
        for t in (cost, sizes, offsets):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
                raise _lib.LLDWTError("gauss_quantise: the rdo tables must be contiguous int32 device tensors")
        if cost.dim() != 2 or sizes.numel() != cost.shape[0] or offsets.numel() != cost.shape[0]:
            raise _lib.LLDWTError("gauss_quantise: rdo needs cost (T, width) with T sizes and offsets")
    if smap is not None:
        ra = (p(cost), p(sizes), p(offsets), cost.shape[0], cost.shape[1], float(k)) if rdo is not None else (None, None, None, 0, 0, 0.0)
        check(_lib.load().lldwt_gauss_quantise_map(_chk(params, "params"), _opt(y, "y"), p(sym), _chk(table63, "table63"), p(idx), p(out),
                                                   _opt(level, "level"), P * B, B, Cc, h, w, H, W, int(r0), int(c0), int(stride),
                                                   *_map_args(smap, B, H, W), *ra, _stream()), "gauss_quantise_map")
        return idx, (out if y is not None else None if sym is None else sym.reshape(P, B, Cc, h, w))
    if rdo is not None:
        check(_lib.load().lldwt_gauss_quantise_rdo(_chk(params, "params"), _chk(y, "y"), _chk(table63, "table63"), p(idx), p(out),
                                                   _chk(level, "level"), P * B, Cc, h, w, H, W, int(r0), int(c0), int(stride), q,
                                                   inv_q, p(cost), p(sizes), p(offsets), cost.shape[0], cost.shape[1], float(k),
                                                   _stream()), "gauss_quantise_rdo")
        return idx, out
    check(_lib.load().lldwt_gauss_quantise(_chk(params, "params"), _opt(y, "y"), p(sym), _chk(table63, "table63"), p(idx), p(out),
                                           _opt(level, "level"), P * B, Cc, h, w, H, W, int(r0), int(c0), int(stride), q, inv_q,
                                           _stream()), "gauss_quantise")
    return idx, (out if y is not None else None if sym is None else sym.reshape(P, B, Cc, h, w))


LAYER_DIVISOR = 3                    # a quality layer divides the step by 3: a mid-tread bin splits exactly into three (7.1.10)


def layer_pair(n, j):
    """The step of quality layer j over a base of step n / 16 (j = 0: the base) -> (q_j, inv_q_j) as Python
    floats holding fp32 values: q_j = fp32(n / (16 * 3^j)), the division in float64, and inv_q_j = fp32(1 / q_j) with the
    division in float64 on the rounded q_j.  The ONE place where the pairs are formed; j = 0 gives step_pair(n / 16).  How many
    layers a step may carry is the codec's rule (n / 3^m >= 1), not checked here."""
    import numpy as np
    n, j = int(n), int(j)
    if not (STEP_N_MIN <= n <= STEP_N_MAX and 0 <= j <= 8):
        raise ValueError("layers: layer %d over the step %d / %d is not defined (n in [%d, %d], j in [0, 8])"
                         % (j, n, STEP_DENOM, STEP_N_MIN, STEP_N_MAX))
    q = np.float32(float(n) / float(STEP_DENOM * LAYER_DIVISOR ** j))
    return float(q), float(np.float32(1.0 / float(q)))


def _layer_level(who, v, params, table63):
    if v.dim() != 5 or params.dim() != 5 or tuple(params.shape) != (v.shape[0], v.shape[1], 2 * v.shape[2], v.shape[3], v.shape[4]):
        raise _lib.LLDWTError("%s: level %s and params %s do not belong together" % (who, tuple(v.shape), tuple(params.shape)))
    if table63.numel() != 63:
        raise _lib.LLDWTError("%s: the table must hold 63 entries (got %d)" % (who, table63.numel()))
    P, B, G, h, w = v.shape
    return P * B, G, h, w


def _i32(t, shape, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == shape.numel()):
        raise _lib.LLDWTError("%s must be a contiguous int32 device tensor of %d values" % (name, shape.numel()))
    return C.c_void_p(t.data_ptr())


def layer_encode(y, v_prev, params, table63, prev, cur, K):
    """The encoder of a quality layer on a level (lldwt_layer_encode).  y, v_prev (P,B,G,h,w): the
    coefficients and the level at the previous step; params (P,B,2G,h,w); prev, cur: the pairs of layer_pair for the previous
    and this layer -> (sym, row, v): the coded symbols and table rows (P,B,G,h,w) int32 and the level at this layer's step."""
    Z, G, h, w = _layer_level("layer_encode", v_prev, params, table63)
    if y.shape != v_prev.shape:
        raise _lib.LLDWTError("layer_encode: y %s and the level %s differ in shape" % (tuple(y.shape), tuple(v_prev.shape)))
    sym = torch.empty(v_prev.shape, device=v_prev.device, dtype=torch.int32)
    row = torch.empty_like(sym)
    v = torch.empty_like(v_prev)
    p = lambda t: C.c_void_p(t.data_ptr())
    check(_lib.load().lldwt_layer_encode(_chk(y, "y"), _chk(v_prev, "v_prev"), _chk(params, "params"), _chk(table63, "table63"),
                                         p(sym), p(row), p(v), Z, G, h, w, prev[0], prev[1], cur[0], cur[1], int(K), _stream()),
          "layer_encode")
    return sym, row, v


def layer_rows(v_prev, params, table63, prev, K):
    """The decoder's half before the symbols are popped (lldwt_layer_rows): -> (row, sign), (P,B,G,h,w) int32."""
    Z, G, h, w = _layer_level("layer_rows", v_prev, params, table63)
    row = torch.empty(v_prev.shape, device=v_prev.device, dtype=torch.int32)
    sign = torch.empty_like(row)
    check(_lib.load().lldwt_layer_rows(_chk(v_prev, "v_prev"), _chk(params, "params"), _chk(table63, "table63"),
                                       C.c_void_p(row.data_ptr()), C.c_void_p(sign.data_ptr()), Z, G, h, w, prev[0], prev[1], int(K),
                                       _stream()), "layer_rows")
    return row, sign


def layer_apply(v_prev, sym, sign, cur, out=None):
    """The decoder's half after (lldwt_layer_apply): v_prev (P,B,G,h,w), sym the popped symbols and sign of layer_rows (int32, as
    many values) -> v = v_prev + sign * sym * q (out: where to write it, v_prev itself allowed)."""
    if v_prev.dim() != 5:
        raise _lib.LLDWTError("layer_apply: the level must be (P,B,G,h,w) (got %s)" % (tuple(v_prev.shape),))
    P, B, G, h, w = v_prev.shape
    v = torch.empty_like(v_prev) if out is None else out
    if v.shape != v_prev.shape:
        raise _lib.LLDWTError("layer_apply: out %s and the level %s differ in shape" % (tuple(v.shape), tuple(v_prev.shape)))
    check(_lib.load().lldwt_layer_apply(_chk(v_prev, "v_prev"), _i32(sym, v_prev.shape, "layer_apply: sym"),
                                        _i32(sign, v_prev.shape, "layer_apply: sign"), _chk(v, "out"), P * B, G, h, w, cur[0], cur[1],
                                        _stream()), "layer_apply")
    return v


RECONS = ("centre", "centroid")      # the decoders' recon argument; None is "centre"


def check_recon(recon):
    """The ``recon`` argument of the decoders -> "centre" (None too) or "centroid".  ValueError naming recon otherwise."""
    if recon is None:
        return RECONS[0]
    if not (isinstance(recon, str) and recon in RECONS):
        raise ValueError("recon must be None or one of %s: where a decoder puts a coefficient inside its quantisation bin (got %r)"
                         % (", ".join(repr(r) for r in RECONS), recon))
    return recon


def gauss_centroid(v, params, pair, out=None):
    """Centroid reconstruction of a level (lldwt_gauss_centroid).  v (P,B,C,h,w): the decoded values; params
    (P,B,2C,h,w): sigma on the even, mu on the odd channels (quality_layers.level_params); pair: the step in force, (q, inv_q)
    of step_pair / layer_pair, or a StepMap over the level (one map per image b of B; lldwt_gauss_centroid_map) -> every value
    moved from the centre of its bin to the bin's mean under N(mu, sigma^2), never out of the bin (out: where to write it, v
    itself allowed)."""
    if v.dim() != 5 or params.dim() != 5 or tuple(params.shape) != (v.shape[0], v.shape[1], 2 * v.shape[2], v.shape[3], v.shape[4]):
        raise _lib.LLDWTError("gauss_centroid: level %s and params %s do not belong together" % (tuple(v.shape), tuple(params.shape)))
    P, B, G, h, w = v.shape
    o = torch.empty_like(v) if out is None else out
    if o.shape != v.shape:
        raise _lib.LLDWTError("gauss_centroid: out %s and the level %s differ in shape" % (tuple(o.shape), tuple(v.shape)))
    if isinstance(pair, StepMap):
        check(_lib.load().lldwt_gauss_centroid_map(_chk(params, "params"), _chk(v, "v"), _chk(o, "out"), P * B, B, G, h, w,
                                                   *_map_args(pair, B, h, w), _stream()), "gauss_centroid_map")
        return o
    q, inv_q = pair
    check(_lib.load().lldwt_gauss_centroid(_chk(params, "params"), _chk(v, "v"), _chk(o, "out"), P * B, G, h, w, float(q),
                                           float(inv_q), _stream()), "gauss_centroid")
    return o


AQ_DENOM = 16                        # a strength of adaptive quantisation is m / AQ_DENOM, m in [1, AQ_M_MAX]
AQ_M_MAX = 32
AQ_L_MIN, AQ_L_MAX = 2, 8            # blocks of 2^L x 2^L pixels


def aq_activity(images_u8, L):
    """The activity of every block of 2^L x 2^L pixels of a (B,H,W,3) uint8 device batch (lldwt_aq_activity)
    -> (a, A): a (B, ceil(H / 2^L), ceil(W / 2^L)) int32, the eighth-octave logarithm of the block's luma AC energy plus its
    floor, and A (B,) int64, the sum of a over each image.  Integers: exact and reproducible."""
    B, H, W = _u8hwc(images_u8, "aq_activity")
    if not (isinstance(L, int) and AQ_L_MIN <= L <= AQ_L_MAX):
        raise _lib.LLDWTError("aq_activity: L must be an integer in [%d, %d] (got %r)" % (AQ_L_MIN, AQ_L_MAX, L))
    a = torch.empty(B, -(-H >> L), -(-W >> L), device=images_u8.device, dtype=torch.int32)
    A = torch.empty(B, device=images_u8.device, dtype=torch.int64)
    check(_lib.load().lldwt_aq_activity(C.c_void_p(images_u8.data_ptr()), C.c_void_p(a.data_ptr()), C.c_void_p(A.data_ptr()),
                                        B, H, W, L, _stream()), "aq_activity")
    return a, A


def aq_steps(a, A, aq, step_n):
    """The step map of adaptive quantisation (lldwt_aq_steps): a (B,hb,wb) int32 and A (B,) int64 of
    aq_activity, the strength aq = m / 16 (m in 1..32) and the base step step_n / 16 (step_n in [4, 1024]) -> (B,hb,wb) int32
    device tensor of n, n / 16 the step of each block.  A byte or quality target reruns only this for every base it tries."""
    if not (isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.int32 and a.is_contiguous() and a.dim() == 3
            and isinstance(A, torch.Tensor) and A.is_cuda and A.dtype == torch.int64 and A.is_contiguous()
            and tuple(A.shape) == (a.shape[0],)):
        raise _lib.LLDWTError("aq_steps: a must be a contiguous (B,hb,wb) int32 and A a (B,) int64 device tensor")
    m = float(aq) * AQ_DENOM
    if not (1 <= m <= AQ_M_MAX and m == int(m)):
        raise _lib.LLDWTError("aq_steps: aq must be m / %d with an integer m in [1, %d] (got %r)" % (AQ_DENOM, AQ_M_MAX, aq))
    if not (isinstance(step_n, int) and STEP_N_MIN <= step_n <= STEP_N_MAX):
        raise _lib.LLDWTError("aq_steps: step_n must be an integer in [%d, %d] (got %r)" % (STEP_N_MIN, STEP_N_MAX, step_n))
    n = torch.empty_like(a)
    check(_lib.load().lldwt_aq_steps(C.c_void_p(a.data_ptr()), C.c_void_p(A.data_ptr()), C.c_void_p(n.data_ptr()), a.shape[0],
                                     a.shape[1] * a.shape[2], int(m), step_n, _stream()), "aq_steps")
    return n


def cost_table(cdf, sizes):
    """Quantised CDF tables (host int32 arrays: cdf (T, width), sizes (T)) -> (T, width) int32 numpy array for code_cost:
    round(-log2(freq / 65536) * 2^16) for the sizes[t] - 2 symbols of table t, COST_ESCAPE elsewhere."""
    import numpy as np
    cdf = np.asarray(cdf, dtype=np.int64)
    freq = np.diff(cdf, axis=1, append=cdf[:, -1:])
    col = np.arange(cdf.shape[1])[None, :]
    ok = (col < np.asarray(sizes)[:, None] - 2) & (freq > 0)
    bits = -np.log2(np.where(ok, freq, 1) / 65536.0)
    return np.where(ok, np.rint(bits * COST_ONE_BIT), COST_ESCAPE).astype(np.int32)


def code_cost(sym, idx, cost, sizes, offsets):
    """sym, idx: (Z, n) int32 device tensors; cost (T, width), sizes (T), offsets (T): int32 device tensors (cost_table)
    -> (sums, escapes): (Z) int64 device tensors, the code length of each stream in units of 2^-16 bit (an escape counts
    COST_ESCAPE) and its number of escapes (lldwt_code_cost; exact integer sums)."""
    for t in (sym, idx, cost, sizes, offsets):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
            raise _lib.LLDWTError("code_cost: every argument must be a contiguous int32 device tensor")
    if sym.dim() != 2 or sym.shape != idx.shape or cost.dim() != 2 or sizes.numel() != cost.shape[0] or offsets.numel() != cost.shape[0]:
        raise _lib.LLDWTError("code_cost: sym / idx must be (Z, n) and cost (T, width) with T sizes and offsets")
    Z, n = sym.shape
    sums = torch.zeros(Z, device=sym.device, dtype=torch.int64)
    esc = torch.zeros(Z, device=sym.device, dtype=torch.int64)
    p = lambda t: C.c_void_p(t.data_ptr())
    check(_lib.load().lldwt_code_cost(p(sym), p(idx), Z, n, p(cost), cost.shape[0], cost.shape[1], p(sizes), p(offsets),
                                      COST_ESCAPE, p(sums), p(esc), _stream()), "code_cost")
    return sums, esc


def cgp_pack(ws, bs, groups):
    """ws: 4 stacked 1x1 conv weights (P, groups*c_{l+1}, c_l, 1, 1); bs: 4 biases (P, groups*c_{l+1})."""
    lib = _lib.load()
    P = ws[0].shape[0]
    c = [ws[0].shape[2]] + [w.shape[1] // groups for w in ws]
    assert c[4] == 2
    n = lib.lldwt_cgp_packed_floats(c[0], c[1], c[2], c[3], groups)
    packed = torch.empty(P, n, device=ws[0].device, dtype=torch.float32)
    args = []
    for w, b in zip(ws, bs):
        args += [_chk(w, "w"), _chk(b, "b")]
    check(lib.lldwt_cgp_pack(*args, _chk(packed), P, c[0], c[1], c[2], c[3], groups, _stream()), "cgp_pack")
    return packed, tuple(c[:4])


def cgp_rate(cat, x, packed, dims, noise=None, want_params=False, bit_sum=None):
    """cat (P,B,groups*c0,h,w), x (P,B,groups,h,w) -> bits (and (sigma,mu) params if asked)."""
    P, B, G, h, w = x.shape
    assert cat.shape == (P, B, G * dims[0], h, w)
    bits = torch.empty_like(x)
    params = torch.empty(P, B, 2 * G, h, w, device=x.device, dtype=torch.float32) if want_params else None
    bs = C.c_void_p(0) if bit_sum is None else C.c_void_p(bit_sum.data_ptr())
    check(_lib.load().lldwt_cgp_rate(_chk(cat, "cat"), _chk(x, "x"), _opt(noise), _chk(packed, "packed"), _chk(bits),
                                     _opt(params), bs, P, B, h * w, dims[0], dims[1], dims[2], dims[3], G, _stream()),
          "cgp_rate")
    return bits, params


def cgp_rate_ctx(plc, xq, x, packed, dims, K, tap_mask, noise=None, bit_sum=None):
    """Fused cgp stack whose first layer also holds the folded masked context conv (include/lldwt.h lldwt_cgp_rate_ctx).
    plc (P,B,G*cplc,h,w); xq, x (P,B,G,h,w); dims = (cplc + ntaps, c1, c2, c3) as returned by cgp_pack."""
    P, B, G, h, w = x.shape
    ntaps = bin(tap_mask & ((1 << (K * K)) - 1)).count("1")
    cplc = dims[0] - ntaps
    assert plc.shape == (P, B, G * cplc, h, w) and xq.shape == x.shape
    bits = torch.empty_like(x)
    bs = C.c_void_p(0) if bit_sum is None else C.c_void_p(bit_sum.data_ptr())
    check(_lib.load().lldwt_cgp_rate_ctx(_chk(plc, "plc"), _chk(xq, "xq"), _chk(x, "x"), _opt(noise), _chk(packed, "packed"),
                                         _chk(bits), C.c_void_p(0), bs, P, B, h, w, cplc, K, int(tap_mask), dims[1], dims[2],
                                         dims[3], G, _stream()), "cgp_rate_ctx")
    return bits


def cgp_rate_train(cat, x, packed, dims, noise):
    """Training forward of the fused cgp stack: -> (bits, params (P,B,2G,h,w), h1, h2, h3)."""
    P, B, G, h, w = x.shape
    assert cat.shape == (P, B, G * dims[0], h, w)
    bits = torch.empty_like(x)
    params = torch.empty(P, B, 2 * G, h, w, device=x.device, dtype=torch.float32)
    hs = [torch.empty(P, B, G * dims[l], h, w, device=x.device, dtype=torch.float32) for l in (1, 2, 3)]
    check(_lib.load().lldwt_cgp_rate_train(_chk(cat, "cat"), _chk(x, "x"), _opt(noise), _chk(packed, "packed"), _chk(bits),
                                           _chk(params), _chk(hs[0]), _chk(hs[1]), _chk(hs[2]), P, B, h * w, dims[0],
                                           dims[1], dims[2], dims[3], G, _stream()), "cgp_rate_train")
    return bits, params, hs[0], hs[1], hs[2]


def cgp_rate_train_ctx(plc, xq, x, packed, dims, noise, K, tap_mask):
    """Training forward of the fused cgp stack reading its input as the eval path does (lldwt_cgp_rate_train_ctx): plc
    (P,B,G*cplc,h,w) + the live taps of the quantised subband xq (P,B,G,h,w) gathered in the kernel -- no concatenated tensor.
    dims[0] = cplc + number of live taps.  -> (bits, params (P,B,2G,h,w), h1, h2, h3)."""
    P, B, G, h, w = x.shape
    ntaps = bin(int(tap_mask)).count("1")
    cplc = dims[0] - ntaps
    if plc.shape != (P, B, G * cplc, h, w) or xq.shape != (P, B, G, h, w):
        raise _lib.LLDWTError("cgp_rate_train_ctx: shapes %r %r %r" % (tuple(plc.shape), tuple(xq.shape), tuple(x.shape)))
    bits = torch.empty_like(x)
    params = torch.empty(P, B, 2 * G, h, w, device=x.device, dtype=torch.float32)
    hs = [torch.empty(P, B, G * dims[l], h, w, device=x.device, dtype=torch.float32) for l in (1, 2, 3)]
    check(_lib.load().lldwt_cgp_rate_train_ctx(_chk(plc, "plc"), _chk(xq, "xq"), _chk(x, "x"), _opt(noise), _chk(packed, "packed"),
                                               _chk(bits), _chk(params), _chk(hs[0]), _chk(hs[1]), _chk(hs[2]), P, B, h, w, cplc,
                                               K, int(tap_mask), dims[1], dims[2], dims[3], G, _stream()), "cgp_rate_train_ctx")
    return bits, params, hs[0], hs[1], hs[2]


def cgp_bwd_split(dparams, h1, h2, h3, packed_bwd, dims, groups, ntaps):
    """lldwt_cgp_bwd_split -> (dplc (P,B,G*cplc,h,w), dtaps (P,B,G*ntaps,h,w), d1, d2, d3)."""
    P, B, _, h, w = dparams.shape
    cplc = dims[0] - ntaps
    d1, d2, d3 = torch.empty_like(h1), torch.empty_like(h2), torch.empty_like(h3)
    dplc = torch.empty(P, B, groups * cplc, h, w, device=dparams.device, dtype=torch.float32)
    dtaps = torch.empty(P, B, groups * ntaps, h, w, device=dparams.device, dtype=torch.float32)
    check(_lib.load().lldwt_cgp_bwd_split(_chk(dparams), _chk(h1), _chk(h2), _chk(h3), _chk(packed_bwd), _chk(d1), _chk(d2), _chk(d3),
                                          _chk(dplc), _chk(dtaps), P, B, h * w, cplc, ntaps, dims[1], dims[2], dims[3], groups,
                                          _stream()), "cgp_bwd_split")
    return dplc, dtaps, d1, d2, d3


def wgrad1x1_split(xa, xb, dy, groups, want_bias=True):
    """Weight gradient of a grouped 1x1 conv whose input is [xa rows | xb rows] per group (lldwt_wgrad1x1_split):
    xa (P,B,G*ca,h,w), xb (P,B,G*cb,h,w), dy (P,B,cout,h,w) -> (dw (P,cout,ca+cb,1,1), db (P,cout) or None)."""
    P, B, ca_t, h, w = xa.shape
    ca, cb, cout = ca_t // groups, xb.shape[2] // groups, dy.shape[2]
    dw = torch.zeros(P, cout, ca + cb, 1, 1, device=xa.device, dtype=torch.float32)
    db = torch.zeros(P, cout, device=xa.device, dtype=torch.float32) if want_bias else None
    check(_lib.load().lldwt_wgrad1x1_split(_chk(xa, "xa"), _chk(xb, "xb"), _chk(dy, "dy"), _chk(dw), _opt(db), P, B, h * w, ca, cb,
                                           cout, groups, _stream()), "wgrad1x1_split")
    return dw, db


def cgp_pack_bwd(ws, groups):
    """The four forward 1x1 weights (P, groups*c_{l+1}, c_l, 1, 1) -> transposed pack for cgp_bwd."""
    lib = _lib.load()
    P = ws[0].shape[0]
    c = [ws[0].shape[2]] + [w.shape[1] // groups for w in ws]
    n = lib.lldwt_cgp_bwd_packed_floats(c[0], c[1], c[2], c[3], groups)
    packed = torch.empty(P, n, device=ws[0].device, dtype=torch.float32)
    check(lib.lldwt_cgp_pack_bwd(*[_chk(w, "w") for w in ws], _chk(packed), P, c[0], c[1], c[2], c[3], groups, _stream()),
          "cgp_pack_bwd")
    return packed


def cgp_bwd(dparams, h1, h2, h3, packed_bwd, dims, groups):
    """-> (dcat, d1, d2, d3): gradients at the input and at the pre-activation outputs of layers 1..3."""
    P, B, _, h, w = dparams.shape
    d1, d2, d3 = torch.empty_like(h1), torch.empty_like(h2), torch.empty_like(h3)
    dcat = torch.empty(P, B, groups * dims[0], h, w, device=dparams.device, dtype=torch.float32)
    check(_lib.load().lldwt_cgp_bwd(_chk(dparams), _chk(h1), _chk(h2), _chk(h3), _chk(packed_bwd), _chk(d1), _chk(d2),
                                    _chk(d3), _chk(dcat), P, B, h * w, dims[0], dims[1], dims[2], dims[3], groups,
                                    _stream()), "cgp_bwd")
    return dcat, d1, d2, d3


_EB_TABLE = {"key": None, "tab": None, "eb": None}


def factorized_rate(x, eb, noise=None, bit_sum=None):
    """x: (P,B,C,h,w); eb: (P,C,59) packed EntropyBottleneck parameters -> (bits, q)."""
    P, B, Cc, h, w = x.shape
    assert eb.shape == (P, Cc, _lib.EB_FLOATS)
    bits = torch.empty_like(x)
    q = torch.empty_like(x)
    bs = C.c_void_p(0) if bit_sum is None else C.c_void_p(bit_sum.data_ptr())
    if noise is None and not eb.requires_grad:
        # eval: the per-offset bit table depends on the parameters only -- kept while `eb` is the same tensor at the same version
        key = (eb.data_ptr(), eb._version, tuple(eb.shape), eb.device)
        if _EB_TABLE["key"] != key:
            tab = torch.empty(P, Cc, 256, device=eb.device, dtype=torch.float32)
            check(_lib.load().lldwt_factorized_table(_chk(eb), _chk(tab), P, Cc, _stream()), "factorized_table")
            _EB_TABLE["key"], _EB_TABLE["tab"], _EB_TABLE["eb"] = key, tab, eb      # eb kept: its address cannot be reused
        check(_lib.load().lldwt_factorized_rate_tab(_chk(x), _chk(eb), _chk(_EB_TABLE["tab"]), _chk(bits), _chk(q), bs, P, B,
                                                    Cc, h * w, _stream()), "factorized_rate_tab")
        return bits, q
    check(_lib.load().lldwt_factorized_rate(_chk(x), _chk(eb), _opt(noise), _chk(bits), _chk(q), bs, P, B, Cc, h * w,
                                            _stream()), "factorized_rate")
    return bits, q


# ------------------------------------------------------------------------------------------------ MS-SSIM
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def ms_ssim_min_side(scales=5):
    """Smallest legal side: the coarsest scale must still hold one 11 x 11 window."""
    return 10 * 2 ** (scales - 1) + 1


def _ms_ssim_check(x, y, scales):
    """Shape rules of MS-SSIM, raised as ValueError on the host before the library is touched."""
    if not (isinstance(scales, int) and 1 <= scales <= len(MS_SSIM_WEIGHTS)):
        raise ValueError("ms_ssim: scales must be an integer in 1..%d (got %r)" % (len(MS_SSIM_WEIGHTS), scales))
    if x.dim() != 4 or tuple(x.shape) != tuple(y.shape):
        raise ValueError("ms_ssim: x and y must be (B,C,H,W) of one shape (got %s and %s)" % (tuple(x.shape), tuple(y.shape)))
    need = ms_ssim_min_side(scales)
    for name, side in (("height", x.shape[2]), ("width", x.shape[3])):
        if side < need:
            raise ValueError("ms_ssim: %s %d is below the minimum side %d for %d scale(s)" % (name, side, need, scales))
    if x.shape[0] * x.shape[1] < 1 or x.shape[0] * x.shape[1] > 65535:
        raise ValueError("ms_ssim: B*C must be in 1..65535 (got %d)" % (x.shape[0] * x.shape[1]))


def ms_ssim_forward(x, y, offset=0.5, scales=5):
    """One fused launch per scale (lldwt_msssim_forward).  x: target, y: reconstruction, (B,C,H,W) fp32; ``offset`` is added
    to both on load.  Returns (v (S,B,C), m (B,C), coef (S,B,C), pyr): float64 terms and values, and what the backward needs."""
    _ms_ssim_check(x, y, scales)
    lib = _lib.load()
    B, Cn, H, W = x.shape
    planes = B * Cn
    dev = x.device
    pyr = torch.empty(max(1, lib.lldwt_msssim_ws_floats(planes, H, W, scales)), dtype=torch.float32, device=dev)
    sums = torch.empty(scales, planes, 2, dtype=torch.float64, device=dev)
    v = torch.empty(scales, B, Cn, dtype=torch.float64, device=dev)
    m = torch.empty(B, Cn, dtype=torch.float64, device=dev)
    coef = torch.empty(scales, B, Cn, dtype=torch.float64, device=dev)
    dp = lambda t: C.c_void_p(t.data_ptr())
    check(lib.lldwt_msssim_forward(_chk(x, "x"), _chk(y, "y"), float(offset), planes, H, W, scales, dp(pyr), dp(sums), dp(v), dp(m),
                                   dp(coef), _stream()), "msssim_forward")
    return v, m, coef, pyr


def ms_ssim_terms(x, y, offset=0.5, scales=5):
    """v (S,B,C) float64: the clamped spatial mean of cs per scale, of l*cs for the last one."""
    return ms_ssim_forward(x, y, offset, scales)[0]


def ms_ssim(x, y, offset=0.5, scales=5):
    """MS-SSIM per image and channel, (B,C) float64 on the device (pytorch-msssim 0.2.1 with data_range 1)."""
    return ms_ssim_forward(x, y, offset, scales)[1]


def ms_ssim_backward(x, y, pyr, coef, g, gscale, offset=0.5, scales=5):
    """grad_y of gscale * g[0] * sum(m) (lldwt_msssim_backward); g: 1-element float64 DEVICE tensor or None."""
    lib = _lib.load()
    B, Cn, H, W = x.shape
    planes = B * Cn
    grad = torch.empty_like(y)
    gpyr = torch.empty(max(1, lib.lldwt_msssim_ws_floats(planes, H, W, scales) // 2), dtype=torch.float32, device=x.device)
    if g is not None and not (g.is_cuda and g.dtype == torch.float64 and g.numel() == 1):
        raise _lib.LLDWTError("ms_ssim_backward: g must be a 1-element float64 device tensor")
    dp = lambda t: C.c_void_p(t.data_ptr())
    check(lib.lldwt_msssim_backward(_chk(x, "x"), _chk(y, "y"), float(offset), planes, H, W, scales, dp(pyr), dp(coef),
                                    dp(g) if g is not None else C.c_void_p(0), float(gscale), dp(gpyr), _chk(grad), _stream()),
          "msssim_backward")
    return grad


def sq_err_sum(a, b, out):
    check(_lib.load().lldwt_sq_err_sum(_chk(a), _chk(b), a.numel(), C.c_void_p(out.data_ptr()), _stream()), "sq_err_sum")


def sum_into(x, out):
    check(_lib.load().lldwt_sum(_chk(x), x.numel(), C.c_void_p(out.data_ptr()), _stream()), "sum")


# ------------------------------------------------------------------------------------------------ training support
def gauss_rate_bwd(x, params, noise, gbits):
    P, B, Cc, h, w = x.shape
    dx = torch.empty_like(x)
    dparams = torch.empty_like(params)
    check(_lib.load().lldwt_gauss_rate_bwd(_chk(x), _chk(params), _opt(noise), _chk(gbits), _chk(dx), _chk(dparams), P * B,
                                           Cc, h * w, _stream()), "gauss_rate_bwd")
    return dx, dparams


def factorized_rate_bwd(x, eb, noise, gbits):
    P, B, Cc, h, w = x.shape
    dx = torch.empty_like(x)
    deb = torch.zeros_like(eb)
    check(_lib.load().lldwt_factorized_rate_bwd(_chk(x), _chk(eb), _opt(noise), _chk(gbits), _chk(dx), _chk(deb), P, B, Cc,
                                                h * w, _stream()), "factorized_rate_bwd")
    return dx, deb


def axpby(a, b, alpha, beta=0.0):
    out = torch.empty_like(a)
    check(_lib.load().lldwt_axpby(_chk(a), _opt(b), _chk(out), a.numel(), float(alpha), float(beta), _stream()), "axpby")
    return out


def ycc_to_rgb_bwd(grgb):
    B, _, H, W = grgb.shape
    g = torch.empty(3, B, 1, H, W, device=grgb.device, dtype=torch.float32)
    check(_lib.load().lldwt_ycc_to_rgb_bwd(_chk(grgb), _chk(g), B, H, W, _stream()), "ycc_to_rgb_bwd")
    return g


def lifting_program(Z, H, W, levels, different, block_offset, inverse, Cc, scale=False):
    """-> (list of LiftOp, saved_floats): the step program of the transform (include/lldwt.h lldwt_lifting_program).
    scale=True: with the gain ops of config.scale == 1 (kind 1..4; each keeps its input in the saved buffer)."""
    lib = _lib.load()
    tot = C.c_int64(0)
    sc = int(bool(scale))
    n = lib.lldwt_lifting_program(None, 0, Z, H, W, levels, int(bool(different)), block_offset, int(bool(inverse)), sc, Cc,
                                  C.byref(tot))
    if n < 0:
        check(n, "lifting_program")
    arr = (_lib.LiftOp * n)()
    lib.lldwt_lifting_program(arr, n, Z, H, W, levels, int(bool(different)), block_offset, int(bool(inverse)), sc, Cc,
                              C.byref(tot))
    return list(arr), int(tot.value)


def lifting_forward_train(x, taps, packed, levels, Cc, K, res_weight, linear, different, block_offset, saved, scale_nh=None,
                          scale_nl=None):
    lib = _lib.load()
    P, B, _, H, W = x.shape
    dev = x.device
    ll = torch.empty(P, B, 1, H >> levels, W >> levels, device=dev, dtype=torch.float32)
    yh = [torch.empty(P, B, 3, H >> (i + 1), W >> (i + 1), device=dev, dtype=torch.float32) for i in range(levels)]
    nb = lib.lldwt_lifting_ws_bytes(P * B, H, W, Cc)
    ws = workspace(nb, dev)
    check(lib.lldwt_lifting_forward_train(_chk(x, "x"), _chk(ll), _ptr_array(yh), P, B, H, W, levels, _chk(taps),
                                             _chk(packed), int(packed.shape[1]), int(block_offset), int(bool(different)), Cc, K,
                                             float(res_weight), int(bool(linear)), _opt(scale_nh), _opt(scale_nl),
                                             C.c_void_p(ws.data_ptr()), nb, _chk(saved), _stream()), "lifting_forward_train")
    return ll, yh


def lifting_inverse_train(ll, yh, taps, packed, Cc, K, res_weight, linear, block_offset, saved, scale_nh=None, scale_nl=None):
    lib = _lib.load()
    levels = len(yh)
    P, B, _, hl, wl = ll.shape
    H, W = hl << levels, wl << levels
    x = torch.empty(P, B, 1, H, W, device=ll.device, dtype=torch.float32)
    for t in yh:
        _chk(t, "yh")
    nb = lib.lldwt_lifting_ws_bytes(P * B, H, W, Cc)
    ws = workspace(nb, ll.device)
    check(lib.lldwt_lifting_inverse_train(_chk(ll), _ptr_array(yh), _chk(x), P, B, H, W, levels, _chk(taps), _chk(packed),
                                             int(packed.shape[1]), int(block_offset), Cc, K, float(res_weight),
                                             int(bool(linear)), _opt(scale_nh), _opt(scale_nl), C.c_void_p(ws.data_ptr()), nb,
                                             _chk(saved), _stream()), "lifting_inverse_train")
    return x


def lift_bwd_pre(g_dout, g_din, g, Z, h, w):
    check(_lib.load().lldwt_lift_bwd_pre(g_dout, g_din, _chk(g), Z, h, w, _stream()), "lift_bwd_pre")


def lift_bwd_fin(g, dsk, srcv, g_src, Z, batch, h, w, taps, dtaps, vertical, sign, rw):
    check(_lib.load().lldwt_lift_bwd_fin(_chk(g), _chk(dsk), _chk(srcv), g_src, Z, batch, h, w, _chk(taps), _chk(dtaps),
                                         int(vertical), float(sign), float(rw), _stream()), "lift_bwd_fin")


def lift_step_bwd(g_dst_out, g_dst_in, g_src, saved_step, P, B, h, w, taps, dtaps, packed, packed_plane_stride, dW, Cc, K,
                  rw, sign, vertical, linear, packed_bwd=None, taps_id=None):
    """Whole backward of one lifting step (include/lldwt.h lldwt_lift_step_bwd).  g_*: lldwt_views over the gradient
    buffers; packed: forward pack of this step's block (pointer already offset to the block); dW: the 8 gradient
    tensors (w1,b1,...,w4,b4) of the block, each (P,...), accumulated in place.  packed_bwd (pointer, offset like packed) +
    taps_id ((P,3) of (0,1,0)): the backward-data chain on the fused split-fp16 kernel (lldwt_lift_step_bwd_f16)."""
    lib = _lib.load()
    nb = lib.lldwt_lift_step_bwd_ws_bytes(P * B, h, w, Cc)
    ws = workspace(nb, taps.device)
    if packed_bwd is not None:
        check(lib.lldwt_lift_step_bwd_f16(g_dst_out, g_dst_in, g_src, _chk(saved_step), P, B, h, w, _chk(taps), _chk(dtaps),
                                          packed, packed_plane_stride, *[_chk(t) for t in dW], Cc, K, float(rw), float(sign),
                                          int(bool(vertical)), int(bool(linear)), C.c_void_p(ws.data_ptr()), nb, packed_bwd,
                                          _chk(taps_id), _stream()), "lift_step_bwd_f16")
        return
    check(lib.lldwt_lift_step_bwd(g_dst_out, g_dst_in, g_src, _chk(saved_step), P, B, h, w, _chk(taps), _chk(dtaps),
                                  packed, packed_plane_stride, *[_chk(t) for t in dW], Cc, K, float(rw), float(sign),
                                  int(bool(vertical)), int(bool(linear)), C.c_void_p(ws.data_ptr()), nb, _stream()),
          "lift_step_bwd")


def ew_mul(a, b, scale=1.0):
    out = torch.empty_like(a)
    check(_lib.load().lldwt_ew_mul(_chk(a), _chk(b), _chk(out), a.numel(), float(scale), _stream()), "ew_mul")
    return out


def gdn_apply(x, nrm, inverse):
    y = torch.empty_like(x)
    check(_lib.load().lldwt_gdn_apply(_chk(x), _chk(nrm), _chk(y), x.numel(), int(bool(inverse)), _stream()), "gdn_apply")
    return y


def gdn_apply_bwd(x, nrm, g, inverse):
    dx, dn = torch.empty_like(x), torch.empty_like(x)
    check(_lib.load().lldwt_gdn_apply_bwd(_chk(x), _chk(nrm), _chk(g), _chk(dx), _chk(dn), x.numel(), int(bool(inverse)),
                                          _stream()), "gdn_apply_bwd")
    return dx, dn
