"""The interleaved rANS coder "irans32" on the device (csrc/rans_gpu.hip; definition tools/irans_ref.py).

Same symbols, order and tables as the host coder (ans.py), other arithmetic: K 32-bit lanes per stream, coded by one wave
per stream.  ``encode`` takes device symbols / indexes and returns byte strings after one launch and one copy;
``Decoder.pop`` queues one launch per call on the current stream and returns a device tensor with no synchronisation;
``Decoder.finish`` synchronises once and raises ValueError("corrupt stream ...") if any stream failed its checks.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

CODER_NAME = "irans32"
_RCP = {}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def lanes(n):
    return int(_lib.load().lldwt_irans_lanes(int(n)))


def capacity(n):
    return int(_lib.load().lldwt_irans_capacity(int(n)))


def _rcp(dev):
    key = str(dev)
    t = _RCP.get(key)
    if t is None:
        r = np.zeros(65537, dtype=np.uint32)
        _lib.check(_lib.load().lldwt_irans_rcp_table(r.ctypes.data_as(C.c_void_p)), "irans_rcp_table")
        t = _RCP[key] = torch.from_numpy(r.view(np.int32)).to(dev)
    return t


class DeviceTables:
    """A set of host int32 tables (cdf (ncdf, stride), sizes, offsets) on the device, with the decoder's LUT."""

    def __init__(self, cdf, sizes, offsets, dev):
        cdf = np.ascontiguousarray(cdf, dtype=np.int32)
        sizes = np.ascontiguousarray(sizes, dtype=np.int32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        self.ncdf, self.stride = int(cdf.shape[0]), int(cdf.shape[1])
        lut = np.empty((self.ncdf, 257), dtype=np.int32)
        pv = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(_lib.load().lldwt_irans_lut(pv(cdf), self.ncdf, self.stride, pv(sizes), pv(lut)), "irans_lut")
        self.cdf, self.sizes, self.offsets, self.lut = (torch.from_numpy(a).to(dev) for a in (cdf, sizes, offsets, lut))
        self.device = dev

    def args(self):
        return (_ptr(self.cdf), self.ncdf, self.stride, _ptr(self.sizes), _ptr(self.offsets))


def device_tables(tables, dev):
    """The DeviceTables of an object with .cdf / .sizes / .offsets host arrays, cached on it per device."""
    cache = tables.__dict__.setdefault("_irans_dev", {})
    key = str(dev)
    if key not in cache:
        cache[key] = DeviceTables(tables.cdf, tables.sizes, tables.offsets, dev)
    return cache[key]


def encode(sym, idx, dt):
    """sym, idx: (Z, n) int32 device tensors (row stride n) -> list of Z byte strings."""
    Z, n = int(sym.shape[0]), int(sym.shape[1])
    dev = sym.device
    sym, idx = sym.contiguous(), idx.contiguous()
    cap = capacity(n)
    out = torch.empty(Z * cap, device=dev, dtype=torch.uint8)
    meta = torch.zeros(Z + 1, device=dev, dtype=torch.int64)          # lengths, then the flag (low 32 bits)
    _lib.check(_lib.load().lldwt_irans_encode(_ptr(sym), _ptr(idx), Z, n, n, *dt.args(), _ptr(_rcp(dev)), _ptr(out), cap,
                                              _ptr(meta), C.c_void_p(meta.data_ptr() + 8 * Z), _stream()), "irans_encode")
    m = meta.cpu().tolist()
    if m[Z] != 0 or min(m[:Z]) < 0:
        raise _lib.LLDWTError("irans_encode: a stream failed (bad cdf index or no room)")
    # the streams end at the end of their buffer slot: the used tails are gathered on the device and copied once
    flat = torch.cat([out[z * cap + cap - m[z]:(z + 1) * cap] for z in range(Z)]).cpu().numpy().tobytes()
    res, p = [], 0
    for L_ in m[:Z]:
        res.append(flat[p:p + L_])
        p += L_
    return res


class Decoder:
    """Z streams of n symbols each, uploaded once; pop(idx) decodes the next cnt symbols of every stream on the device."""

    def __init__(self, streams, n, dt, dev):
        lib = _lib.load()
        self.Z, self.n, self.dt, self.pos = len(streams), int(n), dt, 0
        lens = [len(s) for s in streams]
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        blob = b"".join(bytes(s) for s in streams)
        self.bytes = torch.from_numpy(np.frombuffer(blob + b"\0", dtype=np.uint8).copy()).to(dev)
        self.meta = torch.from_numpy(np.concatenate([offs, np.asarray(lens, dtype=np.int64)])).to(dev)
        self.state = torch.zeros(self.Z * int(lib.lldwt_irans_state_words()), device=dev, dtype=torch.int32)
        self.flag = torch.zeros(1, device=dev, dtype=torch.int32)
        self.dev = dev

    def pop(self, idx, cnt=None, stride=None, out=None):
        """idx: int32 device tensor holding stream z's cnt indexes at z * stride (default: (Z, ...) contiguous, cnt = the
        per-stream element count) -> out (same layout; allocated like idx if None).  No synchronisation."""
        if cnt is None:
            cnt = idx.numel() // self.Z
        stride = cnt if stride is None else stride
        if self.pos + cnt > self.n:
            raise ValueError("corrupt stream: more symbols requested than the stream holds")
        if out is None:
            out = torch.empty_like(idx)
        b0 = self.meta.data_ptr()
        _lib.check(_lib.load().lldwt_irans_decode(_ptr(self.state), _ptr(self.bytes), C.c_void_p(b0),
                                                  C.c_void_p(b0 + 8 * self.Z), self.Z, self.n, self.pos, cnt, _ptr(idx), stride,
                                                  _ptr(out), stride, *self.dt.args(), _ptr(self.dt.lut), _ptr(self.flag),
                                                  _stream()), "irans_decode")
        self.pos += cnt
        return out

    def finish(self):
        """One synchronisation: every symbol popped and every stream's final-state / cursor check passed."""
        if self.pos != self.n:
            raise ValueError("corrupt stream: %d of %d symbols decoded" % (self.pos, self.n))
        if int(self.flag.item()) != 0:
            raise ValueError("corrupt stream: the irans32 decoder's final-state, cursor or bounds check failed")
