"""Real entropy coding of DWTConditioned2EntropyLayerZTsepSubbands -- replaces the per-pixel Python loops of the
reference's ``test`` / ``compress_ar`` / ``decompress_ar`` (graphs/models/LiftingBasedDWT_net.py:374-556).

What the reference does, per tensor: walk the pixels in raster order; at each pixel run the context CNN on a k x k crop of
the values decoded so far, read (sigma, mu) at the crop's centre, code ``round(y - mu)`` with the Gaussian CDF selected by
sigma (64-entry scale table), and write ``round(y - mu) + mu`` back for the pixels that follow.  That is O(pixels) tiny
sequential CNN calls -- minutes per image.

What this module does: the SAME per-pixel maths, scheduled as an anti-diagonal WAVEFRONT.  A pixel only depends on
already-coded neighbours inside the causal footprint of its context model, so every pixel with the same
``t = w + s*h`` is independent of the others once steps < t are done:
  * 3x3-crop stacks (``csc_xe`` and the coarsest ``csc_list`` entry, :311-317,299-305): the crop reaches (h-1, w+1) -> s = 2;
  * masked 5x5 type-A conv + tree context + cgp (:275-289): the mask reaches (h-1, w+2) -> s = 3.
One wavefront step is evaluated for all planes, images, subbands and pixels of the step in a handful of launches of the
kernels the rate path already has (conv engine on the batch of crops; fused cgp kernel with the context conv folded into
its first layer on the gathered taps), so a 256 x 256 subband needs ~1 000 steps instead of 65 536 x 3 Python iterations.
The tree-context conv (243 channels, the expensive part) does not depend on the tensor being coded and runs once, fully
parallel, per level.

Stream layout: one range-ANS stream per (plane, image, tensor) (the reference: per plane and tensor at batch 1), symbols
in WAVEFRONT order -- step t ascending, inside a step h ascending, channels innermost -- because that is the order a
parallel decoder can consume them in (the reference's raster order would serialise it again).  The coder itself is
ans.py (host C++ behind the C-ABI); symbols and CDF indexes are produced on the GPU.  Encoder and decoder evaluate the
context with the same kernels on the same operand shapes, so their (sigma, mu) agree bit for bit; not-yet-coded positions
hold 0 on both sides (the reference's encoder holds the unquantised value there, which the masks multiply by 0).
"""
import numpy as np
import torch

from ... import irans, ops
from ...ans import RansDecoder, decode_streams, encode_streams

CODERS = ("host", "gpu")         # host: ans.py (rans64 on the host, the default); gpu: irans.py (irans32)

_WF_CACHE = {}


def wavefront(H, W, slope, device):
    """-> (hs, ws, starts): pixel coordinates sorted by (t = w + slope*h, h) as device int64 tensors, and the python
    list of step boundaries (len = steps + 1)."""
    key = (H, W, slope, str(device))
    hit = _WF_CACHE.get(key)
    if hit is None:
        h = np.repeat(np.arange(H), W)
        w = np.tile(np.arange(W), H)
        t = w + slope * h
        order = np.lexsort((h, t))
        h, w, t = h[order], w[order], t[order]
        nsteps = W + slope * (H - 1)
        starts = np.searchsorted(t, np.arange(nsteps + 1)).tolist()
        hit = (torch.from_numpy(h).to(device), torch.from_numpy(w).to(device), starts)
        _WF_CACHE[key] = hit
    return hit


def _live_taps(mask_bits, K):
    return [(t // K, t % K) for t in range(K * K) if (mask_bits >> t) & 1]


class _Tables:
    """The Gaussian CDF tables of one entropy model as host int32 arrays (shared by every stream of a tensor)."""

    def __init__(self, emodel, scale_table):
        emodel.update_scale_table(scale_table)
        self.cdf = emodel.quantized_cdf.cpu().numpy().astype(np.int32)
        self.sizes = emodel.cdf_length.cpu().numpy().astype(np.int32)
        self.offsets = emodel.offset.cpu().numpy().astype(np.int32)


class _Sink:
    """Where the symbols of a tensor go (encoder) or come from (decoder), one stream per (plane, image)."""

    def __init__(self, P, B, tables, strings=None):
        self.P, self.B, self.t = P, B, tables
        self.decoding = strings is not None
        self._handles = None
        if self.decoding:
            self.dec = [[RansDecoder() for _ in range(B)] for _ in range(P)]
            for p in range(P):
                for b in range(B):
                    self.dec[p][b].set_stream(strings[p][b])
        else:
            self.sym, self.idx = [], []

    def step(self, idx, sym=None):
        """idx / sym: (P,B,N,g) int32 device tensors of one wavefront step.  Encoder: buffers them (device, no sync).
        Decoder: pops the step's symbols from the streams -> (P,B,N,g) int32 device tensor (one host round trip)."""
        if not self.decoding:
            self.idx.append(idx)
            self.sym.append(sym)
            return sym
        ih = np.ascontiguousarray(idx.cpu().numpy(), dtype=np.int32)
        out = np.empty(ih.shape, dtype=np.int32)
        self.pop(ih.ctypes.data, int(ih.shape[2] * ih.shape[3]), out.ctypes.data)
        return torch.from_numpy(out).to(idx.device)

    def pop(self, idx_ptr, per, out_ptr):
        """Decoder: ONE C call that pops the next `per` symbols of every (plane, image) stream.  idx_ptr / out_ptr: addresses of
        the caller's host int32 buffers, (P*B, per) each (numpy or pinned torch memory)."""
        import ctypes as C
        from ... import _lib
        if self._handles is None:
            self._handles = (C.c_void_p * (self.P * self.B))(*[self.dec[p][b]._h for p in range(self.P) for b in range(self.B)])
        pv = lambda a_: a_.ctypes.data_as(C.c_void_p)
        ops.check(_lib.load().lldwt_rans_decode_multi(self._handles, self.P * self.B, C.c_void_p(idx_ptr), per, per, pv(self.t.cdf),
                                                      self.t.cdf.shape[0], self.t.cdf.shape[1], pv(self.t.sizes),
                                                      pv(self.t.offsets), C.c_void_p(out_ptr)), "rans_decode_multi")

    def note(self, idx_host, sym_host):
        """Decoder of code_tree_level: called with every step's (indexes, symbols) as host int32 arrays once they are decoded.
        A hook for diagnostics (the code-length test replaces it); does nothing."""

    def finish(self):
        """Decoder: the end of a tensor (the host coder checks its streams symbol by symbol)."""

    def flush(self):
        """Encoder: -> strings[p][b] (the P * B streams in one parallel call)."""
        idx = torch.cat(self.idx, 2).cpu().numpy()          # (P,B,Npix,g) in wavefront order
        sym = torch.cat(self.sym, 2).cpu().numpy()
        flat = encode_streams(sym.reshape(self.P * self.B, -1), idx.reshape(self.P * self.B, -1), self.t.cdf, self.t.sizes,
                              self.t.offsets)
        return [flat[p * self.B:(p + 1) * self.B] for p in range(self.P)]


class _DeviceSink:
    """_Sink's interface over the irans32 device coder: the encoder buffers the steps on the device and codes every stream
    in one launch at flush(); the decoder pops each step on the device (no synchronisation) and checks the streams once in
    finish().  n: symbols per stream (decoder)."""

    def __init__(self, P, B, tables, strings=None, n=None, device=None):
        self.P, self.B, self.t = P, B, tables
        self.decoding = strings is not None
        self.dt = irans.device_tables(tables, device)
        if self.decoding:
            self.dec = irans.Decoder([strings[p][b] for p in range(P) for b in range(B)], n, self.dt, device)
        else:
            self.sym, self.idx = [], []

    def step(self, idx, sym=None):
        if not self.decoding:
            self.idx.append(idx)
            self.sym.append(sym)
            return sym
        return self.dec.pop(idx.contiguous())

    def note(self, idx_host, sym_host):
        pass

    def finish(self):
        self.dec.finish()

    def flush(self):
        Z = self.P * self.B
        idx = torch.cat([t.reshape(Z, -1) for t in self.idx], 1)
        sym = torch.cat([t.reshape(Z, -1) for t in self.sym], 1)
        flat = irans.encode(sym.int(), idx.int(), self.dt)
        return [flat[p * self.B:(p + 1) * self.B] for p in range(self.P)]


ESTIMATE = "estimate"            # not a coder: the encoder's sink that only measures (the byte-target search)
_STREAM_OVERHEAD = 4             # bytes a coder's final state adds to a stream, as the estimate counts it


def device_cost_tables(tables, dev):
    """(cost, sizes, offsets) int32 device tensors of an object with .cdf / .sizes / .offsets host arrays for ops.code_cost,
    cached on it per device (ops.cost_table: built once per table set)."""
    cache = tables.__dict__.setdefault("_cost_dev", {})
    key = str(dev)
    if key not in cache:
        # the layers build a fresh table object per level and call, from the same scale table: a second cache on the content
        # keeps the logarithms and the three uploads out of every encode with rdo and every probe
        import hashlib
        h = hashlib.sha1()
        for a in (tables.cdf, tables.sizes, tables.offsets):
            h.update(np.ascontiguousarray(a, dtype=np.int32).tobytes())
        ckey = (h.digest(), tuple(tables.cdf.shape), key)
        if ckey not in _COST_TABLES:
            if len(_COST_TABLES) >= 16:
                _COST_TABLES.clear()
            arrs = (ops.cost_table(tables.cdf, tables.sizes), tables.sizes, tables.offsets)
            _COST_TABLES[ckey] = tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev) for a in arrs)
        cache[key] = _COST_TABLES[ckey]
    return cache[key]


_COST_TABLES = {}                # (sha1 of cdf | sizes | offsets, cdf shape, device) -> device_cost_tables' tensors


class _CostSink(_DeviceSink):
    """The encoder side of _DeviceSink's interface without a coder: flush() -> per (plane, image) the ESTIMATED stream length
    in bytes, an int where the other sinks give the stream (lldwt_code_cost: the ideal code length under the quantised
    tables, an escape counted as 32 bits, plus the coder's final state)."""

    def __init__(self, P, B, tables, device):
        self.P, self.B, self.t = P, B, tables
        self.decoding = False
        self.ct = device_cost_tables(tables, device)
        self.sym, self.idx = [], []

    def flush(self):
        Z = self.P * self.B
        idx = torch.cat([t.reshape(Z, -1) for t in self.idx], 1).int().contiguous()
        sym = torch.cat([t.reshape(Z, -1) for t in self.sym], 1).int().contiguous()
        sums, _ = ops.code_cost(sym, idx, *self.ct)
        per_byte = 8 * ops.COST_ONE_BIT
        flat = [(v + per_byte - 1) // per_byte + _STREAM_OVERHEAD for v in sums.tolist()]
        return [flat[p * self.B:(p + 1) * self.B] for p in range(self.P)]


def _make_sink(coder, P, B, tables, strings, n, device):
    """The sink of a tensor for the chosen coder (n: symbols per stream; device: where the coder runs)."""
    if coder == ESTIMATE and strings is None:
        return _CostSink(P, B, tables, device)
    if coder == "host":
        return _Sink(P, B, tables, strings)
    if coder == "gpu":
        return _DeviceSink(P, B, tables, strings, n, device)
    raise ValueError("coder must be one of %s (got %r)" % (", ".join(CODERS), coder))


def _rdo_args(rdo, tables, dev):
    """rdo (the Lagrangian rho of DESIGN.md 7.1.7, None or 0: off) -> None or (k, cost, sizes, offsets) for the encoder half of a
    level: k = ops.rdo_scale(rdo) and the device cost tables of the level's CDF tables."""
    if rdo is None or rdo == 0:
        return None
    return (ops.rdo_scale(rdo),) + tuple(device_cost_tables(tables, dev))


def _finish_step(emodel, sink, sigma, mu, yv, step=1.0, rdo=None):
    """sigma, mu (P,B,g,N); yv (P,B,g,N) or None when decoding -> dequantised values (P,B,g,N).  The quantiser of DESIGN.md 7.1.6
    in fp32 tensor ops: the table entered with sigma * inv_q, symbol round((y - mu) * inv_q), value symbol * q + mu.
    step: a number, or a pair (q, inv_q) of fp32 tensors that broadcast against (P,B,g,N) -- the per-pixel pairs gathered from a
    step map (_pixel_pairs); the arithmetic is the same, elementwise.  At the unit step the multiplications by
    1.0f (exact) are left out: the crop stacks always run there, and keep their launch count.
    rdo (encoder only): (k, cost, sizes, offsets) of _rdo_args -- the symbol is chosen by the rule of DESIGN.md 7.1.7, restated
    in tensor ops (ops.rdo_lookup, ops.rdo_choose); the index does not depend on the choice."""
    unit = not isinstance(step, tuple) and step == 1.0
    q, inv_q = (1.0, 1.0) if unit else step if isinstance(step, tuple) else ops.step_pair(step)
    idx = emodel.build_indexes(sigma if unit else sigma * inv_q)                       # (P,B,g,N)
    sym = None
    if yv is not None:
        v = yv - mu if unit else (yv - mu) * inv_q                                      # the rounded fp32 product
        sym = torch.round(v)
        if rdo is not None:
            k, cost, sizes, offsets = rdo
            s1 = sym - torch.sign(sym)
            sym = ops.rdo_choose(v, sym, ops.rdo_lookup(cost, sizes, offsets, idx, sym), ops.rdo_lookup(cost, sizes, offsets, idx, s1), k)
        sym = sym.int().permute(0, 1, 3, 2).contiguous()
    sym = sink.step(idx.permute(0, 1, 3, 2).contiguous(), sym).permute(0, 1, 3, 2).float()      # the sink's layout: (P,B,N,g)
    return sym + mu if unit else sym * q + mu


def _pixel_pairs(smap, h, w):
    """ops.StepMap, pixel coordinates h, w (N) of a level -> (q, inv_q), each (1,B,1,N): the pairs of the pixels' blocks, for
    _finish_step."""
    pr = smap.pairs[:, h >> smap.shift, w >> smap.shift]                              # (B,N,2)
    return pr[None, :, None, :, 0], pr[None, :, None, :, 1]


def code_crop_stack(seq_stack, emodels, seqs, y, shape, tables, strings=None, coder="host"):
    """The 3x3-crop context (LiftingBasedDWT_net.py:388-401 / :424-433 with compress_ar / decompress_ar at
    network_kernel_size 3).  y: (P,B,g,H,W) coefficients (encoder) or None (decoder); -> (strings or None, dequantised)."""
    P, B, g, H, W = shape
    dev = y.device if y is not None else next(seqs[0].parameters()).device
    hs, ws, starts = wavefront(H, W, 2, dev)
    sink = _make_sink(coder, P, B, tables, strings, H * W * g, dev)
    yhat = torch.zeros(P, B, g, H + 2, W + 2, device=dev, dtype=torch.float32)       # 1-pixel zero frame = the crop padding
    ar = torch.arange(3, device=dev)
    for t in range(len(starts) - 1):
        a, b = starts[t], starts[t + 1]
        if a == b:
            continue
        h, w = hs[a:b], ws[a:b]
        N = b - a
        rows = (h[:, None, None] + ar[None, :, None]).expand(N, 3, 3)
        cols = (w[:, None, None] + ar[None, None, :]).expand(N, 3, 3)
        crop = yhat[:, :, :, rows, cols]                                              # (P,B,g,N,3,3)
        crop = crop.permute(0, 1, 3, 2, 4, 5).reshape(P, B * N, g, 3, 3).contiguous()
        ms = seq_stack(seqs, crop)[:, :, :, 1, 1].reshape(P, B, N, 2 * g)             # centre of every crop
        sigma = ms[..., 0::2].permute(0, 1, 3, 2)                                     # (P,B,g,N): even = sigma, odd = mu
        mu = ms[..., 1::2].permute(0, 1, 3, 2)
        yv = y[:, :, :, h, w] if y is not None else None
        yhat[:, :, :, h + 1, w + 1] = _finish_step(emodels[0], sink, sigma, mu, yv)
    out = yhat[:, :, :, 1:-1, 1:-1].contiguous()
    if sink.decoding:
        sink.finish()
    return (None if sink.decoding else sink.flush()), out


def _step_offsets(H, W, slope):
    """starts[t] = number of pixels in the wavefront steps before t (pixels of step t: rows ascending)."""
    h = np.repeat(np.arange(H), W)
    w = np.tile(np.arange(W), H)
    t = np.sort(w + slope * h)
    return np.searchsorted(t, np.arange(W + slope * (H - 1) + 1)).tolist()


def code_tree_level(emodels, plc, packed16, K, tap_bits, y, shape, tables, strings=None, coder="host", step=1.0, rdo=None):
    """A level with tree context + masked KxK context + cgp (:402-417 / :440-454 with kernel size 5).  plc: (P,B,G*81,H,W)
    tree-context features of the (decoded) parent; packed16: the cgp stack with the masked conv folded into its first layer,
    packed for the register-chain kernel (_fold_csc_into_cgp).

    ONE launch per wavefront step (lldwt_cgp16_wavefront_step): the step's pixels are enumerated in the kernel, the causal
    taps are gathered from the decoded-so-far tensor, the cgp chain runs on the matrix cores and the epilogue produces CDF
    index, symbol and dequantised value -- no per-step tensor ops on the host side.  Encoder: the launches are queued back to
    back (no synchronisation until the streams are written).  Decoder: per step one launch, the step's indexes down to the
    host (pinned buffer), ONE C call that pops the step's symbols from every (plane, image) stream (_Sink.pop), the symbols
    up, one small launch that writes symbol * q + mu.  With coder="gpu" the decoder never waits: per step the step kernel, the
    irans32 pop of every stream and the apply launch are queued back to back, and the streams are checked once at the end of
    the level.  One encoder loop and one decoder loop serve every case; what differs is the pair of launchers chosen per level:
    step: the quantisation step q of DESIGN.md 7.1.6 (lldwt_cgp16_wavefront_step_q / lldwt_wavefront_apply_q; the unit step
    goes through them too and gives the bits of the entry points without a step).
    rdo: the Lagrangian of DESIGN.md 7.1.7 (None or 0: off); the encoder's steps then go through
    lldwt_cgp16_wavefront_step_rdo with the level's cost tables, the decoder ignores it.
    step may be an ops.StepMap over the level: every launch then goes through lldwt_cgp16_wavefront_step_map /
    lldwt_wavefront_apply_map, with or without the cost tables."""
    import ctypes as C
    from ... import _lib
    lib = _lib.load()
    P, B, G, H, W = shape
    dev = plc.device
    starts = _step_offsets(H, W, K // 2 + 1)
    nsteps, ntot = len(starts) - 1, H * W
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    table63 = emodels[0].scale_table.to(dev).float()[:63].contiguous()
    yhat = torch.zeros(P, B, G, H, W, device=dev, dtype=torch.float32)
    sink = _make_sink(coder, P, B, tables, strings, ntot * G, dev)
    ptr = lambda t_: C.c_void_p(t_.data_ptr())
    ra = None if sink.decoding else _rdo_args(rdo, tables, dev)
    if ra is not None:
        k, cost, csizes, coffs = ra
        ra = (ptr(cost), ptr(csizes), ptr(coffs), cost.shape[0], cost.shape[1], k)
    # the two launchers of the level.  step_launch: the step kernel on step t -- encoder (yc, sym: all n = ntot pixels of the level
    # are addressed, the step's start at off) or decoder (mu: the step's n pixels, off = 0); apply_launch: symbol * q + mu
    if isinstance(step, ops.StepMap):
        m = ops._map_args(step, B, H, W)
        rdo_or_none = ra or (None, None, None, 0, 0, 0.0)

        def step_launch(yc, idx, sym, mu, t, n, off):
            ops.check(lib.lldwt_cgp16_wavefront_step_map(ptr(plc), ptr(yhat), yc, ptr(packed16), ptr(table63), ptr(idx), sym, mu, None, P, B,
                                                         H, W, G, K, int(tap_bits), t, n, off, *m, *rdo_or_none, st), "cgp16_wavefront_step_map")

        def apply_launch(sym, mu, t, n):
            ops.check(lib.lldwt_wavefront_apply_map(ptr(sym), ptr(mu), ptr(yhat), P, B, H, W, G, K, t, n, 0, *m, st), "wavefront_apply_map")
    else:
        q, inv_q = ops.step_pair(step)

        def step_launch(yc, idx, sym, mu, t, n, off):
            args = (ptr(plc), ptr(yhat), yc, ptr(packed16), ptr(table63), ptr(idx), sym, mu, None, P, B, H, W, G, K, int(tap_bits), t, n,
                    off, q, inv_q)
            if ra is not None:
                ops.check(lib.lldwt_cgp16_wavefront_step_rdo(*args, *ra, st), "cgp16_wavefront_step_rdo")
            else:
                ops.check(lib.lldwt_cgp16_wavefront_step_q(*args, st), "cgp16_wavefront_step")

        def apply_launch(sym, mu, t, n):
            ops.check(lib.lldwt_wavefront_apply_q(ptr(sym), ptr(mu), ptr(yhat), P, B, H, W, G, K, t, n, 0, q, inv_q, st), "wavefront_apply")

    if not sink.decoding:
        yc = y.contiguous()
        idx_all = torch.empty(P, B, ntot, G, device=dev, dtype=torch.int32)
        sym_all = torch.empty(P, B, ntot, G, device=dev, dtype=torch.int32)
        for t in range(nsteps):
            step_launch(ptr(yc), idx_all, ptr(sym_all), None, t, ntot, starts[t])
        sink.idx, sink.sym = [idx_all], [sym_all]
        return sink.flush(), yhat
    nmax = max(starts[t + 1] - starts[t] for t in range(nsteps))
    Z = P * B
    idx_d = torch.empty(Z * nmax * G, device=dev, dtype=torch.int32)
    sym_d = torch.empty(Z * nmax * G, device=dev, dtype=torch.int32)
    mu_d = torch.empty(Z * G * nmax, device=dev, dtype=torch.float32)
    host = coder != "gpu"
    if host:
        idx_h = torch.empty(Z * nmax * G, dtype=torch.int32).pin_memory()
        sym_h = torch.empty(Z * nmax * G, dtype=torch.int32).pin_memory()
    for t in range(nsteps):
        n = starts[t + 1] - starts[t]
        if n == 0:
            continue
        step_launch(None, idx_d, None, ptr(mu_d), t, n, 0)
        if host:
            cnt = Z * n * G
            idx_h[:cnt].copy_(idx_d[:cnt], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            sink.pop(idx_h.data_ptr(), n * G, sym_h.data_ptr())
            sink.note(idx_h[:cnt].numpy(), sym_h[:cnt].numpy())
            sym_d[:cnt].copy_(sym_h[:cnt], non_blocking=True)
        else:
            sink.dec.pop(idx_d, n * G, n * G, sym_d)
        apply_launch(sym_d, mu_d, t, n)
    sink.finish()
    return None, yhat


def code_tree_level_generic(emodels, plc, cgp_packed, cgp_dims, K, tap_bits, y, shape, tables, strings=None, coder="host",
                            step=1.0, rdo=None):
    """A level with tree context + masked KxK context + cgp (:402-417 / :440-454 with kernel size 5).  plc: (P,B,G*81,H,W)
    tree-context features of the (decoded) parent; cgp_packed/dims: the cgp stack with the masked conv folded into its
    first layer (_fold_csc_into_cgp).  The host-stepped schedule (a handful of tensor ops and launches per step) for cgp widths
    other than the reference's 93 -> 162 -> 54 -> 18 -> 2, which the fused step kernel of code_tree_level is built for.
    step may be an ops.StepMap over the level: each step gathers its pixels' pairs from it (_pixel_pairs)."""
    P, B, G, H, W = shape
    dev = plc.device
    R = K // 2
    taps = _live_taps(tap_bits, K)
    cpl = plc.shape[2] // G
    hs, ws, starts = wavefront(H, W, R + 1, dev)
    sink = _make_sink(coder, P, B, tables, strings, H * W * G, dev)
    ra = None if sink.decoding else _rdo_args(rdo, tables, dev)
    if isinstance(step, ops.StepMap):
        ops._map_args(step, B, H, W)                                                        # the map must cover the level
    yhat = torch.zeros(P, B, G, H + 2 * R, W + 2 * R, device=dev, dtype=torch.float32)
    dy = torch.tensor([t[0] for t in taps], device=dev)
    dx = torch.tensor([t[1] for t in taps], device=dev)
    for t in range(len(starts) - 1):
        a, b = starts[t], starts[t + 1]
        if a == b:
            continue
        h, w = hs[a:b], ws[a:b]
        N = b - a
        ctx = yhat[:, :, :, h[None, :] + dy[:, None], w[None, :] + dx[:, None]]       # (P,B,G,ntaps,N): causal neighbours
        feat = plc[:, :, :, h, w].reshape(P, B, G, cpl, N)                            # (P,B,G,81,N)
        cat = torch.cat((feat, ctx), 3).reshape(P, B, G * (cpl + len(taps)), 1, N).contiguous()
        yv = y[:, :, :, h, w] if y is not None else None
        xarg = (yv if yv is not None else torch.zeros(P, B, G, N, device=dev)).reshape(P, B, G, 1, N).contiguous()
        _, params = ops.cgp_rate(cat, xarg, cgp_packed, cgp_dims, want_params=True)   # (P,B,2G,1,N)
        sigma, mu = params[:, :, 0::2, 0, :], params[:, :, 1::2, 0, :]
        yhat[:, :, :, h + R, w + R] = _finish_step(emodels[0], sink, sigma, mu, yv,
                                                   _pixel_pairs(step, h, w) if isinstance(step, ops.StepMap) else step, ra)
    out = yhat[:, :, :, R:-R, R:-R].contiguous()
    if sink.decoding:
        sink.finish()
    return (None if sink.decoding else sink.flush()), out


ZT_PHASES = ((0, 0), (0, 1), (1, 0), (1, 1))        # ee, eo, oe, oo: (row, column) offset of phase k in the level


def code_ztblock_level(emodels, packs, parent, y, shape, tables, strings=None, coder="host", step=1.0, rdo=None):
    """One finer level of DWTConditioned2EntropyLayerZTBlock (the reference's forward, LiftingBasedDWT_net.py:716-744, coded
    with compressai's GaussianConditional contract).  parent (P,B,3,h,w): the DECODED coarser level; y (P,B,3,2h,2w) the
    coefficients (encoder) or None (decoder); emodels: the GaussianConditional of each subband (build_indexes); packs[k]:
    ops.ztblock_pack of the phase-(k+1) nets.

    The four phases ee, eo, oe, oo run in sequence; each is ONE launch of lldwt_ztblock_phase for every plane, image and
    subband (its contexts are the parent and the phases already decoded, round(y - mu) + mu), then one pass of the range
    coder over every stream.  Symbols inside a stream: phase ascending, then subband, then raster order over the phase grid.
    Index, symbol and the dequantised value written into the phase's positions of the level are one launch of
    lldwt_gauss_quantise per phase (two in the decoder: the indexes before the symbols are popped, the values after), with
    the quantisation step of DESIGN.md 7.1.6; the three subbands' models carry one scale table.  rdo: the Lagrangian of DESIGN.md
    7.1.7 for the encoder's launches (None or 0: off); the decoder ignores it.  step may be an ops.StepMap over the level
    (lldwt_gauss_quantise_map forms each phase position's block).
    -> (strings or None, dequantised (P,B,3,2h,2w))."""
    P, B, G, H, W = shape
    h2, w2 = H // 2, W // 2
    lev = torch.zeros(P, B, G, H, W, device=parent.device, dtype=torch.float32)
    sink = _make_sink(coder, P, B, tables, strings, G * H * W, parent.device)
    table63 = emodels[0].scale_table.to(parent.device).float()[:63].contiguous()
    ra = None if y is None else _rdo_args(rdo, tables, parent.device)
    for k, (r, c) in enumerate(ZT_PHASES):
        params = ops.ztblock_phase(parent, lev, packs[k], k + 1)
        if y is not None:
            idx, sym = ops.gauss_quantise(params, table63, lev, r, c, 2, step, y=y, rdo=ra)
            sink.step(idx.reshape(P, B, G * h2 * w2, 1), sym.reshape(P, B, G * h2 * w2, 1))
        else:
            idx, _ = ops.gauss_quantise(params, table63, None, r, c, 2, step)
            sym = sink.step(idx.reshape(P, B, G * h2 * w2, 1))
            ops.gauss_quantise(params, table63, lev, r, c, 2, step, sym=sym.int().contiguous())
    if sink.decoding:
        sink.finish()
    return (None if sink.decoding else sink.flush()), lev


class _FactorizedTables:
    """The per-channel CDF tables of one EntropyBottleneck as host int32 arrays."""

    def __init__(self, emodel):
        emodel.update()
        self.cdf = emodel.quantized_cdf.cpu().numpy().astype(np.int32)
        self.sizes = emodel.cdf_length.cpu().numpy().astype(np.int32)
        self.offsets = emodel.offset.cpu().numpy().astype(np.int32)


def code_factorized(emodels, y, shape, strings=None, coder="host"):
    """A tensor coded with a factorized prior (EntropyBottleneck; compressai compress / decompress): every coefficient is
    independent, so symbols and indexes of the whole tensor are produced in one pass; one rANS stream per (plane, image),
    raster order, channels outermost.  emodels: one per plane.  -> (strings or None, dequantised (P,B,C,h,w)).
    coder="gpu": symbols and indexes stay on the device (irans32)."""
    P, B, Cc, H, W = shape
    if coder != "host":
        return _code_factorized_device(emodels, y, shape, strings, coder)
    out = []
    strs = []
    for p in range(P):
        em = emodels[p]
        tabs = _FactorizedTables(em)
        if strings is None:
            sym, idx = em.symbols_and_indexes(y[p])                                     # (B,C,h,w)
            sh, ih = sym.cpu().numpy(), idx.cpu().numpy()
            strs.append(encode_streams(sh.reshape(B, -1), ih.reshape(B, -1), tabs.cdf, tabs.sizes, tabs.offsets))
            out.append(em.dequantize_symbols(sym))
        else:
            dev = em.quantiles.device
            idx = np.broadcast_to(np.arange(Cc, dtype=np.int32).reshape(1, Cc, 1, 1), (B, Cc, H, W)).reshape(B, -1)
            syms = decode_streams(strings[p], idx, tabs.cdf, tabs.sizes, tabs.offsets).reshape(B, Cc, H, W)
            out.append(em.dequantize_symbols(torch.from_numpy(syms).to(dev)))
    return (strs if strings is None else None), torch.stack(out, 0)


def _code_factorized_device(emodels, y, shape, strings, coder):
    P, B, Cc, H, W = shape
    out, strs = [], []
    for p in range(P):
        em = emodels[p]
        dev = em.quantiles.device
        tabs = _FactorizedTables(em)
        if strings is None:
            sym, idx = em.symbols_and_indexes(y[p])                                     # (B,C,h,w)
            sink = _make_sink(coder, 1, B, tabs, None, None, dev)
            sink.step(idx.int().reshape(1, B, -1), sym.int().reshape(1, B, -1))
            strs.append(sink.flush()[0])
            out.append(em.dequantize_symbols(sym))
        else:
            sink = _make_sink(coder, 1, B, tabs, [strings[p]], Cc * H * W, dev)
            idx = torch.arange(Cc, device=dev, dtype=torch.int32).reshape(1, Cc, 1, 1).expand(B, Cc, H, W).contiguous()
            syms = sink.step(idx)
            sink.finish()
            out.append(em.dequantize_symbols(syms))
    return (strs if strings is None else None), torch.stack(out, 0)


def code_gaussian_parallel(emodels, params, y, shape, tables, strings=None, coder="host", step=1.0, rdo=None):
    """A level whose (sigma, mu) depend only on already decoded tensors (onlyEZWT: the tree context of the parent level,
    LiftingBasedDWT_net.py:822-835): fully parallel -- indexes and symbols of the whole tensor in one pass, raster order.
    params (P,B,2C,h,w): sigma on the even, mu on the odd channels.  rdo: the Lagrangian of DESIGN.md 7.1.7 for the encoder's
    launch (None or 0: off); the decoder ignores it.  step: a number or an ops.StepMap over the level.
    -> (strings or None, dequantised (P,B,C,h,w))."""
    P, B, Cc, H, W = shape
    params = params.contiguous()
    table63 = emodels[0].scale_table.to(params.device).float()[:63].contiguous()
    out = torch.empty(P, B, Cc, H, W, device=params.device, dtype=torch.float32)
    if strings is None:                                 # index, symbol and value of the whole level: one launch
        idx, sym = ops.gauss_quantise(params, table63, out, 0, 0, 1, step, y=y.contiguous(),
                                      rdo=_rdo_args(rdo, tables, params.device))
    else:
        idx, _ = ops.gauss_quantise(params, table63, None, 0, 0, 1, step)
    if coder != "host":
        sink = _make_sink(coder, P, B, tables, strings, Cc * H * W, params.device)
        if strings is None:
            sink.step(idx, sym)
            return sink.flush(), out
        syms = sink.step(idx)
        sink.finish()
        ops.gauss_quantise(params, table63, out, 0, 0, 1, step, sym=syms.int().contiguous())
        return None, out
    ih = idx.cpu().numpy()
    if strings is None:
        sh = sym.cpu().numpy()
        flat = encode_streams(sh.reshape(P * B, -1), ih.reshape(P * B, -1), tables.cdf, tables.sizes, tables.offsets)
        return [flat[p * B:(p + 1) * B] for p in range(P)], out
    syms = decode_streams([strings[p][b] for p in range(P) for b in range(B)], ih.reshape(P * B, -1), tables.cdf,
                          tables.sizes, tables.offsets).reshape(ih.shape)
    ops.gauss_quantise(params, table63, out, 0, 0, 1, step, sym=torch.from_numpy(syms).to(params.device).int().contiguous())
    return None, out


def ideal_bits(sym, idx, tables):
    """Code length (bits) of integer symbols under the quantised tables; escapes are not modelled (returns their count)."""
    cdf, sizes, offs = tables.cdf, tables.sizes, tables.offsets
    v = sym - offs[idx]
    inside = (v >= 0) & (v < sizes[idx] - 2)
    vi = np.where(inside, v, 0)
    freq = cdf[idx, vi + 1] - cdf[idx, vi]
    return float(-np.log2(freq[inside] / 65536.0).sum()), int((~inside).sum())
