"""Host rANS: time one lldwt_rans_decode_multi call (and lldwt_rans_encode_multi) sequential vs on the stream pool, over a
sweep of stream counts and symbols per stream -- the measurement behind the pool's per-call symbol threshold
(csrc/rans.hip kParallelMinSymbols).  Prints one JSON line per case: best of --reps of the mean over a batch of calls."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import _lib, ans  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="3,12,48,96,120")
    ap.add_argument("--symbols", default="16,64,256,1024,4096,16384")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    lib = _lib.load()
    g = np.random.default_rng(0)
    # a Gaussian-like table set: 64 CDFs of 3..60 slots
    cdfs, sizes, offs = [], [], []
    for i in range(64):
        n = 3 + i
        pmf = np.exp(-0.5 * ((np.arange(n) - n / 2) / (1 + i / 4)) ** 2).astype(np.float32) + 1e-6
        c = ans.pmf_to_quantized_cdf((pmf / pmf.sum()).tolist())
        cdfs.append(c)
        sizes.append(len(c))
        offs.append(-(n // 2))
    cdf, sz, of = ans._tables(cdfs, sizes, offs)
    for S in (int(v) for v in a.streams.split(",")):
        for n in (int(v) for v in a.symbols.split(",")):
            idx = g.integers(0, 64, (S, n)).astype(np.int32)
            sym = (np.round(g.normal(0, 2, (S, n))).astype(np.int32))
            ans.set_parallel(1)
            strs = ans.encode_streams(sym, idx, cdfs, sizes, offs)
            calls = max(2, 400000 // (S * n))
            res = {"streams": S, "symbols_per_stream": n, "symbols": S * n}
            for name, threads in (("seq", 1), ("pool", 0)):
                ans.set_parallel(threads, 0)              # pool: the default thread rule, threshold 0
                best_d = best_e = 1e9
                for _ in range(a.reps):
                    decs = []
                    for _ in range(calls):
                        ds = [ans.RansDecoder() for _ in range(S)]
                        for d, st in zip(ds, strs):
                            d.set_stream(st)
                        decs.append((ds, (C.c_void_p * S)(*[d._h for d in ds])))
                    out = np.empty_like(idx)
                    t0 = time.perf_counter()
                    for _, h in decs:
                        lib.lldwt_rans_decode_multi(h, S, ans._p(idx), n, n, ans._p(cdf), cdf.shape[0], cdf.shape[1],
                                                    ans._p(sz), ans._p(of), ans._p(out))
                    best_d = min(best_d, (time.perf_counter() - t0) / calls)
                    assert np.array_equal(out, sym)
                    t0 = time.perf_counter()
                    for _ in range(max(1, calls // 4)):
                        got = ans.encode_streams(sym, idx, cdfs, sizes, offs)
                    best_e = min(best_e, (time.perf_counter() - t0) / max(1, calls // 4))
                    assert got == strs
                res[name + "_decode_us"] = best_d * 1e6
                res[name + "_encode_us"] = best_e * 1e6
            res["decode_speedup"] = res["seq_decode_us"] / res["pool_decode_us"]
            res["encode_speedup"] = res["seq_encode_us"] / res["pool_encode_us"]
            print(json.dumps(res), flush=True)
    ans.set_parallel(0, -1)


if __name__ == "__main__":
    main()
