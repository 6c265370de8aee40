// rans_gpu.hip -- the interleaved rANS coder "irans32" (DESIGN.md 7.1.2): encoder and decoder as kernels, one wave per stream.
//
// A stream of n symbols is split into K = lanes(n) rANS lanes (symbol i -> lane i mod K).  Each lane is a 32-bit state in
// [2^23, 2^31) with byte-wise renormalisation at precision 16; all lanes share one byte sequence.  The byte order is the
// symbol order: the decoder reads symbol i's renormalisation bytes, then those of its bypass digits (escapes), then symbol
// i + 1's.  It depends on symbol positions only, so a wavefront step may start or end anywhere inside a round of K symbols.
// The definition is tools/irans_ref.py; the tests pin these kernels' bytes and symbols to it.
//
// Encoder: the wave walks rounds of K symbols from last to first.  Every lane codes its symbol on a copy of its state to
// count the bytes it emits, a suffix sum over the lanes places them (lane K-1 emits first), and a second pass writes them
// from the end of the stream's buffer downwards.  x / freq uses a reciprocal table (no integer divide on gfx950).
// Decoder: per round every active lane decodes its regular code (coarse LUT + binary search in the CDF row) and knows how
// many renormalisation bytes it needs without reading them; an exclusive prefix sum gives each lane its offset.  A lane
// with an escape splits the round: the lanes up to it renormalise, it reads its bypass digits alone, and the rest follow
// at the new cursor.  Lane states and the cursor persist in a device buffer between launches.
#include "common.h"

namespace {

constexpr uint32_t kL = 1u << 23;
constexpr int kMaxLanes = 32;
constexpr int kStateWords = 34;          // per stream: x[32], cursor low, cursor high
constexpr int kLutBuckets = 256;         // LUT row: kLutBuckets + 1 entries

__host__ __device__ inline int lanes_of(int64_t n) {
    const int64_t q = n >> 12;
    int k = 1;
    while (k < kMaxLanes && 2 * k <= q) k *= 2;
    return k;
}

struct Tabs {
    const int32_t* cdf;
    const int32_t* sizes;
    const int32_t* offs;
    int32_t ncdf, stride;
};

__device__ inline uint32_t div_freq(uint32_t x, uint32_t freq, const uint32_t* rcp) {
    if (freq == 1) return x;
    const uint32_t shift = 32 - __clz(freq - 1);                         // ceil(log2(freq)), freq >= 2
    return (uint32_t)(((uint64_t)x * rcp[freq]) >> 32) >> (shift - 1);
}

// Codes one symbol into state x (codes in reverse: raw digits, count digit, regular code).  kWrite: byte c goes to dst[-1-c].
template <bool kWrite>
__device__ inline int enc_symbol(uint32_t& x, uint32_t start, uint32_t freq, bool esc, uint32_t raw, int nb, const uint32_t* rcp,
                                 uint8_t* dst) {
    int c = 0;
    auto put = [&](uint32_t st, uint32_t fr) {
        const uint32_t xmax = fr << 15;                                  // ((L >> 16) << 8) * freq
        while (x >= xmax) {
            if (kWrite) dst[-1 - c] = (uint8_t)(x & 0xFF);
            ++c;
            x >>= 8;
        }
        const uint32_t q = div_freq(x, fr, rcp);
        x = (q << 16) + (x - q * fr) + st;
    };
    if (esc) {
        for (int k = nb - 1; k >= 0; --k) put(((raw >> (4 * k)) & 15u) << 12, 4096u);
        put((uint32_t)nb << 12, 4096u);                                  // nb <= 8: one count digit
    }
    put(start, freq);
    return c;
}

__global__ __launch_bounds__(64) void k_irans_encode(const int32_t* __restrict__ sym, const int32_t* __restrict__ idx, int64_t n,
                                                     int64_t stride, Tabs t, const uint32_t* __restrict__ rcp, uint8_t* out,
                                                     int64_t cap, int64_t* lens, int32_t* flag) {
    const int z = blockIdx.x, lane = threadIdx.x;
    const int K = lanes_of(n);
    const int32_t* S = sym + (int64_t)z * stride;
    const int32_t* I = idx + (int64_t)z * stride;
    uint8_t* O = out + (int64_t)z * cap;
    uint32_t x = kL;
    int64_t wp = cap;                                                    // bytes [wp, cap) are written
    bool ok = true;
    for (int64_t r = (n + K - 1) / K - 1; r >= 0; --r) {
        const int64_t i = r * K + lane;
        const bool act = lane < K && i < n;
        uint32_t start = 0, freq = 1, raw = 0;
        int nb = 0;
        bool esc = false, bad = false;
        if (act) {
            const int32_t ci = I[i];
            bad = ci < 0 || ci >= t.ncdf;
            if (!bad) {
                const int32_t* row = t.cdf + (int64_t)ci * t.stride;
                const int32_t maxv = t.sizes[ci] - 2;
                bad = maxv < 0 || maxv + 1 >= t.stride;
                if (!bad) {
                    int64_t v = (int64_t)S[i] - t.offs[ci];
                    if (v < 0) {
                        raw = (uint32_t)(-2 * v - 1);
                        v = maxv;
                    } else if (v >= maxv) {
                        raw = (uint32_t)(2 * (v - maxv));
                        v = maxv;
                    }
                    esc = v == maxv;
                    start = (uint32_t)row[v];
                    freq = (uint32_t)(row[v + 1] - row[v]);
                    bad = freq == 0 || freq > 65536u;
                    while (esc && nb < 8 && (raw >> (4 * nb)) != 0) ++nb;
                }
            }
        }
        if (__any(bad)) {
            ok = false;
            break;
        }
        uint32_t xs = x;
        const int c = act ? enc_symbol<false>(xs, start, freq, esc, raw, nb, rcp, nullptr) : 0;
        int incl = c;                                                    // sum of c over lanes >= this one
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_down(incl, d, 64);
            if (lane + d < 64) incl += v;
        }
        const int total = __shfl(incl, 0, 64);
        if (wp - total < 4 * K) {                                        // no room for the bytes and the final states
            ok = false;
            break;
        }
        if (act) enc_symbol<true>(x, start, freq, esc, raw, nb, rcp, O + wp - (incl - c));
        wp -= total;
    }
    if (ok) {
        const int64_t base = wp - 4 * K;
        if (lane < K)
            for (int b = 0; b < 4; ++b) O[base + 4 * lane + b] = (uint8_t)(x >> (8 * b));
        if (lane == 0) lens[z] = cap - base;
    } else if (lane == 0) {
        lens[z] = -1;
        atomicOr(flag, 1);
    }
}

__global__ __launch_bounds__(64) void k_irans_decode(uint32_t* state, const uint8_t* __restrict__ bytes,
                                                     const int64_t* __restrict__ boffs, const int64_t* __restrict__ blens,
                                                     int64_t n, int64_t pos, int64_t cnt, const int32_t* __restrict__ idx,
                                                     int64_t istride, int32_t* out, int64_t ostride, Tabs t,
                                                     const int32_t* __restrict__ lut, int32_t* flag) {
    const int z = blockIdx.x, lane = threadIdx.x;
    const int K = lanes_of(n);
    const uint8_t* B = bytes + boffs[z];
    const int64_t len = blens[z];
    uint32_t* st = state + (int64_t)z * kStateWords;
    bool bad = false;
    auto rd = [&](int64_t off) -> uint32_t {
        if (off >= len) {
            bad = true;
            return 0u;
        }
        return B[off];
    };
    uint32_t x = kL;
    int64_t cur;
    if (pos == 0) {
        cur = 4 * K;
        if (len < 4 * K)
            bad = true;
        else if (lane < K)
            x = rd(4 * lane) | (rd(4 * lane + 1) << 8) | (rd(4 * lane + 2) << 16) | (rd(4 * lane + 3) << 24);
    } else {
        if (lane < K) x = st[lane];
        cur = (int64_t)((uint64_t)st[kMaxLanes] | ((uint64_t)st[kMaxLanes + 1] << 32));
    }
    const int32_t* I = idx + (int64_t)z * istride;
    int32_t* O = out + (int64_t)z * ostride;
    const int64_t end = pos + cnt;
    for (int64_t i = pos; i < end;) {
        const int64_t r0 = i - i % K;
        const int a = (int)(i - r0);
        const int b = (int)min<int64_t>(K, end - r0);
        const bool act = lane >= a && lane < b;
        const int64_t si = r0 + lane;
        int32_t ci = 0, s = 0, maxv = 0;
        int need = 0;
        if (act) {
            ci = I[si - pos];
            if (ci < 0 || ci >= t.ncdf) {
                bad = true;
                ci = 0;
            }
            const int32_t* row = t.cdf + (int64_t)ci * t.stride;
            maxv = t.sizes[ci] - 2;
            const uint32_t cum = x & 0xFFFFu;
            const int32_t* L = lut + (int64_t)ci * (kLutBuckets + 1);
            int lo = L[cum >> 8], hi = L[(cum >> 8) + 1];                 // the slot of cum lies in [lo, hi]
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if ((uint32_t)row[mid] <= cum)
                    lo = mid;
                else
                    hi = mid - 1;
            }
            s = lo;
            const uint32_t start = (uint32_t)row[s], freq = (uint32_t)(row[s + 1] - row[s]);
            x = freq * (x >> 16) + cum - start;
            if (x < (1u << 7)) {                                         // never on a valid stream: stop here, bounded
                bad = true;
                x = kL;
            }
            need = x < (1u << 15) ? 2 : (x < kL ? 1 : 0);
        }
        uint64_t emask = __ballot(act && s == maxv);
        int done = a;
        int32_t value = s;
        for (;;) {
            const int e = emask ? __ffsll((long long)emask) - 1 : b;
            const int last = e < b ? e : b - 1;
            const bool seg = lane >= done && lane <= last;
            const int v = seg ? need : 0;
            int incl = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int u = __shfl_up(incl, d, 64);
                if (lane >= d) incl += u;
            }
            const int total = __shfl(incl, 63, 64);
            if (seg)
                for (int k = 0, off = incl - v; k < v; ++k) x = (x << 8) | rd(cur + off + k);
            cur += total;
            if (e >= b) break;
            if (lane == e) {                                             // the escape: bypass digits, this lane alone
                auto digit = [&]() -> uint32_t {
                    const uint32_t d = (x & 0xFFFFu) >> 12;
                    x = 4096u * (x >> 16) + (x & 0xFFFu);
                    for (int k = 0; k < 3 && x < kL; ++k) x = (x << 8) | rd(cur++);
                    if (x < kL) bad = true;
                    return d;
                };
                uint32_t d = digit();
                int nb = (int)d;
                while (d == 15u && nb <= 8) {
                    d = digit();
                    nb += (int)d;
                }
                if (nb > 8) {
                    bad = true;
                    nb = 0;
                }
                uint32_t raw = 0;
                for (int k = 0; k < nb; ++k) raw |= digit() << (4 * k);
                value = (int32_t)(raw >> 1);
                value = (raw & 1u) ? -value - 1 : value + maxv;
            }
            const int lo32 = __shfl((int)(uint32_t)cur, e, 64);
            const int hi32 = __shfl((int)(uint32_t)((uint64_t)cur >> 32), e, 64);
            cur = (int64_t)(((uint64_t)(uint32_t)hi32 << 32) | (uint32_t)lo32);
            emask &= emask - 1;
            done = e + 1;
        }
        if (act) O[si - pos] = value + t.offs[ci];
        i = r0 + b;
    }
    if (lane < K) st[lane] = x;
    if (lane == 0) {
        st[kMaxLanes] = (uint32_t)cur;
        st[kMaxLanes + 1] = (uint32_t)((uint64_t)cur >> 32);
    }
    if (end == n && ((lane < K && x != kL) || cur != len)) bad = true;  // the last symbol: lanes back at L, stream used up
    if (__any(bad) && lane == 0) atomicOr(flag, 1);
}

}  // namespace

extern "C" int lldwt_irans_lanes(int64_t n) { return lanes_of(n); }

extern "C" int64_t lldwt_irans_capacity(int64_t n) { return 8 * n + 4 * kMaxLanes + 16; }

extern "C" int lldwt_irans_state_words(void) { return kStateWords; }

// rcp[f] for f in [2, 65536] (rcp[0] = rcp[1] = 0): ceil(2^(31 + ceil(log2 f)) / f), so that for x < 2^31
// x / f == ((x * rcp[f]) >> 32) >> (ceil(log2 f) - 1).
extern "C" int lldwt_irans_rcp_table(uint32_t* rcp) {
    LLDWT_REQUIRE(rcp, "irans_rcp_table: bad arguments");
    rcp[0] = rcp[1] = 0;
    for (uint32_t f = 2; f <= 65536u; ++f) {
        uint32_t shift = 0;
        while (f > (1u << shift)) ++shift;
        rcp[f] = (uint32_t)(((1ull << (shift + 31)) + f - 1) / f);
    }
    return LLDWT_OK;
}

// lut[(ci, b)] for b in [0, 256]: the largest slot s in [0, sizes[ci] - 2] with cdf[ci][s] <= 256 b.
extern "C" int lldwt_irans_lut(const int32_t* cdfs, int32_t ncdf, int32_t cdf_stride, const int32_t* cdf_sizes, int32_t* lut) {
    LLDWT_REQUIRE(cdfs && cdf_sizes && lut && ncdf > 0 && cdf_stride > 1, "irans_lut: bad arguments");
    for (int32_t r = 0; r < ncdf; ++r) {
        const int32_t* row = cdfs + (int64_t)r * cdf_stride;
        const int32_t maxv = cdf_sizes[r] - 2;
        LLDWT_REQUIRE(maxv >= 0 && maxv + 1 < cdf_stride, "irans_lut: bad cdf size %d", cdf_sizes[r]);
        int32_t s = 0;
        for (int b = 0; b <= kLutBuckets; ++b) {
            while (s < maxv && row[s + 1] <= 256 * b) ++s;
            lut[(int64_t)r * (kLutBuckets + 1) + b] = s;
        }
    }
    return LLDWT_OK;
}

extern "C" int lldwt_irans_encode(const int32_t* symbols, const int32_t* indexes, int64_t nstreams, int64_t n, int64_t stride,
                                  const int32_t* cdfs, int32_t ncdf, int32_t cdf_stride, const int32_t* cdf_sizes,
                                  const int32_t* offsets, const uint32_t* rcp, uint8_t* out, int64_t out_stride, int64_t* nbytes,
                                  int32_t* flag, void* stream) {
    LLDWT_REQUIRE(symbols && indexes && cdfs && cdf_sizes && offsets && rcp && out && nbytes && flag && nstreams > 0 &&
                      nstreams <= 65535 && n >= 0 && stride >= n && ncdf > 0 && cdf_stride > 1,
                  "irans_encode: bad arguments");
    LLDWT_REQUIRE(out_stride >= lldwt_irans_capacity(n), "irans_encode: out_stride %lld < capacity %lld", (long long)out_stride,
                  (long long)lldwt_irans_capacity(n));
    Tabs t{cdfs, cdf_sizes, offsets, ncdf, cdf_stride};
    hipLaunchKernelGGL(k_irans_encode, dim3((unsigned)nstreams), dim3(64), 0, (hipStream_t)stream, symbols, indexes, n, stride, t,
                       rcp, out, out_stride, nbytes, flag);
    return lldwt::check_launch("irans_encode");
}

extern "C" int lldwt_irans_decode(uint32_t* state, const uint8_t* bytes, const int64_t* byte_offsets, const int64_t* byte_lengths,
                                  int64_t nstreams, int64_t n, int64_t pos, int64_t cnt, const int32_t* indexes, int64_t idx_stride,
                                  int32_t* symbols, int64_t sym_stride, const int32_t* cdfs, int32_t ncdf, int32_t cdf_stride,
                                  const int32_t* cdf_sizes, const int32_t* offsets, const int32_t* lut, int32_t* flag,
                                  void* stream) {
    LLDWT_REQUIRE(state && bytes && byte_offsets && byte_lengths && cdfs && cdf_sizes && offsets && lut && flag && nstreams > 0 &&
                      nstreams <= 65535 && n >= 0 && pos >= 0 && cnt >= 0 && pos + cnt <= n && ncdf > 0 && cdf_stride > 1,
                  "irans_decode: bad arguments");
    if (cnt == 0) return LLDWT_OK;
    LLDWT_REQUIRE(indexes && symbols && idx_stride >= cnt && sym_stride >= cnt, "irans_decode: bad index / symbol arrays");
    Tabs t{cdfs, cdf_sizes, offsets, ncdf, cdf_stride};
    hipLaunchKernelGGL(k_irans_decode, dim3((unsigned)nstreams), dim3(64), 0, (hipStream_t)stream, state, bytes, byte_offsets,
                       byte_lengths, n, pos, cnt, indexes, idx_stride, symbols, sym_stride, t, lut, flag);
    return lldwt::check_launch("irans_decode");
}
