// quant.hip -- variable-rate coding: the Gaussian quantiser with a step as ONE launch per ZTBlock phase / onlyEZWT
// level, and the code length of (symbol, index) streams under the quantised tables for the byte-target search.  gfx950 only.
#include "common.h"

using namespace lldwt;

namespace {

constexpr int NT = 256;
constexpr int NTABLE = 63;                       // scale-table entries the CDF index counts over (the 64th is the catch-all)

struct QuantArgs {
    const float* params;                         // (Z, 2C, h, w): sigma of channel c on 2c, mu on 2c + 1
    const float* y;                              // encoder: (Z, C, H, W) coefficients, read at (r0 + s i, c0 + s j); decoder: null
    const int* sym_in;                           // decoder: (Z, C, h, w) symbols; both null: the indexes only (level null too)
    const float* table;                          // NTABLE floats
    int* idx;                                    // (Z, C, h, w) CDF indexes
    int* sym_out;                                // encoder: (Z, C, h, w) symbols
    float* level;                                // (Z, C, H, W): receives symbol * q + mu at (r0 + s i, c0 + s j), nothing elsewhere
    int C, h, w, H, W, r0, c0, s;
    int lvec;                                    // VEC 4: the four level elements of a thread are one aligned float4 (s == 1)
    float q, inv_q;
    RdoTables rdo;                               // RDO (lldwt_gauss_quantise_rdo): the code-length tables and k of DESIGN.md 7.1.7
    // MAP (lldwt_gauss_quantise_map): (units, mh, mw, 2) fp32 pairs (q, inv_q), one per block of 2^shift x 2^shift
    // level positions; stream z reads the map of unit z % units.  q, inv_q above are not read.
    const float* qpairs;
    int units, mh, mw, shift;
};

// the normative quantiser (the epilogue of k_cgp16's wavefront mode, csrc/cgp_f16x3.hip, is the same three lines)
__device__ __forceinline__ int cdf_index(float sigma, float inv_q, const float (&tab)[NTABLE]) {
    const float sb = fmaxf(sigma * inv_q, 0.11f);
    int n = 0;
#pragma unroll
    for (int k = 0; k < NTABLE; ++k) n += tab[k] < sb ? 1 : 0;
    return n;
}

// RDO: the encoder's symbol is chosen by rdo_symbol (common.h) between the nearest level and the one next to it toward zero
// MAP: every element takes the pair of its block of the step map instead of the launch's one pair; the arithmetic is the same
template <int VEC, bool RDO = false, bool MAP = false>
__global__ __launch_bounds__(NT) void k_gauss_quantise(QuantArgs a) {
    const int64_t hw = (int64_t)a.h * a.w;
    const int64_t v = ((int64_t)blockIdx.x * NT + threadIdx.x) * VEC;          // first element of this thread inside the (z, c) grid
    if (v >= hw) return;
    float tab[NTABLE];                                                          // uniform addresses: read once per wave
#pragma unroll
    for (int k = 0; k < NTABLE; ++k) tab[k] = a.table[k];
    const int64_t zc = blockIdx.y, z = zc / a.C;
    const int c = (int)(zc - z * a.C);
    const float* sg = a.params + ((z * 2 * a.C + 2 * c) * hw + v);
    const int i = (int)(v / a.w), j = (int)(v - (int64_t)i * a.w);               // VEC 4: w % 4 == 0, the four share the row
    const int64_t lv = zc * a.H * a.W + (int64_t)(a.r0 + a.s * i) * a.W + a.c0 + a.s * j;
    float sigma[VEC], mu[VEC], val[VEC], q[VEC], inv_q[VEC];
    int sym[VEC], idx[VEC];
    if constexpr (MAP) {                                                        // the host checked that the map covers the level
        const float* row = a.qpairs + ((int64_t)(z % a.units) * a.mh + ((a.r0 + a.s * i) >> a.shift)) * a.mw * 2;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float2 pr = *reinterpret_cast<const float2*>(row + 2 * ((a.c0 + a.s * (j + e)) >> a.shift));
            q[e] = pr.x;
            inv_q[e] = pr.y;
        }
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            q[e] = a.q;
            inv_q[e] = a.inv_q;
        }
    }
    if constexpr (VEC == 4) {
        const float4 s4 = *reinterpret_cast<const float4*>(sg), m4 = *reinterpret_cast<const float4*>(sg + hw);
        sigma[0] = s4.x; sigma[1] = s4.y; sigma[2] = s4.z; sigma[3] = s4.w;
        mu[0] = m4.x; mu[1] = m4.y; mu[2] = m4.z; mu[3] = m4.w;
    } else {
        sigma[0] = sg[0];
        mu[0] = sg[hw];
    }
    if (a.y) {
        if (VEC == 4 && a.lvec) {
            const float4 y4 = *reinterpret_cast<const float4*>(a.y + lv);
            val[0] = y4.x; val[1] = y4.y; val[2] = y4.z; val[3] = y4.w;
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) val[e] = a.y[lv + e * a.s];
        }
        if constexpr (RDO) {                                                     // the index does not depend on the choice
#pragma unroll
            for (int e = 0; e < VEC; ++e) sym[e] = rdo_symbol(val[e] - mu[e], inv_q[e], cdf_index(sigma[e], inv_q[e], tab), a.rdo);
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) sym[e] = (int)rintf((val[e] - mu[e]) * inv_q[e]);
        }
    } else if (a.sym_in) {
        if constexpr (VEC == 4) {
            const int4 q4 = *reinterpret_cast<const int4*>(a.sym_in + zc * hw + v);
            sym[0] = q4.x; sym[1] = q4.y; sym[2] = q4.z; sym[3] = q4.w;
        } else {
            sym[0] = a.sym_in[zc * hw + v];
        }
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) sym[e] = 0;
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        idx[e] = cdf_index(sigma[e], inv_q[e], tab);
        val[e] = (float)sym[e] * q[e] + mu[e];
    }
    if constexpr (VEC == 4) {
        *reinterpret_cast<int4*>(a.idx + zc * hw + v) = make_int4(idx[0], idx[1], idx[2], idx[3]);
        if (a.y) *reinterpret_cast<int4*>(a.sym_out + zc * hw + v) = make_int4(sym[0], sym[1], sym[2], sym[3]);
    } else {
        a.idx[zc * hw + v] = idx[0];
        if (a.y) a.sym_out[zc * hw + v] = sym[0];
    }
    if (!a.level) return;                                                       // indexes only
    if (VEC == 4 && a.lvec) {
        *reinterpret_cast<float4*>(a.level + lv) = make_float4(val[0], val[1], val[2], val[3]);
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) a.level[lv + e * a.s] = val[e];
    }
}

constexpr int COST_PER_THREAD = 8;

// per stream z: sums[z] += sum of cost[idx][sym - offset] (escape: esc_cost, counted in escapes[z]); integers, so the result
// does not depend on the order of the additions.  One 64-bit atomic per wave (and one more if the wave saw an escape).
__global__ __launch_bounds__(NT) void k_code_cost(const int* __restrict__ sym, const int* __restrict__ idx, int64_t n,
                                                  const int* __restrict__ cost, int ntab, int width, const int* __restrict__ sizes,
                                                  const int* __restrict__ offsets, int esc_cost, unsigned long long* sums,
                                                  unsigned long long* escapes) {
    const int64_t z = blockIdx.y;
    const int* s = sym + z * n;
    const int* ix = idx + z * n;
    long long acc = 0, esc = 0;
    const int64_t stride = (int64_t)gridDim.x * NT;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += stride) {
        const int t = ix[e];
        int cst = esc_cost;
        bool inside = false;
        if (t >= 0 && t < ntab) {
            const int v = s[e] - offsets[t];
            inside = v >= 0 && v < sizes[t] - 2 && v < width;
            if (inside) cst = cost[(int64_t)t * width + v];
        }
        acc += cst;
        esc += inside ? 0 : 1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc += __shfl_down(acc, o, 64);
        esc += __shfl_down(esc, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(sums + z, (unsigned long long)acc);
        if (esc) atomicAdd(escapes + z, (unsigned long long)esc);
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

// a step map as the entry points take it
struct StepMap {
    const float* qpairs;
    int64_t units, mh, mw;
    int shift;
};

// rdo: null for the plain quantiser.  map: null for one step (q, inv_q), else the step map, and q, inv_q are not read.
static int gauss_quantise(const float* params, const float* y, const int32_t* sym_in, const float* table63, int32_t* idx,
                          int32_t* sym_out, float* level, int64_t streams, int channels, int64_t h, int64_t w, int64_t H, int64_t W,
                          int r0, int c0, int stride, float q, float inv_q, const RdoTables* rdo, const StepMap* map, void* stream) {
    LLDWT_REQUIRE(params && table63 && idx, "gauss_quantise: null pointer");
    LLDWT_REQUIRE(!(y && sym_in), "gauss_quantise: give y (encoder) or sym_in (decoder), not both");
    LLDWT_REQUIRE((level != nullptr) == (y || sym_in), "gauss_quantise: level goes with y or sym_in (neither: the indexes only)");
    LLDWT_REQUIRE(!y || sym_out, "gauss_quantise: the encoder needs sym_out");
    if (!map) {
        const float n = q * 16.f;
        LLDWT_REQUIRE(n >= 4.f && n <= 1024.f && n == (float)(int)n && inv_q == (float)(1.0 / (double)q),
                      "gauss_quantise: step %g (1 / step %g) is not n / 16 with n in [4, 1024]", (double)q, (double)inv_q);
    }
    LLDWT_REQUIRE(streams > 0 && channels > 0 && streams * channels <= 65535 && h > 0 && w > 0 && h * w < ((int64_t)1 << 31),
                  "gauss_quantise: bad sizes (streams %lld, channels %d, grid %lld x %lld)", (long long)streams, channels, (long long)h,
                  (long long)w);
    LLDWT_REQUIRE(stride >= 1 && r0 >= 0 && c0 >= 0 && r0 + (int64_t)stride * (h - 1) < H && c0 + (int64_t)stride * (w - 1) < W &&
                      H * W < ((int64_t)1 << 31),
                  "gauss_quantise: the grid (%d, %d, stride %d) of %lld x %lld does not fit the %lld x %lld level", r0, c0, stride,
                  (long long)h, (long long)w, (long long)H, (long long)W);
    if (map) {
        LLDWT_REQUIRE(map->qpairs && (reinterpret_cast<uintptr_t>(map->qpairs) & 7) == 0,
                      "gauss_quantise_map: null step map (or one not aligned to its pairs)");
        LLDWT_REQUIRE(map->units > 0 && streams % map->units == 0, "gauss_quantise_map: %lld streams are not whole planes of %lld units",
                      (long long)streams, (long long)map->units);
        LLDWT_REQUIRE(map->shift >= 0 && map->shift <= 30 && map->mh > 0 && map->mw > 0 && map->mh < ((int64_t)1 << 31) &&
                          map->mw < ((int64_t)1 << 31) && map->mh >= cdiv(H, (int64_t)1 << map->shift) &&
                          map->mw >= cdiv(W, (int64_t)1 << map->shift),
                      "gauss_quantise_map: a %lld x %lld map at shift %d does not cover the %lld x %lld level", (long long)map->mh,
                      (long long)map->mw, map->shift, (long long)H, (long long)W);
    }
    QuantArgs a;
    a.params = params; a.y = y; a.sym_in = sym_in; a.table = table63; a.idx = idx; a.sym_out = sym_out; a.level = level;
    a.C = channels; a.h = (int)h; a.w = (int)w; a.H = (int)H; a.W = (int)W; a.r0 = r0; a.c0 = c0; a.s = stride;
    a.q = q; a.inv_q = inv_q;
    a.rdo = rdo ? *rdo : RdoTables{nullptr, nullptr, nullptr, 0, 0, 0.f};
    a.qpairs = map ? map->qpairs : nullptr;
    a.units = map ? (int)map->units : 1; a.mh = map ? (int)map->mh : 0; a.mw = map ? (int)map->mw : 0; a.shift = map ? map->shift : 0;
    const bool vec = w % 4 == 0 && aligned16(params) && aligned16(idx) && (!sym_in || aligned16(sym_in)) && (!sym_out || aligned16(sym_out));
    a.lvec = vec && stride == 1 && W % 4 == 0 && c0 % 4 == 0 && (!level || aligned16(level)) && (!y || aligned16(y));
    const int per = vec ? 4 : 1;
    dim3 grid((unsigned)cdiv(cdiv(h * w, per), NT), (unsigned)(streams * channels));
    if (map) {
        if (rdo && vec) hipLaunchKernelGGL((k_gauss_quantise<4, true, true>), grid, dim3(NT), 0, (hipStream_t)stream, a);
        else if (rdo) hipLaunchKernelGGL((k_gauss_quantise<1, true, true>), grid, dim3(NT), 0, (hipStream_t)stream, a);
        else if (vec) hipLaunchKernelGGL((k_gauss_quantise<4, false, true>), grid, dim3(NT), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL((k_gauss_quantise<1, false, true>), grid, dim3(NT), 0, (hipStream_t)stream, a);
        return check_launch("gauss_quantise_map");
    }
    if (rdo && vec) hipLaunchKernelGGL((k_gauss_quantise<4, true>), grid, dim3(NT), 0, (hipStream_t)stream, a);
    else if (rdo) hipLaunchKernelGGL((k_gauss_quantise<1, true>), grid, dim3(NT), 0, (hipStream_t)stream, a);
    else if (vec) hipLaunchKernelGGL(k_gauss_quantise<4>, grid, dim3(NT), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_gauss_quantise<1>, grid, dim3(NT), 0, (hipStream_t)stream, a);
    return check_launch("gauss_quantise");
}

extern "C" int lldwt_gauss_quantise(const float* params, const float* y, const int32_t* sym_in, const float* table63, int32_t* idx,
                                    int32_t* sym_out, float* level, int64_t streams, int channels, int64_t h, int64_t w, int64_t H,
                                    int64_t W, int r0, int c0, int stride, float q, float inv_q, void* stream) {
    return gauss_quantise(params, y, sym_in, table63, idx, sym_out, level, streams, channels, h, w, H, W, r0, c0, stride, q, inv_q,
                          nullptr, nullptr, stream);
}

// the encoder with rate-distortion optimised quantisation: encoder mode only, the decoder is
// lldwt_gauss_quantise as ever
extern "C" int lldwt_gauss_quantise_rdo(const float* params, const float* y, const float* table63, int32_t* idx, int32_t* sym_out,
                                        float* level, int64_t streams, int channels, int64_t h, int64_t w, int64_t H, int64_t W,
                                        int r0, int c0, int stride, float q, float inv_q, const int32_t* cost, const int32_t* sizes,
                                        const int32_t* offsets, int32_t ntab, int32_t width, float k, void* stream) {
    LLDWT_REQUIRE(y && level && sym_out, "gauss_quantise_rdo: encoder only (y, level and sym_out must be given)");
    LLDWT_REQUIRE(cost && sizes && offsets, "gauss_quantise_rdo: null cost table pointer");
    LLDWT_REQUIRE(ntab > 0 && width > 0, "gauss_quantise_rdo: bad cost table sizes (%d x %d)", ntab, width);
    LLDWT_REQUIRE(rdo_k_ok(k), "gauss_quantise_rdo: k %g is not (m / 64) * 2^-16 with an integer m in [1, %d]", (double)k, RDO_M_MAX);
    const RdoTables rdo{cost, sizes, offsets, ntab, width, k};
    return gauss_quantise(params, y, nullptr, table63, idx, sym_out, level, streams, channels, h, w, H, W, r0, c0, stride, q, inv_q, &rdo,
                          nullptr, stream);
}

// the quantiser with a step map: the three modes of lldwt_gauss_quantise, and with cost != null the encoder of
// lldwt_gauss_quantise_rdo
extern "C" int lldwt_gauss_quantise_map(const float* params, const float* y, const int32_t* sym_in, const float* table63, int32_t* idx,
                                        int32_t* sym_out, float* level, int64_t streams, int64_t units, int channels, int64_t h,
                                        int64_t w, int64_t H, int64_t W, int r0, int c0, int stride, const float* qpairs, int64_t mh,
                                        int64_t mw, int shift, const int32_t* cost, const int32_t* sizes, const int32_t* offsets,
                                        int32_t ntab, int32_t width, float k, void* stream) {
    const StepMap map{qpairs, units, mh, mw, shift};
    if (!cost)
        return gauss_quantise(params, y, sym_in, table63, idx, sym_out, level, streams, channels, h, w, H, W, r0, c0, stride, 1.f, 1.f,
                              nullptr, &map, stream);
    LLDWT_REQUIRE(y && level && sym_out, "gauss_quantise_map: rdo is a choice of the encoder (y, level and sym_out must be given)");
    LLDWT_REQUIRE(sizes && offsets, "gauss_quantise_map: null cost table pointer");
    LLDWT_REQUIRE(ntab > 0 && width > 0, "gauss_quantise_map: bad cost table sizes (%d x %d)", ntab, width);
    LLDWT_REQUIRE(rdo_k_ok(k), "gauss_quantise_map: k %g is not (m / 64) * 2^-16 with an integer m in [1, %d]", (double)k, RDO_M_MAX);
    const RdoTables rdo{cost, sizes, offsets, ntab, width, k};
    return gauss_quantise(params, y, nullptr, table63, idx, sym_out, level, streams, channels, h, w, H, W, r0, c0, stride, 1.f, 1.f,
                          &rdo, &map, stream);
}

extern "C" int lldwt_code_cost(const int32_t* sym, const int32_t* idx, int64_t streams, int64_t n, const int32_t* cost, int32_t ntab,
                               int32_t width, const int32_t* sizes, const int32_t* offsets, int32_t esc_cost, int64_t* sums,
                               int64_t* escapes, void* stream) {
    LLDWT_REQUIRE(sym && idx && cost && sizes && offsets && sums && escapes, "code_cost: null pointer");
    LLDWT_REQUIRE(streams > 0 && streams <= 65535 && n >= 0 && ntab > 0 && width > 0 && esc_cost >= 0,
                  "code_cost: bad sizes (streams %lld, n %lld, tables %d x %d)", (long long)streams, (long long)n, ntab, width);
    if (n == 0) return LLDWT_OK;
    int64_t bx = cdiv(n, (int64_t)NT * COST_PER_THREAD);
    if (bx > 1024) bx = 1024;
    dim3 grid((unsigned)bx, (unsigned)streams);
    hipLaunchKernelGGL(k_code_cost, grid, dim3(NT), 0, (hipStream_t)stream, sym, idx, n, cost, ntab, width, sizes, offsets, esc_cost,
                       reinterpret_cast<unsigned long long*>(sums), reinterpret_cast<unsigned long long*>(escapes));
    return check_launch("code_cost");
}
