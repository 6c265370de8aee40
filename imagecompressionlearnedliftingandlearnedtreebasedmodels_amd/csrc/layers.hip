// layers.hip -- quality layers of the codec: SNR refinement of the levels that carry a step.  Layer j brings
// every coefficient of such a level from the step q_{j-1} to q_j = q / 3^j; a mid-tread bin of width q_{j-1} is exactly three
// bins of width q_j, so the refinement symbol t is one of {-1, 0, +1}.  Three element-wise kernels over a level (Z, C, h, w)
// with its Gaussian parameters (Z, 2C, h, w), sigma of channel c on 2c and mu on 2c + 1 (as lldwt_gauss_quantise takes them):
//   encode   t = clamp(rint((y - v) * inv_q_j), -1, 1), v' = v + t * q_j, table row and the coded symbol (t mirrored, below)
//   rows     the decoder's half before the symbols are popped: table row and mirror sign from (v, params) alone
//   apply    the decoder's half after: v' = v + sign * symbol * q_j
// with v the level at the previous step.  The table row is idx * (K + 1) + a:
//   idx = #(table63 < max(sigma * inv_q_prev, 0.11))             the scale index of lldwt_gauss_quantise, in units of q_prev
//   m   = rint((v - mu) * inv_q_prev),  a = min(|m|, K)          the bin's position in the bell
// and where m < 0 the coded symbol is -t, so that one row serves both sides of the bell.
// All fp32 with every product rounded before the sum (__fmul_rn / __fadd_rn: no fused multiply-add), so that a tensor
// restatement on the host agrees bit for bit.
// Memory: encode reads 16 and writes 12 bytes per coefficient, rows 12 and 8, apply 12 and 4; nothing is reused, so the
// kernels are bound by HBM.  A thread handles 4 consecutive coefficients of a row as one 16-byte access per array where
// w % 4 == 0 and the arrays are 16-byte aligned (a wave then touches 1 KiB of each array per access), one coefficient otherwise.
#include "common.h"

using namespace lldwt;

namespace {

constexpr int NT = 256;
constexpr int NTABLE = 63;                       // scale-table entries the index counts over (the 64th is the catch-all)

struct LayerArgs {
    const float* y;                              // encode: (Z, C, h, w) coefficients
    const float* v;                              // (Z, C, h, w): the level at the previous step
    const float* params;                         // (Z, 2C, h, w)
    const float* table;                          // NTABLE floats
    const int* sym_in;                           // apply: the popped symbols
    const int* sign_in;                          // apply: the mirror signs of rows
    int* sym;                                    // encode: the coded symbols
    int* row;                                    // encode, rows: table rows
    int* sign;                                   // rows: +1 / -1
    float* out;                                  // encode, apply: the level at the step q_j (may be v)
    int C, h, w;
    float inv_q_prev, q, inv_q, Kf;
    int K1;                                      // K + 1
};

enum Mode { ENCODE, ROWS, APPLY };

template <int VEC>
__device__ __forceinline__ void load(const float* p, float (&d)[VEC]) {
    if constexpr (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w;
    } else {
        d[0] = p[0];
    }
}

template <int VEC>
__device__ __forceinline__ void load(const int* p, int (&d)[VEC]) {
    if constexpr (VEC == 4) {
        const int4 t = *reinterpret_cast<const int4*>(p);
        d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w;
    } else {
        d[0] = p[0];
    }
}

template <int VEC>
__device__ __forceinline__ void store(float* p, const float (&d)[VEC]) {
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(d[0], d[1], d[2], d[3]);
    else p[0] = d[0];
}

template <int VEC>
__device__ __forceinline__ void store(int* p, const int (&d)[VEC]) {
    if constexpr (VEC == 4) *reinterpret_cast<int4*>(p) = make_int4(d[0], d[1], d[2], d[3]);
    else p[0] = d[0];
}

template <int VEC, int MODE>
__global__ __launch_bounds__(NT) void k_layer(LayerArgs a) {
    const int64_t hw = (int64_t)a.h * a.w;
    const int64_t e0 = ((int64_t)blockIdx.x * NT + threadIdx.x) * VEC;         // first element of this thread inside the (z, c) grid
    if (e0 >= hw) return;                                                       // VEC 4: w % 4 == 0, so hw % 4 == 0 and no group straddles
    const int64_t zc = blockIdx.y, z = zc / a.C;
    const int c = (int)(zc - z * a.C);
    const int64_t at = zc * hw + e0;
    float v[VEC], nv[VEC];
    load<VEC>(a.v + at, v);
    if constexpr (MODE == APPLY) {
        int s[VEC], g[VEC];
        load<VEC>(a.sym_in + at, s);
        load<VEC>(a.sign_in + at, g);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const int t = (s[e] < -1 ? -1 : (s[e] > 1 ? 1 : s[e])) * (g[e] < 0 ? -1 : 1);   // a symbol outside the alphabet moves one bin
            nv[e] = __fadd_rn(v[e], __fmul_rn((float)t, a.q));
        }
        store<VEC>(a.out + at, nv);
        return;
    } else {
        float tab[NTABLE];                                                      // uniform addresses: read once per wave
#pragma unroll
        for (int k = 0; k < NTABLE; ++k) tab[k] = a.table[k];
        const float* sg = a.params + ((z * 2 * a.C + 2 * c) * hw + e0);
        float sigma[VEC], mu[VEC];
        load<VEC>(sg, sigma);
        load<VEC>(sg + hw, mu);
        int row[VEC], sgn[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float sb = fmaxf(__fmul_rn(sigma[e], a.inv_q_prev), 0.11f);
            int n = 0;
#pragma unroll
            for (int k = 0; k < NTABLE; ++k) n += tab[k] < sb ? 1 : 0;
            const float m = rintf(__fmul_rn(__fsub_rn(v[e], mu[e]), a.inv_q_prev));
            const float pos = fminf(fabsf(m), a.Kf);                           // a NaN position takes row K
            row[e] = n * a.K1 + (int)pos;
            sgn[e] = m < 0.f ? -1 : 1;
        }
        store<VEC>(a.row + at, row);
        if constexpr (MODE == ROWS) {
            store<VEC>(a.sign + at, sgn);
            return;
        } else {
            float y[VEC];
            int sym[VEC];
            load<VEC>(a.y + at, y);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                float t = rintf(__fmul_rn(__fsub_rn(y[e], v[e]), a.inv_q));
                t = t < -1.f ? -1.f : (t > 1.f ? 1.f : t);
                t = t == t ? t : 0.f;                                           // a NaN residual codes 0
                nv[e] = __fadd_rn(v[e], __fmul_rn(t, a.q));
                sym[e] = (int)t * sgn[e];
            }
            store<VEC>(a.sym + at, sym);
            store<VEC>(a.out + at, nv);
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// q > 0 finite and inv_q == fp32(1 / q) with the division in double: the pair as the host forms it
inline bool pair_ok(float q, float inv_q) { return q > 0.f && q <= 64.f && inv_q == (float)(1.0 / (double)q); }

int geometry(const char* who, int64_t streams, int channels, int64_t h, int64_t w, dim3& grid, bool vec) {
    LLDWT_REQUIRE(streams > 0 && channels > 0 && streams * channels <= 65535 && h > 0 && w > 0 && h * w < ((int64_t)1 << 31),
                  "%s: bad sizes (streams %lld, channels %d, grid %lld x %lld)", who, (long long)streams, channels, (long long)h,
                  (long long)w);
    grid = dim3((unsigned)cdiv(cdiv(h * w, vec ? 4 : 1), NT), (unsigned)(streams * channels));
    return LLDWT_OK;
}

}  // namespace

extern "C" int lldwt_layer_encode(const float* y, const float* v_prev, const float* params, const float* table63, int32_t* sym,
                                  int32_t* row, float* v_out, int64_t streams, int channels, int64_t h, int64_t w, float q_prev,
                                  float inv_q_prev, float q, float inv_q, int K, void* stream) {
    LLDWT_REQUIRE(y && v_prev && params && table63 && sym && row && v_out, "layer_encode: null pointer");
    LLDWT_REQUIRE(pair_ok(q_prev, inv_q_prev) && pair_ok(q, inv_q) && q < q_prev,
                  "layer_encode: steps %g (1 / step %g) -> %g (1 / step %g) are not two pairs (q, fp32(1 / q)) with the second finer",
                  (double)q_prev, (double)inv_q_prev, (double)q, (double)inv_q);
    LLDWT_REQUIRE(K >= 1 && K <= LLDWT_LAYER_MAX_K, "layer_encode: K %d outside [1, %d]", K, LLDWT_LAYER_MAX_K);
    const bool vec = w % 4 == 0 && aligned16(y) && aligned16(v_prev) && aligned16(params) && aligned16(sym) && aligned16(row) &&
                     aligned16(v_out);
    dim3 grid;
    if (const int rc = geometry("layer_encode", streams, channels, h, w, grid, vec)) return rc;
    LayerArgs a{};
    a.y = y; a.v = v_prev; a.params = params; a.table = table63; a.sym = sym; a.row = row; a.out = v_out;
    a.C = channels; a.h = (int)h; a.w = (int)w; a.inv_q_prev = inv_q_prev; a.q = q; a.inv_q = inv_q; a.Kf = (float)K; a.K1 = K + 1;
    if (vec) hipLaunchKernelGGL((k_layer<4, ENCODE>), grid, dim3(NT), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((k_layer<1, ENCODE>), grid, dim3(NT), 0, (hipStream_t)stream, a);
    return check_launch("layer_encode");
}

extern "C" int lldwt_layer_rows(const float* v_prev, const float* params, const float* table63, int32_t* row, int32_t* sign,
                                int64_t streams, int channels, int64_t h, int64_t w, float q_prev, float inv_q_prev, int K,
                                void* stream) {
    LLDWT_REQUIRE(v_prev && params && table63 && row && sign, "layer_rows: null pointer");
    LLDWT_REQUIRE(pair_ok(q_prev, inv_q_prev), "layer_rows: step %g (1 / step %g) is not a pair (q, fp32(1 / q))", (double)q_prev,
                  (double)inv_q_prev);
    LLDWT_REQUIRE(K >= 1 && K <= LLDWT_LAYER_MAX_K, "layer_rows: K %d outside [1, %d]", K, LLDWT_LAYER_MAX_K);
    const bool vec = w % 4 == 0 && aligned16(v_prev) && aligned16(params) && aligned16(row) && aligned16(sign);
    dim3 grid;
    if (const int rc = geometry("layer_rows", streams, channels, h, w, grid, vec)) return rc;
    LayerArgs a{};
    a.v = v_prev; a.params = params; a.table = table63; a.row = row; a.sign = sign;
    a.C = channels; a.h = (int)h; a.w = (int)w; a.inv_q_prev = inv_q_prev; a.Kf = (float)K; a.K1 = K + 1;
    if (vec) hipLaunchKernelGGL((k_layer<4, ROWS>), grid, dim3(NT), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((k_layer<1, ROWS>), grid, dim3(NT), 0, (hipStream_t)stream, a);
    return check_launch("layer_rows");
}

extern "C" int lldwt_layer_apply(const float* v_prev, const int32_t* sym, const int32_t* sign, float* v_out, int64_t streams,
                                 int channels, int64_t h, int64_t w, float q, float inv_q, void* stream) {
    LLDWT_REQUIRE(v_prev && sym && sign && v_out, "layer_apply: null pointer");
    LLDWT_REQUIRE(pair_ok(q, inv_q), "layer_apply: step %g (1 / step %g) is not a pair (q, fp32(1 / q))", (double)q, (double)inv_q);
    const bool vec = w % 4 == 0 && aligned16(v_prev) && aligned16(sym) && aligned16(sign) && aligned16(v_out);
    dim3 grid;
    if (const int rc = geometry("layer_apply", streams, channels, h, w, grid, vec)) return rc;
    LayerArgs a{};
    a.v = v_prev; a.sym_in = sym; a.sign_in = sign; a.out = v_out;
    a.C = channels; a.h = (int)h; a.w = (int)w; a.q = q; a.inv_q = inv_q;
    if (vec) hipLaunchKernelGGL((k_layer<4, APPLY>), grid, dim3(NT), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((k_layer<1, APPLY>), grid, dim3(NT), 0, (hipStream_t)stream, a);
    return check_launch("layer_apply");
}
