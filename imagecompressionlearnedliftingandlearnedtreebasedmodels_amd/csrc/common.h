// common.h -- shared helpers for the lldwt HIP library (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/lldwt.h"

namespace lldwt {

void set_error(const char* fmt, ...);

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return LLDWT_EHIP;
    }
    return LLDWT_OK;
}

#define LLDWT_REQUIRE(cond, ...)          \
    do {                                  \
        if (!(cond)) {                    \
            lldwt::set_error(__VA_ARGS__); \
            return LLDWT_EINVAL;          \
        }                                 \
    } while (0)

// compute units of the current device (256 on MI355X); 256 if the query fails
static inline int lldwt_num_cus() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
        return 256;
    return n;
}

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline int64_t round_up(int64_t a, int64_t b) { return cdiv(a, b) * b; }

// tanh(x) = sign(x) * (1 - 2 / (exp(2|x|) + 1)) on the hardware exp2 / rcp units (v_exp_f32, v_rcp_f32): ~8 instructions
// instead of ocml's ~40; absolute error <= 3e-7 over the whole range (checked against torch.tanh in the parity tests),
// exact saturation to +-1 for |x| > 10.
__device__ __forceinline__ float fast_tanh(float x) {
    // exp(2|x|) = 2^(2|x| log2 e); no clamp needed: a huge |x| gives e = inf, rcp = 0, t = 1
    const float e = __builtin_amdgcn_exp2f(fabsf(x) * 2.88539008177792681472f);
    const float t = __builtin_fmaf(-2.f, __builtin_amdgcn_rcpf(e + 1.f), 1.f);    // = 1 - 2r (2r is exact: same rounding)
    return copysignf(t, x);
}

__device__ __forceinline__ float act_apply(float v, int act) {
    if (act == LLDWT_ACT_TANH) return fast_tanh(v);
    if (act == LLDWT_ACT_LRELU) return v >= 0.f ? v : 0.01f * v;
    if (act == LLDWT_ACT_RELU) return v > 0.f ? v : 0.f;
    return v;
}

// 64-lane wavefront sum via DPP-free shuffles (wave = 64 on CDNA4)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// ---- rate-distortion optimised quantisation, the one statement of the rule for both encoder kernels
// (k_gauss_quantise, csrc/quant.hip; the wavefront epilogue of k_cgp16, csrc/cgp_f16x3.hip)
constexpr int RDO_COST_ESCAPE = 32 << 16;            // ops.COST_ESCAPE: a symbol outside its table, in units of 2^-16 bit
constexpr int RDO_M_MAX = 256;                       // rho = m / 64 with an integer m in [1, RDO_M_MAX]

struct RdoTables {                                   // the tables of lldwt_code_cost
    const int* cost;                                 // (ntab, width) code lengths in units of 2^-16 bit
    const int* sizes;                                // (ntab): table t holds sizes[t] - 2 symbols
    const int* offsets;                              // (ntab): the symbol of column 0
    int ntab, width;
    float k;                                         // fp32(rho) * 2^-16
};

// k = (m / 64) * 2^-16 with an integer m in [1, 256]: k * 2^22 is that integer
static inline bool rdo_k_ok(float k) {
    const float m = k * 4194304.f;
    return m >= 1.f && m <= (float)RDO_M_MAX && m == (float)(int)m;
}

__device__ __forceinline__ int rdo_code_cost(const RdoTables& t, int idx, int sym) {       // the lookup of k_code_cost
    if (idx < 0 || idx >= t.ntab) return RDO_COST_ESCAPE;
    const int v = sym - t.offsets[idx];
    return (v >= 0 && v < t.sizes[idx] - 2 && v < t.width) ? t.cost[(int64_t)idx * t.width + v] : RDO_COST_ESCAPE;
}

// d = y - mu -> the symbol: the nearest level s0, or the level next to it toward zero when the bits that saves, times
// rho, outweigh the squared error it adds (in units of q^2: t = 1 + 2 sign(s0) r with r = v - s0).
__device__ __forceinline__ int rdo_symbol(float d, float inv_q, int idx, const RdoTables& t) {
    float s0f, r;
    {
        // v is the ROUNDED fp32 product and r a subtraction of its own: contracted into fmaf(d, inv_q, -s0) the residual
        // would be that of the unrounded product, which is not what the host restatement (and the decision) is made of
#pragma clang fp contract(off)
        const float v = d * inv_q;
        s0f = rintf(v);
        r = v - s0f;                                                             // exact: |r| <= 0.5
    }
    const int s0 = (int)s0f;
    if (s0 == 0) return 0;                                                       // nothing to decide
    const int g = s0 > 0 ? 1 : -1;
    const int s1 = s0 - g;
    const float tt = __builtin_fmaf(g > 0 ? 2.f : -2.f, r, 1.f);                 // 2 g r is exact: fma and mul + add agree
    const int dc = rdo_code_cost(t, idx, s0) - rdo_code_cost(t, idx, s1);        // |dc| <= 2^21: exact as a float
    return (float)dc * t.k > tt ? s1 : s0;
}

}  // namespace lldwt
