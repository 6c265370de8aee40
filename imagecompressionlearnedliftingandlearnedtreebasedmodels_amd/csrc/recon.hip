// recon.hip -- centroid reconstruction of the levels that carry a step: a decoder's choice that moves every
// coefficient from the centre of its quantisation bin to the bin's mean under the Gaussian (sigma, mu) the entropy model gives it.
// gfx950 only.  One element-wise kernel over a level (Z, C, h, w) with its parameters (Z, 2C, h, w), sigma of channel c on 2c and mu
// on 2c + 1 (the layout of QuantArgs, csrc/quant.hip); the step is one pair (q, inv_q) or, MAP, the pair of the element's block of a
// step map, exactly as k_gauss_quantise takes it.
//   u = (v - mu) * inv_q,  a = |u|,  s = max(sigma * inv_q, 0.11)
//   out = clamp(v - copysign(q * delta(a, s), u), v - q / 2, v + q / 2),   out = v where u, sigma * inv_q or delta is not finite
//   delta(a, s) = a - E[X | a - 1/2 <= X <= a + 1/2], X ~ N(0, s^2)        0 <= delta <= 1/2, delta(0, s) = 0
// delta in fp32, three regimes (D = a / s^2, the drop of the exponent across the bin; the cuts are those of tests/centroid_ref.py
// and DESIGN.md 7.1.13 says how they were measured):
//   wide  s > S_CUT and D < D_CUT: int_0^1/2 y exp(-gamma y^2) sinh(beta y) dy / int_0^1/2 exp(-gamma y^2) cosh(beta y) dy with
//         beta = D, gamma = 1 / (2 s^2) -- the mean of a uniform density tilted by beta and bent by gamma, y and -y folded together
//         so that delta itself is computed and never a - E; 5-point Gauss-Legendre
//   zero  else a < 1/2: a - s phi(l) (1 - exp(-D)) / (Phi(h) - Phi(l)), the mass a sum of two erf (l < 0 < h)
//   tail  else: 1/2 - s (K(l) - r (K(h) + w)) / (1 - r), r = exp(-D) R(h) / R(l), everything divided by the density at the inner
//         edge: l = (a - 1/2) / s, w = 1 / s, h = l + w, R the Mills ratio (erfcxf below X_CUT) and K(x) = 1 / R(x) - x, both from
//         the continued fraction 1 / (x + 1 / (x + 2 / (x + ...))) from X_CUT on.  The far tail is 1/2 - s K(l) = 1/2 - s^2 / lo.
// Memory: 12 bytes read and 4 written per coefficient, nothing reused; a thread handles 4 consecutive coefficients of a row as
// one 16-byte access per array where w % 4 == 0 and the arrays are 16-byte aligned, one coefficient otherwise.  No LDS, no
// atomics, nothing waits on another workgroup.
#include "common.h"

using namespace lldwt;

namespace {

constexpr int NT = 256;
constexpr float S_CUT = 0.75f, D_CUT = 4.f, X_CUT = 3.f;
constexpr int CF_DEPTH = 12;
constexpr int GL = 5;                            // Gauss-Legendre on [0, 1/2]: nodes and weights
__constant__ const float GL_X[GL] = {2.345503852e-02f, 1.153826725e-01f, 2.500000000e-01f, 3.846173275e-01f, 4.765449615e-01f};
__constant__ const float GL_W[GL] = {5.923172126e-02f, 1.196571676e-01f, 1.422222222e-01f, 1.196571676e-01f, 5.923172126e-02f};
constexpr float SQRT_HALF_PI = 1.253314137f, INV_SQRT2 = 0.7071067812f, INV_SQRT_2PI = 0.3989422804f;
constexpr float FLT_BIG = 3.402823466e38f;

struct ReconArgs {
    const float* params;                         // (Z, 2C, h, w)
    const float* v;                              // (Z, C, h, w) decoded values
    float* out;                                  // (Z, C, h, w), may be v
    int C, h, w;
    float q, inv_q;
    const float* qpairs;                         // MAP: (units, mh, mw, 2) pairs, stream z reads the map of unit z % units
    int units, mh, mw, shift;
};

__device__ __forceinline__ bool finite(float x) { return fabsf(x) <= FLT_BIG; }   // false for NaN too

// x >= 0 -> the Mills ratio R(x) = (1 - Phi(x)) / phi(x) and K(x) = 1 / R(x) - x
__device__ __forceinline__ void mills(float x, float& R, float& K) {
    if (x < X_CUT) {
        R = SQRT_HALF_PI * erfcxf(x * INV_SQRT2);
        K = 1.f / R - x;
        return;
    }
    // with y = 1 / x, z = y^2: C = 1 + 2 z / (1 + 3 z / (1 + ...)) = num / den, K = y / C and R = y / (1 + z / C)
    const float y = 1.f / x, z = y * y;
    float num = 1.f + (float)CF_DEPTH * z, den = 1.f;
#pragma unroll
    for (int n = CF_DEPTH - 1; n >= 2; --n) {
        const float t = num + (float)n * z * den;
        den = num;
        num = t;
    }
    K = y * den / num;
    R = y * num / (num + z * den);
}

__device__ __forceinline__ float centroid_delta(float a, float s) {
    const float w = 1.f / s, D = a * w * w;
    if (s > S_CUT && D < D_CUT) {
        const float gamma = 0.5f * w * w;
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int i = 0; i < GL; ++i) {
            const float g = GL_W[i] * expf(-(gamma * (GL_X[i] * GL_X[i])));
            const float e = expf(D * GL_X[i]), ie = 1.f / e;
            num += g * GL_X[i] * (e - ie);
            den += g * (e + ie);
        }
        return num / den;
    }
    float l = (a - 0.5f) / s;
    if (a < 0.5f) {
        const float h = (a + 0.5f) / s;
        const float mass = 0.5f * (erff(h * INV_SQRT2) + erff(-l * INV_SQRT2));
        const float phi_l = expf(-(0.5f * l * l)) * INV_SQRT_2PI;
        return a - s * phi_l * -expm1f(-D) / mass;
    }
    l = fminf(l, 1e30f);                         // a / s beyond the format: delta is 1/2 to 1e-22 there
    float Rl, Kl, m;
    mills(l, Rl, Kl);
    const float t = expf(-D);
    if (t > 1e-10f) {                            // the outer edge still weighs in
        float Rh, Kh;
        mills(l + w, Rh, Kh);
        const float r = t * (Rh / Rl);
        m = (Kl - r * (Kh + w)) / (1.f - r);
    } else {
        m = Kl;
    }
    return 0.5f - s * m;
}

__device__ __forceinline__ float centroid(float v, float sigma, float mu, float q, float inv_q) {
    const float u = (v - mu) * inv_q, sb = sigma * inv_q;
    if (!(finite(u) && finite(sb))) return v;
    const float d = centroid_delta(fabsf(u), fmaxf(sb, 0.11f));
    if (!finite(d)) return v;
    const float half = 0.5f * q;
    const float r = v - copysignf(q * fminf(fmaxf(d, 0.f), 0.5f), u);
    return fminf(fmaxf(r, v - half), v + half);
}

template <int VEC, bool MAP>
__global__ __launch_bounds__(NT) void k_gauss_centroid(ReconArgs a) {
    const int64_t hw = (int64_t)a.h * a.w;
    const int64_t e0 = ((int64_t)blockIdx.x * NT + threadIdx.x) * VEC;         // first element of this thread inside the (z, c) grid
    if (e0 >= hw) return;                                                       // VEC 4: w % 4 == 0, the four share the row
    const int64_t zc = blockIdx.y, z = zc / a.C;
    const int c = (int)(zc - z * a.C);
    const float* sg = a.params + ((z * 2 * a.C + 2 * c) * hw + e0);
    const int64_t at = zc * hw + e0;
    float sigma[VEC], mu[VEC], v[VEC], q[VEC], inv_q[VEC], o[VEC];
    if constexpr (MAP) {                                                        // the host checked that the map covers the level
        const int i = (int)(e0 / a.w), j = (int)(e0 - (int64_t)i * a.w);
        const float* row = a.qpairs + ((int64_t)(z % a.units) * a.mh + (i >> a.shift)) * a.mw * 2;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float2 pr = *reinterpret_cast<const float2*>(row + 2 * ((j + e) >> a.shift));
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
        const float4 v4 = *reinterpret_cast<const float4*>(a.v + at);
        sigma[0] = s4.x; sigma[1] = s4.y; sigma[2] = s4.z; sigma[3] = s4.w;
        mu[0] = m4.x; mu[1] = m4.y; mu[2] = m4.z; mu[3] = m4.w;
        v[0] = v4.x; v[1] = v4.y; v[2] = v4.z; v[3] = v4.w;
    } else {
        sigma[0] = sg[0];
        mu[0] = sg[hw];
        v[0] = a.v[at];
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] = centroid(v[e], sigma[e], mu[e], q[e], inv_q[e]);
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(a.out + at) = make_float4(o[0], o[1], o[2], o[3]);
    else a.out[at] = o[0];
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// map: qpairs null for one pair (q, inv_q), else the step map, and q, inv_q are not read
int gauss_centroid(const char* who, const float* params, const float* v, float* out, int64_t streams, int channels, int64_t h,
                   int64_t w, float q, float inv_q, const float* qpairs, int64_t units, int64_t mh, int64_t mw, int shift,
                   bool map, void* stream) {
    LLDWT_REQUIRE(params && v && out, "%s: null pointer", who);
    LLDWT_REQUIRE(streams > 0 && channels > 0 && streams * channels <= 65535 && h > 0 && w > 0 && h * w < ((int64_t)1 << 31),
                  "%s: bad sizes (streams %lld, channels %d, grid %lld x %lld)", who, (long long)streams, channels, (long long)h,
                  (long long)w);
    if (map) {
        LLDWT_REQUIRE(qpairs && (reinterpret_cast<uintptr_t>(qpairs) & 7) == 0, "%s: null step map (or one not aligned to its pairs)",
                      who);
        LLDWT_REQUIRE(units > 0 && streams % units == 0, "%s: %lld streams are not whole planes of %lld units", who, (long long)streams,
                      (long long)units);
        LLDWT_REQUIRE(shift >= 0 && shift <= 30 && mh > 0 && mw > 0 && mh < ((int64_t)1 << 31) && mw < ((int64_t)1 << 31) &&
                          mh >= cdiv(h, (int64_t)1 << shift) && mw >= cdiv(w, (int64_t)1 << shift),
                      "%s: a %lld x %lld map at shift %d does not cover the %lld x %lld level", who, (long long)mh, (long long)mw, shift,
                      (long long)h, (long long)w);
    } else {
        // q > 0 and inv_q == fp32(1 / q) with the division in double: the pair as ops.step_pair / ops.layer_pair form it
        LLDWT_REQUIRE(q > 0.f && q <= 64.f && inv_q == (float)(1.0 / (double)q), "%s: step %g (1 / step %g) is not a pair (q, fp32(1 / q))",
                      who, (double)q, (double)inv_q);
    }
    ReconArgs a;
    a.params = params; a.v = v; a.out = out; a.C = channels; a.h = (int)h; a.w = (int)w; a.q = q; a.inv_q = inv_q;
    a.qpairs = qpairs; a.units = map ? (int)units : 1; a.mh = (int)mh; a.mw = (int)mw; a.shift = shift;
    const bool vec = w % 4 == 0 && aligned16(params) && aligned16(v) && aligned16(out);
    dim3 grid((unsigned)cdiv(cdiv(h * w, vec ? 4 : 1), NT), (unsigned)(streams * channels));
    if (map && vec) hipLaunchKernelGGL((k_gauss_centroid<4, true>), grid, dim3(NT), 0, (hipStream_t)stream, a);
    else if (map) hipLaunchKernelGGL((k_gauss_centroid<1, true>), grid, dim3(NT), 0, (hipStream_t)stream, a);
    else if (vec) hipLaunchKernelGGL((k_gauss_centroid<4, false>), grid, dim3(NT), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((k_gauss_centroid<1, false>), grid, dim3(NT), 0, (hipStream_t)stream, a);
    return check_launch(who);
}

}  // namespace

extern "C" int lldwt_gauss_centroid(const float* params, const float* v, float* out, int64_t streams, int channels, int64_t h,
                                    int64_t w, float q, float inv_q, void* stream) {
    return gauss_centroid("gauss_centroid", params, v, out, streams, channels, h, w, q, inv_q, nullptr, 1, 0, 0, 0, false, stream);
}

extern "C" int lldwt_gauss_centroid_map(const float* params, const float* v, float* out, int64_t streams, int64_t units, int channels,
                                        int64_t h, int64_t w, const float* qpairs, int64_t mh, int64_t mw, int shift, void* stream) {
    return gauss_centroid("gauss_centroid_map", params, v, out, streams, channels, h, w, 1.f, 1.f, qpairs, units, mh, mw, shift, true,
                          stream);
}
