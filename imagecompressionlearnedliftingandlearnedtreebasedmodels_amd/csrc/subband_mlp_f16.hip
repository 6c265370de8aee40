// subband_mlp_f16.hip -- SubbandAutoEncoder forward (lifting_dwt_nets.py:99-110): 1 -> 32 -> 32 -> 32 -> 1 per coefficient,
// tanh between, with the two 32 x 32 layers as split-fp16 products on v_mfma_f32_16x16x32_f16 (hi*hi + hi*lo + lo*hi, fp32
// accumulate: one layer's K = 32 is exactly one k-step, 3 MFMAs per 16 x 16 tile).
//
// A wave takes 64 coefficients (4 column tiles of 16).  A layer's output comes out of the MFMA as D[row = oc][col = coef] with
// lane (col, kk) holding rows 4kk..4kk+3 of both 16-row tiles m.  Those 8 values are the lane's 8 K-values of the NEXT layer's
// B fragment if K is taken in the order  k = 8kk + j,  j = m*4 + r  <->  channel m*16 + 4kk + r,  so the weights are packed in
// that permuted K order and no activation goes through LDS or a lane shuffle.  The 1 -> 32 layer is computed straight into the
// layout, the 32 -> 1 layer is a dot product over the lane's 8 rows plus two xor-shuffles across kk; both stay fp32 vector code.
//
// Scales.  Activations are tanh outputs in [-1, 1] and travel multiplied by 2^14 (the lifting kernels' convention); the factor is
// folded into the last fma of the tanh, fma(-2^15, r, 2^14) for fma(-2, r, 1), which changes no bit of the unscaled value.
// A layer's weights are multiplied by s = 2^k with max|W| * s in [2^14, 2^15) (pow2_scale<15>, k clamped to [-113, 112]) before
// the split; the accumulator is multiplied by the exact power of two 1 / (s * 2^14) where the bias is added.
//
// The pack (lldwt_subband_mlp_pack) is built once per weight update, for either orientation of the weights, so the kernel has
// one load path: per (plane, channel) SMLP_PC_FLOATS 32-bit words,
//   [0, 2048)     8 A fragments of 64 lanes x 8 halves, fragment f = (layer*2 + m)*2 + part (part 0 = hi, 1 = lo), lane
//                 (col, kk) holding  s_layer * W_layer[oc = m*16 + col][ic = (j>>2)*16 + 4kk + (j&3)],  j = 0..7
//   [2048, 2208)  w0, b0, b1, b2, w3 (in that order), each as [kk][j] = value of channel (j>>2)*16 + 4kk + (j&3)
//   [2208, 2216)  s_1, s_2, 1/(s_1 * 2^14), 1/(s_2 * 2^14), b3, 0, 0, 0
// The kernel ignores lldwt_set_precision: it is bound by its vector instructions, the lo products are hidden behind them.
#include "split_f16.h"

namespace lldwt {
namespace {

constexpr int SMLP_HD = 32;
constexpr int SMLP_A_FLOATS = 2048, SMLP_V_FLOATS = 160, SMLP_S_FLOATS = 8;
constexpr int SMLP_PC_FLOATS = SMLP_A_FLOATS + SMLP_V_FLOATS + SMLP_S_FLOATS;
constexpr float SMLP_ACT_SCALE = 16384.f;          // 2^14

// the lane's channel for slot j of its 8 rows / K-values
__device__ __forceinline__ int smlp_channel(int kk, int j) { return (j >> 2) * 16 + 4 * kk + (j & 3); }

// One wave per (plane, channel).
__global__ __launch_bounds__(64) void k_subband_mlp_pack(const float* __restrict__ w0, const float* __restrict__ b0,
                                                         const float* __restrict__ w1, const float* __restrict__ b1,
                                                         const float* __restrict__ w2, const float* __restrict__ b2,
                                                         const float* __restrict__ w3, const float* __restrict__ b3,
                                                         int transposed, float* __restrict__ pack) {
    constexpr int HD = SMLP_HD;
    const int64_t pc = blockIdx.x;
    const int lane = threadIdx.x, col = lane & 15, kk = lane >> 4;
    float* out = pack + pc * SMLP_PC_FLOATS;
    float scale[2];
#pragma unroll
    for (int layer = 0; layer < 2; ++layer) {
        const float* W = (layer == 0 ? w1 : w2) + pc * HD * HD;
        float amax = 0.f;
        for (int i = lane; i < HD * HD; i += 64) amax = fmaxf(amax, fabsf(W[i]));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
        const float s = fminf(fmaxf(pow2_scale<15>(amax), 0x1p-113f), 0x1p112f);
        scale[layer] = s;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int oc = m * 16 + col, ic = smlp_channel(kk, j);
                v[j] = W[transposed ? ic * HD + oc : oc * HD + ic] * s;
            }
            h8_t hi, lo;
            split8v(v, hi, lo);
            h8_t* frag = reinterpret_cast<h8_t*>(out) + ((layer * 2 + m) * 2) * 64 + lane;
            frag[0] = hi;
            frag[64] = lo;
        }
    }
    if (lane < 32) {
        const int k4 = lane >> 3, j = lane & 7, ch = smlp_channel(k4, j);
        const float* src[5] = {w0, b0, b1, b2, w3};
#pragma unroll
        for (int a = 0; a < 5; ++a) out[SMLP_A_FLOATS + a * 32 + lane] = src[a][pc * HD + ch];
    }
    if (lane < 8) {
        float v = 0.f;
        if (lane < 2) v = scale[lane];
        else if (lane < 4) v = (1.f / scale[lane - 2]) * (1.f / SMLP_ACT_SCALE);
        else if (lane == 4) v = b3[pc];
        out[SMLP_A_FLOATS + SMLP_V_FLOATS + lane] = v;
    }
}

// 2^14 * fast_tanh(x) (common.h), the factor folded into the last fma: 2^14 - 2^15 r is 2^14 (1 - 2r) bit for bit
__device__ __forceinline__ float tanh_act(float x) {
    const float e = __builtin_amdgcn_exp2f(fabsf(x) * 2.88539008177792681472f);
    const float t = __builtin_fmaf(-2.f * SMLP_ACT_SCALE, __builtin_amdgcn_rcpf(e + 1.f), SMLP_ACT_SCALE);
    return copysignf(t, x);
}

// A workgroup belongs to one (plane, channel) pair (blockIdx.y) and its waves stride over the 64-coefficient blocks of all
// images of that pair: block t = image t / nblk, coefficients (t % nblk) * 64 .. + 63 of it (the last block of an image may be
// partial; blocks never mix images).  The weights are fetched once per wave; the grid is one resident set of workgroups.
// Two workgroups per CU at least: with a 256-register budget the compiler keeps the MFMA results in VGPRs (left at one, it
// puts them in AGPRs and pays 64 v_accvgpr_read per block).
__global__ __launch_bounds__(256, 2) void k_subband_mlp_f16(const float* __restrict__ x, float* __restrict__ y, int batch, int C,
                                                         int64_t hw, int64_t nblk, const float* __restrict__ pack) {
    const int64_t pc = blockIdx.y;
    const int plane = (int)(pc / C), c = (int)(pc % C);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, kk = lane >> 4;
    const float* pk = pack + pc * SMLP_PC_FLOATS;
    h8_t A[2][2][2];                                            // [layer][m][hi, lo]
#pragma unroll
    for (int f = 0; f < 8; ++f) A[f >> 2][(f >> 1) & 1][f & 1] = reinterpret_cast<const h8_t*>(pk)[f * 64 + lane];
    float vec[5][8];                                            // w0, b0, b1, b2, w3 in the lane's channel order
#pragma unroll
    for (int a = 0; a < 5; ++a)
#pragma unroll
        for (int hlf = 0; hlf < 2; ++hlf) {
            const floatx4 v = reinterpret_cast<const floatx4*>(pk + SMLP_A_FLOATS)[(a * 4 + kk) * 2 + hlf];
#pragma unroll
            for (int r = 0; r < 4; ++r) vec[a][hlf * 4 + r] = v[r];
        }
    const floatx4 sc = reinterpret_cast<const floatx4*>(pk + SMLP_A_FLOATS + SMLP_V_FLOATS)[0];
    const float inv[2] = {sc[2], sc[3]};
    const float bb3 = pk[SMLP_A_FLOATS + SMLP_V_FLOATS + 4];
#pragma unroll
    for (int q = 0; q < 8; ++q) vec[4][q] *= 1.f / SMLP_ACT_SCALE;      // the last layer reads the scaled activations

    // block walk without a division per block: (img, blk) advances by the wave-uniform stride split into (images, blocks)
    const int64_t stride = (int64_t)gridDim.x * 4, first = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(wave);
    const int64_t simg = stride / nblk, sblk = stride - simg * nblk;
    int64_t img = first / nblk, blk = first - img * nblk;
    for (; img < batch; img += simg, blk += sblk) {
        if (blk >= nblk) {
            blk -= nblk;
            if (++img >= batch) break;
        }
        const int64_t i0 = blk * 64;
        const int64_t base = (((int64_t)plane * batch + img) * C + c) * hw;
        const float* xp = x + base;
        float* yp = y + base;
        float xv[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int64_t i = i0 + n * 16 + col;
            xv[n] = xp[i < hw ? i : 0];
        }
        float h[4][8];                                          // activations * 2^14 in B-fragment order: [column tile][j]
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int q = 0; q < 8; ++q) h[n][q] = tanh_act(fmaf(vec[0][q], xv[n], vec[1][q]));
#pragma unroll
        for (int layer = 0; layer < 2; ++layer) {
            f4_t acc[2][4];
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                h8_t hi, lo;
                split8v(h[n], hi, lo);
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    f4_t a = {0.f, 0.f, 0.f, 0.f};
                    a = mma16<0>(A[layer][m][1], hi, a);        // small terms first
                    a = mma16<0>(A[layer][m][0], lo, a);
                    acc[m][n] = mma16<0>(A[layer][m][0], hi, a);
                }
            }
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        h[n][m * 4 + r] = tanh_act(fmaf(acc[m][n][r], inv[layer], vec[2 + layer][m * 4 + r]));
        }
        float o[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            float s = 0.f;
#pragma unroll
            for (int q = 0; q < 8; ++q) s = fmaf(vec[4][q], h[n][q], s);
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            o[n] = s;
        }
        // every lane holds all four tiles' sums: lane (col, kk) stores tile kk, one 64-lane store per block
        const float ov = kk == 0 ? o[0] : kk == 1 ? o[1] : kk == 2 ? o[2] : o[3];
        const int64_t i = i0 + lane;
        if (i < hw) yp[i] = ov + bb3;
    }
}

}  // namespace
}  // namespace lldwt

using namespace lldwt;

extern "C" int64_t lldwt_subband_mlp_packed_bytes(int64_t planes, int C) {
    if (planes <= 0 || C <= 0) return 0;
    return planes * C * SMLP_PC_FLOATS * (int64_t)sizeof(float);
}

extern "C" int lldwt_subband_mlp_pack(const float* w0, const float* b0, const float* w1, const float* b1, const float* w2,
                                      const float* b2, const float* w3, const float* b3, int64_t planes, int C, int Hd,
                                      int transposed, void* pack, int64_t pack_bytes, void* stream) {
    LLDWT_REQUIRE(w0 && b0 && w1 && b1 && w2 && b2 && w3 && b3 && pack, "subband_mlp_pack: null pointer");
    LLDWT_REQUIRE(planes > 0 && C > 0 && planes * C <= 0x7fffffff, "subband_mlp_pack: bad dims");
    LLDWT_REQUIRE(Hd == SMLP_HD, "subband_mlp_pack: hidden width %d unsupported (reference uses H=32, lifting_dwt_nets.py:98)", Hd);
    LLDWT_REQUIRE(((uintptr_t)pack & 15) == 0, "subband_mlp_pack: pack must be 16-byte aligned");
    LLDWT_REQUIRE(pack_bytes >= lldwt_subband_mlp_packed_bytes(planes, C), "subband_mlp_pack: pack of %ld bytes, %ld needed",
                  (long)pack_bytes, (long)lldwt_subband_mlp_packed_bytes(planes, C));
    hipLaunchKernelGGL(k_subband_mlp_pack, dim3((unsigned)(planes * C)), dim3(64), 0, (hipStream_t)stream, w0, b0, w1, b1, w2, b2,
                       w3, b3, transposed, (float*)pack);
    return check_launch("subband_mlp_pack");
}

extern "C" int lldwt_subband_mlp(const float* x, float* y, int64_t planes, int64_t batch, int C, int64_t hw, int Hd,
                                 const void* pack, int64_t pack_bytes, void* stream) {
    LLDWT_REQUIRE(x && y && pack, "subband_mlp: null pointer");
    LLDWT_REQUIRE(planes > 0 && batch > 0 && C > 0 && hw > 0, "subband_mlp: bad dims");
    LLDWT_REQUIRE(Hd == SMLP_HD, "subband_mlp: hidden width %d unsupported (reference uses H=32, lifting_dwt_nets.py:98)", Hd);
    LLDWT_REQUIRE(planes * C <= 65535 && batch <= 0x7fffffff, "subband_mlp: grid too large");
    LLDWT_REQUIRE(((uintptr_t)pack & 15) == 0, "subband_mlp: pack must be 16-byte aligned");
    LLDWT_REQUIRE(pack_bytes >= lldwt_subband_mlp_packed_bytes(planes, C), "subband_mlp: pack of %ld bytes, %ld needed",
                  (long)pack_bytes, (long)lldwt_subband_mlp_packed_bytes(planes, C));
    // workgroups per (plane, channel) pair: one resident set of the device, never more than the pair's blocks need
    static int occ = 0;
    if (occ <= 0 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_subband_mlp_f16, 256, 0) != hipSuccess || occ <= 0)) {
        (void)hipGetLastError();
        occ = 2;
    }
    const int64_t nblk = cdiv(hw, 64), pairs = planes * C;
    int64_t g = (int64_t)lldwt_num_cus() * occ / pairs;
    if (g < 1) g = 1;
    if (g > cdiv(nblk * batch, 4)) g = cdiv(nblk * batch, 4);
    hipLaunchKernelGGL(k_subband_mlp_f16, dim3((unsigned)g, (unsigned)pairs), dim3(256), 0, (hipStream_t)stream, x, y, (int)batch,
                       C, hw, nblk, (const float*)pack);
    return check_launch("subband_mlp");
}
