// ztblock.hip -- one polyphase phase of DWTConditioned2EntropyLayerZTBlock's context model in one launch (the real coder of
// that layer, graphs/models/entropy_coding.py code_ztblock_level; reference nets: LiftingBasedDWT_net.py:618-624,716-744).
//
// A finer level splits into the phases ee (0::2,0::2), eo (0::2,1::2), oe (1::2,0::2), oo (1::2,1::2).  Phase k (1..4) of
// subband j is predicted from the k-channel dependency tensor [parent_j, ee_j, eo_j, oe_j][:k] by two 5-layer nets (sigma
// head, mu head): 3x3 k->32, 3x3 32->32, 1x1 32->32, 1x1 32->32, 1x1 32->1, LeakyReLU(0.01) between layers, zero padding.
// One launch covers every plane, image, the 3 subbands and both heads, and writes (sigma, mu) of the phase grid as
// params (P,B,6,h2,w2): sigma of subband j on channel 2j, mu on channel 2j+1.
//
// Inputs are read in place: the parent from (P,B,3,h2,w2), the decoded phases strided out of the level tensor
// (P,B,3,2*h2,2*w2).  Workgroup = one 8 x 16 output tile of one (plane, image, subband), 4 waves:
//   * stage the k input channels of the tile plus a 2-pixel halo in LDS (zero outside the phase grid);
//   * per head: conv1 over the tile plus a 1-pixel ring on the VALU (fixed-order fmaf chains), LeakyReLU, into LDS; ring
//     positions outside the phase grid hold 0 (conv2's zero padding applies to conv1's OUTPUT);
//   * conv2 (K = 288, tap-major / channel-minor) and the two 32->32 1x1 layers on v_mfma_f32_16x16x4_f32 (exact fp32: a
//     k-ordered fmaf chain per output); M = the 16 pixels of a tile row, N = 2 x 16 channels, each wave 2 rows x 2 N-blocks;
//   * the 32->1 layer per pixel on the VALU.
// Every output's reduction order is fixed and independent of the tile position, of P, B and of the other images in the
// launch: encoder and decoder compute the same (sigma, mu) to the bit.  No atomics.
#include "common.h"

namespace {

constexpr int TH = 8, TW = 16;                       // output tile (phase-grid pixels); TW = the MFMA M dimension
constexpr int IH = TH + 4, IW = TW + 4;              // input tile with the 2-pixel halo
constexpr int RH = TH + 2, RW = TW + 2;              // conv1 output: tile + 1-pixel ring
constexpr int HID = 32;
constexpr int CS = 36;                               // LDS row stride (floats) of a pixel's 32 channels (bank spread)
constexpr int NTHREADS = 256;

// packed record of one (plane, subband, head), in floats
constexpr int KS2 = 9 * HID / 4;                     // 72 k-steps of conv2
constexpr int OFF_W2 = 0;                            // [72][2][64]  B fragments of conv2
constexpr int OFF_W3 = OFF_W2 + KS2 * 2 * 64;        // [8][2][64]   B fragments of the first 1x1
constexpr int OFF_W4 = OFF_W3 + 8 * 2 * 64;          // [8][2][64]   B fragments of the second 1x1
constexpr int OFF_W1 = OFF_W4 + 8 * 2 * 64;          // [36][32]     conv1, row ci*9 + tap (ci < 4, zero rows past k)
constexpr int OFF_B1 = OFF_W1 + 36 * HID;
constexpr int OFF_B2 = OFF_B1 + HID;
constexpr int OFF_B3 = OFF_B2 + HID;
constexpr int OFF_B4 = OFF_B3 + HID;
constexpr int OFF_W5 = OFF_B4 + HID;                 // [32]
constexpr int OFF_B5 = OFF_W5 + HID;                 // [1], padded to 32
constexpr int REC = OFF_B5 + HID;

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float lrelu(float v) { return v >= 0.f ? v : 0.01f * v; }

// D (2 rows x 2 N-blocks of 16x16) += A (pixels x K, from LDS rows of stride CS) * B (packed fragments), K = 4 * nks.
// a_row(r, s) -> LDS float index of the A element (pixel = lane & 15, k = 4 s + lane >> 4) for tile row r.
template <int NKS, typename ARow>
__device__ __forceinline__ void mfma_rows(const float* __restrict__ lds, const float* __restrict__ wfrag, int lane, int r0,
                                          ARow a_row, f32x4 (&acc)[2][2]) {
#pragma unroll 4
    for (int s = 0; s < NKS; ++s) {
        const float b0 = wfrag[(s * 2 + 0) * 64 + lane];
        const float b1 = wfrag[(s * 2 + 1) * 64 + lane];
        const float a0 = lds[a_row(r0, s)];
        const float a1 = lds[a_row(r0 + 1, s)];
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
}

// bias + LeakyReLU of the accumulators, stored as out[pixel][channel] (C/D map: row = 4 (lane >> 4) + reg, col = lane & 15)
__device__ __forceinline__ void store_rows(float* __restrict__ out, const float* __restrict__ bias, int lane, int r0,
                                           const f32x4 (&acc)[2][2]) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int ch = n * 16 + (lane & 15);
            const float b = bias[ch];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int px = (r0 + m) * TW + (lane >> 4) * 4 + r;
                out[px * CS + ch] = lrelu(acc[m][n][r] + b);
            }
        }
}

__global__ void __launch_bounds__(NTHREADS) k_ztblock_phase(const float* __restrict__ parent, const float* __restrict__ level,
                                                            const float* __restrict__ packed, float* __restrict__ params,
                                                            int B, int h2, int w2, int k, int tiles_x) {
    __shared__ float in_s[4 * IH * IW];
    __shared__ float act1[RH * RW * CS];
    __shared__ float act2[TH * TW * CS];
    float* const act3 = act1;                           // conv1's output is dead once conv2 has read it
    __shared__ float w1s[36 * HID];
    __shared__ float smalls[4 * HID];                   // b1, b2, b3, b4
    __shared__ float w5s[HID + 1];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x;
    const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
    const int j = blockIdx.y;                           // subband
    const int z = blockIdx.z;                           // plane * B + image
    const int p = z / B;
    const int64_t hw = (int64_t)h2 * w2;
    const int H = 2 * h2, W = 2 * w2;

    // ---- input tile + 2-pixel halo, zero outside the phase grid
    const float* par = parent + ((int64_t)z * 3 + j) * hw;
    const float* lev = level ? level + ((int64_t)z * 3 + j) * (int64_t)H * W : nullptr;
    for (int e = tid; e < k * IH * IW; e += NTHREADS) {
        const int c = e / (IH * IW), rem = e - c * IH * IW;
        const int gy = y0 - 2 + rem / IW, gx = x0 - 2 + rem % IW;
        float v = 0.f;
        if (gy >= 0 && gy < h2 && gx >= 0 && gx < w2) {
            if (c == 0) {
                v = par[(int64_t)gy * w2 + gx];
            } else {                                    // c = 1 ee, 2 eo, 3 oe
                const int ry = (c == 3), rx = (c == 2);
                v = lev[(int64_t)(2 * gy + ry) * W + 2 * gx + rx];
            }
        }
        in_s[e] = v;
    }

    for (int head = 0; head < 2; ++head) {
        const float* rec = packed + ((int64_t)(p * 3 + j) * 2 + head) * REC;
        for (int e = tid; e < k * 9 * HID; e += NTHREADS) w1s[e] = rec[OFF_W1 + e];
        if (tid < 4 * HID) smalls[tid] = rec[OFF_B1 + tid];
        if (tid < HID + 1) w5s[tid] = rec[OFF_W5 + tid];
        __syncthreads();

        // ---- conv1 (k -> 32) on the tile + ring, LeakyReLU; 0 at ring positions outside the grid
        for (int e = tid; e < RH * RW * HID; e += NTHREADS) {
            const int co = e & (HID - 1), pos = e >> 5;
            const int ry = pos / RW, rx = pos - ry * RW;
            const int gy = y0 - 1 + ry, gx = x0 - 1 + rx;
            float v = 0.f;
            if (gy >= 0 && gy < h2 && gx >= 0 && gx < w2) {
                float a = smalls[co];
                for (int ci = 0; ci < k; ++ci) {
                    const float* src = in_s + ci * IH * IW + ry * IW + rx;
                    const float* w = w1s + ci * 9 * HID + co;
#pragma unroll
                    for (int t = 0; t < 9; ++t) a = fmaf(w[t * HID], src[(t / 3) * IW + t % 3], a);
                }
                v = lrelu(a);
            }
            act1[pos * CS + co] = v;
        }
        __syncthreads();

        // ---- conv2 (32 -> 32, K = 288) on the matrix cores; wave w owns tile rows 2w, 2w+1
        const int r0 = 2 * wave;
        {
            f32x4 acc[2][2] = {};
            mfma_rows<KS2>(act1, rec + OFF_W2, lane, r0, [lane](int r, int s) {
                const int tap = s >> 3, ci = (s & 7) * 4 + (lane >> 4);
                return ((r + tap / 3) * RW + (lane & 15) + tap % 3) * CS + ci;
            }, acc);
            store_rows(act2, smalls + HID, lane, r0, acc);
        }
        __syncthreads();
        // ---- the two 32 -> 32 1x1 layers
        const auto a_pix = [lane](int r, int s) { return (r * TW + (lane & 15)) * CS + s * 4 + (lane >> 4); };
        {
            f32x4 acc[2][2] = {};
            mfma_rows<8>(act2, rec + OFF_W3, lane, r0, a_pix, acc);
            store_rows(act3, smalls + 2 * HID, lane, r0, acc);
        }
        __syncthreads();
        {
            f32x4 acc[2][2] = {};
            mfma_rows<8>(act3, rec + OFF_W4, lane, r0, a_pix, acc);
            store_rows(act2, smalls + 3 * HID, lane, r0, acc);
        }
        __syncthreads();
        // ---- 32 -> 1 per pixel
        if (tid < TH * TW) {
            const int ty = tid / TW, tx = tid % TW;
            const int gy = y0 + ty, gx = x0 + tx;
            if (gy < h2 && gx < w2) {
                float a = w5s[HID];
                const float* src = act2 + tid * CS;
#pragma unroll
                for (int c = 0; c < HID; ++c) a = fmaf(w5s[c], src[c], a);
                params[((int64_t)z * 6 + 2 * j + (head == 0 ? 0 : 1)) * hw + (int64_t)gy * w2 + gx] = a;
            }
        }
        __syncthreads();                                // LDS weights / activations are rewritten by the next head
    }
}

}  // namespace

extern "C" int64_t lldwt_ztblock_packed_floats(void) { return REC; }

extern "C" int lldwt_ztblock_phase(const float* parent, const float* level, const float* packed, float* params, int64_t planes,
                                   int64_t batch, int64_t h2, int64_t w2, int64_t H, int64_t W, int k, void* stream) {
    LLDWT_REQUIRE(k >= 1 && k <= 4, "ztblock_phase: phase k must be 1..4 (got %d)", k);
    LLDWT_REQUIRE(parent && packed && params && (level || k == 1), "ztblock_phase: null pointer");
    LLDWT_REQUIRE(planes > 0 && batch > 0 && planes * batch <= 65535 && h2 > 0 && w2 > 0 && h2 <= (1 << 24) && w2 <= (1 << 24),
                  "ztblock_phase: bad sizes (planes %lld, batch %lld, grid %lld x %lld)", (long long)planes, (long long)batch,
                  (long long)h2, (long long)w2);
    LLDWT_REQUIRE(H == 2 * h2 && W == 2 * w2, "ztblock_phase: level %lld x %lld is not twice the parent / phase grid %lld x %lld",
                  (long long)H, (long long)W, (long long)h2, (long long)w2);
    const int64_t tx = lldwt::cdiv(w2, TW), ty = lldwt::cdiv(h2, TH);
    LLDWT_REQUIRE(tx * ty <= 0x7fffffff, "ztblock_phase: grid too large");
    dim3 grid((unsigned)(tx * ty), 3u, (unsigned)(planes * batch));
    hipLaunchKernelGGL(k_ztblock_phase, grid, dim3(NTHREADS), 0, (hipStream_t)stream, parent, level, packed, params, (int)batch,
                       (int)h2, (int)w2, k, (int)tx);
    return lldwt::check_launch("ztblock_phase");
}
