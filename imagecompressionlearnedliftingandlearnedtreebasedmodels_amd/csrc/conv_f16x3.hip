// conv_f16x3.hip -- dense 3x3 convolution with fp32-level accuracy on the fp16 matrix cores ("split-fp16", f16x3).
//
// Target: the tree-context conv 243 -> 243, 3x3 (LiftingBasedDWT_net.py:271-272, :793-795) -- 61 % of the headline
// step's FLOPs and, on the fp32 MFMA (v_mfma_f32_16x16x4_f32, 64 FLOP/clk/SIMD), bound at 157 TFLOP/s.  The fp16 MFMA
// (v_mfma_f32_32x32x16_f16) runs 16x that rate.  Every fp32 operand is split EXACTLY-to-2^-22 into two fp16 values
//     v = s * x  (s a power of two chosen so that max|v| is in [2^14, 2^15): no overflow, lo stays a normal number)
//     hi = fp16(v),  lo = fp16(v - hi)            |v - hi - lo| <= 2^-22 |v|
// and the product is accumulated in fp32 from three MFMAs:  x*w ~ hi_x*hi_w + hi_x*lo_w + lo_x*hi_w  (the dropped
// lo*lo term is 2^-22 relative).  fp16 x fp16 products are exact in fp32, so the result carries ~2^-21 relative error
// per product -- the same order as the fp32 fmaf chain's own accumulation error at K = 2187 (3.5e-7) -- at 16/3 = 5.3x
// fewer matrix cycles.  bf16 would not do: its 8-bit mantissa gives 2^-16 per split pair, 64x worse.
// The scales are powers of two, so applying 1/(s_x*s_w) to the accumulator is exact.
//   s_w: per plane, fixed at pack time (lldwt_conv_f16x3_pack).   s_x: per plane, from the |x| maximum of the input
//   tensor, produced on the device by lldwt_absmax_slots (no host sync) and read by the conv kernel.
//
// Kernel shape (one 256-thread workgroup per CU, ONE wave per SIMD with the whole 512-entry register file):
//   workgroup tile = 128 output channels x (8 rows x 32 pixels); wave w owns channels 32w..32w+31 x all 256 pixels
//   = 8 accumulator tiles of 32x32 (128 VGPRs).  K loop = 8 chunks of 32 input channels x 9 taps x 2 k-steps of 16.
//   B (activations): fp32 planes -> registers -> split -> LDS image [10x34 pixels][32 ch] fp16, pixel pitch 80 B
//      (20 dwords: 16 lanes of a ds_read_b128 group hit 64 distinct banks), hi and lo images, double-buffered, so the
//      global loads of chunk c+1 fly during the MFMAs of chunk c and there is one barrier per chunk.
//   A (weights): pre-split, pre-packed in lane order per (wave, chunk, tap, k-step): each wave streams ITS fragments
//      straight from L2 into registers (1 KB coalesced per instruction, no LDS), two k-steps ahead.
#include "common.h"
#include "split_f16.h"
#include "lifting_f16.h"      // split_precision(): the one-product fp16 / bf16 modes of the fused pair (lldwt_set_precision)
#include "plc_fold.h"         // plc_fold_pays(): one workgroup per tile or per (tile, channel block) in k_plc_wino
#include <string.h>
#include <type_traits>

namespace lldwt {

constexpr int F3_CK = 32;                       // input channels per chunk
constexpr int F3_TH = 8, F3_TW = 32;            // output pixels per workgroup
constexpr int F3_IH = F3_TH + 2, F3_IW = F3_TW + 2, F3_NPX = F3_IH * F3_IW;   // 10 x 34 = 340 staged pixels
constexpr int F3_PITCH = F3_CK * 2 + 16;        // 80 B per pixel
constexpr int F3_PART = F3_NPX * F3_PITCH;      // 27,200 B: one image (hi or lo)
constexpr int F3_BUF = 2 * F3_PART;             // hi + lo
constexpr int F3_LDS = 2 * F3_BUF + 64;         // double buffer: 108,800 B + a 64-B dump slot for dead staging tasks
constexpr int F3_OCB = 128;                     // output channels per workgroup
constexpr int F3_STEP_BYTES = 2048;             // one (tap, k-step) of one wave: hi fragment + lo fragment, 1 KB each
constexpr int F3_CHUNK_BYTES = 9 * 2 * F3_STEP_BYTES;
constexpr int F3_HDR = 256;                     // per-plane header: [0] = s_w
constexpr int F3_NTASK = F3_NPX * (F3_CK / 8);  // staging tasks (pixel, group of 8 channels) per chunk
constexpr int F3_R = (F3_NTASK + 255) / 256;    // per thread: 6

constexpr int F1_HDR = 2048;                    // conv1 pack: [0] s_w1, [1] max row L1 norm, [2] max |b|; floats [16 .. 16+256) bias
constexpr int F1_CHUNK_BYTES = 2 * F3_STEP_BYTES;   // 2 k-steps (K = 27 -> 32) x (hi, lo)
constexpr int F1_NBLK = (F3_NPX + 31) / 32;     // 11 pixel blocks of 32 cover the 340-pixel patch (12 slots: 3 per wave)
constexpr int F1_COL = 12 * 4 * 1024;           // the split im2col of the parent patch, [block][k-step][hi|lo][lane][8 x fp16]
constexpr int F1_PP = 3 * 6 * 18;               // parent values under a tile (see the kernel)
constexpr int F1_LDS = F3_LDS + F1_COL + 1536;  // + the parent patch: 159,552 B
// behind the (hi, lo) fp16 fragments: a bf16 copy of the scaled weights, half a step's bytes per step (one-product bf16 mode)
static inline int64_t f1_bf_off(int cmid) { return F1_HDR + (int64_t)cdiv(cmid, F3_CK) * F1_CHUNK_BYTES; }
// then the 16x16x32 fragments of the Winograd kernel (k_plc_wino): [chunk of 16 channels][hi|lo][lane][8 x fp16],
// A[row = channel lane&15][k = 8*(lane>>4) + j]
constexpr int W3_CK = 16;                       // input channels per chunk of the Winograd kernel
static inline __host__ __device__ int w3_nch(int cin) { return (cin + W3_CK - 1) / W3_CK; }
static inline __host__ __device__ int64_t f1_w16_off(int cmid) {
    const int nch = (cmid + F3_CK - 1) / F3_CK;
    return F1_HDR + (int64_t)nch * F1_CHUNK_BYTES + (int64_t)nch * (F1_CHUNK_BYTES / 2);
}
static inline int64_t f1_plane_bytes(int cmid) { return f1_w16_off(cmid) + (int64_t)w3_nch(cmid) * F3_STEP_BYTES; }

static inline int f3_nch(int cin) { return (int)cdiv(cin, F3_CK); }
static inline int f3_nocb(int cout) { return (int)cdiv(cout, F3_OCB); }
static inline __host__ __device__ int64_t f3_bf_off_n(int nocb, int nch) {
    // + 5 steps of padding: the kernel prefetches weight fragments 5 steps ahead without a bounds branch
    return F3_HDR + (int64_t)nocb * 4 * nch * F3_CHUNK_BYTES + 5 * F3_STEP_BYTES;
}
// the (hi, lo) fp16 steps, then a bf16 copy at half the bytes per step (same 5 steps of padding), then the Winograd section of
// k_plc_wino: [hdr: s_u][ocb][wave][chunk of 16][12 steps (dy, xi)][hi|lo][lane][8 x fp16] + 5 steps of padding
constexpr int W3_NST = 12;                       // weight steps (dy, xi) per chunk
static inline __host__ __device__ int64_t f3_wino_off(int cin, int cout) {
    const int nocb = (cout + F3_OCB - 1) / F3_OCB, nch = (cin + F3_CK - 1) / F3_CK;
    return f3_bf_off_n(nocb, nch) + (int64_t)nocb * 4 * nch * (F3_CHUNK_BYTES / 2) + 5 * (F3_STEP_BYTES / 2);
}
static inline int64_t f3_plane_bytes(int cin, int cout) {
    return f3_wino_off(cin, cout) + F3_HDR + (int64_t)f3_nocb(cout) * 4 * w3_nch(cin) * W3_NST * F3_STEP_BYTES + 5 * F3_STEP_BYTES;
}

// ---- |x| maximum per plane into 64 slots (spreads the atomics; the consumer takes the max of the 64)
__global__ void k_absmax_slots(const float* __restrict__ x, int64_t n_per_plane, float* __restrict__ slots, int vec) {
    const int plane = blockIdx.y;
    const float* xp = x + (int64_t)plane * n_per_plane;
    float m = 0.f;
    if (vec) {                     // every plane base is 16-byte aligned and n_per_plane % 4 == 0 (checked by the host)
        const float4* p = reinterpret_cast<const float4*>(xp);
        const int64_t n4 = n_per_plane >> 2;
        for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
            const float4 v = p[i];
            m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
        }
    } else {
        for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_per_plane; i += (int64_t)gridDim.x * blockDim.x)
            m = fmaxf(m, fabsf(xp[i]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_down(m, o, 64));
    if ((threadIdx.x & 63) == 0 && m > 0.f)
        atomicMax(reinterpret_cast<int*>(slots + plane * 64 + (blockIdx.x & 63)), __float_as_int(m));   // m >= 0: int order == float order
}

// ---- weight pack: (planes, cout, cin, 3, 3) fp32 -> per plane [hdr][ocb][wave][chunk][tap][ks][hi|lo][lane][8 x fp16]
__global__ void k_f3_wmax(const float* __restrict__ w, int64_t n_per_plane, float* __restrict__ hdr_base, int64_t plane_bytes) {
    const int plane = blockIdx.y;
    float m = 0.f;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_per_plane; i += (int64_t)gridDim.x * blockDim.x)
        m = fmaxf(m, fabsf(w[(int64_t)plane * n_per_plane + i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_down(m, o, 64));
    float* hdr = reinterpret_cast<float*>(reinterpret_cast<char*>(hdr_base) + (int64_t)plane * plane_bytes);
    if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(reinterpret_cast<int*>(hdr + 1), __float_as_int(m));   // hdr[1] = max|w|
}

// shape16: fragments for v_mfma_f32_16x16x32_f16 -- the two "k-steps" of a tap become the two 16-channel halves of the wave's 32
// output channels, each spanning the chunk's 32 input channels: A[row = lane&15][k = 8*(lane>>4) + j]
__global__ void k_f3_pack(const float* __restrict__ w, uint8_t* __restrict__ packed, int cin, int cout, int64_t plane_bytes,
                          int shape16) {
    const int plane = blockIdx.y;
    uint8_t* pp = packed + (int64_t)plane * plane_bytes;
    float* hdr = reinterpret_cast<float*>(pp);
    const float sw = pow2_scale<15>(hdr[1]);
    const int nch = (cin + F3_CK - 1) / F3_CK, nocb = (cout + F3_OCB - 1) / F3_OCB;
    const int64_t nfrag_elems = (int64_t)nocb * 4 * nch * 9 * 2 * 64 * 8;       // (hi, lo) pairs
    const float* wp = w + (int64_t)plane * cout * cin * 9;
    _Float16* out = reinterpret_cast<_Float16*>(pp + F3_HDR);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nfrag_elems; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t r = i;
        const int j = (int)(r % 8); r /= 8;
        const int lane = (int)(r % 64); r /= 64;
        const int ks = (int)(r % 2); r /= 2;
        const int tap = (int)(r % 9); r /= 9;
        const int chunk = (int)(r % nch); r /= nch;
        const int wv = (int)(r % 4); r /= 4;
        const int ocb = (int)r;
        const int oc = shape16 ? ocb * F3_OCB + wv * 32 + ks * 16 + (lane & 15)
                               : ocb * F3_OCB + wv * 32 + (lane & 31);          // A[row = lane&31][k = 8*(lane>>5) + j]
        const int ic = shape16 ? chunk * F3_CK + 8 * (lane >> 4) + j : chunk * F3_CK + ks * 16 + 8 * (lane >> 5) + j;
        float v = 0.f;
        if (oc < cout && ic < cin) v = wp[((int64_t)oc * cin + ic) * 9 + tap] * sw;
        const _Float16 hi = (_Float16)v;
        const _Float16 lo = (_Float16)(v - (float)hi);
        const int64_t step = ((((int64_t)(ocb * 4 + wv) * nch + chunk) * 9 + tap) * 2 + ks);
        out[step * 1024 + lane * 8 + j] = hi;                                   // 1024 halves = 2048 B per step
        out[step * 1024 + 512 + lane * 8 + j] = lo;
        reinterpret_cast<__bf16*>(pp + f3_bf_off_n(nocb, nch))[step * 512 + lane * 8 + j] = (__bf16)v;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) hdr[0] = sw;
}

// ---- FUSED mode: first tree conv (cmid, 3, 3, 3) -> per plane [hdr | chunk][ks][hi|lo][lane][8 x fp16]
// A[row = channel of the chunk][k = ci*9 + tap], k < 27
__global__ void k_f1_pack(const float* __restrict__ w1, const float* __restrict__ b1, uint8_t* __restrict__ packed, int cmid,
                          int64_t plane_bytes) {
    const int plane = blockIdx.x, tid = threadIdx.x;
    const float* wp = w1 + (int64_t)plane * cmid * 27;
    const float* bp = b1 + (int64_t)plane * cmid;
    uint8_t* pp = packed + (int64_t)plane * plane_bytes;
    float* hdr = reinterpret_cast<float*>(pp);
    __shared__ float red[3][4];
    float mw = 0.f, ml1 = 0.f, mb = 0.f;
    for (int r = tid; r < cmid; r += 256) {
        float s1 = 0.f;
        for (int k = 0; k < 27; ++k) {
            const float v = fabsf(wp[r * 27 + k]);
            s1 += v;
            mw = fmaxf(mw, v);
        }
        ml1 = fmaxf(ml1, s1);
        mb = fmaxf(mb, fabsf(bp[r]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mw = fmaxf(mw, __shfl_xor(mw, o, 64));
        ml1 = fmaxf(ml1, __shfl_xor(ml1, o, 64));
        mb = fmaxf(mb, __shfl_xor(mb, o, 64));
    }
    if ((tid & 63) == 0) { red[0][tid >> 6] = mw; red[1][tid >> 6] = ml1; red[2][tid >> 6] = mb; }
    __syncthreads();
    const float amw = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
    const float sw1 = pow2_scale<15>(amw);
    if (tid == 0) {
        hdr[0] = sw1;
        hdr[1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
        hdr[2] = fmaxf(fmaxf(red[2][0], red[2][1]), fmaxf(red[2][2], red[2][3]));
    }
    const int nch = (cmid + F3_CK - 1) / F3_CK;
    for (int i = tid; i < nch * F3_CK; i += 256) hdr[16 + i] = i < cmid ? bp[i] : 0.f;
    _Float16* fr = reinterpret_cast<_Float16*>(pp + F1_HDR);
    for (int i = tid; i < nch * 2 * 512; i += 256) {
        const int j = i & 7, lane = (i >> 3) & 63, ks = (i >> 9) & 1, chunk = i >> 10;
        const int c = chunk * F3_CK + (lane & 31), k = 16 * ks + 8 * (lane >> 5) + j;
        float v = 0.f;
        if (c < cmid && k < 27) v = wp[c * 27 + k] * sw1;
        const _Float16 hi = (_Float16)v;
        fr[(chunk * 2 + ks) * 1024 + lane * 8 + j] = hi;
        fr[(chunk * 2 + ks) * 1024 + 512 + lane * 8 + j] = (_Float16)(v - (float)hi);
        reinterpret_cast<__bf16*>(pp + F1_HDR + (int64_t)nch * F1_CHUNK_BYTES)[(chunk * 2 + ks) * 512 + lane * 8 + j] = (__bf16)v;
    }
    _Float16* f16 = reinterpret_cast<_Float16*>(pp + f1_w16_off(cmid));
    for (int i = tid; i < w3_nch(cmid) * 512; i += 256) {
        const int j = i & 7, lane = (i >> 3) & 63, chunk = i >> 9;
        const int c = chunk * W3_CK + (lane & 15), k = 8 * (lane >> 4) + j;
        float v = 0.f;
        if (c < cmid && k < 27) v = wp[c * 27 + k] * sw1;
        const _Float16 hi = (_Float16)v;
        f16[chunk * 1024 + lane * 8 + j] = hi;
        f16[chunk * 1024 + 512 + lane * 8 + j] = (_Float16)(v - (float)hi);
    }
}

struct F3Args {
    const float* x;
    float* y;
    const uint8_t* packed;
    const float* bias;
    const float* slots;
    const _Float16* x16;     // IN16: the input tensor stored as fp16 (already multiplied by xscale[plane]); x is unused
    const float* xscale;     // IN16: (planes) power-of-two storage scale of x16
    const float* parent;     // FUSED: (planes*batch, 3, h/2, w/2) fp32, the tensor the FIRST tree conv reads (2x-upsampled)
    const uint8_t* packed1;  // FUSED: first conv's split-fp16 fragments + bias + bounds (lldwt_plc_fused_pack1)
    int64_t plane_bytes1;
    int cin, cout, act, batch, h, w, tiles_x, nch;
    int64_t plane_bytes;
    unsigned long long* stamps;   // diagnostics only (lldwt_set_diagnostics kind 1): [workgroup][wave][16] s_memtime stamps
};
// in-kernel clock stamps of a diagnostic run (tools/plc_stamps.py); a null pointer (always, outside that tool) skips them
#define F3_STAMP(i)                                                                                                     \
    if (a.stamps && lane == 0)                                                                                          \
        a.stamps[((((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 4 + wave) * 16 + (i)] =   \
            (i) >= 14 ? __builtin_amdgcn_s_memrealtime() : __builtin_amdgcn_s_memtime();

// IN16 = false: fp32 input, split on the way into LDS, three MFMA products per k-step (fp32-level accuracy).
// IN16 = true : "fp16 storage" (BASELINE configs[4]): the input tensor lives in HBM as fp16 (half the bytes), it is the hi
//               part and there is no lo: two products (w_hi x + w_lo x), 2^-11 relative on the activations.
// MODE 2 (FUSED): the input tensor does not exist.  It is LeakyReLU(conv3x3(3 -> cin) of the 2x-upsampled parent), and
//               each chunk of 32 of its channels is computed ON THE FLY for the 10 x 34 patch by the matrix cores
//               (M = 32 channels, N = pixels, K = 27 -> 32; B = the im2col of the parent patch, gathered and split ONCE per
//               tile and kept in registers) and written straight into the LDS image that the second conv reads: no first
//               conv launch, no 243-channel tensor in HBM (1.5 GB written + 2 GB read per level-0 launch), no global
//               staging loads, no |x|-max pass (the activation scale comes from a per-workgroup bound).
// PREC (FUSED only; lldwt_set_precision): 0 = three products per MAC as above; 1 / 2 = ONE product on fp16 / bf16 operands -- the
//               lo images and lo fragments are neither written nor read, a third of the MFMAs.
// S16: the second conv's MFMAs in the 16x16x32 shape (same cycles per MAC; the chip holds a higher clock on it under this MFMA
//               density -- MI355X guide, DVFS item 7 -- measured here, see DESIGN): wave tile still 32 channels x 256 pixels,
//               as 2 channel halves x 16 blocks of 16 pixels; one MFMA k-step spans the chunk's 32 channels, so a tap is ONE step
//               of 2 A fragments; same LDS image, same number of fragment reads and weight bytes.  Weights packed for the shape
//               (k_f3_pack shape16): the shape is a process-wide choice (LLDWT_PLC_SHAPE=16; the default is 32x32x16, the faster one here).
template <int MODE, int PREC = 0, bool S16 = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_conv3_f16x3(F3Args a) {
    constexpr bool IN16 = MODE == 1, FUSED = MODE == 2;
    static_assert(PREC == 0 || FUSED, "the one-product modes exist for the fused pair (eval path)");
    constexpr int SB = PREC == 2 ? F3_STEP_BYTES / 2 : F3_STEP_BYTES;      // bytes per weight step in the section being read
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t z = blockIdx.z;
    const int plane = (int)(z / a.batch);
    const int ocb = blockIdx.y;
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int y0 = ty * F3_TH, x0 = tx * F3_TW;
    const int h = a.h, w = a.w;
    const int64_t hw = (int64_t)h * w;

    F3_STAMP(0)
    F3_STAMP(14)
    // ---- scales (exact powers of two)
    float sx = 1.f;
    if constexpr (IN16) {
        sx = a.xscale[plane];
    } else if constexpr (FUSED) {
        // set after the parent patch has been gathered (below)
    } else {
        float amax = a.slots[plane * 64 + lane];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
        sx = pow2_scale<15>(amax);
    }
    const uint8_t* pp = a.packed + (int64_t)plane * a.plane_bytes;
    const float sw = *reinterpret_cast<const float*>(pp);
    float out_scale = (1.f / sx) * (1.f / sw);

    // ---- staging tasks of this thread: (pixel p of the 10x34 patch, group of 8 channels icg).  Branch-free: padding
    // pixels and dead tasks load pixel 0 of a real plane and are zeroed at the split; dead tasks store to a dump slot.
    unsigned pix[F3_R];         // byte offset of the pixel inside a channel plane (0 for padding / dead tasks)
    int icg8[F3_R];             // first channel of the task's group inside the chunk
    int woff[F3_R];             // LDS byte offset inside a part
    bool inimg[F3_R];
#pragma unroll
    for (int r = 0; r < F3_R; ++r) {
        const int task = tid + r * 256;
        const bool live = task < F3_NTASK;
        const int icg = live ? task / F3_NPX : 0, p = live ? task - icg * F3_NPX : 0;
        const int ly = p / F3_IW, lx = p - ly * F3_IW;
        const int gy = y0 - 1 + ly, gx = x0 - 1 + lx;
        const bool in = live && gy >= 0 && gy < h && gx >= 0 && gx < w;
        inimg[r] = in;
        icg8[r] = icg * 8;
        woff[r] = p * F3_PITCH + icg * 16;
        pix[r] = in ? (IN16 ? 2u : 4u) * (unsigned)(gy * w + gx) : 0u;
    }
    using in_t = typename std::conditional<IN16, _Float16, float>::type;
    const in_t* xg = (IN16 ? reinterpret_cast<const in_t*>(a.x16) : reinterpret_cast<const in_t*>(a.x)) + z * (int64_t)a.cin * hw;
    const unsigned hw4 = (IN16 ? 2u : 4u) * (unsigned)hw;
    in_t xin[F3_R][8];

    // loads of staging task R of the chunk whose first channel is C1 (channels past cin-1 read plane cin-1, zeroed later)
#define F3_TASK_LOAD(R, C1)                                                                                           \
    {                                                                                                                 \
        const char* cb_ = reinterpret_cast<const char*>(xg + (int64_t)(C1) * hw);       /* wave-uniform */            \
        const unsigned rcmax_ = (unsigned)(a.cin - 1 - (C1));                                                         \
        _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                                               \
            const unsigned rc_ = min((unsigned)(icg8[R] + j), rcmax_);                                                \
            xin[R][j] = *reinterpret_cast<const in_t*>(cb_ + (rc_ * hw4 + pix[R]));                                   \
        }                                                                                                             \
    }
    // split + store of channels 4*HALF .. 4*HALF+3 of staging task R into the LDS buffer at DST
#define F3_TASK_STORE(R, HALF, C1, DST)                                                                               \
    {                                                                                                                 \
        typedef _Float16 half4_ __attribute__((ext_vector_type(4)));                                                  \
        half4_ hi_, lo_;                                                                                              \
        const bool dead_ = (tid + (R) * 256) >= F3_NTASK;                                                             \
        uint8_t* d_ = dead_ ? lds + 2 * F3_BUF + (HALF) * 8 : (DST) + woff[R] + (HALF) * 8;                           \
        if constexpr (IN16) {                                                                                         \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                           \
                const bool ok_ = inimg[R] && ((C1) + icg8[R] + (HALF) * 4 + j) < a.cin;                               \
                hi_[j] = ok_ ? (_Float16)xin[R][(HALF) * 4 + j] : (_Float16)0.f;                                      \
            }                                                                                                         \
            *reinterpret_cast<half4_*>(d_) = hi_;                                                                     \
        } else {                                                                                                      \
            float v4_[4];                                                                                             \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                           \
                const bool ok_ = inimg[R] && ((C1) + icg8[R] + (HALF) * 4 + j) < a.cin;                               \
                v4_[j] = ok_ ? (float)xin[R][(HALF) * 4 + j] * sx : 0.f;                                              \
            }                                                                                                         \
            split4v(v4_, hi_, lo_);                                                                                   \
            *reinterpret_cast<half4_*>(d_) = hi_;                                                                     \
            *reinterpret_cast<half4_*>(d_ + (dead_ ? 16 : F3_PART)) = lo_;                                            \
        }                                                                                                             \
    }

    typedef float floatx4 __attribute__((ext_vector_type(4)));
    floatx16 acc[S16 ? 1 : 8];
    floatx4 acc16[S16 ? 2 : 1][S16 ? 16 : 1];       // S16: [channel half][pixel block = row * 2 + half row]
    if constexpr (S16) {
#pragma unroll
        for (int hv = 0; hv < 2; ++hv)
#pragma unroll
            for (int n = 0; n < 16; ++n) acc16[hv][n] = floatx4{0.f, 0.f, 0.f, 0.f};
    } else {
#pragma unroll
        for (int n = 0; n < 8; ++n)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[n][q] = 0.f;
    }

    const uint8_t* wbase = pp + (PREC == 2 ? f3_bf_off_n((a.cout + F3_OCB - 1) / F3_OCB, a.nch) : (int64_t)F3_HDR) +
                           ((int64_t)(ocb * 4 + wave) * a.nch) * (18 * SB) + lane * 16;
    // B fragment: pixel column lane&31, k half lane>>5 (S16: pixel lane&15, 8-channel group lane>>4 of the chunk's 32)
    const int boff = S16 ? (lane & 15) * F3_PITCH + (lane >> 4) * 16 : (lane & 31) * F3_PITCH + (lane >> 5) * 16;

    // ---- FUSED: the im2col of the parent patch for this wave's pixel blocks (wave, wave + 4, wave + 8), once per tile
    uint8_t* col1 = lds + F3_LDS + lane * 16;     // each lane writes and reads only its own 16-byte slots: no barrier needed
    int p1[3];
    bool pin1[3];
    float inv1 = 1.f, inv1sx = 1.f;
    const uint8_t* pk1 = nullptr;
    const float* bias1 = nullptr;
    if constexpr (FUSED) {
        pk1 = a.packed1 + (int64_t)plane * a.plane_bytes1;
        const float* h1 = reinterpret_cast<const float*>(pk1);
        bias1 = h1 + 16;
        const int hp = h >> 1, wp_ = w >> 1;
        const float* par = a.parent + z * 3 * (int64_t)hp * wp_;
        const int hh = lane >> 5;
        // the parent values under the tile: 3 channels x 6 rows x 18 columns (the 10 x 34 patch and conv1's one-pixel rim,
        // halved), zero outside the parent image = the zero padding of the upsampled image.  Into LDS once, then every
        // lane gathers its 48 im2col values from there.
        float* PP = reinterpret_cast<float*>(lds + F3_LDS + F1_COL);
        float amax = 0.f;
#pragma unroll
        for (int i = tid; i < F1_PP; i += 256) {
            const int ci = i / 108, rem = i - ci * 108, r = rem / 18, c = rem - r * 18;
            const int Yp = (y0 >> 1) - 1 + r, Xp = (x0 >> 1) - 1 + c;
            const bool in = Yp >= 0 && Yp < hp && Xp >= 0 && Xp < wp_;
            const float v = par[(int64_t)ci * hp * wp_ + min(max(Yp, 0), hp - 1) * wp_ + min(max(Xp, 0), wp_ - 1)];
            const float vz = in ? v : 0.f;
            PP[i] = vz;
            amax = fmaxf(amax, fabsf(vz));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
        float* red = reinterpret_cast<float*>(lds + 2 * F3_BUF + 32);      // second half of the 64-byte dump slot
        if (lane == 0) red[wave] = amax;
        __syncthreads();
        amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        const float s_p = pow2_scale<15>(amax);
        sx = pow2_scale<15>(amax * h1[1] + h1[2]);                           // bound on |LeakyReLU(conv1)|: max|parent| * L1max + |b|max
        out_scale = (1.f / sx) * (1.f / sw);
        inv1 = (1.f / s_p) * (1.f / h1[0]);
        inv1sx = inv1 * sx;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const int p = (wave + 4 * b) * 32 + (lane & 31);
            const bool live = p < F3_NPX;
            const int pc = live ? p : 0;
            const int ly = pc / F3_IW, lx = pc - ly * F3_IW;
            const int gy = y0 - 1 + ly, gx = x0 - 1 + lx;
            p1[b] = live ? p : -1;
            pin1[b] = live && gy >= 0 && gy < h && gx >= 0 && gx < w;
            // PP index of tap (dy, dx) of channel ci for this pixel: ci * 108 + ((ly + dy) >> 1) * 18 + ((lx + dx) >> 1)
            int ro[3], co[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                ro[d] = ((ly + d) >> 1) * 18;
                co[d] = (lx + d) >> 1;
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                float v8[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    // k = 16 ks + 8 hh + j -> (channel, dy, dx) = (k / 9, (k % 9) / 3, k % 3); k >= 27 meets zero weights
                    const int k0 = 16 * ks + j, k1 = k0 + 8;
                    const int q0 = k0 < 27 ? k0 : 26, q1 = k1 < 27 ? k1 : 26;
                    const int i0 = (q0 / 9) * 108 + ro[(q0 % 9) / 3] + co[q0 % 3];
                    const int i1 = (q1 / 9) * 108 + ro[(q1 % 9) / 3] + co[q1 % 3];
                    v8[j] = PP[hh ? i1 : i0] * s_p;
                }
                if constexpr (PREC == 0) {
                    half8 ch_, cl_;
                    split8v(v8, ch_, cl_);
                    *reinterpret_cast<half8*>(col1 + (((wave + 4 * b) * 2 + ks) * 2 + 0) * 1024) = ch_;
                    *reinterpret_cast<half8*>(col1 + (((wave + 4 * b) * 2 + ks) * 2 + 1) * 1024) = cl_;
                } else {
                    *reinterpret_cast<half8*>(col1 + (((wave + 4 * b) * 2 + ks) * 2 + 0) * 1024) = cvt8<PREC>(v8);
                }
            }
        }
    }
    // conv1 operands of the chunk being staged: weight fragments (2 k-steps x hi, lo) and the 16 bias values of this lane's
    // rows -- the same for the wave's three pixel blocks, loaded once per chunk a few units ahead of their first use
    half8 w1h[2], w1l[2];
    floatx4 b1r[4], b1v[4];     // raw bias as loaded; scaled by sx at its FIRST USE (block 0): a multiply at the load site is a
                                // vmcnt(0) wait there, which drains the whole weight ring (vmcnt retires in order)
#define F3_FUSED_LOAD(C1)                                                                                             \
    {                                                                                                                 \
        const uint8_t* w1_ = pk1 + F1_HDR + (PREC == 2 ? (int64_t)a.nch * F1_CHUNK_BYTES : (int64_t)0) +                \
                             (int64_t)((C1) / F3_CK) * (2 * SB) + lane * 16;                                          \
        _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) {                                                            \
            w1h[ks] = *reinterpret_cast<const half8*>(w1_ + ks * SB);                                                 \
            if constexpr (PREC == 0) w1l[ks] = *reinterpret_cast<const half8*>(w1_ + ks * SB + 1024);                 \
        }                                                                                                             \
        _Pragma("unroll") for (int gq = 0; gq < 4; ++gq)                                                              \
            b1r[gq] = *reinterpret_cast<const floatx4*>(bias1 + (C1) + 8 * gq + 4 * (lane >> 5));                     \
    }
    // channels C1 .. C1+31 of the first conv for pixel block B of this wave -> split -> the LDS image at DST
#define F3_FUSED_BLOCK(B, DST)                                                                                        \
    {                                                                                                                 \
        floatx16 t_;                                                                                                  \
        if ((B) == 0) { _Pragma("unroll") for (int gq = 0; gq < 4; ++gq) b1v[gq] = b1r[gq] * sx; }                    \
        _Pragma("unroll") for (int q = 0; q < 16; ++q) t_[q] = 0.f;                                                   \
        _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) {                                                            \
            const half8 ch_ = *reinterpret_cast<const half8*>(col1 + (((wave + 4 * (B)) * 2 + ks) * 2 + 0) * 1024);  \
            if constexpr (PREC == 0) {                                                                                \
                const half8 cl_ = *reinterpret_cast<const half8*>(col1 + (((wave + 4 * (B)) * 2 + ks) * 2 + 1) * 1024); \
                t_ = mma32<0>(w1l[ks], ch_, t_);                                                                      \
                t_ = mma32<0>(w1h[ks], cl_, t_);                                                                      \
            }                                                                                                         \
            t_ = mma32<PREC>(w1h[ks], ch_, t_);                                                                       \
        }                                                                                                             \
        typedef _Float16 half4_ __attribute__((ext_vector_type(4)));                                                  \
        const bool livep_ = p1[B] >= 0;                                                                               \
        uint8_t* d0_ = livep_ ? (DST) + p1[B] * F3_PITCH + (lane >> 5) * 8 : lds + 2 * F3_BUF;                        \
        const int lo_off_ = livep_ ? F3_PART : 16;                                                                    \
        const int gstep_ = livep_ ? 16 : 0;                                                                           \
        _Pragma("unroll") for (int gq = 0; gq < 4; ++gq) {                                                            \
            float v4_[4];                                                                                             \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                           \
                const float v_ = __builtin_fmaf(t_[4 * gq + i], inv1sx, b1v[gq][i]);   /* sx (2^k) folded in */       \
                v4_[i] = pin1[B] ? fmaxf(v_, 0.01f * v_) : 0.f;                                                       \
            }                                                                                                         \
            if constexpr (PREC == 0) {                                                                                \
                half4_ hi_, lo_;                                                                                      \
                split4v(v4_, hi_, lo_);                                                                               \
                *reinterpret_cast<half4_*>(d0_ + gq * gstep_) = hi_;                                                  \
                *reinterpret_cast<half4_*>(d0_ + gq * gstep_ + lo_off_) = lo_;                                        \
            } else {                                                                                                  \
                typedef float f4_ __attribute__((ext_vector_type(4)));                                                \
                typedef __bf16 b4_ __attribute__((ext_vector_type(4)));                                               \
                const f4_ x_ = {v4_[0], v4_[1], v4_[2], v4_[3]};                                                      \
                if constexpr (PREC == 2) *reinterpret_cast<b4_*>(d0_ + gq * gstep_) = __builtin_convertvector(x_, b4_); \
                else *reinterpret_cast<half4_*>(d0_ + gq * gstep_) = __builtin_convertvector(x_, half4_);             \
            }                                                                                                         \
        }                                                                                                             \
    }

    // ---- prologue: chunk 0 into buffer 0
    if constexpr (FUSED) {
        F3_FUSED_LOAD(0)
        F3_FUSED_BLOCK(0, lds)
        F3_FUSED_BLOCK(1, lds)
        F3_FUSED_BLOCK(2, lds)
    } else {
#pragma unroll
        for (int r = 0; r < F3_R; ++r) F3_TASK_LOAD(r, 0)
#pragma unroll
        for (int r = 0; r < F3_R; ++r) {
            F3_TASK_STORE(r, 0, 0, lds)
            F3_TASK_STORE(r, 1, 0, lds)
        }
    }
    __syncthreads();

    // Per chunk: 36 units = (tap, k-step, half of the 8 pixel rows), 12 MFMAs each (384 matrix cycles).  Everything else
    // is cut into per-unit pieces and interleaved BETWEEN the MFMAs with sched_group_barrier (one wave per SIMD: nothing
    // else hides it): the 8 LDS fragment reads of unit u+1; the weight fragments of step st+5 (ring of 6, straight from
    // L2, continuous across chunks, packed buffer padded by 5 steps); the 48 global loads of the next chunk's patch
    // (units 0-5, 8 each, issued AFTER the unit's weight loads so that a later wait on a weight fragment never drags a
    // younger HBM load along); the split + LDS store of the next chunk (units 24-35, half a task each).  The unit body
    // has no branch (the last chunk re-loads itself and stores into the idle buffer), so each unit is one basic block
    // for the scheduler.  One barrier per chunk.
    if constexpr (S16) {
    // 36 units per chunk = (tap, pair of pixel rows): 4 pixel blocks x 2 channel halves x 3 products = 24 MFMAs (384 matrix
    // cycles, as in the 32x32x16 form), 8 fragment reads for the next unit; the 4 weight fragments of tap + 2 at the first
    // unit of a tap (ring of 3 taps, continuous across chunks; the packed buffer is padded by 5 steps).  The products of one
    // accumulator are 8 MFMAs apart (no back-to-back dependent pair)
    half8 ah[3][2], al[3][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int hv = 0; hv < 2; ++hv) {
            ah[i][hv] = *reinterpret_cast<const half8*>(wbase + (2 * i + hv) * SB);
            if constexpr (PREC == 0) al[i][hv] = *reinterpret_cast<const half8*>(wbase + (2 * i + hv) * SB + 1024);
        }
    F3_STAMP(1)
    for (int chunk = 0; chunk < a.nch; ++chunk) {
        if (chunk < 8) F3_STAMP(2 + chunk)
        const int buf = chunk & 1;
        const uint8_t* wp = wbase + (int64_t)chunk * (18 * SB);
        const uint8_t* bb = lds + buf * F3_BUF + boff;
        uint8_t* sdst = lds + (buf ^ 1) * F3_BUF;
        const int c1 = (chunk + 1 < a.nch ? chunk + 1 : chunk) * F3_CK;     // chunk being staged (last: itself, unused)
        half8 bh[2][4], bl[2][4];
#define F3_BLOAD16(U, SET)                                                                             \
        {                                                                                              \
            const int tap_ = (U) >> 2, rp_ = (U) & 3;                                                  \
            const int dy_ = tap_ / 3, dx_ = tap_ - dy_ * 3;                                            \
            _Pragma("unroll") for (int n = 0; n < 4; ++n) {                                            \
                const int off = ((2 * rp_ + (n >> 1) + dy_) * F3_IW + dx_ + 16 * (n & 1)) * F3_PITCH;  \
                bh[SET][n] = *reinterpret_cast<const half8*>(bb + off);                                \
                if constexpr (!IN16 && PREC == 0) bl[SET][n] = *reinterpret_cast<const half8*>(bb + F3_PART + off); \
            }                                                                                          \
        }
        F3_BLOAD16(0, 0)
#pragma unroll
        for (int u = 0; u < 36; ++u) {
            const int tap = u >> 2, rp = u & 3;
            if (rp == 0) {                                      // weight fragments of tap + 2 (may belong to the next chunk)
#pragma unroll
                for (int hv = 0; hv < 2; ++hv) {
                    ah[(tap + 2) % 3][hv] = *reinterpret_cast<const half8*>(wp + (2 * (tap + 2) + hv) * SB);
                    if constexpr (PREC == 0)
                        al[(tap + 2) % 3][hv] = *reinterpret_cast<const half8*>(wp + (2 * (tap + 2) + hv) * SB + 1024);
                }
            }
            if (u + 1 < 36) F3_BLOAD16(u + 1, (u + 1) & 1)
            if constexpr (FUSED) {
                if (u == 14) F3_FUSED_LOAD(c1)
                if (u == 22) F3_FUSED_BLOCK(0, sdst)
                if (u == 26) F3_FUSED_BLOCK(1, sdst)
                if (u == 30) F3_FUSED_BLOCK(2, sdst)
            } else {
                if (u < F3_R) F3_TASK_LOAD(u, c1)
                if (u >= 24) F3_TASK_STORE((u - 24) >> 1, (u - 24) & 1, c1, sdst)
            }
            if constexpr (PREC == 0) {
#pragma unroll
                for (int n = 0; n < 4; ++n)
#pragma unroll
                    for (int hv = 0; hv < 2; ++hv)
                        acc16[hv][4 * rp + n] = mma16<0>(al[tap % 3][hv], bh[u & 1][n], acc16[hv][4 * rp + n]);
                if constexpr (!IN16) {
#pragma unroll
                    for (int n = 0; n < 4; ++n)
#pragma unroll
                        for (int hv = 0; hv < 2; ++hv)
                            acc16[hv][4 * rp + n] = mma16<0>(ah[tap % 3][hv], bl[u & 1][n], acc16[hv][4 * rp + n]);
                }
            }
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int hv = 0; hv < 2; ++hv)
                    acc16[hv][4 * rp + n] = mma16<PREC>(ah[tap % 3][hv], bh[u & 1][n], acc16[hv][4 * rp + n]);
#pragma unroll
            for (int i = 0; i < (PREC == 0 ? 24 : 8); ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                        // one MFMA
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                        // one LDS read
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                        // one global load
                __builtin_amdgcn_sched_group_barrier(0x002, PREC == 0 ? 2 : 5, 0);        // a few vector ALU instructions
                __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);                        // one LDS write
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#undef F3_BLOAD16
        __syncthreads();
    }
    } else {
    half8 ah[6], al[6];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        ah[i] = *reinterpret_cast<const half8*>(wbase + i * SB);
        if constexpr (PREC == 0) al[i] = *reinterpret_cast<const half8*>(wbase + i * SB + 1024);
    }
    F3_STAMP(1)
    for (int chunk = 0; chunk < a.nch; ++chunk) {
        if (chunk < 8) F3_STAMP(2 + chunk)
        const int buf = chunk & 1;
        const uint8_t* wp = wbase + (int64_t)chunk * (18 * SB);
        const uint8_t* bb = lds + buf * F3_BUF + boff;
        uint8_t* sdst = lds + (buf ^ 1) * F3_BUF;
        const int c1 = (chunk + 1 < a.nch ? chunk + 1 : chunk) * F3_CK;     // chunk being staged (last: itself, unused)
        half8 bh[2][4], bl[2][4];
#define F3_BLOAD(U, SET)                                                                               \
        {                                                                                              \
            const int st_ = (U) >> 1, hf_ = (U) & 1;                                                   \
            const int tap_ = st_ >> 1, ks_ = st_ & 1;                                                  \
            const int dy_ = tap_ / 3, dx_ = tap_ - dy_ * 3;                                            \
            _Pragma("unroll") for (int n = 0; n < 4; ++n) {                                            \
                const int off = ((hf_ * 4 + n + dy_) * F3_IW + dx_) * F3_PITCH + ks_ * 32;             \
                bh[SET][n] = *reinterpret_cast<const half8*>(bb + off);                                \
                if constexpr (!IN16 && PREC == 0) bl[SET][n] = *reinterpret_cast<const half8*>(bb + F3_PART + off); \
            }                                                                                          \
        }
        F3_BLOAD(0, 0)
#pragma unroll
        for (int u = 0; u < 36; ++u) {
            const int st = u >> 1, hf = u & 1;
            if (hf == 0) {                                      // weight fragments of step st+5 (may belong to the next chunk)
                ah[(st + 5) % 6] = *reinterpret_cast<const half8*>(wp + (st + 5) * SB);
                if constexpr (PREC == 0) al[(st + 5) % 6] = *reinterpret_cast<const half8*>(wp + (st + 5) * SB + 1024);
            }
            if (u + 1 < 36) F3_BLOAD(u + 1, (u + 1) & 1)
            if constexpr (FUSED) {
                if (u == 14) F3_FUSED_LOAD(c1)
                if (u == 22) F3_FUSED_BLOCK(0, sdst)
                if (u == 26) F3_FUSED_BLOCK(1, sdst)
                if (u == 30) F3_FUSED_BLOCK(2, sdst)
            } else {
                if (u < F3_R) F3_TASK_LOAD(u, c1)
                if (u >= 24) F3_TASK_STORE((u - 24) >> 1, (u - 24) & 1, c1, sdst)
            }
            const half8 A_h = ah[st % 6], A_l = al[st % 6];
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                if constexpr (PREC == 0) {
                    acc[hf * 4 + n] = mma32<0>(A_l, bh[u & 1][n], acc[hf * 4 + n]);
                    if constexpr (!IN16) acc[hf * 4 + n] = mma32<0>(A_h, bl[u & 1][n], acc[hf * 4 + n]);
                }
                acc[hf * 4 + n] = mma32<PREC>(A_h, bh[u & 1][n], acc[hf * 4 + n]);
            }
#pragma unroll
            for (int i = 0; i < (PREC == 0 ? 12 : 4); ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                        // one MFMA
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                        // one LDS read
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                        // one global load
                __builtin_amdgcn_sched_group_barrier(0x002, PREC == 0 ? 4 : 10, 0);       // a few vector ALU instructions
                __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);                        // one LDS write
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#undef F3_BLOAD
        __syncthreads();
    }
    }
#undef F3_TASK_LOAD
#undef F3_TASK_STORE
#undef F3_FUSED_BLOCK
#undef F3_FUSED_LOAD

    F3_STAMP(10)
    // ---- epilogue: D col = lane&31 (pixel), row = (q&3) + 8*(q>>2) + 4*(lane>>5) (channel of the wave's 32).
    // 128 stores per lane: a wave-uniform base (scalar registers) + one per-lane offset, the activation resolved outside
    // the loops, no per-element address arithmetic (the first version of this epilogue took a fifth of the kernel's time)
    if constexpr (S16) {
        // D col = lane&15 (pixel of the block), row = q + 4*(lane>>4) (channel of the half).  64 stores per lane and half:
        // wave-uniform base + one per-lane offset, 16 consecutive pixels x 4 channel rows per store instruction
        const int px = lane & 15;
        const int ocw = ocb * F3_OCB + __builtin_amdgcn_readfirstlane(wave) * 32;
        const int och = 4 * (lane >> 4);
        float* ybase = a.y + (z * a.cout + ocw) * hw + (int64_t)y0 * w;                  // wave-uniform
        const unsigned loff = (unsigned)och * (unsigned)hw + (unsigned)(x0 + px);
        const bool full = y0 + F3_TH <= h && x0 + F3_TW <= w;                            // uniform
        const float slope = a.act == LLDWT_ACT_LRELU ? 0.01f : (a.act == LLDWT_ACT_RELU ? 0.f : 1.f);   // none: max(v, v)
#pragma unroll
        for (int hv = 0; hv < 2; ++hv) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int oc = ocw + 16 * hv + och + q;
                if (oc < a.cout) {
                    const float bq = a.bias ? a.bias[plane * a.cout + oc] : 0.f;
                    float* yq = ybase + (int64_t)(16 * hv + q) * hw;
                    if (full && a.act != LLDWT_ACT_TANH) {
#pragma unroll
                        for (int n = 0; n < 16; ++n) {
                            const float v = acc16[hv][n][q] * out_scale + bq;
                            yq[(n >> 1) * w + 16 * (n & 1) + loff] = fmaxf(v, v * slope);
                        }
                    } else {
#pragma unroll
                        for (int n = 0; n < 16; ++n)
                            if (y0 + (n >> 1) < h && x0 + 16 * (n & 1) + px < w)
                                yq[(n >> 1) * w + 16 * (n & 1) + loff] = act_apply(acc16[hv][n][q] * out_scale + bq, a.act);
                    }
                }
            }
        }
    } else {
        const int gx = x0 + (lane & 31);
        const int ocw = ocb * F3_OCB + __builtin_amdgcn_readfirstlane(wave) * 32;       // first channel of this wave
        const int och = 4 * (lane >> 5);
        float* ybase = a.y + (z * a.cout + ocw) * hw + (int64_t)y0 * w;                  // wave-uniform
        const unsigned loff = (unsigned)och * (unsigned)hw + (unsigned)gx;              // this lane's element offset
        float bq[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int oc = ocw + (q & 3) + 8 * (q >> 2) + och;
            bq[q] = a.bias ? a.bias[plane * a.cout + (oc < a.cout ? oc : a.cout - 1)] : 0.f;
        }
        // every bias register is used once HERE, in code all lanes run: the wait for the loads lands in front of the first store.
        // Without it the first use of bq[q] sits in a block only some lanes run (oc < cout), where the wait counters are
        // conservative: vmcnt(0) per q, which also waits for the eight stores of the q before to be acknowledged
#pragma unroll
        for (int q = 0; q < 16; ++q) asm volatile("" ::"v"(bq[q]));
        const bool full = y0 + F3_TH <= h && x0 + F3_TW <= w;                            // uniform
        if (full && a.act != LLDWT_ACT_TANH) {
            const float slope = a.act == LLDWT_ACT_LRELU ? 0.01f : (a.act == LLDWT_ACT_RELU ? 0.f : 1.f);   // none: max(v, v)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                if (ocw + (q & 3) + 8 * (q >> 2) + och < a.cout) {
                    float* yq = ybase + (int64_t)((q & 3) + 8 * (q >> 2)) * hw;
#pragma unroll
                    for (int n = 0; n < 8; ++n) {
                        const float v = acc[n][q] * out_scale + bq[q];
                        yq[n * w + loff] = fmaxf(v, v * slope);
                    }
                }
            }
        } else if (full) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                if (ocw + (q & 3) + 8 * (q >> 2) + och < a.cout) {
                    float* yq = ybase + (int64_t)((q & 3) + 8 * (q >> 2)) * hw;
#pragma unroll
                    for (int n = 0; n < 8; ++n) yq[n * w + loff] = fast_tanh(acc[n][q] * out_scale + bq[q]);
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                if (ocw + (q & 3) + 8 * (q >> 2) + och < a.cout) {
                    float* yq = ybase + (int64_t)((q & 3) + 8 * (q >> 2)) * hw;
#pragma unroll
                    for (int n = 0; n < 8; ++n)
                        if (y0 + n < h && gx < w) yq[n * w + loff] = act_apply(acc[n][q] * out_scale + bq[q], a.act);
                }
            }
        }
    }
    F3_STAMP(11)
    F3_STAMP(15)
}

// ======================================================================================================================
// Row-wise Winograd F(2,3) form of the fused pair (MODE 2, PREC 0; the default -- LLDWT_PLC_ALGO=direct keeps the kernel
// above).  Two outputs of a 3-tap row filter from four products instead of six: for a pixel pair (x, x+1) of an output row
// and one filter row dy, with the input window d0..d3 = row dy, pixels x-1 .. x+2, and the weight row g0..g2
//     U = (g0, (g0+g1+g2)/2, (g0-g1+g2)/2, g2)           (weights, formed in fp64 at pack time, k_f3w_pack)
//     V = (d0-d2, d1+d2, d2-d1, d1-d3)                    (activations, formed in fp32 before the split)
//     M_xi = sum_ic sum_dy U_xi V_xi,   y_x = M0+M1+M2,   y_x+1 = M1-M2-M3
// The main conv issues 3 dy x 4 xi MFMA k-steps per pixel PAIR instead of 9 taps per pixel: two thirds of the MFMAs.
// Scales: |V| <= 2 max|d|, so the activation scale is half the direct kernel's; the weight scale comes from max|U|
// (<= 1.5 max|g|).  tools/winograd_numerics.py emulates both forms: the error stays at the direct form's level.
//
// Kernel shape: the direct kernel's workgroup tile (128 output channels x 8 rows x 32 pixels = 16 pixel pairs per row);
//   wave w owns channels 32w..32w+31 x all 128 pairs = 4 xi x 4 N-tiles of 32 pairs (2 rows x 16 pairs) = 16 accumulator
//   tiles of 32x32 (256 registers).  K loop: chunks of 16 input channels (one 32x32x16 k-step): 12 units (dy, xi) of
//   4 N-tiles x 3 products per chunk.
//   V image in LDS: [10 patch rows][4 xi][16 pairs][16 ch] fp16, hi and lo, double-buffered (80 KB).  The 16-byte halves of
//      an entry swap places on bit 3 of the pair index: each 16-lane group of a ds_read_b128 hits 16 distinct slots.
//   The first conv (3 -> cmid, K = 27 -> 32) runs on v_mfma_f32_16x16x32_f16 (16 channels x 16 pairs, K = 32 in one step) on the
//      pixel sets s = 0, 1 (pixel 2p + s of pair p): 2 sets x 3 products per patch row, 10 patch rows per chunk (waves 0, 1 take three,
//      waves 2, 3 two and one dead row).  V needs d0..d3 = the sets 0..3 of a pair in one lane: the sets 2, 3 are the neighbouring
//      pair's sets 0, 1 and come from lane p + 1 by a DPP row shift behind the activation; pair 16, for lane 15, from one extra
//      16-column tile per chunk and wave.  21 MFMAs per chunk and wave (the earlier form recomputed all four sets in every lane: 36).  Its B operand is the split im2col of the
//      parent patch, built once per tile in LDS as [pixel parity][row][17 pixels] at a 144-byte pitch (9 slots: the 16
//      pairs one read touches map to 16 distinct slots).
constexpr int W3_NE = F3_IH * 4 * 16;            // V entries: 10 rows x 4 xi x 16 pairs = 640
constexpr int W3_PART = W3_NE * 32;              // 20,480 B: one V image (hi or lo)
constexpr int W3_BUF = 2 * W3_PART;
constexpr int W3_DUMP = 2 * W3_BUF;              // 64-byte slot: dead conv1 rows write here; [32, 48) the amax reduction
constexpr int W3_COLP = 144;                     // im2col pitch
constexpr int W3_COL = W3_DUMP + 64;
constexpr int W3_PP = W3_COL + 2 * F3_IH * 17 * W3_COLP;   // parent patch (F1_PP floats)
constexpr int W3_BIAS = W3_PP + 1536;            // the workgroup's 128 output biases (zero without bias or beyond cout)
constexpr int W3_LDS = W3_BIAS + 2 * F3_OCB * 4; // 133,504 B: two bias images, alternating by the pass over the channel blocks
constexpr int W3_LDS_EARLIER = W3_BIAS;          // the earlier form has no bias image
constexpr int W3_RING = 6;                       // weight steps in flight + 1 (12 % W3_RING == 0: the ring slot of a unit is
                                                 // the same in every chunk)
static_assert(12 % W3_RING == 0 && W3_RING <= 6, "weight ring");
static_assert(W3_PP % 16 == 0 && F1_PP * 4 <= 1536, "LDS layout");

// The first conv's 12 MFMAs of one patch row (4 shifted pixel sets x 3 products) with their results in VGPRs.  As builtins their
// results take accumulator registers, and the main loop's 16 tiles fill all 256 of them: the compiler then moves main tiles
// in and out around every row.  Hazards inside the statement: each chain takes the previous result whole as C (0 wait
// states); the trailing 21 states cover the read of D by whatever follows (12 for this 8-pass MFMA).
__device__ __forceinline__ void w3_row_mma(f4_t (&t)[4], const h8_t& wh, const h8_t& wl, const h8_t (&ch)[4], const h8_t (&cl)[4]) {
    asm volatile(
        "v_mfma_f32_16x16x32_f16 %0, %4, %6, 0\n\t"
        "v_mfma_f32_16x16x32_f16 %1, %4, %7, 0\n\t"
        "v_mfma_f32_16x16x32_f16 %2, %4, %8, 0\n\t"
        "v_mfma_f32_16x16x32_f16 %3, %4, %9, 0\n\t"
        "v_mfma_f32_16x16x32_f16 %0, %5, %10, %0\n\t"
        "v_mfma_f32_16x16x32_f16 %1, %5, %11, %1\n\t"
        "v_mfma_f32_16x16x32_f16 %2, %5, %12, %2\n\t"
        "v_mfma_f32_16x16x32_f16 %3, %5, %13, %3\n\t"
        "v_mfma_f32_16x16x32_f16 %0, %5, %6, %0\n\t"
        "v_mfma_f32_16x16x32_f16 %1, %5, %7, %1\n\t"
        "v_mfma_f32_16x16x32_f16 %2, %5, %8, %2\n\t"
        "v_mfma_f32_16x16x32_f16 %3, %5, %9, %3\n\t"
        "s_nop 7\n\ts_nop 7\n\ts_nop 4"
        : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3])
        : "v"(wl), "v"(wh), "v"(ch[0]), "v"(ch[1]), "v"(ch[2]), "v"(ch[3]), "v"(cl[0]), "v"(cl[1]), "v"(cl[2]), "v"(cl[3]));
}

// The same chains for two pixel sets (the current form computes every first-conv pixel once: sets 0 and 1 of a pair), and for two sets
// plus the extra tile that holds pair 16 of the wave's rows.  Product order per accumulator as above; a dependent MFMA follows its
// producer two (three) issues later, and the matrix pipe interlocks on a result taken whole as C.
__device__ __forceinline__ void w3_row_mma2(f4_t& t0, f4_t& t1, const h8_t& wh, const h8_t& wl, const h8_t& ch0, const h8_t& ch1,
                                            const h8_t& cl0, const h8_t& cl1) {
    asm volatile(
        "v_mfma_f32_16x16x32_f16 %0, %2, %4, 0\n\t"
        "v_mfma_f32_16x16x32_f16 %1, %2, %5, 0\n\t"
        "v_mfma_f32_16x16x32_f16 %0, %3, %6, %0\n\t"
        "v_mfma_f32_16x16x32_f16 %1, %3, %7, %1\n\t"
        "v_mfma_f32_16x16x32_f16 %0, %3, %4, %0\n\t"
        "v_mfma_f32_16x16x32_f16 %1, %3, %5, %1\n\t"
        "s_nop 7\n\ts_nop 7\n\ts_nop 4"
        : "=&v"(t0), "=&v"(t1)
        : "v"(wl), "v"(wh), "v"(ch0), "v"(ch1), "v"(cl0), "v"(cl1));
}
__device__ __forceinline__ void w3_row_mma3(f4_t& t0, f4_t& t1, f4_t& t2, const h8_t& wh, const h8_t& wl, const h8_t& ch0,
                                            const h8_t& ch1, const h8_t& ch2, const h8_t& cl0, const h8_t& cl1, const h8_t& cl2) {
    asm volatile(
        "v_mfma_f32_16x16x32_f16 %0, %3, %5, 0\n\t"
        "v_mfma_f32_16x16x32_f16 %1, %3, %6, 0\n\t"
        "v_mfma_f32_16x16x32_f16 %2, %3, %7, 0\n\t"
        "v_mfma_f32_16x16x32_f16 %0, %4, %8, %0\n\t"
        "v_mfma_f32_16x16x32_f16 %1, %4, %9, %1\n\t"
        "v_mfma_f32_16x16x32_f16 %2, %4, %10, %2\n\t"
        "v_mfma_f32_16x16x32_f16 %0, %4, %5, %0\n\t"
        "v_mfma_f32_16x16x32_f16 %1, %4, %6, %1\n\t"
        "v_mfma_f32_16x16x32_f16 %2, %4, %7, %2\n\t"
        "s_nop 7\n\ts_nop 7\n\ts_nop 4"
        : "=&v"(t0), "=&v"(t1), "=&v"(t2)
        : "v"(wl), "v"(wh), "v"(ch0), "v"(ch1), "v"(ch2), "v"(cl0), "v"(cl1), "v"(cl2));
}
// one accumulator value into a vector register, from the accumulator register it lives in (the caller keeps the MFMA's wait states)
__device__ __forceinline__ float w3_acc_read(float v) {
    float r;
    asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(r) : "a"(v));
    return r;
}
// a lane's value from another lane of its 16-lane row (v_mov_b32 with a DPP control); a lane whose source lies outside the row
// keeps OLD (BOUND = false) or takes zero (BOUND = true).  0x101 = row_shl:1 (lane i reads lane i + 1), 0x110 + k = row_shr:k
// (lane i reads lane i - k)
template <int CTRL, bool BOUND>
__device__ __forceinline__ float w3_dpp(float old, float src) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src), CTRL, 0xf, 0xf, BOUND));
}
// split4v in plain C: the same bits (v - hi is exact in fp32, see split_f16.h), twelve vector instructions instead of six.  The pieces
// of the chunk loop are placed between the MFMAs by sched_group_barrier, which sorts instructions by class and has no class for an
// inline-assembly statement: the v_fma_mix forms and the LDS stores behind them gathered at the end of their unit, where nothing hid
// them (measured per unit: a unit with three STORE pieces took 590 cycles more than one without, one with a single piece 80).
__device__ __forceinline__ void w3_split4(const float (&v)[4], h4_t& hi, h4_t& lo) {
    const f4_t x = {v[0], v[1], v[2], v[3]};
    hi = __builtin_convertvector(x, h4_t);
    lo = __builtin_convertvector(x - __builtin_convertvector(hi, f4_t), h4_t);
}
// k-group G (k = 8G .. 8G+7 of the first conv's K = 27 -> 32) of the split im2col for the patch pixels lane, lane + 64, ...: one
// wave per k-group, so that the tap offsets are constants and all four waves stay busy over the 340 pixels
template <int G>
__device__ __forceinline__ void w3_im2col_group(uint8_t* lds, const float* PP, float s_p, int lane) {
    // six passes of 64 pixels, branch-free and unrolled: the 48 patch reads of a lane are in flight before the first split (as a loop,
    // every pass was an LDS round trip of its own).  A lane past the last pixel repeats it: the same values to the same place.
    constexpr int NP = (F3_NPX + 63) / 64;
    float v8[NP][8];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int px = min(lane + 64 * k, F3_NPX - 1);
        const int ly = px / F3_IW, lx = px - ly * F3_IW;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int kk = 8 * G + j, q = kk < 27 ? kk : 26;      // k >= 27 meets zero weights
            const int dy = (q % 9) / 3, dx = q % 3;
            v8[k][j] = PP[(q / 9) * 108 + ((ly + dy) >> 1) * 18 + ((lx + dx) >> 1)];
        }
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int px = min(lane + 64 * k, F3_NPX - 1);
        const int ly = px / F3_IW, lx = px - ly * F3_IW;
        uint8_t* dst = lds + W3_COL + ((lx & 1) * (F3_IH * 17) + ly * 17 + (lx >> 1)) * W3_COLP;
#pragma unroll
        for (int j = 0; j < 8; ++j) v8[k][j] *= s_p;
        half8 ch_, cl_;
        split8v(v8[k], ch_, cl_);
        *reinterpret_cast<half8*>(dst + G * 16) = ch_;
        *reinterpret_cast<half8*>(dst + 64 + G * 16) = cl_;
    }
}

__device__ __forceinline__ void wino_u(const float* g, double (&u)[4]) {
    const double g0 = g[0], g1 = g[1], g2 = g[2];
    u[0] = g0; u[1] = (g0 + g1 + g2) * 0.5; u[2] = (g0 - g1 + g2) * 0.5; u[3] = g2;
}

// max |U| per plane into the Winograd header's [1]
__global__ void k_f3w_umax(const float* __restrict__ w, int64_t nrows, uint8_t* __restrict__ packed, int64_t plane_bytes, int64_t woff) {
    const int plane = blockIdx.y;
    float m = 0.f;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nrows; i += (int64_t)gridDim.x * blockDim.x) {
        double u[4];
        wino_u(w + ((int64_t)plane * nrows + i) * 3, u);
        for (int k = 0; k < 4; ++k) m = fmaxf(m, fabsf((float)u[k]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_down(m, o, 64));
    float* hdr = reinterpret_cast<float*>(packed + (int64_t)plane * plane_bytes + woff);
    if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(reinterpret_cast<int*>(hdr + 1), __float_as_int(m));
}

// U fragments: step (ocb, wave, chunk, st = dy*4 + xi), A[row = oc lane&31][k = ic 8*(lane>>5) + j]
__global__ void k_f3w_pack(const float* __restrict__ w, uint8_t* __restrict__ packed, int cin, int cout, int64_t plane_bytes, int64_t woff) {
    const int plane = blockIdx.y;
    uint8_t* pp = packed + (int64_t)plane * plane_bytes + woff;
    float* hdr = reinterpret_cast<float*>(pp);
    const double su = pow2_scale<15>(hdr[1]);
    const int nch = w3_nch(cin), nocb = (cout + F3_OCB - 1) / F3_OCB;
    const int64_t n = (int64_t)nocb * 4 * nch * W3_NST * 64 * 8;
    const float* wp = w + (int64_t)plane * cout * cin * 9;
    _Float16* out = reinterpret_cast<_Float16*>(pp + F3_HDR);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t r = i;
        const int j = (int)(r % 8); r /= 8;
        const int lane = (int)(r % 64); r /= 64;
        const int st = (int)(r % W3_NST); r /= W3_NST;
        const int chunk = (int)(r % nch); r /= nch;
        const int wv = (int)(r % 4); r /= 4;
        const int ocb = (int)r;
        const int oc = ocb * F3_OCB + wv * 32 + (lane & 31), ic = chunk * W3_CK + 8 * (lane >> 5) + j;
        const int dy = st >> 2, xi = st & 3;
        float v = 0.f;
        if (oc < cout && ic < cin) {
            double u[4];
            wino_u(wp + ((int64_t)oc * cin + ic) * 9 + dy * 3, u);
            v = (float)(u[xi] * su);
        }
        const _Float16 hi = (_Float16)v;
        const int64_t step = ((int64_t)(ocb * 4 + wv) * nch + chunk) * W3_NST + st;
        out[step * 1024 + lane * 8 + j] = hi;
        out[step * 1024 + 512 + lane * 8 + j] = (_Float16)(v - (float)hi);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) hdr[0] = (float)su;
}

// EARLIER (lldwt_set_diagnostics kind 1, flags bit 0; tools/plc_stamps.py, tests/test_gpu_plc_wino_sched.py and
// tests/test_gpu_plc_wino_once.py): the kernel as it was before its epilogue stopped waiting between stores, before the first conv's
// ACT / STORE work was dealt over the units in pieces and before the first conv ran once per pixel (four shifted pixel sets in every
// lane, the im2col one pixel per thread, a barrier behind unit 11) -- the A/B leg and the bit-equality reference.  Same arithmetic
// per value and same MFMA order per accumulator in both forms: the outputs are equal bit for bit.
template <bool EARLIER>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_plc_wino(F3Args a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t z = blockIdx.z;
    const int plane = (int)(z / a.batch);
    // The current form folds the channel blocks of a pixel tile into one workgroup when the grid has one block in y (the host's
    // choice, lldwt_plc_fused): pass p runs channel block p, and everything that depends on the tile only -- the parent patch, its
    // |max|, the scales, the split im2col and the chunk-0 rows of the first conv -- is computed once.  With a grid of nocb blocks in
    // y a workgroup runs one pass, as the earlier form always does.
    const int nocb = (a.cout + F3_OCB - 1) / F3_OCB;
    const int npass = (!EARLIER && gridDim.y == 1) ? nocb : 1;
    int ocb = blockIdx.y;              // the channel block of the current pass
// stamps are indexed by the logical channel block, so that the buffer has one layout whatever the grid
#define W3_STAMP(i)                                                                                                     \
    if (a.stamps && lane == 0)                                                                                          \
        a.stamps[((((int64_t)blockIdx.z * nocb + ocb) * gridDim.x + blockIdx.x) * 4 + wave) * 16 + (i)] =               \
            (i) >= 14 ? __builtin_amdgcn_s_memrealtime() : __builtin_amdgcn_s_memtime();
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int y0 = ty * F3_TH, x0 = tx * F3_TW;
    const int h = a.h, w = a.w;
    const int64_t hw = (int64_t)h * w;

    W3_STAMP(0)
    W3_STAMP(14)
    const uint8_t* pp = a.packed + (int64_t)plane * a.plane_bytes + f3_wino_off(a.cin, a.cout);
    const float su = *reinterpret_cast<const float*>(pp);
    const uint8_t* pk1 = a.packed1 + (int64_t)plane * a.plane_bytes1;
    const float* h1 = reinterpret_cast<const float*>(pk1);
    const float* bias1 = h1 + 16;
    // The current form issues the parent patch's loads first.  vmcnt retires in order: behind the ten ring loads and the first conv's
    // operands, the patch waited for all of them, and the patch is what the prologue needs first.
    const int hp = h >> 1, wp_ = w >> 1;
    const float* par = a.parent + z * 3 * (int64_t)hp * wp_;
    static_assert(F1_PP <= 512, "two patch values per thread");
    float pv[2] = {0.f, 0.f};
    if constexpr (!EARLIER) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            // no branch around a load: at the join the compiler waits for it (threads past the patch's end load its last value again)
            const int i = min(tid + 256 * k, F1_PP - 1);
            const int ci = i / 108, rem = i - ci * 108, r = rem / 18, c = rem - r * 18;
            const int Yp = (y0 >> 1) - 1 + r, Xp = (x0 >> 1) - 1 + c;
            pv[k] = par[(int64_t)ci * hp * wp_ + min(max(Yp, 0), hp - 1) * wp_ + min(max(Xp, 0), wp_ - 1)];
        }
    }
    // the weight ring's first steps and the first conv's chunk-0 operands: in flight during the whole prologue
    const uint8_t* wbase = pp + F3_HDR + ((int64_t)(ocb * 4 + wave) * a.nch) * (W3_NST * F3_STEP_BYTES) + lane * 16;
    half8 ah[W3_RING], al[W3_RING];
#pragma unroll
    for (int i = 0; i < W3_RING - 1; ++i) {
        ah[i] = *reinterpret_cast<const half8*>(wbase + i * F3_STEP_BYTES);
        al[i] = *reinterpret_cast<const half8*>(wbase + i * F3_STEP_BYTES + 1024);
    }
    half8 w1h, w1l;
    f4_t b1r, b1v;
#define W3_FUSED_LOAD(C1)                                                                                             \
    {                                                                                                                 \
        const uint8_t* w1_ = pk1 + f1_w16_off(a.cin) + (int64_t)((C1) / W3_CK) * F3_STEP_BYTES + lane * 16;           \
        w1h = *reinterpret_cast<const half8*>(w1_);                                                                   \
        w1l = *reinterpret_cast<const half8*>(w1_ + 1024);                                                            \
        b1r = *reinterpret_cast<const f4_t*>(bias1 + (C1) + 4 * (lane >> 4));                                        \
    }
    W3_FUSED_LOAD(0)
    // the second conv's bias goes through LDS: loaded here, its latency under the prologue; read back before the epilogue's first
    // store by an LDS read, which no store of the epilogue counts against
    float bias2 = 0.f, bias2n = 0.f;   // bias2n: the next pass's values, loaded a pass ahead (pass 1's: here), for the other image
#define W3_BIAS_LOAD(DST, OCB)                                                                                        \
    {                                                                                                                 \
        const int oc_ = (OCB) * F3_OCB + tid;                                                                         \
        if (tid < F3_OCB && a.bias && oc_ < a.cout) DST = a.bias[plane * a.cout + oc_];                               \
    }
    if constexpr (!EARLIER) {
        W3_BIAS_LOAD(bias2, ocb)
        if (npass > 1) W3_BIAS_LOAD(bias2n, ocb + 1)
    }

    // ---- the parent patch (as in the direct kernel), then its split im2col for every patch pixel, once per tile
    float* PP = reinterpret_cast<float*>(lds + W3_PP);
    float amax = 0.f;
#pragma unroll
    for (int i = tid; i < F1_PP; i += 256) {
        const int ci = i / 108, rem = i - ci * 108, r = rem / 18, c = rem - r * 18;
        const int Yp = (y0 >> 1) - 1 + r, Xp = (x0 >> 1) - 1 + c;
        const bool in = Yp >= 0 && Yp < hp && Xp >= 0 && Xp < wp_;
        const float v = EARLIER ? par[(int64_t)ci * hp * wp_ + min(max(Yp, 0), hp - 1) * wp_ + min(max(Xp, 0), wp_ - 1)] : pv[i >> 8];
        const float vz = in ? v : 0.f;
        PP[i] = vz;
        amax = fmaxf(amax, fabsf(vz));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    float* red = reinterpret_cast<float*>(lds + W3_DUMP + 32);
    if (lane == 0) red[wave] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float s_p = pow2_scale<15>(amax);
    // V spans twice the activation bound: half the direct kernel's scale keeps max|V * sx| below 2^15
    const float sx = 0.5f * pow2_scale<15>(amax * h1[1] + h1[2]);
    const float out_scale = (1.f / sx) * (1.f / su);
    const float inv1sx = (1.f / s_p) * (1.f / h1[0]) * sx;
    W3_STAMP(12)                       // prologue stamps: 0 .. 12 the parent patch and its |max|, 12 .. 13 the split im2col,
                                       // 13 .. 2 the wait at its barrier, 2 .. 1 the chunk-0 rows and their barrier
    if constexpr (EARLIER) {
    for (int px = tid; px < F3_NPX; px += 256) {
        const int ly = px / F3_IW, lx = px - ly * F3_IW;
        uint8_t* dst = lds + W3_COL + ((lx & 1) * (F3_IH * 17) + ly * 17 + (lx >> 1)) * W3_COLP;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float v8[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = 8 * g + j, q = k < 27 ? k : 26;         // k >= 27 meets zero weights
                const int dy = (q % 9) / 3, dx = q % 3;
                v8[j] = PP[(q / 9) * 108 + ((ly + dy) >> 1) * 18 + ((lx + dx) >> 1)] * s_p;
            }
            half8 ch_, cl_;
            split8v(v8, ch_, cl_);
            *reinterpret_cast<half8*>(dst + g * 16) = ch_;
            *reinterpret_cast<half8*>(dst + 64 + g * 16) = cl_;
        }
    }
    } else {
        // the same values over (pixel, k-group) tasks, 1 360 of them: wave w takes k-group w of every pixel, six passes of 64 pixels
        // with all four waves busy (the pixel loop above: two passes of four groups in sequence, the second a third full)
        switch (__builtin_amdgcn_readfirstlane(wave)) {
            case 0: w3_im2col_group<0>(lds, PP, s_p, lane); break;
            case 1: w3_im2col_group<1>(lds, PP, s_p, lane); break;
            case 2: w3_im2col_group<2>(lds, PP, s_p, lane); break;
            default: w3_im2col_group<3>(lds, PP, s_p, lane); break;
        }
    }

    // ---- this wave's first-conv rows (wave, wave + 4, wave + 8; the last one dead for waves 2, 3): pair p = lane&15,
    // channel group g = lane>>4 (D rows 4g .. 4g+3 of the 16x16 tile)
    const int p = lane & 15, g = lane >> 4;
    int colw[3], vw[3];
    unsigned pinm = 0;                 // bit 4*B + s: pixel 2p + s of row B inside the image
    bool pin[3][4];                    // the same as twelve conditions: they stay in scalar registers as lane masks over the loop
#pragma unroll
    for (int B = 0; B < 3; ++B) {
        const int r = wave + 4 * B;
        const bool live = r < F3_IH;
        const int rr = live ? r : 0;
        colw[B] = W3_COL + (rr * 17 + p) * W3_COLP + g * 16;
        vw[B] = live ? ((rr * 4) * 16 + p) * 32 + (((g >> 1) ^ (p >> 3)) * 16) + (g & 1) * 8 : -1;
        const int gy = y0 - 1 + r;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int gx = x0 - 1 + 2 * p + s;
            pin[B][s] = live && gy >= 0 && gy < h && gx >= 0 && gx < w;
            if (pin[B][s]) pinm |= 1u << (4 * B + s);
        }
    }
    // The current form computes the sets 0 and 1 only: sets 2 and 3 of pair p are sets 0 and 1 of pair p + 1, the same dot products in
    // the same k order, so lane p takes them from lane p + 1 of its 16-lane row (same g) after ACT.  Pair 16, which lane 15 needs, comes
    // from one extra 16-column tile per chunk: column n = 2B + s < 6 is pixel 32 + s of the wave's row B (the im2col holds 17 pairs per
    // row); columns 6 .. 15 repeat column 0 and are masked.  Its B fragments do not depend on the chunk: read once, kept in registers.
    const int en = p < 6 ? p : 0, er = wave + 4 * (en >> 1);
    const bool elive = p < 6 && er < F3_IH;
    const int cole = W3_COL + (((en & 1) * F3_IH + (elive ? er : 0)) * 17 + 16) * W3_COLP + g * 16;
    // the image mask of the extra tile's column as an AND mask (all ones inside the image): as a condition the compiler turns the
    // four selects of the tile's ACT into branches, which split the unit's scheduling region
    const int pine = (elive && y0 - 1 + er >= 0 && y0 - 1 + er < h && x0 + 31 + (en & 1) < w) ? -1 : 0;
    // row B of the first conv for channels C1 .. C1+15 on the 4 shifted pixel sets, in four stages that run in consecutive
    // units of the chunk loop (one wave per SIMD: nothing else hides an LDS read, an MFMA result or a block of vector
    // instructions): READ the im2col fragments, MMA, ACT = bias + LeakyReLU, STORE = V (4 xi) -> split -> the LDS image at DST
    half8 c1h[4], c1l[4];
    f4_t t1[4];
    float d1[4][4];                    // [shift][channel]: LeakyReLU(conv1) of the row, zero outside the image
#define W3_ROW_READ(B)                                                                                                \
    {                                                                                                                 \
        _Pragma("unroll") for (int s = 0; s < 4; ++s) {                                                               \
            const uint8_t* c_ = lds + colw[B] + ((s & 1) * (F3_IH * 17) + (s >> 1)) * W3_COLP;                        \
            c1h[s] = *reinterpret_cast<const half8*>(c_);                                                             \
            c1l[s] = *reinterpret_cast<const half8*>(c_ + 64);                                                        \
        }                                                                                                             \
    }
#define W3_ROW_MMA() w3_row_mma(t1, w1h, w1l, c1h, c1l);
#define W3_ROW_ACT(B)                                                                                                 \
    {                                                                                                                 \
        if ((B) == 0) b1v = b1r * sx;                                                                                 \
        _Pragma("unroll") for (int s = 0; s < 4; ++s)                                                                 \
            _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                           \
                const float v_ = __builtin_fmaf(t1[s][q], inv1sx, b1v[q]);                                            \
                d1[s][q] = (pinm >> (4 * (B) + s)) & 1 ? fmaxf(v_, 0.01f * v_) : 0.f;                                 \
            }                                                                                                         \
    }
#define W3_ROW_STORE(B, DST)                                                                                          \
    {                                                                                                                 \
        const bool livev_ = vw[B] >= 0;                                                                               \
        uint8_t* d0_ = livev_ ? (DST) + vw[B] : lds + W3_DUMP;                                                        \
        const int xs_ = livev_ ? 16 * 32 : 0, lo_ = livev_ ? W3_PART : 8;                                             \
        _Pragma("unroll") for (int xi = 0; xi < 4; ++xi) {                                                            \
            float v4_[4];                                                                                             \
            _Pragma("unroll") for (int q = 0; q < 4; ++q)                                                             \
                v4_[q] = xi == 0 ? d1[0][q] - d1[2][q] : xi == 1 ? d1[1][q] + d1[2][q]                                \
                       : xi == 2 ? d1[2][q] - d1[1][q] : d1[1][q] - d1[3][q];                                         \
            h4_t hi_, lo4_;                                                                                           \
            split4v(v4_, hi_, lo4_);                                                                                  \
            *reinterpret_cast<h4_t*>(d0_ + xi * xs_) = hi_;                                                           \
            *reinterpret_cast<h4_t*>(d0_ + xi * xs_ + lo_) = lo4_;                                                    \
        }                                                                                                             \
    }
    if constexpr (!EARLIER) {
        // pass 0's image, and pass 1's into the other one: both values were loaded at the kernel's start
        if (tid < F3_OCB) reinterpret_cast<float*>(lds + W3_BIAS)[tid] = bias2;
        if (npass > 1 && tid < F3_OCB) reinterpret_cast<float*>(lds + W3_BIAS)[F3_OCB + tid] = bias2n;
    }
    // The current form's pieces, which the chunk loop deals over its units; every row has registers of its own (what is live is what
    // the order of the pieces makes live).  READ2 the two sets' im2col fragments; MMA2 / MMA3 (row 0 with the extra tile); ACT2 = bias +
    // LeakyReLU + image mask of one set, once per pixel; SHIFT = sets 2, 3 from lane p + 1 (lane 15: from column 2B + s of the extra
    // tile, moved there by a row shift of 15 - 2B - s lanes); STORE2 = one xi of V -> split -> the LDS image at DST.  Value for value what
    // the whole-row stages compute: xi = 0 needs the sets 0, 2; xi = 1, 2 the sets 1, 2; xi = 3 the sets 1, 3
    half8 c2h[3][2], c2l[3][2], ceh, cel;
    f4_t t2[3][2], te;
    float d2[3][4][4], de[4];
#define W3_ROW_READ2(B)                                                                                               \
    {                                                                                                                 \
        _Pragma("unroll") for (int s = 0; s < 2; ++s) {                                                               \
            const uint8_t* c_ = lds + colw[B] + s * (F3_IH * 17) * W3_COLP;                                           \
            c2h[B][s] = *reinterpret_cast<const half8*>(c_);                                                          \
            c2l[B][s] = *reinterpret_cast<const half8*>(c_ + 64);                                                     \
        }                                                                                                             \
    }
#define W3_ROW_MMA2(B) w3_row_mma2(t2[B][0], t2[B][1], w1h, w1l, c2h[B][0], c2h[B][1], c2l[B][0], c2l[B][1]);
#define W3_ROW_MMA3() w3_row_mma3(t2[0][0], t2[0][1], te, w1h, w1l, c2h[0][0], c2h[0][1], ceh, c2l[0][0], c2l[0][1], cel);
#define W3_ROW_ACT2(B, S)                                                                                             \
    {                                                                                                                 \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                               \
            const float v_ = __builtin_fmaf(t2[B][S][q], inv1sx, b1v[q]);                                             \
            d2[B][S][q] = pin[B][S] ? fmaxf(v_, 0.01f * v_) : 0.f;                                                    \
        }                                                                                                             \
    }
#define W3_EXTRA_ACT()                                                                                                \
    {                                                                                                                 \
        b1v = b1r * sx;                                                                                               \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                               \
            const float v_ = __builtin_fmaf(te[q], inv1sx, b1v[q]);                                                   \
            de[q] = __int_as_float(__float_as_int(fmaxf(v_, 0.01f * v_)) & pine);                                     \
        }                                                                                                             \
    }
#define W3_ROW_SHIFT(B)                                                                                               \
    {                                                                                                                 \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                               \
            d2[B][2][q] = w3_dpp<0x101, false>(w3_dpp<0x110 + 15 - 2 * (B), true>(0.f, de[q]), d2[B][0][q]);          \
            d2[B][3][q] = w3_dpp<0x101, false>(w3_dpp<0x110 + 14 - 2 * (B), true>(0.f, de[q]), d2[B][1][q]);          \
        }                                                                                                             \
    }
#define W3_ROW_STORE2(B, DST, XI)                                                                                     \
    {                                                                                                                 \
        const bool livev_ = vw[B] >= 0;                                                                               \
        uint8_t* d0_ = livev_ ? (DST) + vw[B] : lds + W3_DUMP;                                                        \
        const int xs_ = livev_ ? 16 * 32 : 0, lo_ = livev_ ? W3_PART : 8;                                             \
        float v4_[4];                                                                                                 \
        _Pragma("unroll") for (int q = 0; q < 4; ++q)                                                                 \
            v4_[q] = (XI) == 0 ? d2[B][0][q] - d2[B][2][q] : (XI) == 1 ? d2[B][1][q] + d2[B][2][q]                    \
                   : (XI) == 2 ? d2[B][2][q] - d2[B][1][q] : d2[B][1][q] - d2[B][3][q];                               \
        h4_t hi_, lo4_;                                                                                               \
        w3_split4(v4_, hi_, lo4_);                                                                                    \
        *reinterpret_cast<h4_t*>(d0_ + (XI) * xs_) = hi_;                                                             \
        *reinterpret_cast<h4_t*>(d0_ + (XI) * xs_ + lo_) = lo4_;                                                      \
    }
    W3_STAMP(13)
    __syncthreads();                   // the im2col is read across lanes
    W3_STAMP(2)

    floatx16 acc[4][4];                // [xi][N-tile]
#define W3_ZERO_ACC()                                                                                                 \
    _Pragma("unroll") for (int xi = 0; xi < 4; ++xi)                                                                  \
        _Pragma("unroll") for (int n = 0; n < 4; ++n)                                                                 \
            _Pragma("unroll") for (int q = 0; q < 16; ++q) acc[xi][n][q] = 0.f;
    if constexpr (EARLIER) {
        W3_ZERO_ACC()
#pragma unroll
        for (int B = 0; B < 3; ++B) {
            W3_ROW_READ(B)
            W3_ROW_MMA()
            W3_ROW_ACT(B)
            W3_ROW_STORE(B, lds)
        }
    } else {
        // chunk 0's rows as a pipeline: every fragment read in flight at once, then the three MMA statements, then the vector work;
        // the accumulators are zeroed behind it (at the head of pass 0), so that the rows' registers cost nothing
        ceh = *reinterpret_cast<const half8*>(lds + cole);
        cel = *reinterpret_cast<const half8*>(lds + cole + 64);
        W3_ROW_READ2(0) W3_ROW_READ2(1) W3_ROW_READ2(2)
        W3_ROW_MMA3() W3_ROW_MMA2(1) W3_ROW_MMA2(2)
        W3_EXTRA_ACT()
        W3_FUSED_LOAD((a.nch > 1 ? 1 : 0) * W3_CK)       // the operands of the chunk that chunk 0 stages (b1v holds chunk 0's bias)
        W3_ROW_ACT2(0, 0) W3_ROW_ACT2(0, 1) W3_ROW_SHIFT(0)
        W3_ROW_STORE2(0, lds, 0) W3_ROW_STORE2(0, lds, 1) W3_ROW_STORE2(0, lds, 2) W3_ROW_STORE2(0, lds, 3)
        W3_ROW_ACT2(1, 0) W3_ROW_ACT2(1, 1) W3_ROW_SHIFT(1)
        W3_ROW_STORE2(1, lds, 0) W3_ROW_STORE2(1, lds, 1) W3_ROW_STORE2(1, lds, 2) W3_ROW_STORE2(1, lds, 3)
        W3_ROW_ACT2(2, 0) W3_ROW_ACT2(2, 1) W3_ROW_SHIFT(2)
        W3_ROW_STORE2(2, lds, 0) W3_ROW_STORE2(2, lds, 1) W3_ROW_STORE2(2, lds, 2) W3_ROW_STORE2(2, lds, 3)
    }
    if constexpr (EARLIER) __syncthreads();      // the current form: at the head of pass 0, behind the zeroing

    // B fragment of N-tile n, filter row dy, xi: pair p of output row 2n + ((lane>>4)&1), channel half lane>>5
    const int boff = (((lane >> 4) & 1) * 64 + p) * 32 + (((lane >> 5) ^ (p >> 3)) * 16);
    // Per chunk: 12 units (dy, xi), 12 MFMAs each (384 matrix cycles); interleaved between them as in the direct kernel: the
    // 8 fragment reads of unit u+1, the weight step u+5 (ring of 6, continuous across chunks, pack padded by 5 steps), the
    // first-conv operands of the chunk after the next (unit 8) and the next chunk's three rows into the idle buffer: READ at 0, 1, 2,
    // MMA at 1, 2, 4, the ACT, SHIFT and STORE pieces over units 2 .. 10 (EARLIER: operands in unit 0, each row over four units, READ
    // at 2, 5, 8; MMA at 3, 6, 9; ACT at 4, 7, 10; STORE at 5, 8, 11).  One barrier per chunk: at the end of unit 10 (EARLIER: behind unit 11), so that unit 11 can load the
    // next chunk's unit-0 fragments in its gaps and no chunk starts with an LDS round trip that nothing hides.  The order that keeps
    // this free of races, with buf the buffer chunk c reads and the other one the buffer it stages chunk c + 1 into:
    //   - every store of chunk c + 1's V image is issued in units 3 .. 10 of chunk c, in front of the barrier; chunk c's unit 11 and
    //     chunk c + 1 read that image behind it;
    //   - unit 11's own fragments (buf) are loaded in unit 10 and waited for in front of the barrier (the barrier's fence drains
    //     every LDS read of the wave), so no wave reads buf behind the barrier of chunk c;
    //   - the next stores into buf are chunk c + 1's, from its unit 3 on: behind that barrier in every wave.
    // The last chunk of the last pass has no successor: its unit 11 loads fragments of the unused staged image (inside the buffer; a
    // branch around the eight reads would split the unit's scheduling region) and nothing consumes them.
    // Passes: the chunks of all passes form one sequence, g = pass * nch + chunk.  Chunk g reads buffer g & 1 and stages chunk g + 1
    // into the other one, so the last chunk of a pass with a successor stages chunk 0 again (with one chunk: itself, into the other
    // buffer), its unit 11 loads the next pass's first fragments, the first conv's operands wrap with it (loaded a chunk ahead:
    // the chunk before the last loads chunk 0's, the last chunk 1's) and its units 7 .. 11 load the weight steps 0 .. 4 of the next
    // channel block into the ring.  A later pass therefore starts with everything the loop's unit 0 needs in registers or in LDS:
    // it zeroes its accumulators and moves wbase.
    half8 bh[2][4], bl[2][4];
#define W3_BLOAD_AT(BB, U, SET)                                                                        \
        {                                                                                              \
            const int dy_ = (U) >> 2, xi_ = (U) & 3;                                                   \
            _Pragma("unroll") for (int n = 0; n < 4; ++n) {                                            \
                const int off = ((2 * n + dy_) * 4 + xi_) * 512;                                       \
                bh[SET][n] = *reinterpret_cast<const half8*>((BB) + off);                              \
                bl[SET][n] = *reinterpret_cast<const half8*>((BB) + W3_PART + off);                    \
            }                                                                                          \
        }
#pragma nounroll
    for (int pass = 0; pass < npass; ++pass) {
    const bool succ = !EARLIER && pass + 1 < npass;
    if constexpr (!EARLIER) {
        if (pass > 0) {
            // a later pass: no patch, no |max|, no im2col, no chunk-0 rows (slots 12, 13, 2 close its empty prologue parts)
            W3_STAMP(0)
            W3_STAMP(14)
            W3_STAMP(12)
            W3_STAMP(13)
            W3_STAMP(2)
            wbase += (int64_t)4 * a.nch * (W3_NST * F3_STEP_BYTES);
            bias2n = 0.f;
            if (succ) W3_BIAS_LOAD(bias2n, ocb + 1)
            // the pass's first fragments and the extra tile's are read again here, behind the epilogue, so that its registers are
            // free of them: 40 fewer live across it, two LDS round trips per pass
            W3_BLOAD_AT(lds + ((pass * a.nch) & 1) * W3_BUF + boff, 0, 0)
            ceh = *reinterpret_cast<const half8*>(lds + cole);
            cel = *reinterpret_cast<const half8*>(lds + cole + 64);
        }
        // every pass zeroes its accumulators here: defined at the head of the pass and dead behind its epilogue, they are not carried
        // around the loop over the passes (zeroed in the prologue as well, they were, as copies of sixteen registers each, and spilled)
        W3_ZERO_ACC()
        if (pass == 0) {
            __syncthreads();           // chunk 0's image is read across waves; the zeroing in front of it covers the waves' skew
            W3_BLOAD_AT(lds + boff, 0, 0)
        }
    }
    W3_STAMP(1)
    for (int chunk = 0; chunk < a.nch; ++chunk) {
        if (chunk >= 2 && chunk < 16 && !(chunk & 1)) W3_STAMP(2 + (chunk >> 1))   // slot 2 is the prologue's
        const int buf = EARLIER ? chunk & 1 : (pass * a.nch + chunk) & 1;
        const uint8_t* wp = wbase + (int64_t)chunk * (W3_NST * F3_STEP_BYTES);
        // the ring steps that lie behind this chunk's twelve: the next chunk's, or steps 0 .. 4 of the next pass's channel block,
        // which starts 4 nch chunks behind this one's; behind the last chunk of the last pass the 5 steps of padding
        const uint8_t* wpn = wp + (succ && chunk + 1 == a.nch ? (int64_t)3 * a.nch * (W3_NST * F3_STEP_BYTES) : 0);
        const uint8_t* bb = lds + buf * W3_BUF + boff;
        uint8_t* sdst = lds + (buf ^ 1) * W3_BUF;
        // chunk being staged (the last of a pass: chunk 0 for the next pass; the last of all: itself, unused)
        const int c1 = (chunk + 1 < a.nch ? chunk + 1 : succ ? 0 : chunk) * W3_CK;
        // the current form loads the first conv's operands a chunk ahead, in unit 8, behind the last MMA and ACT that read the present
        // ones: the rows of the staged chunk then start in unit 0 and their pieces have units 2 .. 10
        int n2 = chunk + 2;
        if (n2 >= a.nch) {
            n2 = succ ? n2 - a.nch : a.nch - 1;
            if (n2 >= a.nch) n2 -= a.nch;              // one chunk per pass
        }
        const int c2 = n2 * W3_CK;
#define W3_BLOAD(U, SET) W3_BLOAD_AT(bb, U, SET)
        if constexpr (EARLIER) {
            W3_BLOAD(0, 0)
            // all 8 reads of unit 0 in flight before its first MFMA: interleaved by the unit's schedule, each would wait alone
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int u = 0; u < W3_NST; ++u) {
            const int xi = u & 3;
            const uint8_t* wr = u + W3_RING - 1 < W3_NST ? wp : wpn;
            ah[(u + W3_RING - 1) % W3_RING] = *reinterpret_cast<const half8*>(wr + (u + W3_RING - 1) * F3_STEP_BYTES);
            al[(u + W3_RING - 1) % W3_RING] = *reinterpret_cast<const half8*>(wr + (u + W3_RING - 1) * F3_STEP_BYTES + 1024);
            if (u + 1 < W3_NST) W3_BLOAD(u + 1, (u + 1) & 1)
            if constexpr (EARLIER) {
                if (u == 0) W3_FUSED_LOAD(c1)
                if (u == 2 || u == 5 || u == 8) W3_ROW_READ((u - 2) / 3)
                if (u == 3 || u == 6 || u == 9) W3_ROW_MMA()
                if (u == 4 || u == 7 || u == 10) W3_ROW_ACT((u - 4) / 3)
                if (u == 5 || u == 8 || u == 11) W3_ROW_STORE((u - 5) / 3, sdst)
            } else {
                if (u == W3_NST - 1) W3_BLOAD_AT(sdst + boff, 0, 0)
                // The pieces of the three rows and the extra tile dealt over units 0 .. 10, at most 56 vector instructions a unit (16
                // an ACT2 piece, 16 a SHIFT, 19 a STORE2 piece) and at most 12 LDS reads (8 fragment reads + 4 of a READ2).  In program
                // order every piece follows the MMA, ACT2 or SHIFT it reads; the rows have registers of their own, so no piece
                // overwrites another's input.
                if (u == 0) W3_ROW_READ2(0)
                if (u == 1) { W3_ROW_MMA3() W3_ROW_READ2(1) }
                if (u == 2) { W3_EXTRA_ACT() W3_ROW_ACT2(0, 0) W3_ROW_ACT2(0, 1) W3_ROW_MMA2(1) W3_ROW_READ2(2) }
                if (u == 3) { W3_ROW_SHIFT(0) W3_ROW_STORE2(0, sdst, 0) W3_ROW_STORE2(0, sdst, 1) }
                if (u == 4) { W3_ROW_STORE2(0, sdst, 2) W3_ROW_STORE2(0, sdst, 3) W3_ROW_ACT2(1, 0) W3_ROW_MMA2(2) }
                if (u == 5) { W3_ROW_ACT2(1, 1) W3_ROW_SHIFT(1) W3_ROW_STORE2(1, sdst, 0) }
                if (u == 6) { W3_ROW_STORE2(1, sdst, 1) W3_ROW_STORE2(1, sdst, 2) W3_ROW_ACT2(2, 0) }
                if (u == 7) { W3_ROW_STORE2(1, sdst, 3) W3_ROW_ACT2(2, 1) W3_ROW_SHIFT(2) }
                if (u == 8) { W3_ROW_STORE2(2, sdst, 0) W3_ROW_STORE2(2, sdst, 1) W3_FUSED_LOAD(c2) }
                if (u == 9) W3_ROW_STORE2(2, sdst, 2)
                if (u == 10) W3_ROW_STORE2(2, sdst, 3)
            }
            const half8 A_h = ah[u % W3_RING], A_l = al[u % W3_RING];
            // product-major: the three MFMAs of one accumulator are 4 apart (no back-to-back dependent pair)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[xi][n] = mma32<0>(A_l, bh[u & 1][n], acc[xi][n]);
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[xi][n] = mma32<0>(A_h, bl[u & 1][n], acc[xi][n]);
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[xi][n] = mma32<0>(A_h, bh[u & 1][n], acc[xi][n]);
#pragma unroll
            for (int i = 0; i < 12; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                        // one MFMA
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                        // one LDS read
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                        // one global load
                // a gap has 24 free issue cycles beside its MFMA: four vector instructions beside an LDS read, six without one
                // (the eight fragment reads of the next unit take the first eight gaps)
                if constexpr (EARLIER) __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
                else if (i >= 8) __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);
                else __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);                        // one LDS write
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (!EARLIER) {
                if (u == W3_NST - 2) __syncthreads();
            }
        }
#undef W3_BLOAD
        if constexpr (EARLIER) __syncthreads();
    }
#undef W3_BLOAD_AT
#undef W3_ROW_READ
#undef W3_ROW_MMA
#undef W3_ROW_ACT
#undef W3_ROW_STORE
#undef W3_ROW_READ2
#undef W3_ROW_MMA2
#undef W3_ROW_MMA3
#undef W3_ROW_ACT2
#undef W3_EXTRA_ACT
#undef W3_ROW_SHIFT
#undef W3_ROW_STORE2

    W3_STAMP(10)
    // the next pass's bias into the image this pass does not read: its last readers were the previous pass's epilogues, in front of
    // this pass's barriers in every wave, and its next readers stand behind the next pass's.  (Pass 1's image is the prologue's:
    // with two passes, the usual case, no wave waits here for a load)
    if constexpr (!EARLIER) {
        if (succ && pass > 0 && tid < F3_OCB) reinterpret_cast<float*>(lds + W3_BIAS)[((pass + 1) & 1) * F3_OCB + tid] = bias2n;
    }
    // ---- epilogue: the inverse transform is lane-local (the four M_xi tiles share one layout): D col = lane&31 = pair p of
    // row 2n + ((lane>>4)&1), D row = (q&3) + 8*(q>>2) + 4*(lane>>5) = channel of the wave's 32.  Two adjacent pixels per
    // store (w is even, so a pair is either inside the image or wholly outside it)
    // What the epilogue derives from the tile and the lane alone is the same in every pass, and the compiler would compute it once, in
    // front of the loop over the passes: some 85 registers more that live through the chunk loop, which has none to spare (they went
    // to scratch).  The current form takes these inputs through an empty assembly statement per pass: recomputed behind every chunk
    // loop, as the single pass of the earlier form computes them.
    int eh = h, ew = w, ey0 = y0, ex0 = x0, elane = lane;
    if constexpr (!EARLIER) asm volatile("" : "+s"(eh), "+s"(ew), "+s"(ey0), "+s"(ex0), "+v"(elane));
    const int64_t ehw = (int64_t)eh * ew;
    const int ep = elane & 15;
    const int ocw = ocb * F3_OCB + __builtin_amdgcn_readfirstlane(wave) * 32;
    const int och = 4 * (elane >> 5), orow = (elane >> 4) & 1;
    float* ybase = a.y + (z * a.cout + ocw) * ehw + (int64_t)ey0 * ew;               // wave-uniform
    const unsigned loff = (unsigned)och * (unsigned)ehw + (unsigned)(orow * ew + ex0 + 2 * ep);
    const bool full = ey0 + F3_TH <= eh && ex0 + F3_TW <= ew;                        // uniform
    if constexpr (EARLIER) {
    // the activation and the bounds resolved outside the store loops (as in the direct kernel's epilogue)
#define W3_EPI(COND, ACT0, ACT1)                                                                                      \
    _Pragma("unroll") for (int q = 0; q < 16; ++q) {                                                                  \
        const int ocq = (q & 3) + 8 * (q >> 2);                                                                       \
        if (ocw + ocq + och < a.cout) {                                                                               \
            const float bq = a.bias ? a.bias[plane * a.cout + ocw + ocq + och] : 0.f;                                 \
            float* yq = ybase + (int64_t)ocq * ehw + loff;                                                            \
            _Pragma("unroll") for (int n = 0; n < 4; ++n) {                                                           \
                const float v0 = (acc[0][n][q] + acc[1][n][q] + acc[2][n][q]) * out_scale + bq;                       \
                const float v1 = (acc[1][n][q] - acc[2][n][q] - acc[3][n][q]) * out_scale + bq;                       \
                if (COND) *reinterpret_cast<f2_t*>(yq + 2 * n * ew) = f2_t{ACT0, ACT1};                               \
            }                                                                                                         \
        }                                                                                                             \
    }
    if (full && a.act != LLDWT_ACT_TANH) {
        const float slope = a.act == LLDWT_ACT_LRELU ? 0.01f : (a.act == LLDWT_ACT_RELU ? 0.f : 1.f);   // none: max(v, v)
        W3_EPI(true, fmaxf(v0, v0 * slope), fmaxf(v1, v1 * slope))
    } else {
        const bool colin = ex0 + 2 * ep < ew;     // w is even: a pair is either inside the image or wholly outside it
        W3_EPI(colin && ey0 + 2 * n + orow < eh, act_apply(v0, a.act), act_apply(v1, a.act))
    }
#undef W3_EPI
    } else {
    // The 16 bias values of the lane are in registers before the first store, read from the LDS image the prologue wrote.  A bias
    // load from global memory BETWEEN the stores stays behind them (a.bias may alias a.y for all the compiler knows), and vmcnt
    // counts loads and stores in issue order: every wait for a bias value was a wait for the stores in front of it to be
    // acknowledged, 16 store round trips in sequence.  Global loads hoisted in front of the stores do not cure it: a channel
    // block only some lanes run (oc < cout) makes the wait counters conservative, and the first use of each bias register in
    // such a block waits for vmcnt(0) again.  An LDS read counts on lgkmcnt, which no store touches.
    float bq[16];
    {
        const f4_t* bl = reinterpret_cast<const f4_t*>(lds + W3_BIAS +
                                                       ((pass & 1) * F3_OCB + __builtin_amdgcn_readfirstlane(wave) * 32 + och) * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const f4_t b4 = bl[2 * k];                  // channels 8k + och .. + 3 of the wave's 32: q = 4k .. 4k + 3
#pragma unroll
            for (int j = 0; j < 4; ++j) bq[4 * k + j] = b4[j];
        }
    }
    // The accumulators stay where the matrix pipe wrote them and every value is read next to its use (w3_acc_read).  Left to the
    // compiler, the epilogue's vector instructions pull all sixteen tiles into vector registers at the loop's exit, 256 at once, and
    // with the ring and the first conv's operands live through the epilogue the overflow went to scratch.  The compiler does not
    // see a read inside an assembly statement: the wait states between the last MFMA and the first read (19 for 16 passes) are here.
    asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 4");
    // the activation is resolved outside the store loops, one copy per activation and no branch per value: a block that only
    // some lanes run (a partial tile's store) makes the wait counters conservative for whatever follows it
    // The five copies below start with the same 256 values (transform, scale, bias); taken as common code they are computed in front
    // of the branch that picks a copy, 256 registers at once -- which a single pass had and a pass with a successor has not (the
    // weight ring and the first conv's operands live through the epilogue).  Each copy takes the output scale through an empty
    // assembly statement of its own, so that nothing is common and every value is formed next to its store.
#define W3_EPI(COND, ACT0, ACT1)                                                                                      \
    float os_ = out_scale;                                                                                            \
    asm volatile("" : "+v"(os_));                                                                                     \
    _Pragma("unroll") for (int q = 0; q < 16; ++q) {                                                                  \
        const int ocq = (q & 3) + 8 * (q >> 2);                                                                       \
        if (ocw + ocq + och < a.cout) {                                                                               \
            float* yq = ybase + (int64_t)ocq * ehw + loff;                                                            \
            _Pragma("unroll") for (int n = 0; n < 4; ++n) {                                                           \
                const float m0 = w3_acc_read(acc[0][n][q]), m1 = w3_acc_read(acc[1][n][q]);                           \
                const float m2 = w3_acc_read(acc[2][n][q]), m3 = w3_acc_read(acc[3][n][q]);                           \
                const float v0 = (m0 + m1 + m2) * os_ + bq[q];                                                        \
                const float v1 = (m1 - m2 - m3) * os_ + bq[q];                                                        \
                if (COND) *reinterpret_cast<f2_t*>(yq + 2 * n * ew) = f2_t{ACT0, ACT1};                               \
            }                                                                                                         \
        }                                                                                                             \
    }
    if (full && a.act != LLDWT_ACT_TANH) {
        const float slope = a.act == LLDWT_ACT_LRELU ? 0.01f : (a.act == LLDWT_ACT_RELU ? 0.f : 1.f);   // none: max(v, v)
        { W3_EPI(true, fmaxf(v0, v0 * slope), fmaxf(v1, v1 * slope)) }
    } else {
        const bool colin = ex0 + 2 * ep < ew;     // w is even: a pair is either inside the image or wholly outside it
#define W3_IN (colin && ey0 + 2 * n + orow < eh)
        // the four cases of act_apply, value for value
        if (a.act == LLDWT_ACT_TANH) {
            { W3_EPI(W3_IN, fast_tanh(v0), fast_tanh(v1)) }
        } else if (a.act == LLDWT_ACT_LRELU) {
            { W3_EPI(W3_IN, v0 >= 0.f ? v0 : 0.01f * v0, v1 >= 0.f ? v1 : 0.01f * v1) }
        } else if (a.act == LLDWT_ACT_RELU) {
            { W3_EPI(W3_IN, v0 > 0.f ? v0 : 0.f, v1 > 0.f ? v1 : 0.f) }
        } else {
            { W3_EPI(W3_IN, v0, v1) }
        }
#undef W3_IN
    }
#undef W3_EPI
    }
    W3_STAMP(11)
    W3_STAMP(15)
    ++ocb;
    }   // pass
#undef W3_FUSED_LOAD
#undef W3_BIAS_LOAD
#undef W3_ZERO_ACC
#undef W3_STAMP
}
#undef F3_STAMP

}  // namespace lldwt
using namespace lldwt;

// MFMA shape of the second conv's main loop, fixed for the process (weights are packed for it).  Default 32x32x16: measured
// 1.80 ms per level-0 launch against 1.91 ms for 16x16x32 (8 x 3 x 256 x 256, f16x3) -- the higher clock the chip holds on the
// small shape does not pay for the halved issue room between two MFMAs (8 free cycles instead of 24 for the fragment reads, the
// weight stream and the first conv's epilogue).  LLDWT_PLC_SHAPE=16 selects the 16x16x32 kernels (kept, tested)
static const int g_f3_shape16 = [] { const char* e = getenv("LLDWT_PLC_SHAPE"); return (e && !strcmp(e, "16")) ? 1 : 0; }();
static int f3_shape16() { return g_f3_shape16; }
extern "C" int lldwt_plc_shape16(void) { return g_f3_shape16; }

// Algorithm of the fused pair at PREC 0 with the 32x32x16 shape, fixed for the process: row-wise Winograd F(2,3) (k_plc_wino,
// the default: two thirds of the direct kernel's MFMAs) or the direct kernel (LLDWT_PLC_ALGO=direct, kept for A/B timing and
// the tests).  The other modes and the S16 shape always run the direct kernel.
static const int g_plc_wino = [] { const char* e = getenv("LLDWT_PLC_ALGO"); return (e && !strcmp(e, "direct")) ? 0 : 1; }();
static bool plc_wino_active() { return g_plc_wino && !g_f3_shape16; }
extern "C" int lldwt_plc_winograd(void) { return plc_wino_active() ? 1 : 0; }

extern "C" int64_t lldwt_conv_f16x3_packed_bytes(int cin, int cout) {
    if (cin <= 0 || cout <= 0) return -1;
    return f3_plane_bytes(cin, cout);
}

extern "C" int lldwt_conv_f16x3_pack(const float* w, void* packed, int cin, int cout, int64_t planes, void* stream) {
    LLDWT_REQUIRE(w && packed && cin > 0 && cout > 0 && planes > 0 && planes <= 65535, "conv_f16x3_pack: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const int64_t pb = f3_plane_bytes(cin, cout);
    for (int64_t p = 0; p < planes; ++p)
        if (hipMemsetAsync(reinterpret_cast<char*>(packed) + p * pb, 0, F3_HDR, st) != hipSuccess) {
            set_error("conv_f16x3_pack: memset failed");
            return LLDWT_EHIP;
        }
    const int64_t nw = (int64_t)cout * cin * 9;
    hipLaunchKernelGGL(k_f3_wmax, dim3(64, (unsigned)planes), dim3(256), 0, st, w, nw, reinterpret_cast<float*>(packed), pb);
    hipLaunchKernelGGL(k_f3_pack, dim3(1024, (unsigned)planes), dim3(256), 0, st, w, reinterpret_cast<uint8_t*>(packed), cin, cout, pb,
                       f3_shape16());
    if (plc_wino_active()) {          // the fused pair's Winograd weights (the section stays unwritten when nothing reads it)
        const int64_t wo = f3_wino_off(cin, cout);
        for (int64_t p = 0; p < planes; ++p)
            if (hipMemsetAsync(reinterpret_cast<char*>(packed) + p * pb + wo, 0, F3_HDR, st) != hipSuccess) {
                set_error("conv_f16x3_pack: memset failed");
                return LLDWT_EHIP;
            }
        hipLaunchKernelGGL(k_f3w_umax, dim3(64, (unsigned)planes), dim3(256), 0, st, w, (int64_t)cout * cin * 3,
                           reinterpret_cast<uint8_t*>(packed), pb, wo);
        hipLaunchKernelGGL(k_f3w_pack, dim3(1024, (unsigned)planes), dim3(256), 0, st, w, reinterpret_cast<uint8_t*>(packed), cin, cout,
                           pb, wo);
    }
    return check_launch("conv_f16x3_pack");
}

extern "C" int lldwt_absmax_slots(const float* x, int64_t planes, int64_t n_per_plane, float* slots, void* stream) {
    LLDWT_REQUIRE(x && slots && planes > 0 && planes <= 65535 && n_per_plane > 0, "absmax_slots: bad arguments");
    const int vec = (((uintptr_t)x) & 15) == 0 && (n_per_plane & 3) == 0;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(slots, 0, sizeof(float) * 64 * planes, st) != hipSuccess) {
        set_error("absmax_slots: memset failed");
        return LLDWT_EHIP;
    }
    int64_t gx = cdiv(n_per_plane / 4 + 1, 256 * 8);
    gx = gx < 1 ? 1 : (gx > 2048 ? 2048 : gx);
    hipLaunchKernelGGL(k_absmax_slots, dim3((unsigned)gx, (unsigned)planes), dim3(256), 0, st, x, n_per_plane, slots, vec);
    return check_launch("absmax_slots");
}

extern "C" int lldwt_conv3x3_f16x3(const float* x, float* y, const void* packed, const float* bias, const float* slots,
                                   int cin, int cout, int act, int64_t planes, int64_t batch, int64_t h, int64_t w_,
                                   void* stream) {
    LLDWT_REQUIRE(x && y && packed && slots, "conv3x3_f16x3: null pointer");
    LLDWT_REQUIRE(cin > 0 && cout > 0 && planes > 0 && batch > 0 && h > 0 && w_ > 0 && planes * batch <= 65535,
                  "conv3x3_f16x3: bad dims");
    LLDWT_REQUIRE(act == LLDWT_ACT_NONE || act == LLDWT_ACT_LRELU || act == LLDWT_ACT_TANH || act == LLDWT_ACT_RELU, "conv3x3_f16x3: bad activation");
    LLDWT_REQUIRE((int64_t)F3_CK * h * w_ * 4 < (int64_t)1 << 32, "conv3x3_f16x3: image too large for 32-bit chunk offsets");
    F3Args a;
    a.x = x; a.y = y; a.packed = reinterpret_cast<const uint8_t*>(packed); a.bias = bias; a.slots = slots;
    a.x16 = nullptr; a.xscale = nullptr; a.parent = nullptr; a.packed1 = nullptr; a.plane_bytes1 = 0; a.stamps = nullptr;
    a.cin = cin; a.cout = cout; a.act = act; a.batch = (int)batch; a.h = (int)h; a.w = (int)w_;
    a.tiles_x = (int)cdiv(w_, F3_TW);
    a.nch = f3_nch(cin);
    a.plane_bytes = f3_plane_bytes(cin, cout);
    const int tiles_y = (int)cdiv(h, F3_TH);
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void*)k_conv3_f16x3<0>, hipFuncAttributeMaxDynamicSharedMemorySize, F3_LDS) != hipSuccess ||
            hipFuncSetAttribute((const void*)k_conv3_f16x3<0, 0, true>, hipFuncAttributeMaxDynamicSharedMemorySize, F3_LDS) != hipSuccess ||
            hipFuncSetAttribute((const void*)k_conv3_f16x3<1>, hipFuncAttributeMaxDynamicSharedMemorySize, F3_LDS) != hipSuccess) {
            set_error("conv3x3_f16x3: cannot reserve %d bytes of LDS", F3_LDS);
            return LLDWT_EHIP;
        }
        attr_set = true;
    }
    dim3 grid((unsigned)(a.tiles_x * tiles_y), (unsigned)f3_nocb(cout), (unsigned)(planes * batch));
    if (g_f3_shape16) hipLaunchKernelGGL((k_conv3_f16x3<0, 0, true>), grid, dim3(256), F3_LDS, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_conv3_f16x3<0>, grid, dim3(256), F3_LDS, (hipStream_t)stream, a);
    return check_launch("conv3x3_f16x3");
}

// fp16-storage variant: x16 (planes,batch,cin,h,w) fp16 = fp32 activations x xscale[plane] (a power of two), as written by
// lldwt_conv2d_f16out; two MFMA products per k-step.
extern "C" int lldwt_conv3x3_f16in(const void* x16, float* y, const void* packed, const float* bias, const float* xscale,
                                   int cin, int cout, int act, int64_t planes, int64_t batch, int64_t h, int64_t w_,
                                   void* stream) {
    LLDWT_REQUIRE(x16 && y && packed && xscale, "conv3x3_f16in: null pointer");
    LLDWT_REQUIRE(cin > 0 && cout > 0 && planes > 0 && batch > 0 && h > 0 && w_ > 0 && planes * batch <= 65535,
                  "conv3x3_f16in: bad dims");
    LLDWT_REQUIRE(act == LLDWT_ACT_NONE || act == LLDWT_ACT_LRELU || act == LLDWT_ACT_TANH || act == LLDWT_ACT_RELU, "conv3x3_f16in: bad activation");
    LLDWT_REQUIRE((int64_t)F3_CK * h * w_ * 2 < (int64_t)1 << 32, "conv3x3_f16in: image too large for 32-bit chunk offsets");
    F3Args a;
    a.x = nullptr; a.y = y; a.packed = reinterpret_cast<const uint8_t*>(packed); a.bias = bias; a.slots = nullptr;
    a.x16 = reinterpret_cast<const _Float16*>(x16); a.xscale = xscale;
    a.parent = nullptr; a.packed1 = nullptr; a.plane_bytes1 = 0; a.stamps = nullptr;
    a.cin = cin; a.cout = cout; a.act = act; a.batch = (int)batch; a.h = (int)h; a.w = (int)w_;
    a.tiles_x = (int)cdiv(w_, F3_TW);
    a.nch = f3_nch(cin);
    a.plane_bytes = f3_plane_bytes(cin, cout);
    const int tiles_y = (int)cdiv(h, F3_TH);
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void*)k_conv3_f16x3<1>, hipFuncAttributeMaxDynamicSharedMemorySize, F3_LDS) != hipSuccess ||
            hipFuncSetAttribute((const void*)k_conv3_f16x3<1, 0, true>, hipFuncAttributeMaxDynamicSharedMemorySize, F3_LDS) != hipSuccess) {
            set_error("conv3x3_f16in: cannot reserve %d bytes of LDS", F3_LDS);
            return LLDWT_EHIP;
        }
        attr_set = true;
    }
    dim3 grid((unsigned)(a.tiles_x * tiles_y), (unsigned)f3_nocb(cout), (unsigned)(planes * batch));
    if (g_f3_shape16) hipLaunchKernelGGL((k_conv3_f16x3<1, 0, true>), grid, dim3(256), F3_LDS, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_conv3_f16x3<1>, grid, dim3(256), F3_LDS, (hipStream_t)stream, a);
    return check_launch("conv3x3_f16in");
}


// ---- the tree-context PAIR in one launch: y = act2(conv3x3(LeakyReLU(conv3x3(up2(parent)) + b1)) + b2)
extern "C" int64_t lldwt_plc_fused_pack1_bytes(int cmid) { return cmid > 0 && cmid <= 256 ? f1_plane_bytes(cmid) : -1; }

extern "C" int lldwt_plc_fused_pack1(const float* w1, const float* b1, void* packed1, int cmid, int64_t planes, void* stream) {
    LLDWT_REQUIRE(w1 && b1 && packed1 && cmid > 0 && cmid <= 256 && planes > 0 && planes <= 65535, "plc_fused_pack1: bad arguments");
    hipLaunchKernelGGL(k_f1_pack, dim3((unsigned)planes), dim3(256), 0, (hipStream_t)stream, w1, b1,
                       reinterpret_cast<uint8_t*>(packed1), cmid, f1_plane_bytes(cmid));
    return check_launch("plc_fused_pack1");
}

static unsigned long long* g_f3_stamps = nullptr;
static int64_t g_f3_stamps_bytes = 0;
namespace lldwt { void f3_set_stamps(void* p, int64_t nbytes) { g_f3_stamps = reinterpret_cast<unsigned long long*>(p); g_f3_stamps_bytes = p ? nbytes : 0; } }
// diagnostics flags of the pair (lldwt_set_diagnostics kind 1; read per launch): bit 0 = k_plc_wino in its earlier form; bit 1 =
// k_plc_wino with one workgroup per (tile, channel block); bit 2 = one workgroup per tile at any size (lldwt_plc_fused)
static int g_f3_flags = 0;
namespace lldwt { void f3_set_debug(int flags) { g_f3_flags = flags; } }

extern "C" int lldwt_plc_fused(const float* parent, float* y, const void* packed1, const void* packed2, const float* bias2,
                               int cmid, int cout, int act, int64_t planes, int64_t batch, int64_t h, int64_t w_, void* stream) {
    LLDWT_REQUIRE(parent && y && packed1 && packed2, "plc_fused: null pointer");
    LLDWT_REQUIRE(cmid > 0 && cmid <= 256 && cout > 0 && planes > 0 && batch > 0 && h > 0 && w_ > 0 && planes * batch <= 65535,
                  "plc_fused: bad dims");
    LLDWT_REQUIRE(h % 2 == 0 && w_ % 2 == 0, "plc_fused: the output is the 2x-upsampled parent's size: even h, w");
    LLDWT_REQUIRE(act == LLDWT_ACT_NONE || act == LLDWT_ACT_LRELU || act == LLDWT_ACT_TANH || act == LLDWT_ACT_RELU, "plc_fused: bad activation");
    F3Args a;
    a.x = nullptr; a.y = y; a.packed = reinterpret_cast<const uint8_t*>(packed2); a.bias = bias2; a.slots = nullptr;
    a.x16 = nullptr; a.xscale = nullptr;
    a.parent = parent; a.packed1 = reinterpret_cast<const uint8_t*>(packed1); a.plane_bytes1 = f1_plane_bytes(cmid);
    a.cin = cmid; a.cout = cout; a.act = act; a.batch = (int)batch; a.h = (int)h; a.w = (int)w_;
    a.tiles_x = (int)cdiv(w_, F3_TW);
    a.nch = f3_nch(cmid);
    a.plane_bytes = f3_plane_bytes(cmid, cout);
    const int tiles_y = (int)cdiv(h, F3_TH);
    {   // diagnostics (tools/plc_stamps.py, lldwt_set_diagnostics): only when the registered buffer holds this grid's stamps
        const int64_t need = (int64_t)a.tiles_x * tiles_y * f3_nocb(cout) * planes * batch * 4 * 16 * 8;
        a.stamps = (g_f3_stamps && g_f3_stamps_bytes >= need) ? g_f3_stamps : nullptr;
    }
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void*)k_conv3_f16x3<2, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, F1_LDS) != hipSuccess ||
            hipFuncSetAttribute((const void*)k_conv3_f16x3<2, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, F1_LDS) != hipSuccess ||
            hipFuncSetAttribute((const void*)k_conv3_f16x3<2, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, F1_LDS) != hipSuccess ||
            hipFuncSetAttribute((const void*)k_conv3_f16x3<2, 0, true>, hipFuncAttributeMaxDynamicSharedMemorySize, F1_LDS) != hipSuccess ||
            hipFuncSetAttribute((const void*)k_conv3_f16x3<2, 1, true>, hipFuncAttributeMaxDynamicSharedMemorySize, F1_LDS) != hipSuccess ||
            hipFuncSetAttribute((const void*)k_conv3_f16x3<2, 2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, F1_LDS) != hipSuccess) {
            set_error("plc_fused: cannot reserve %d bytes of LDS", F1_LDS);
            return LLDWT_EHIP;
        }
        attr_set = true;
    }
    dim3 grid((unsigned)(a.tiles_x * tiles_y), (unsigned)f3_nocb(cout), (unsigned)(planes * batch));
    const int prec = split_precision();
    if (prec == 0 && plc_wino_active()) {
        static bool wattr_set = false;
        if (!wattr_set) {
            if (hipFuncSetAttribute((const void*)k_plc_wino<false>, hipFuncAttributeMaxDynamicSharedMemorySize, W3_LDS) != hipSuccess ||
                hipFuncSetAttribute((const void*)k_plc_wino<true>, hipFuncAttributeMaxDynamicSharedMemorySize, W3_LDS_EARLIER) != hipSuccess) {
                set_error("plc_fused: cannot reserve %d bytes of LDS", W3_LDS);
                return LLDWT_EHIP;
            }
            wattr_set = true;
        }
        a.nch = w3_nch(cmid);
        if (g_f3_flags & 1) hipLaunchKernelGGL(k_plc_wino<true>, grid, dim3(256), W3_LDS_EARLIER, (hipStream_t)stream, a);
        else {
            // One workgroup per pixel tile that loops over the tile's channel blocks (grid.y = 1), or one per (tile, channel block).
            // With n = tiles x images, T a single-block workgroup's time and s what a later pass saves, the fold pays when
            // ceil(n / CUs) (nocb T - (nocb - 1) s) < ceil(nocb n / CUs) T (plc_fold.h; s / T = 0.09 from the stamps of round 11).
            // Diagnostics flags: bit 1 forces one workgroup per block, bit 2 the fold.
            static const int cus = [] {
                int dev = 0, n = 0;
                if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 0;
                return n;
            }();
            const bool fold = (g_f3_flags & 2) ? false : (g_f3_flags & 4) ? true : plc_fold_pays((int64_t)grid.x * grid.z, cus, (int)grid.y);
            if (fold) grid.y = 1;
            hipLaunchKernelGGL(k_plc_wino<false>, grid, dim3(256), W3_LDS, (hipStream_t)stream, a);
        }
    } else if (g_f3_shape16) {
        if (prec == 1) hipLaunchKernelGGL((k_conv3_f16x3<2, 1, true>), grid, dim3(256), F1_LDS, (hipStream_t)stream, a);
        else if (prec == 2) hipLaunchKernelGGL((k_conv3_f16x3<2, 2, true>), grid, dim3(256), F1_LDS, (hipStream_t)stream, a);
        else hipLaunchKernelGGL((k_conv3_f16x3<2, 0, true>), grid, dim3(256), F1_LDS, (hipStream_t)stream, a);
    } else if (prec == 1) hipLaunchKernelGGL((k_conv3_f16x3<2, 1>), grid, dim3(256), F1_LDS, (hipStream_t)stream, a);
    else if (prec == 2) hipLaunchKernelGGL((k_conv3_f16x3<2, 2>), grid, dim3(256), F1_LDS, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((k_conv3_f16x3<2, 0>), grid, dim3(256), F1_LDS, (hipStream_t)stream, a);
    return check_launch("plc_fused");
}
