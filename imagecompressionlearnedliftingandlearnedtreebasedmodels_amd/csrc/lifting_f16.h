// lifting_f16.h -- shared between lifting.hip (pack layout, step dispatch) and lifting_f16.hip (the fused split-fp16
// lifting-step kernel).  Internal to the library.
#pragma once
#include "common.h"

namespace lldwt {

// The fused kernel exists for the reference's configuration: 16 channels (depth_scale*8, liftingDWT.json:22), 5x5.
constexpr int LF_C = 16, LF_K = 5, LF_KK = 25;
constexpr int LF_KS = 13;                 // k-steps of 32 = 2 taps x 16 channels (25 taps -> 26, the last one zero)
constexpr int LF_KS4 = 3;                 // conv4 as D[dx][px]: K = 5 dy x 16 ch = 80 -> 3 k-steps of 32
constexpr int LF_FRAG = 1024;             // halves per k-step: (hi, lo) x 64 lanes x 8
// per orientation, in HALVES: conv1 | conv2 | conv3 | conv4 fragments; then 16 floats: s_w1..s_w4, b1[16]... (see .hip)
constexpr int LF_H_C1 = 0;
constexpr int LF_H_C2 = LF_H_C1 + LF_FRAG;
constexpr int LF_H_C3 = LF_H_C2 + LF_KS * LF_FRAG;
constexpr int LF_H_C4 = LF_H_C3 + LF_KS * LF_FRAG;
constexpr int LF_KSC = 5;                 // conv4 o conv3 composed (9x9, 16 -> 1) as D[dx][px]: K = 9 dy x 16 ch = 144 -> 5 k-steps
constexpr int LF_H_CC = LF_H_C4 + LF_KS4 * LF_FRAG;           // composite fragments
constexpr int LF_H_END = LF_H_CC + LF_KSC * LF_FRAG;          // 35 * 1024 halves
// floats after the fragments: [0..3] s_w1..s_w4, [4] s_wc, [5] b4 + sum_oc (b3 + b1)[oc] * sum_taps w4[oc] (the composed path's
// constant), [16..31] sum over taps of w4[oc], [32..112] Wr[81] = w4 o w1
constexpr int LF_TAIL_FLOATS = 128;
// behind the tail, in HALVES from the section start: a bf16 copy of the scaled weights, 512 per k-step (the one-product bf16 mode)
constexpr int LF_H_BF = LF_H_END + 2 * LF_TAIL_FLOATS;
constexpr int LF_NSTEP = LF_H_END / LF_FRAG;                  // 35 k-steps
constexpr int LF_ORIENT_FLOATS = (LF_H_BF + LF_NSTEP * 512) / 2;
constexpr int LF_FLOATS = 2 * LF_ORIENT_FLOATS;               // both orientations

constexpr __host__ __device__ int lift_f16_floats(int C, int K) { return (C == LF_C && K == LF_K) ? LF_FLOATS : 0; }

// Float offsets inside one packed P/U block (lldwt_pack_pblock): two fp32 orientation sections of `orient` floats each
// (w1 | b1 | w2 | b2 | w3 | b3 | w4 | b4, every part padded to 16 floats), then at f16 the split-fp16 section laid out above.
// The ONE definition of the layout: the pack kernels, the fp32 step kernels and the fused kernel's launch all read it here.
constexpr __host__ __device__ int pad16(int n) { return (n + 15) & ~15; }
struct PackOff {
    int w1, b1, w2, b2, w3, b3, w4, b4, orient, f16, total;
};
constexpr __host__ __device__ PackOff pack_off(int C, int K) {
    PackOff o{};
    int KK = K * K;
    o.w1 = 0;
    o.b1 = o.w1 + pad16(KK * C);
    o.w2 = o.b1 + pad16(C);
    o.b2 = o.w2 + pad16(C * KK * C);
    o.w3 = o.b2 + pad16(C);
    o.b3 = o.w3 + pad16(C * KK * C);
    o.w4 = o.b3 + pad16(C);
    o.b4 = o.w4 + pad16(C * KK);
    o.orient = o.b4 + 16;
    o.f16 = 2 * o.orient;
    o.total = o.f16 + lift_f16_floats(C, K);
    return o;
}

// pack the f16 section of one P/U block of the fused kernel's configuration (called from lldwt_pack_pblock after the fp32
// section is written); plane_stride: floats between the planes' blocks
int lift_f16_pack(const float* w1, const float* w2, const float* w3, const float* w4, const float* b1, const float* b3,
                  const float* b4, float* packed, int64_t plane_stride, int planes, int compose, hipStream_t st);
// the "backward pack": the transposed, mirrored weights in the same section (fp32 section left to the caller, who zeroes it)
int lift_f16_pack_bwd(const float* w1, const float* w2, const float* w3, const float* w4, float* scratch, float* packed,
                      int64_t plane_stride, int planes, hipStream_t st);
int64_t lift_f16_bwd_scratch_floats(int planes);

struct LiftF16Views {
    const float* src;  int64_t src_sz, src_sy, src_sx;
    const float* din;  int64_t din_sz, din_sy, din_sx;
    float* dout;       int64_t dout_sz, dout_sy, dout_sx;
};
// the training forward of one step on the fused kernel's sequential path: the same step, and the tile interiors of src, skip
// (Z, h, w) and t1, t2, t3 (Z, 16, h, w) written out for the backward (what k_lift_a/b/c save on the fp32 path)
struct LiftF16Saved { float* src; float* skip; float* t1; float* t2; float* t3; };
// backward-data of one step on the same kernel (BWD mode): g = dL/dnet dense (Z, h, w); t1, t2 = the saved tanh outputs; out:
// dt3, dpre2, dr (Z, 16, h, w) and dsk (Z, h, w)
// mx: null, or (planes, 2, 64) floats zeroed by the caller: the launch leaves max |dt3| (row 0) and max |dpre2| (row 1) of every
// plane spread over the 64 slots (atomic max), the form lldwt::wgrad16_f16x3 takes its dY maximum in
struct LiftF16Bwd { const float* g; const float* t1; const float* t2; float* dt3; float* dpre2; float* dr; float* dsk; float* mx; };

// One launch of the fused lifting step: dst_out = dst_in + sign * (skip + rw * P(skip)) over the views v.
//   v2    : null, or a second, independent view set of the same geometry and parameters in the same launch: images
//           0 .. Z-1 use v, images Z .. 2Z-1 use *v2
//   saved : null, or the training forward: the step on the sequential path with its intermediates written out
//   bwd   : null, or the backward-data chain of the step instead: v, v2, saved, sign and rw are ignored (the kernel's input
//           is bwd->g), taps = (planes, 3) floats (0, 1, 0), packed = lift_f16_pack_bwd's buffer
//   packed / pstride : the planes' packed blocks (pack_off(LF_C, LF_K) layout) and the floats between them
struct LiftF16Call {
    LiftF16Views v;
    const LiftF16Views* v2;
    const LiftF16Saved* saved;
    const LiftF16Bwd* bwd;
    int64_t Z, batch, h, w;             // Z images of h x w per view set, `batch` of them per plane
    const float* taps;                  // (planes, 3) skip filter
    const float* packed;
    int64_t pstride;
    int vertical;
    float sign, rw;
    hipStream_t st;
};
int lift_f16_launch(const LiftF16Call& c);         // LLDWT_OK or an error

// arithmetic of the split-fp16 kernel families (lldwt_set_precision): 0 = f16x3 (three products per MAC, fp32-level accuracy),
// 1 = fp16, 2 = bf16 (one product per MAC).  Defined in lifting_f16.hip, read at launch by conv_f16x3.hip and cgp_f16x3.hip too
int split_precision();
void split_set_precision(int p);

// diagnostics (lldwt_set_diagnostics): debug mask of the fused step (bit i = skip phase i+1, 16 = sequential conv3 / conv4,
// 32 = no vertical reuse, 64 = the border tiles' strip correction in its earlier form: every k-step of the strips, half a wave
// per corrected pixel; same output bits, 128 = correction sums behind the composite loop's barrier and no skipped MFMA tiles
// at the image's top / bottom; same output bits, 256 = conv2's weight fragments requested at the head of P2 instead of during P1: the
// earlier form; same output bits, 512 = with a registered stamp buffer, the f16x3 eval kernels that also stamp inside P2)
// and the stamp buffers of the three split-fp16 kernel families (the fused step's: 32 slots per wave and tile)
void lift_f16_set_debug(int dbg);
void lift_f16_set_stamps(void* p, int64_t nbytes);
void f3_set_stamps(void* p, int64_t nbytes);
void cgp16_set_stamps(void* p, int64_t nbytes);

}  // namespace lldwt
