/*
 * lldwt.h -- C-ABI of the MI355X-native learned-lifting DWT + CNN entropy-model hot path.
 *
 * Drop-in boundary.  The reference (uberkk/ImageCompressionLearnedLiftingandLearnedTreeBasedModels)
 * is pure PyTorch and defines no FFI; its boundary for this path is the Python module API
 * (agents/liftingDWT_agent.py, graphs/models/LiftingBasedDWT_net.py).  The entry points below are what the
 * host-side mirror of those modules binds through ctypes; each one cites the reference
 * code it replaces (paths relative to the reference root).
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller (allocated by the host
 *    framework, e.g. PyTorch's caching allocator).  The library never allocates or frees user-visible memory;
 *    scratch space is passed in as `ws` and sized by the matching *_ws_bytes() query.
 *  - `stream` is a hipStream_t passed as void*; kernels are enqueued on it, no call synchronises.
 *  - return value: 0 on success, negative LLDWT_E* otherwise; lldwt_last_error() gives a message
 *    (thread-local, valid until the next failing call on the thread).  No exceptions cross the boundary.
 *  - tensors are fp32, dense, "plane-major NCHW": shape (Z, C, h, w) with Z = planes*batch, plane-major
 *    (z = plane*batch + b).  A *plane* is one colour channel processed by its own network (clrch == 1:
 *    LiftingBasedDWT_net.py:43-46); parameters of the `planes` networks are stacked on a leading axis and
 *    addressed as base + plane*stride.
 */
#ifndef LLDWT_H
#define LLDWT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LLDWT_OK 0
#define LLDWT_EINVAL (-1)   /* bad argument / unsupported shape */
#define LLDWT_EHIP (-2)     /* HIP runtime error (launch failed) */
#define LLDWT_EWS (-3)      /* workspace too small */

#define LLDWT_ACT_NONE 0
#define LLDWT_ACT_TANH 1
#define LLDWT_ACT_LRELU 2   /* LeakyReLU(0.01) */
#define LLDWT_ACT_RELU 3    /* ReLU (post-processing networks, post_processing_networks.py:45,60-70) */

const char* lldwt_last_error(void);
/* ABI version; raised whenever an entry point is removed, renamed or changes its arguments (101: one entry point per operation). */
int lldwt_version(void);
/* 1 if the calling process sees a gfx950 device, 0 otherwise (no compute is launched). */
int lldwt_device_ok(void);

/* ---------------------------------------------------------------------------------------------------------
 * Strided view of a (Z, h, w) single-channel tensor: element (z,y,x) at p[z*sz + y*sy + x*sx].
 * Used for the polyphase components: the even/odd rows (or columns) of an array are views with sy (sx)
 * doubled, so the split (wavelet_forward_v2.py:27-28,33-34,45-46) and the merge
 * (wavelet_inverse_v2.py:49-53) are pure addressing -- no copies, bit-exact by construction.            */
typedef struct lldwt_view {
    float* p;
    int64_t sz, sy, sx;
} lldwt_view;

/* ---------------------------------------------------------------------------------------------------------
 * Colour transforms of the agent (agents/liftingDWT_agent.py:86-87,90-94; compressai RGB2YCbCr/YCbCr2RGB,
 * BT.709).  rgb: (B,3,H,W) NCHW in [0,1].  ycc: plane-major (3,B,1,H,W) with 0.5 subtracted from Y only.
 * inverse: ycc -> rgb, then "- 0.5" (agents/liftingDWT_agent.py:94) and optional clamp to [-0.5,0.5] (:181). */
int lldwt_rgb_to_ycc(const float* rgb, float* ycc, int64_t B, int64_t H, int64_t W, void* stream);
int lldwt_ycc_to_rgb(const float* ycc, float* rgb, int64_t B, int64_t H, int64_t W, int clamp, void* stream);
/* backward of lldwt_ycc_to_rgb without clamp (training): grgb (B,3,H,W) -> gycc plane-major (3,B,1,H,W). */
int lldwt_ycc_to_rgb_bwd(const float* grgb, float* gycc, int64_t B, int64_t H, int64_t W, void* stream);

/* Input pipeline (dataloaders/image_dl.py:63-105: PIL decode, crop, ToTensor): the host decodes and crops to uint8
 * HWC (3 B/pixel over PCIe instead of 12); this converts a (B,H,W,3) uint8 batch to (B,3,H,W) fp32 in [0,1] with
 * ToTensor's arithmetic (x / 255 in fp32), bit-exact.                                                          */
int lldwt_u8hwc_to_f32chw(const uint8_t* src, float* dst, int64_t B, int64_t H, int64_t W, void* stream);

/* Image codec I/O (the package's codec.py; the reference has no file codec), on a tile grid: each of the B images of a
 * (B,H,W,3) uint8 RGB batch is cut into ny x nx tiles of th x tw; tile index t = (b * ny + ty) * nx + tx covers rows
 * [ty*th, (ty+1)*th) and columns [tx*tw, (tx+1)*tw); positions past the last row / column take the value of the clamped
 * source pixel (replicate-edge padding).  The untiled codec is the 1 x 1 grid with (th, tw) = (Hp, Wp).
 * lldwt_u8hwc_to_ycc_tiles: the tiles first .. first+n-1 -> ycc plane-major (3,n,1,th,tw) YCbCr with Y-0.5; every value
 *   bitwise equal to lldwt_u8hwc_to_f32chw followed by lldwt_rgb_to_ycc on the padded tile.  n, th <= 65535.
 * lldwt_ycc_tiles_to_u8hwc: ycc (3,n,1,th,tw) of the tiles tiles[0..n-1] (a device int32 array; NULL: first .. first+n-1)
 *   -> the pixels of those tiles inside the image and inside the region [y0, y0+h) x [x0, x0+w) (which must lie in the
 *   image), written to dst (B,h,w,3) uint8 RGB at the tile's image b: floor((v + 0.5f) * 255.0f + 0.5f) of
 *   v = lldwt_ycc_to_rgb(..., clamp=1).  Pixels of the region no listed tile covers are left as they are.  n, th <= 65535.
 * lldwt_u8hwc_to_ycc_pad: src (B,H,W,3) -> ycc (3,B,1,Hp,Wp), Hp >= H, Wp >= W: the 1 x 1 grid.  B, Hp <= 65535.
 * lldwt_ycc_to_u8hwc_crop: ycc (3,B,1,Hp,Wp) -> dst (B,H,W,3) of the top-left H x W: the 1 x 1 grid, region = the image.
 *   B, H <= 65535.
 * lldwt_ll_tiles_to_u8hwc: lldwt_ycc_tiles_to_u8hwc for a reduced-resolution decode: ycc holds the decoded LL band at level
 *   k of each tile (3,n,1,th,tw) with th, tw, H, W the reduced tile and image sizes; every sample s of plane p becomes
 *   (s - b[p]) * inv_a[p] (inv_a, b: 3 host floats each, lifting_dwt_nets.ll_affine) before the same colour and u8 rule.
 *   Refuses a non-finite or zero inv_a, a non-finite b, and every grid / region lldwt_ycc_tiles_to_u8hwc refuses.
 *   With inv_a = 1, b = 0 the bytes are those of lldwt_ycc_tiles_to_u8hwc.
 * lldwt_ycc_tiles_sq_err: the exact squared error of the bytes lldwt_ycc_tiles_to_u8hwc would write with the region being
 *   the whole image: for every in-image pixel of the tiles tiles[0..n-1] (NULL: first .. first+n-1) the
 *   three bytes are formed by the same device function and their squared differences to src (B,H,W,3) uint8 are added to
 *   sse[b], b the tile's image; sse: B device uint64, which the caller zeroes (the entry point accumulates).  No image is
 *   written.  A tile index outside [0, B * ny * nx) adds nothing.  Integer sums and 64-bit integer atomics: the value is
 *   exact and does not depend on the order of arrival.  The 1 x 1 grid (tiles == NULL, th = Hp, tw = Wp) is the untiled
 *   codec's case and, over the blended buffer of lldwt_ycc_tiles_blend, the lapped one.  n <= 65535, th <= 8 * 65535.
 * Every tile entry point requires ny * th >= H and nx * tw >= W.                                                                                                   */
int lldwt_u8hwc_to_ycc_tiles(const uint8_t* src, float* ycc, int64_t B, int64_t H, int64_t W, int64_t th, int64_t tw,
                             int64_t ny, int64_t nx, int64_t first, int64_t n, void* stream);
int lldwt_ycc_tiles_to_u8hwc(const float* ycc, const int32_t* tiles, int64_t first, int64_t n, int64_t B, int64_t H, int64_t W,
                             int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0, int64_t x0, int64_t h, int64_t w,
                             uint8_t* dst, void* stream);
int lldwt_ll_tiles_to_u8hwc(const float* ycc, const int32_t* tiles, int64_t first, int64_t n, int64_t B, int64_t H, int64_t W,
                            int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0, int64_t x0, int64_t h, int64_t w,
                            const float* inv_a, const float* b, uint8_t* dst, void* stream);
int lldwt_ycc_tiles_sq_err(const float* ycc, const int32_t* tiles, int64_t first, int64_t n, int64_t B, int64_t H, int64_t W,
                           int64_t th, int64_t tw, int64_t ny, int64_t nx, const uint8_t* src, uint64_t* sse, void* stream);
/* Lapped tile grid (codec.py encode_tiled(..., overlap=ov)): ny x nx tiles of th x tw at the stride
 * (sh, sw) = (th - ov, tw - ov); tile (ty, tx) covers rows [ty*sh, ty*sh + th) and columns [tx*sw, tx*sw + tw), so
 * neighbours share a band of ov pixels.  Both entry points require ov to be a power of two with 2 * ov <= min(th, tw)
 * (at most two tiles cover a pixel along an axis) and (ny-1)*sh + th >= H, (nx-1)*sw + tw >= W; H, W < 2^31, th <= 65535.
 * lldwt_u8hwc_to_ycc_tiles_lapped: lldwt_u8hwc_to_ycc_tiles at that stride: the tiles first .. first+n-1 (index
 *   (b * ny + ty) * nx + tx) -> ycc (3,n,1,th,tw); every value bitwise lldwt_u8hwc_to_ycc_pad of the replicate-padded crop
 *   at (ty*sh, tx*sw).  n <= 65535.
 * lldwt_ycc_tiles_blend: accumulates one group of n decoded tiles of ONE image, ycc (3,n,1,th,tw), into the fp32 region
 *   buffer acc (3,1,1,h,w) of the region [y0, y0+h) x [x0, x0+w) (inside the image; h <= 65535), which the caller zeroes
 *   before the first group.  slots: a device int32 array of nslots == ny * nx entries, slots[ty * nx + tx] = the tile's
 *   slot in ycc, or -1 when it is not in this group.  Per region pixel and plane, for the covering tiles of the group in
 *   ascending tile index: acc = fadd(acc, fmul(wy * wx, v)), separately rounded (no FMA), with the 1-D weight of local
 *   index i in tile q of n: (i + 0.5) / ov if q > 0 and i < ov; (t - i - 0.5) / ov if q < n-1 and i >= t - ov; else 1.  Groups
 *   fed in ascending tile index give the same bits whatever the grouping; a pixel one tile covers gets acc == v.  Samples
 *   are blended raw (a reduced decode's LL band before the lldwt_ll_tiles_to_u8hwc affine map, with th, tw, ov, H, W the
 *   reduced sizes); acc is then a 1 x 1 grid for lldwt_ycc_tiles_to_u8hwc / lldwt_ll_tiles_to_u8hwc.                      */
int lldwt_u8hwc_to_ycc_tiles_lapped(const uint8_t* src, float* ycc, int64_t B, int64_t H, int64_t W, int64_t th, int64_t tw,
                                    int64_t ov, int64_t ny, int64_t nx, int64_t first, int64_t n, void* stream);
int lldwt_ycc_tiles_blend(const float* ycc, const int32_t* slots, int64_t nslots, int64_t n, int64_t H, int64_t W, int64_t th,
                          int64_t tw, int64_t ov, int64_t ny, int64_t nx, int64_t y0, int64_t x0, int64_t h, int64_t w,
                          float* acc, void* stream);
int lldwt_u8hwc_to_ycc_pad(const uint8_t* src, float* ycc, int64_t B, int64_t H, int64_t W, int64_t Hp, int64_t Wp,
                           void* stream);
int lldwt_ycc_to_u8hwc_crop(const float* ycc, uint8_t* dst, int64_t B, int64_t H, int64_t W, int64_t Hp, int64_t Wp,
                            void* stream);
/* Chroma formats 4:2:0 and 4:0:0 (codec.py chroma=; csrc/chroma.hip) on the plain tile grid above.  A 4:2:0
 * tile is a luma plane (1,n,1,th,tw) and a chroma plane pair (2,n,1,th/2,tw/2) (Cb, Cr); th, tw even.  A 4:0:0 tile is one
 * plane (1,n,1,th,tw) of a (B,H,W,1) uint8 image.  The limits of the 4:4:4 entry points hold (n, th <= 65535).
 * lldwt_u8hwc_to_ycc420_tiles: the tiles first .. first+n-1 of src (B,H,W,3).  Per source pixel, coordinates clamped to the
 *   image, Y-0.5, Cb, Cr are the values of lldwt_u8hwc_to_ycc_tiles; luma holds Y-0.5 (bitwise plane 0 of that entry point) and
 *   chroma sample (i, j) of a tile is ((c00 + c01) + (c10 + c11)) * 0.25f over the tile pixels (2i..2i+1, 2j..2j+1), every
 *   add separately rounded.  One pass; luma must be 8-byte aligned.
 * lldwt_ycc420_tiles_to_u8hwc: the tiles tiles[0..n-1] (NULL: first .. first+n-1) -> the pixels inside the image and the
 *   region, dst (B,h,w,3), as lldwt_ycc_tiles_to_u8hwc.  For tile pixel (y, x): cy = y >> 1, ny = cy + 1 if y is odd else
 *   cy - 1, clamped to [0, th/2 - 1] (the tile's own plane; cx, nx alike); t(r) = 0.75f * c[r][cx] + 0.25f * c[r][nx];
 *   v = 0.75f * t(cy) + 0.25f * t(ny), every product and sum separately rounded; (Y-0.5, v_cb, v_cr) then give the bytes of
 *   lldwt_ycc_tiles_to_u8hwc.  inv_a, b: 3 host floats each or both NULL; given, every luma and chroma SAMPLE s of plane p
 *   becomes (s - b[p]) * inv_a[p] before the upsampling (a reduced-resolution decode, as lldwt_ll_tiles_to_u8hwc).
 * lldwt_u8hw_to_y_tiles: src (B,H,W,1) -> y (1,n,1,th,tw), g / 255.0f - 0.5f at the clamped source pixel.
 * lldwt_y_tiles_to_u8hw: y (1,n,1,th,tw) -> dst (B,h,w,1), floor((clamp(s, -0.5, 0.5) + 0.5f) * 255.0f + 0.5f), tile list, grid
 *   and region as above; inv_a, b: 1 host float each or both NULL, s -> (s - b[0]) * inv_a[0] first.                          */
int lldwt_u8hwc_to_ycc420_tiles(const uint8_t* src, float* luma, float* chroma, int64_t B, int64_t H, int64_t W, int64_t th,
                                int64_t tw, int64_t ny, int64_t nx, int64_t first, int64_t n, void* stream);
int lldwt_ycc420_tiles_to_u8hwc(const float* luma, const float* chroma, const int32_t* tiles, int64_t first, int64_t n, int64_t B,
                                int64_t H, int64_t W, int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0, int64_t x0,
                                int64_t h, int64_t w, const float* inv_a, const float* b, uint8_t* dst, void* stream);
int lldwt_u8hw_to_y_tiles(const uint8_t* src, float* y, int64_t B, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t ny,
                          int64_t nx, int64_t first, int64_t n, void* stream);
int lldwt_y_tiles_to_u8hw(const float* y, const int32_t* tiles, int64_t first, int64_t n, int64_t B, int64_t H, int64_t W,
                          int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0, int64_t x0, int64_t h, int64_t w,
                          const float* inv_a, const float* b, uint8_t* dst, void* stream);
/* Samples of 9 to 16 bits (codec.py depth=; csrc/depth.hip): the uint16 siblings of the tile entry points
 * above, with their tile grid, tile list or first / n, region, limits and refusals.  src and dst hold uint16_t samples (passed as
 * void*; 2-byte aligned, HWC) and depth is 8 .. 16 with M = 2^depth - 1 as an fp32 constant.  Input: v / M, a true fp32 division,
 * then exactly the expressions of the uint8 entry point (greyscale: v / M - 0.5f).  Output: the expressions of the uint8 entry
 * point with floorf((c + 0.5f) * M + 0.5f) stored as uint16_t.  So depth 8 gives the floats and values of the uint8 entry
 * points bit for bit.  flag: a 4-byte aligned device int32 the caller zeroes; an input kernel that meets a sample above M stores
 * 1 there (the floats written are then meaningless) and never writes it otherwise.  inv_a, b: host floats (3 each; 1 each for
 * y_tiles) or both NULL, as lldwt_ll_tiles_to_u8hwc / lldwt_ycc420_tiles_to_u8hwc: one output entry point serves the full and
 * the reduced decode.  lldwt_u16hwc_to_f32chw: lldwt_u8hwc_to_f32chw on uint16, v / M.                                         */
int lldwt_u16hwc_to_ycc_tiles(const void* src, float* ycc, int64_t B, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t ny,
                              int64_t nx, int64_t first, int64_t n, int depth, int32_t* flag, void* stream);
int lldwt_ycc_tiles_to_u16hwc(const float* ycc, const int32_t* tiles, int64_t first, int64_t n, int64_t B, int64_t H, int64_t W,
                              int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0, int64_t x0, int64_t h, int64_t w,
                              const float* inv_a, const float* b, int depth, void* dst, void* stream);
int lldwt_u16hwc_to_ycc420_tiles(const void* src, float* luma, float* chroma, int64_t B, int64_t H, int64_t W, int64_t th,
                                 int64_t tw, int64_t ny, int64_t nx, int64_t first, int64_t n, int depth, int32_t* flag,
                                 void* stream);
int lldwt_ycc420_tiles_to_u16hwc(const float* luma, const float* chroma, const int32_t* tiles, int64_t first, int64_t n, int64_t B,
                                 int64_t H, int64_t W, int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0, int64_t x0,
                                 int64_t h, int64_t w, const float* inv_a, const float* b, int depth, void* dst, void* stream);
int lldwt_u16hw_to_y_tiles(const void* src, float* y, int64_t B, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t ny,
                           int64_t nx, int64_t first, int64_t n, int depth, int32_t* flag, void* stream);
int lldwt_y_tiles_to_u16hw(const float* y, const int32_t* tiles, int64_t first, int64_t n, int64_t B, int64_t H, int64_t W,
                           int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0, int64_t x0, int64_t h, int64_t w,
                           const float* inv_a, const float* b, int depth, void* dst, void* stream);
int lldwt_u16hwc_to_f32chw(const void* src, float* dst, int64_t B, int64_t H, int64_t W, int depth, int32_t* flag, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * P/U block parameters (graphs/layers/P_block_v2.py:15-33) packed for the kernels.
 * lldwt_pack_pblock: in = the four conv weights/biases of `planes` stacked blocks in PyTorch layout
 *   w1 (planes,C,1,K,K)  w2,w3 (planes,C,C,K,K)  w4 (planes,1,C,K,K), b1,b2,b3 (planes,C), b4 (planes,1);
 *   out = packed buffer of lldwt_pblock_packed_floats(C,K) floats PER PLANE holding both orientations
 *   (vertical pass uses W, horizontal pass uses W transposed in (kh,kw): conv(x^T,W)^T == conv(x,W^T), which
 *   removes every torch.transpose of wavelet_forward_v2.py:32,38-39,43,50-51).                           */
int64_t lldwt_pblock_packed_floats(int C, int K);
/* Arithmetic of the eval-path lifting step for C = 16, K = 5 (the reference's configuration): 1 (default) = ONE fused
 * launch per step with the 16 -> 16 convolutions on the fp16 matrix cores, split-fp16 operands, intermediates in LDS
 * (csrc/lifting_f16.hip); 0 = the three fp32-MFMA launches (exact fp32 products; also what training uses).       */
int lldwt_set_lift_mode(int mode);
/* Arithmetic of the split-fp16 kernel families on the EVAL path (fused lifting step, tree-context pair, cgp chain):
 *   0 (default) = f16x3: every fp32 MAC is three fp16 MFMA products (hi hi + hi lo + lo hi), fp32 accumulate: fp32-level
 *                 accuracy; every parity bar against the fp32 reference is stated for this mode;
 *   1 = fp16, 2 = bf16: ONE MFMA product per MAC on operands rounded to fp16 / bf16 (fp32 accumulate, fp32 tensors in HBM,
 *                 biases / activations / rate arithmetic in fp32).  BASELINE configs[4] ("fp16") and configs[1] ("bf16");
 *                 their own tolerance class (<= 1e-2 relative on coefficients and summed bits), never the headline.
 * The reference itself is fp32-only (graphs/layers/wavelet_inverse_v2.py:49-51).  Training always runs f16x3 / fp32.   */
int lldwt_set_precision(int prec);
int lldwt_get_precision(void);
/* Diagnostics hook of the three split-fp16 kernel families (tools/lift_stamps.py, plc_stamps.py, cgp_stamps.py; the
 * product never calls it).  kind 0 = fused lifting step, 1 = tree-pair conv, 2 = cgp chain.  stamps / nbytes: a device
 * buffer the kernels of that kind write s_memtime stamps into (null = off); a launch whose stamps would not fit in
 * nbytes ignores the buffer.  flags, kind 0: debug mask -- bit 0..3 skip a phase (results are then wrong),
 * 16 = sequential conv3 / conv4 for every tile (the check of the composed 9x9 kernel), 32 = no vertical reuse
 * between the tiles of a column, 64 = the border tiles' strip correction in its earlier form (every k-step of the strip
 * convolutions, half a wave per corrected pixel): same output bits, kept for A/B timing and as a test reference;
 * 128 = the tile as it was before the correction sums left the critical path: the sums behind a barrier that follows the
 * composite loop (flag 64 implies this order too), and every MFMA tile of conv1 / conv2 computed at the top and bottom of the
 * image although all its pixels lie outside it: same output bits, a test reference;
 * 256 = the eval kernels that request conv2's weight fragments at the head of P2 instead of between the pieces of P1 (the
 * skip bit 0 is honoured by this form only): same fragments, same MFMA sequence and same output bits, the A/B leg of
 * tools/lift_stamps.py and a test reference; 512 = with a registered buffer, the f16x3 eval kernels that also stamp inside P2 (tools/lift_stamps.py --p2).
 * A buffer of kind 0 holds 32 stamps per wave and tile.
 * flags, kind 1: bit 0 = the Winograd pair kernel (k_plc_wino) in its earlier form -- the epilogue that loads each bias value
 * between the stores and waits for them, the first conv's ACT and STORE stages whole inside one unit of the chunk loop, eight
 * vector instructions offered per MFMA gap: same output bits, kept for A/B timing (tools/plc_stamps.py) and as a test reference.
 * flags, kind 2 (lldwt_cgp16_params only): bits 0-1 = bound-only variant of the streaming
 * chain, timing only (1 = every step reads step 0's weight fragments, 2 = constant inputs; results are then wrong),
 * bits 2-3 = force a form whatever the size (1 << 2 = streaming, 2 << 2 = persistent; 0 = the dispatch's choice, which
 * LLDWT_CGP16=stream, read when the library loads, pins to streaming).
 * The caller keeps the buffer alive until it unregisters it.                                                       */
int lldwt_set_diagnostics(int kind, void* stamps, int64_t nbytes, int flags);
int lldwt_get_lift_mode(void);
/* 1 when the TRAINING forward of the lifting steps (lldwt_lifting_forward_train / _inverse_train, C = 16, K = 5, tanh blocks)
 * runs on the fused f16x3 kernel's sequential path, which writes (src, skip, t1, t2, t3) for the backward: lift mode 1 and the
 * environment variable LLDWT_TRAIN_LIFT != "f32".  The packed blocks must then come from lldwt_pack_pblock (with the split-fp16
 * section), not lldwt_pack_pblock_train. */
int lldwt_train_lift_f16(void);
int lldwt_pack_pblock(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                      const float* b3, const float* w4, const float* b4, float* packed, int planes, int C, int K,
                      void* stream);
/* The same buffer WITHOUT its split-fp16 section (left unwritten): for the training step, which re-packs the changed
 * weights every iteration and only runs the fp32 kernels that save their intermediates.  A buffer packed this way must
 * not be handed to the eval path (lldwt_lift_step with lift mode 1 reads the split-fp16 section).                     */
int lldwt_pack_pblock_train(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                            const float* b3, const float* w4, const float* b4, float* packed, int planes, int C, int K,
                            void* stream);
/* As lldwt_pack_pblock without the composed 9x9 kernels of the eval path (left zero): the pack of the fused kernel's sequential
 * path -- the training forward (lldwt_lifting_forward_train / _inverse_train), rebuilt at every weight update.  NOT for the eval
 * entry points.                                                                                                              */
int lldwt_pack_pblock_seq(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                          const float* b3, const float* w4, const float* b4, float* packed, int planes, int C, int K,
                          void* stream);

/* One lifting step (wavelet_forward_v2.py:60-62 and the three like it; inverse wavelet_inverse_v2.py:76-90):
 *     skip = conv3x1(src, taps)            zero padded, along rows if vertical else along columns
 *     net  = P_block(skip)                 conv1 -> tanh -> conv2 -> tanh -> conv3 (+conv1 pre-act) -> conv4
 *     dst_out = dst_in + sign * (skip + res_weight * net)
 * src/dst_in/dst_out are (Z,h,w) views; dst_out may alias dst_in.  taps: (planes,3) device floats
 * (preProcessingList.{j}.weight, lifting_dwt_nets.py:785-819).  packed: lldwt_pack_pblock output.
 * linear != 0 drops the tanh (linearity_flag != 1, P_block_v2.py:42-49).
 * ws: >= lldwt_lift_step_ws_bytes(Z,h,w,C) bytes.                                                        */
int64_t lldwt_lift_step_ws_bytes(int64_t Z, int64_t h, int64_t w, int C);
int lldwt_lift_step(lldwt_view src, lldwt_view dst_in, lldwt_view dst_out, int64_t Z, int64_t batch, int64_t h,
                    int64_t w, const float* taps, const float* packed, int C, int K, int vertical, float sign,
                    float res_weight, int linear, void* ws, int64_t ws_bytes, void* stream);

/* Whole multi-level transform of LiftingBasedNeuralWaveletv4.encode (lifting_dwt_nets.py:728-732), all planes
 * and images in one call.  x: (Z,1,H,W) plane-major; ll: (Z,1,H>>L,W>>L); yh[i]: (Z,3,H>>(i+1),W>>(i+1)) with
 * channels (LH,HL,HH), finest first (the layout of out_xo_list before the subband auto-encoder, :739-740).
 * taps: (4,planes,3) = preProcessingList.{j}.weight of every plane, j-major.
 * packed: (planes, nblocks, 2 (P,U), packed_floats); nblocks = 2 for block_property=="same", 2*2*levels for
 * "different" (lifting_dwt_nets.py:688-722).  Level `lev` of the forward uses block pairs
 * block_offset + (different ? 2*lev : 0) + {0,1}; EVERY level of the inverse uses block_offset + {0,1}
 * (lifting_dwt_nets.py:718-722 slices the inverse blocks from waveletLevel*liftingLevel for every level, so the
 * caller passes block_offset = 2*levels there when block_property=="different").
 * scale_nh/scale_nl: device (planes) floats = lifting_coeff[4/5] + n*0.1 when config.scale==1, else NULL.  */
int64_t lldwt_lifting_ws_bytes(int64_t Z, int64_t H, int64_t W, int C);
int lldwt_lifting_forward(const float* x, float* ll, float* const* yh, int64_t planes, int64_t batch, int64_t H,
                          int64_t W, int levels, const float* taps, const float* packed, int nblocks,
                          int block_offset, int different, int C, int K, float res_weight, int linear,
                          const float* scale_nh, const float* scale_nl, void* ws, int64_t ws_bytes, void* stream);
/* lldwt_lifting_forward forked at a level: the ops of the levels < split_level (lldwt_lift_op.level) are enqueued on `stream`,
 * then `fork_event` (a hipEvent_t of the caller's, as void*; the library creates none) is recorded there, `tail_stream` waits
 * for it, and the ops of the levels >= split_level -- their gain ops and the final ll included -- are enqueued on `tail_stream`.
 * Plain stream and event calls only; no kernel waits for another.  The results have the bits of the unsplit call.
 *   ordered on `stream`:      yh[0 .. split_level-1]
 *   ordered on `tail_stream`: yh[split_level .. levels-1] and ll
 *   `ws` (the LL ping-pong of the levels below the fork, the row / column temporaries, the step workspace) is read and
 *   written by the tail stream's launches: it must not be handed to any other work, on either stream, until the tail
 *   stream's work of this call is done (the caller joins: an event recorded on `tail_stream` that `stream` waits for).
 *   x is read on `stream` only when split_level >= 1.
 * split_level <= 0 or >= levels: the unsplit call on `stream` (tail_stream and fork_event are not touched).
 * lldwt_lift_split_level: where the eval step of the tree-pair layers forks the transform (csrc/lift_split.h, the one rule):
 *   0 = do not fork, else the split_level.  Z = planes*batch; cus = compute units, <= 0: those of the current device. */
int lldwt_lifting_forward_split(const float* x, float* ll, float* const* yh, int64_t planes, int64_t batch, int64_t H,
                                int64_t W, int levels, const float* taps, const float* packed, int nblocks,
                                int block_offset, int different, int C, int K, float res_weight, int linear,
                                const float* scale_nh, const float* scale_nl, void* ws, int64_t ws_bytes,
                                int split_level, void* stream, void* tail_stream, void* fork_event);
int lldwt_lift_split_level(int64_t Z, int64_t H, int64_t W, int levels, int cus);
/* Inverse (LiftingBasedNeuralWaveletv4.decode, lifting_dwt_nets.py:762-781; wavelet_inverse_v2.py:20-92).  */
int lldwt_lifting_inverse(const float* ll, const float* const* yh, float* x, int64_t planes, int64_t batch,
                          int64_t H, int64_t W, int levels, const float* taps, const float* packed, int nblocks,
                          int block_offset, int C, int K, float res_weight, int linear, const float* scale_nh,
                          const float* scale_nl, void* ws, int64_t ws_bytes, void* stream);

/* Training support of the lifting transform.  The transform is a PROGRAM of lifting steps over symbolic buffers
 * (0 = x, 1 = Lrow, 2 = Hrow, 3 = tmpL, 4 = tmpH, 5/6 = LL ping-pong, 7 = ll, 8+i = yh[i]); views are
 * (buffer, element offset, z/row/col strides).  kind 0 = lifting step, 1..4 = per-plane scale (config.scale == 1).
 * lldwt_lifting_program fills `ops` (pass NULL/0 to count) and reports the floats of the per-step `saved`
 * intermediates [src | skip | t1 | t2 | t3] kept by the *_train variants; the backward pass walks the program in
 * reverse over gradient buffers of identical layout (see autograd.py: G[dst_in] = G[dst_out];
 * G[src] += J^T G[dst_out]; dW/dtaps accumulate).                                                          */
typedef struct lldwt_lift_op {
    int32_t kind, buf_src, buf_din, buf_dout;
    int64_t off_src, sz_src, sy_src, sx_src;
    int64_t off_din, sz_din, sy_din, sx_din;
    int64_t off_dout, sz_dout, sy_dout, sx_dout;
    int32_t h, w, vertical, tap, block, is_u;
    float sign;
    int32_t level;      /* the transform level whose buffers the op writes (0 = finest) */
    int64_t saved_off;
} lldwt_lift_op;
int lldwt_lifting_program(lldwt_lift_op* ops, int max_ops, int64_t Z, int64_t H, int64_t W, int levels, int different,
                          int block_offset, int inverse, int scale, int C, int64_t* saved_floats);
/* The *_train variants: lldwt_lifting_forward / _inverse with every step's intermediates kept in `saved`.  scale_nh / scale_nl:
 * the per-plane gains of config.scale == 1 (wavelet_forward_v2.py:76-80, wavelet_inverse_v2.py:70-74; both null = no scaling).
 * Build the program with scale = 1 then: every scale op (kind 1..4) owns h*w*Z floats of `saved` at its saved_off and keeps
 * its INPUT there (dense Z,h,w), which the host-side backward needs for d(gain). */
int lldwt_lifting_forward_train(const float* x, float* ll, float* const* yh, int64_t planes, int64_t batch, int64_t H,
                                int64_t W, int levels, const float* taps, const float* packed, int nblocks,
                                int block_offset, int different, int C, int K, float res_weight, int linear,
                                const float* scale_nh, const float* scale_nl, void* ws, int64_t ws_bytes, float* saved,
                                void* stream);
int lldwt_lifting_inverse_train(const float* ll, const float* const* yh, float* x, int64_t planes, int64_t batch,
                                int64_t H, int64_t W, int levels, const float* taps, const float* packed, int nblocks,
                                int block_offset, int C, int K, float res_weight, int linear, const float* scale_nh,
                                const float* scale_nl, void* ws, int64_t ws_bytes, float* saved, void* stream);
/* backward pieces of one step (chained by the host with lldwt_conv2d / lldwt_conv2d_wgrad):
 *   pre: g (dense Z,h,w) = G[dst_out];  G[dst_in] = g
 *   fin: dskip = sign*(g + res_weight*dsk);  G[src] += taps^T (x) dskip;  dtaps (planes,3) += sum dskip * src shifted */
int lldwt_lift_bwd_pre(lldwt_view g_dst_out, lldwt_view g_dst_in, float* g, int64_t Z, int64_t h, int64_t w, void* stream);
int lldwt_lift_bwd_fin(const float* g, const float* dsk, const float* srcv, lldwt_view g_src, int64_t Z, int64_t batch,
                       int64_t h, int64_t w, const float* taps, float* dtaps, int vertical, float sign, float res_weight,
                       void* stream);

/* Whole backward of one lifting step with C == 16 (replaces autograd through wavelet_forward_v2.py:60-74 /
 * wavelet_inverse_v2.py:76-90 + P_block_v2.py:40-55): fused backward-data kernels on the matrix cores, the four
 * weight gradients (accumulated, scaled by sign*res_weight, row passes in (kw,kh) order like the weights' use), the
 * skip-filter transpose and its tap gradients.  saved_step: this step's slice of the forward `saved` buffer
 * [src | skip | t1 | t2 | t3]; packed/packed_plane_stride: the FORWARD pack of this step's P/U block
 * (lldwt_pack_pblock); dw1..db4: (planes, ...) gradients of that block, accumulated; taps/dtaps: (planes,3) of this
 * step's skip filter.  ws: lldwt_lift_step_bwd_ws_bytes. */
int64_t lldwt_lift_step_bwd_ws_bytes(int64_t Z, int64_t h, int64_t w, int C);
int lldwt_lift_step_bwd(lldwt_view g_dst_out, lldwt_view g_dst_in, lldwt_view g_src, const float* saved_step,
                        int64_t planes, int64_t batch, int64_t h, int64_t w, const float* taps, float* dtaps,
                        const float* packed, int64_t packed_plane_stride, float* dw1, float* db1, float* dw2, float* db2,
                        float* dw3, float* db3, float* dw4, float* db4, int C, int K, float res_weight, float sign,
                        int vertical, int linear, void* ws, int64_t ws_bytes, void* stream);

/* The same with the backward-data chain (dt3 = conv4^T g, dpre2 = tanh'(t2) conv3^T dt3, dr = tanh'(t1) conv2^T dpre2 + dt3,
 * dsk = conv1^T dr) as ONE launch of the fused split-fp16 lifting kernel in its backward mode (C == 16, K == 5, tanh block;
 * anything else, LLDWT_BWD_LIFT=f32 or lift mode f32 takes the launches of lldwt_lift_step_bwd).  packed_bwd: the "backward
 * pack" of the block from lldwt_pack_pblock_bwd -- transposed, mirrored weights in the forward pack's layout, same plane stride;
 * taps_id: (planes, 3) floats (0, 1, 0).  lldwt_bwd_lift_f16(): 1 when the fused backward is what this entry runs. */
int lldwt_bwd_lift_f16(void);
int64_t lldwt_pack_pblock_bwd_ws_bytes(int planes);
int lldwt_pack_pblock_bwd(const float* w1, const float* w2, const float* w3, const float* w4, float* packed, void* ws,
                          int64_t ws_bytes, int planes, int C, int K, void* stream);
int lldwt_lift_step_bwd_f16(lldwt_view g_dst_out, lldwt_view g_dst_in, lldwt_view g_src, const float* saved_step,
                            int64_t planes, int64_t batch, int64_t h, int64_t w, const float* taps, float* dtaps,
                            const float* packed, int64_t packed_plane_stride, float* dw1, float* db1, float* dw2, float* db2,
                            float* dw3, float* db3, float* dw4, float* db4, int C, int K, float res_weight, float sign,
                            int vertical, int linear, void* ws, int64_t ws_bytes, const float* packed_bwd,
                            const float* taps_id, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * SubbandAutoEncoder (lifting_dwt_nets.py:99-110): per-coefficient scalar MLP 1 -> Hd -> Hd -> Hd -> 1, tanh
 * between, grouped 1x1 convs (groups == channels).  x,y: (Z,C,h,w).  Parameters per plane, PyTorch layouts:
 *   encode: w0 (C*Hd,1) b0 (C*Hd)  w1,w2 (C*Hd,Hd) b1,b2 (C*Hd)  w3 (C,Hd) b3 (C)         [Conv2d]
 *   decode: ConvTranspose2d weights (in, out/groups): w0 (C,Hd) w1,w2 (C*Hd,Hd) w3 (C*Hd,1); transposed != 0.
 * The forward reads the parameters from a pack that lldwt_subband_mlp_pack builds from either orientation (once per weight
 * update; lldwt_subband_mlp_packed_bytes sizes it, 16-byte aligned): per (plane, channel) the two Hd x Hd layers as split-fp16
 * MFMA fragments (hi, lo) in the kernel's lane order, each layer multiplied by s = 2^k with max|W| * s in [2^14, 2^15), then
 * w0, b0, b1, b2, w3 in the lane's channel order, then s_1, s_2, 1/(s_1 2^14), 1/(s_2 2^14), b3 (csrc/subband_mlp_f16.hip
 * states the layout word by word).  k is clamped to [-113, 112]: every finite max|W| >= 2^-97 gets its exact scale, a smaller
 * layer (all-zero included: s = 1) keeps an absolute error below 2^-118 per weight, and a non-finite weight gives a finite
 * scale and non-finite outputs, as it does in fp32.  The hidden layers run as hi*hi + hi*lo + lo*hi on the fp16 matrix cores
 * with fp32 accumulation whatever lldwt_set_precision says; layers 0 and 3 are fp32. */
int64_t lldwt_subband_mlp_packed_bytes(int64_t planes, int C);
int lldwt_subband_mlp_pack(const float* w0, const float* b0, const float* w1, const float* b1, const float* w2,
                           const float* b2, const float* w3, const float* b3, int64_t planes, int C, int Hd, int transposed,
                           void* pack, int64_t pack_bytes, void* stream);
int lldwt_subband_mlp(const float* x, float* y, int64_t planes, int64_t batch, int C, int64_t hw, int Hd, const void* pack,
                      int64_t pack_bytes, void* stream);
/* Backward of the encode-layout MLP (training; replaces autograd through lifting_dwt_nets.py:99-104 / :105-110 once the
 * decoder's ConvTranspose2d weights are viewed in Conv2d layout): recomputes the forward, returns gx (Z,C,hw) and, for
 * the four weight-gradient GEMMs (lldwt_conv2d_wgrad, groups == C), the activations h0,h1,h2 and the pre-activation
 * gradients d0,d1,d2, all (Z, C*Hd, hw). */
int lldwt_subband_mlp_bwd(const float* x, const float* gy, float* gx, float* h0, float* h1, float* h2, float* d0, float* d1,
                          float* d2, int64_t planes, int64_t batch, int C, int64_t hw, int Hd, const float* w0,
                          const float* b0, const float* w1, const float* b1, const float* w2, const float* b2,
                          const float* w3, void* stream);
/* The same backward with the eight parameter gradients formed inside the kernel (training default): only x, gy and gx touch HBM.
 * dw0, db0, db1, db2, dw3: (planes, C*Hd); dw1, dw2: (planes, C*Hd, Hd); db3: (planes, C) -- WRITTEN (not accumulated; fixed
 * summation order: the result does not depend on scheduling).  ws: lldwt_subband_mlp_bwd_w_ws_bytes (per-wave partial sums). */
int64_t lldwt_subband_mlp_bwd_w_ws_bytes(int64_t planes, int C, int64_t hw);
int lldwt_subband_mlp_bwd_w(const float* x, const float* gy, float* gx, int64_t planes, int64_t batch, int C, int64_t hw, int Hd,
                            const float* w0, const float* b0, const float* w1, const float* b1, const float* w2,
                            const float* b2, const float* w3, float* dw0, float* db0, float* dw1, float* db1, float* dw2,
                            float* db2, float* dw3, float* db3, void* ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * General conv layer for the context models and the Berk auto-encoder
 * (LiftingBasedDWT_net.py:271-289,299-317,793-795; lifting_dwt_nets.py:139-150; masked_conv2d.py:19-21).
 *   y[z, oc', :, :] = act( bias[oc] + sum_{ic,ky,kx} w[oc, ic, ky, kx] * x[z, g*cin_g + ic, .+ky-K/2, .+kx-K/2] )
 * zero padded, stride 1.  x: (Z,cin,h,w) (if upsample2: (Z,cin,h/2,w/2), read through the nearest-neighbour 2x
 * upsampling of LiftingBasedDWT_net.py:348,367,822,835).  w: (planes,cout,cin/groups,K,K) (if transposed:
 * ConvTranspose2d layout (planes,cin,cout/groups,K,K), any groups), bias (planes,cout) or NULL.
 * tap_mask: bit (ky*K+kx) set = tap is live (MaskedConv2d type A/B; the caller has already applied
 * weight *= mask as the reference does); pass (1<<K*K)-1 for a dense conv.
 * Output channel placement (removes the chunk/cat regrouping of LiftingBasedDWT_net.py:357-359):
 *   oc' = (oc / oc_block) * oc_stride + oc_off + oc % oc_block   in a tensor of ytot channels;
 *   dense placement is oc_block = cout, oc_stride = 0, oc_off = 0, ytot = cout.                           */
typedef struct lldwt_conv_desc {
    int cin, cout, K, groups;
    int act;          /* LLDWT_ACT_* */
    int upsample2;
    int transposed;
    uint32_t tap_mask;
    int oc_block, oc_stride, oc_off, ytot;
    /* input channel placement (mirror of the output placement; used by the backward-data pass, whose input is the
     * gradient of a tensor written with oc_* placement): channel c is read at (c / ic_block)*ic_stride + ic_off +
     * c % ic_block of a tensor with xtot channels; ic_block == 0 means dense (xtot = cin).                    */
    int ic_block, ic_stride, ic_off, xtot;
    /* gradient epilogue: LLDWT_EPI_NONE, or multiply the result by act'(aux) with aux = the forward OUTPUT of the
     * layer whose pre-activation gradient is being formed (tanh: 1-aux^2, LeakyReLU: aux>0 ? 1 : 0.01).       */
    int epi;
} lldwt_conv_desc;
#define LLDWT_EPI_NONE 0
#define LLDWT_EPI_TANH_BWD 1
#define LLDWT_EPI_LRELU_BWD 2
/* Weights are pre-packed once per update into the MFMA A-operand lane order (csrc/conv_mfma.hip):
 * packed holds lldwt_conv_packed_floats(d) floats PER PLANE.  residual (optional): tensor laid out like y, added before
 * the activation (P_block_v2.py:53 "tmp + out_res").  swap_hw != 0 packs the (kh,kw)-transposed kernel W^T (the
 * horizontal lifting pass: conv(x^T, W)^T == conv(x, W^T), replaces the torch.transpose calls of
 * wavelet_forward_v2.py:32-51).                                                                             */
int64_t lldwt_conv_packed_floats(const lldwt_conv_desc* d);
int lldwt_conv_pack(const float* w, float* packed, const lldwt_conv_desc* d, int64_t planes, int swap_hw, void* stream);
/* y = act( (conv(x) + bias) * epi(aux) + residual ).  transposed != 0 builds the operator from a weight in
 * ConvTranspose2d layout (planes, cin, cout/groups, K, K) with the taps flipped: that is ConvTranspose2d (stride 1)
 * itself and, applied to a forward Conv2d weight with cin/cout swapped, the BACKWARD-DATA pass of that conv.      */
int lldwt_conv2d(const float* x, float* y, const float* packed, const float* bias, const float* residual,
                 const float* aux, const lldwt_conv_desc* d, int64_t planes, int64_t batch, int64_t h, int64_t w_,
                 void* stream);
/* Two independent stacks of grouped convs with the same per-group layer shapes, run as one grouped problem per layer (nlayers
 * launches instead of 2 * nlayers): stack A's groups_a groups first, then stack B's.  descs[i] / packed[i] / bias[i] describe
 * layer i of the MERGED problem (groups = groups_a + groups_b; packed and bias are stack A's per-plane block followed by stack
 * B's; descs[i].act is applied as given).  xa (planes,batch,groups_a*cin_g,h,w) and xb (planes,batch,groups_b*cin_g,h,w) are
 * the two inputs, ya / yb the two outputs of the last layer in the same manner; ws0 (ws0_floats) receives the even layers'
 * outputs and ws1 (ws1_floats) the odd ones': each >= planes*batch*h*w * the widest layer it receives (the last layer writes ya / yb).  Every output is bit-identical to the one lldwt_conv2d
 * gives for its stack alone.  Plain placement only (no upsample2 / transposed / ic_block / oc placement / epi).               */
int lldwt_conv_stack_pair(const float* xa, const float* xb, float* ya, float* yb, const float* const* packed,
                          const float* const* bias, const lldwt_conv_desc* descs, int nlayers, int groups_a, float* ws0,
                          float* ws1, int64_t ws0_floats, int64_t ws1_floats, int64_t planes, int64_t batch, int64_t h, int64_t w_, void* stream);
/* As lldwt_conv2d; additionally absmax_slots (planes,64), if not null, receives max |y| of each plane spread over 64
 * slots (the consumer takes their maximum): the activation scale of a following lldwt_conv3x3_f16x3, produced in the
 * epilogue instead of by a separate pass over y.                                                                  */
int lldwt_conv2d_absmax(const float* x, float* y, const float* packed, const float* bias, const float* residual,
                        const float* aux, float* absmax_slots, const lldwt_conv_desc* d, int64_t planes, int64_t batch,
                        int64_t h, int64_t w_, void* stream);
/* Backward-weights: dw (planes,cout,cin/groups,K,K) += alpha * sum over batch and pixels of dy[.,oc,p] * x[.,ic,p+tap]
 * (dead taps of tap_mask are skipped), dbias (planes,cout) += alpha * sum dy (optional).  dy is read through the OUTPUT
 * placement (oc_*), x through upsample2 / the input placement.  Accumulates with float atomics: zero dw/dbias first.
 * swap_hw != 0: the conv was applied with the (kh,kw)-transposed kernel, so tap (ky,kx) of the contraction is
 * accumulated into dw[..][kx][ky].                                                                         */
int lldwt_conv2d_wgrad(const float* x, const float* dy, float* dw, float* dbias, const lldwt_conv_desc* d,
                       int64_t planes, int64_t batch, int64_t h, int64_t w_, float alpha, int swap_hw, void* stream);
/* Backward-weights of a DENSE 3x3 conv (groups 1, no placement, no upsampling, no dead taps) on the fp16 matrix cores with
 * split-fp16 operands (fp32-level accuracy; csrc/conv_wgrad_f16x3.hip): dw (planes,cout,cin,3,3) += alpha * sum over batch
 * and pixels of dy[.,oc,p] * x[.,ic,p+tap], dbias (planes,cout) += alpha * sum dy (optional).  x (planes,batch,cin,h,w),
 * dy (planes,batch,cout,h,w), both 16-byte aligned, w % 4 == 0.  slots_ws: planes * 128 floats of scratch (the per-plane
 * max |x| and max |dy| the power-of-two operand scales come from).  Float atomics: zero dw / dbias first.  The training
 * path of the 243 -> 243 tree-context conv (LiftingBasedDWT_net.py:271-272); lldwt_conv2d_wgrad covers every other shape.
 * x_slots / dy_slots (planes,64), if not null, are the per-plane |max| slots of x / dy the caller holds already
 * (lldwt_absmax_slots, lldwt_conv2d_absmax): the pass over that tensor is skipped -- in a training step the forward conv has
 * measured x and the backward-data conv dy (autograd of LiftingBasedDWT_net.py:271-272).  slots_ws may be null when both are
 * given. */
int lldwt_conv3x3_wgrad_f16x3(const float* x, const float* dy, float* dw, float* dbias, float* slots_ws,
                              const float* x_slots, const float* dy_slots, int cin, int cout, int64_t planes, int64_t batch,
                              int64_t h, int64_t w_, float alpha, void* stream);
/* Backward-weights of the 16 -> 16 5x5 convs of a P/U block (conv2 / conv3 of graphs/layers/P_block_v2.py:40-55; autograd of
 * agents/liftingDWT_agent.py:97) on the fp16 matrix cores, split-fp16 operands (fp32-level accuracy):
 *   dw[p][oc][ic][ty][tx] += alpha * sum_{b,y,x} dy[p][b][oc][y][x] * x[p][b][ic][y+ty-2][x+tx-2],  dbias += alpha * sum dy.
 * x (planes, batch, 16, h, w) must be bounded by 1 in magnitude (the tanh outputs t1 / t2: its split uses the fixed scale
 * 2^14); dy any magnitude (one power-of-two scale per plane from its |max|).  w % 4 == 0, 16-byte aligned tensors.
 * slots_ws: planes * 64 floats of scratch.  swap_hw != 0: the (kh, kw) axes of dw are stored swapped (row passes).
 * lldwt_lift_step_bwd uses it for K == 5 tanh blocks from LLDWT_WGRAD16_MIN pixels per plane up (below: the fp32-MFMA kernel). */
int lldwt_wgrad16_f16x3(const float* x, const float* dy, float* dw, float* dbias, float* slots_ws, int64_t planes,
                        int64_t batch, int64_t h, int64_t w, float alpha, int swap_hw, void* stream);
/* dx = dy * act'(y) elementwise (y = forward output); act as in lldwt_conv_desc. */
int lldwt_act_bwd(const float* dy, const float* y, float* dx, int64_t n, int act, void* stream);
/* backward of the nearest-neighbour 2x upsampling: out (Z,C,h/2,w/2) = sum over each 2x2 block of g (Z,C,h,w). */
int lldwt_downsum2(const float* g, float* out, int64_t zc, int64_t h, int64_t w_, void* stream);
/* Dense 3x3 conv (groups 1, no placement, no upsampling) on the fp16 matrix cores with fp32-level accuracy
 * ("f16x3", csrc/conv_f16x3.hip): every fp32 operand is scaled by a power of two and split into hi + lo fp16 values
 * (|v - hi - lo| <= 2^-22 |v|), the product is hi*hi + hi*lo + lo*hi accumulated in fp32.  For the tree-context conv
 * 243 -> 243 (LiftingBasedDWT_net.py:271-272, :793-795).  The fp32 engine above stays the reference arithmetic.
 *   lldwt_conv_f16x3_pack : w (planes,cout,cin,3,3) -> packed (lldwt_conv_f16x3_packed_bytes(cin,cout) bytes per plane)
 *   lldwt_absmax_slots    : slots (planes,64) <- max |x| of each plane's n_per_plane values (the activation scale is
 *                           derived from it on the device; no host synchronisation)
 *   lldwt_conv3x3_f16x3   : y (planes,batch,cout,h,w) = act(conv3x3(x (planes,batch,cin,h,w)) + bias (planes,cout)) */
int64_t lldwt_conv_f16x3_packed_bytes(int cin, int cout);
int lldwt_conv_f16x3_pack(const float* w, void* packed, int cin, int cout, int64_t planes, void* stream);
int lldwt_absmax_slots(const float* x, int64_t planes, int64_t n_per_plane, float* slots, void* stream);
int lldwt_conv3x3_f16x3(const float* x, float* y, const void* packed, const float* bias, const float* slots, int cin,
                        int cout, int act, int64_t planes, int64_t batch, int64_t h, int64_t w_, void* stream);

/* Reduced-precision STORAGE of the tree-context tensor (BASELINE.json configs[4] "fp16"): the first tree
 * conv writes its output as fp16 (half the HBM bytes), multiplied by a power of two oscale[plane] chosen by the caller from
 * a bound (max |parent| x max row L1 norm + max |bias|) so that it cannot overflow; the second conv consumes it as the hi
 * half with no lo (two MFMA products instead of three): 2^-11 relative on the activations, fp32 accumulate.  Its own
 * tolerance (1e-2) and bench config; never the headline.
 *   lldwt_conv2d_f16out : lldwt_conv2d with y16 (planes,batch,ytot,h,w) fp16 = act(conv(x) + bias) * oscale[plane]
 *   lldwt_conv3x3_f16in : lldwt_conv3x3_f16x3 reading such a tensor (xscale = the oscale it was written with)        */
int lldwt_conv2d_f16out(const float* x, void* y16, const float* packed, const float* bias, const float* oscale,
                        const lldwt_conv_desc* d, int64_t planes, int64_t batch, int64_t h, int64_t w_, void* stream);
int lldwt_conv3x3_f16in(const void* x16, float* y, const void* packed, const float* bias, const float* xscale, int cin,
                        int cout, int act, int64_t planes, int64_t batch, int64_t h, int64_t w_, void* stream);

/* The tree-context PAIR in ONE launch (LiftingBasedDWT_net.py:271-272 / :793-795):
 *   y = act(conv3x3_{cmid->cout}(LeakyReLU(conv3x3_{3->cmid}(up2(parent)) + b1)) + b2)
 * parent (planes,batch,3,h/2,w/2) fp32, y (planes,batch,cout,h,w) fp32.  The first conv is evaluated on the fly by the
 * matrix cores for each workgroup's 10x34 halo patch (K = 27, split-fp16 like the second) and written straight into the
 * LDS image the second conv consumes: the cmid-channel tensor never exists in HBM.  Scales are per workgroup: the parent
 * patch by its own |max|, the intermediate by the bound max|patch| * max row L1 norm(w1) + max|b1| (a power of two either
 * way, so the choice does not change the result beyond the 2^-21 split error).
 *   packed1 = lldwt_plc_fused_pack1(w1 (planes,cmid,3,3,3), b1 (planes,cmid)), cmid <= 256
 *   packed2 = lldwt_conv_f16x3_pack(w2 (planes,cout,cmid,3,3));  bias2 (planes,cout) or NULL                              */
int64_t lldwt_plc_fused_pack1_bytes(int cmid);
/* 1 when this process packs and runs the split-fp16 3x3 conv kernels in the 16x16x32 MFMA shape (LLDWT_PLC_SHAPE=16, read when
 * the library loads), 0 for the default 32x32x16. */
int lldwt_plc_shape16(void);
/* 1 when lldwt_plc_fused runs its split-fp16 (precision 0) 32x32x16 path as row-wise Winograd F(2,3) (the default), 0 for the
 * direct kernel (LLDWT_PLC_ALGO=direct, read when the library loads) or the 16x16x32 shape.  The packed sizes of
 * lldwt_conv_f16x3_packed_bytes and lldwt_plc_fused_pack1_bytes include the Winograd sections either way. */
int lldwt_plc_winograd(void);
int lldwt_plc_fused_pack1(const float* w1, const float* b1, void* packed1, int cmid, int64_t planes, void* stream);
int lldwt_plc_fused(const float* parent, float* y, const void* packed1, const void* packed2, const float* bias2, int cmid,
                    int cout, int act, int64_t planes, int64_t batch, int64_t h, int64_t w_, void* stream);

/* Same maths from the raw PyTorch-layout weights w, reference-order direct kernel (VALU); cross-checks the MFMA engine. */
int lldwt_conv2d_direct(const float* x, float* y, const float* w, const float* bias, const lldwt_conv_desc* d,
                        int64_t planes, int64_t batch, int64_t h, int64_t w_, void* stream);

/* GDN / inverse GDN (graphs/layers/gdn.py:77-92) with the NonNegativeParametrizer re-parametrisation
 * (utils/parametrizers.py:45-48) applied in-kernel to the raw beta (planes,C) / gamma (planes,C,C).         */
int lldwt_gdn(const float* x, float* y, const float* beta, const float* gamma, int64_t planes, int64_t batch,
              int C, int64_t hw, int inverse, float beta_min, void* stream);

/* Differentiable (training) composition of GDN: nrm = conv1x1(x*x, gamma', beta') on the conv engine, then
 * y = x * rsqrt(nrm) (inverse: x * sqrt(nrm)); these are its elementwise pieces and their backward.           */
int lldwt_ew_mul(const float* a, const float* b, float* out, int64_t n, float scale, void* stream);     /* out = scale*a*b */
int lldwt_gdn_apply(const float* x, const float* nrm, float* y, int64_t n, int inverse, void* stream);
int lldwt_gdn_apply_bwd(const float* x, const float* nrm, const float* g, float* dx, float* dn, int64_t n, int inverse,
                        void* stream);

/* LowerBound (utils/bound_ops.py:22-28) and NonNegativeParametrizer (utils/parametrizers.py:45-48), elementwise. */
int lldwt_lower_bound_fwd(const float* x, float* y, int64_t n, float bound, void* stream);
int lldwt_lower_bound_bwd(const float* x, const float* gy, float* gx, int64_t n, float bound, void* stream);
int lldwt_nonneg_param_fwd(const float* x, float* y, int64_t n, float minimum, void* stream);
int lldwt_nonneg_param_bwd(const float* x, const float* gy, float* gx, int64_t n, float minimum, void* stream);

/* The cgp stack with the folded context (as lldwt_cgp_rate_ctx) on the fp16 matrix cores, split-fp16 operands
 * (csrc/cgp_f16x3.hip): a register-resident chain per wave, layer l's accumulator tile is layer l+1's MFMA operand.  Built
 * for the reference's dimensions after the fold, 93 -> 162 -> 54 -> 18 -> 2 per subband (LiftingBasedDWT_net.py:282-289);
 * lldwt_cgp16_packed_bytes returns -1 for any other.  w_l: (planes, groups*c_{l+1}, c_l), b_l: (planes, groups*c_{l+1})
 * -- the folded first layer from the host (_fold_csc_into_cgp).  params: (planes, batch, 2*groups, h, w), sigma on the
 * even and mu on the odd channels, to be fed to lldwt_gauss_rate.                                                    */
int64_t lldwt_cgp16_packed_bytes(int c0, int c1, int c2, int c3, int groups);
int lldwt_cgp16_pack(const float* w0, const float* b0, const float* w1, const float* b1, const float* w2, const float* b2,
                     const float* w3, const float* b3, void* packed, int64_t planes, int c0, int c1, int c2, int c3,
                     int groups, void* stream);
int lldwt_cgp16_params(const float* plc, const float* xq, const void* packed, float* params, int64_t planes, int64_t batch,
                       int64_t h, int64_t w_, int groups, int K, uint32_t tap_mask, void* stream);
/* The training forward on the same register chain (always the fp32-accurate split-fp16 arithmetic, whatever lldwt_set_precision
 * says): lldwt_cgp16_params + the hidden activations after LeakyReLU in the layout of the unfused convs, h1 (Z, groups*162, hw),
 * h2 (Z, groups*54, hw), h3 (Z, groups*18, hw) -- what lldwt_cgp_bwd_split gates with and the 1x1 weight-gradient GEMMs read.
 * The bits follow from lldwt_gauss_rate on (x, params, noise).  Training forward of LiftingBasedDWT_net.py:282-289,357-365.   */
int lldwt_cgp16_params_train(const float* plc, const float* xq, const void* packed, float* params, float* h1, float* h2, float* h3,
                             int64_t planes, int64_t batch, int64_t h, int64_t w_, int groups, int K, uint32_t tap_mask,
                             void* stream);
/* Backward-data of the stack on the same register chain (replaces lldwt_cgp_bwd_split's fp32-MFMA kernel for the reference's
 * widths): dparams (Z, 2*groups, hw) = gradient at (sigma, mu); h1 / h2 / h3 = the activations lldwt_cgp16_params_train stored (their
 * SIGN gates LeakyReLU); -> d1 (Z, groups*162, hw), d2 (Z, groups*54, hw), d3 (Z, groups*18, hw) = gradients at the pre-activation
 * outputs (the dY of the 1x1 weight-gradient GEMMs) and the input gradient as dplc (Z, groups*81, hw) + dtaps (Z, groups*12, hw).
 * lldwt_cgp16_pack_bwd: the four forward weights (PyTorch layout, as lldwt_cgp16_pack) -> the transposed pack.                    */
int64_t lldwt_cgp16_bwd_packed_bytes(int c0, int c1, int c2, int c3, int groups);
int lldwt_cgp16_pack_bwd(const float* w0, const float* w1, const float* w2, const float* w3, void* packed, int64_t planes, int c0,
                         int c1, int c2, int c3, int groups, void* stream);
int lldwt_cgp16_bwd(const float* dparams, const float* h1, const float* h2, const float* h3, const void* packed_bwd, float* d1,
                    float* d2, float* d3, float* dplc, float* dtaps, int64_t planes, int64_t batch, int64_t hw, int groups,
                    void* stream);
/* Real entropy coding of a level with tree context + masked KxK context + cgp (the reference walks its pixels in raster
 * order with a CNN call on a crop each, graphs/models/LiftingBasedDWT_net.py:402-417,440-454,458-556): ONE anti-diagonal
 * wavefront step t = x + (K/2 + 1) * y, all planes / images / subbands / pixels of the step in one launch of the cgp
 * register chain (fp32-accurate f16x3 arithmetic whatever lldwt_set_precision says: encoder and decoder must agree bit for
 * bit).  yhat (Z, groups, h, w): the values decoded so far, 0 elsewhere (the masked taps only reach coded positions).
 * table63: the first 63 entries of the Gaussian scale table; CDF index = number of entries < max(sigma, 0.11).
 * idx / sym (Z, ntot, groups) int32 in wavefront order, this step's pixels at positions off .. off + n - 1 (rows ascending).
 *   encoder (y != null): sym = round(y - mu), yhat[pixel] = sym + mu, idx written.
 *   decoder (y == null): idx written, mu (Z, groups, n) kept for lldwt_wavefront_apply once the host has decoded sym.    */
int lldwt_cgp16_wavefront_step(const float* plc, float* yhat, const float* y, const void* packed, const float* table63,
                               int* idx, int* sym, float* mu, int64_t planes, int64_t batch, int64_t h, int64_t w,
                               int groups, int K, uint32_t tap_mask, int t, int64_t ntot, int64_t off, void* stream);
int lldwt_wavefront_apply(const int* sym, const float* mu, float* yhat, int64_t planes, int64_t batch, int64_t h, int64_t w,
                          int groups, int K, int t, int64_t ntot, int64_t off, void* stream);
/* The same two with a quantisation step (variable-rate coding): q = n / 16 with an integer n in [4, 1024] and
 * inv_q = fp32(1 / q), both formed on the host and checked here.  All in fp32:
 *   CDF index = number of table63 entries < max(sigma * inv_q, 0.11);  sym = rint((y - mu) * inv_q);  yhat = sym * q + mu
 * (sym * q is exact for |sym| < 2^12, so a fused and an unfused multiply-add agree).  q = inv_q = 1 gives the bits of the two
 * entry points above, which forward here.  sigma_out (decoder mode only, may be null): the step's sigmas in mu's layout. */
int lldwt_cgp16_wavefront_step_q(const float* plc, float* yhat, const float* y, const void* packed, const float* table63,
                                 int* idx, int* sym, float* mu, float* sigma_out, int64_t planes, int64_t batch, int64_t h,
                                 int64_t w, int groups, int K, uint32_t tap_mask, int t, int64_t ntot, int64_t off, float q,
                                 float inv_q, void* stream);
int lldwt_wavefront_apply_q(const int* sym, const float* mu, float* yhat, int64_t planes, int64_t batch, int64_t h, int64_t w,
                            int groups, int K, int t, int64_t ntot, int64_t off, float q, float inv_q, void* stream);
/* The same quantiser for a level whose (sigma, mu) are known for a whole grid at once (csrc/quant.hip): a ZTBlock phase or an
 * onlyEZWT level in one launch.  params (streams, 2 channels, h, w): sigma of channel c on 2c, mu on 2c + 1.  The grid is the
 * positions (r0 + stride i, c0 + stride j), i < h, j < w, of the (streams, channels, H, W) tensors y and level; level is
 * written there and nowhere else.  Encoder (y != null, sym_in null): idx and sym_out (streams, channels, h, w) int32 and the
 * dequantised value into level.  Decoder (sym_in != null, y null): idx again and the value into level.  Neither (level null
 * too): idx alone, which the decoder needs before it can pop the symbols.  y may be level itself. */
int lldwt_gauss_quantise(const float* params, const float* y, const int32_t* sym_in, const float* table63, int32_t* idx,
                         int32_t* sym_out, float* level, int64_t streams, int channels, int64_t h, int64_t w, int64_t H, int64_t W,
                         int r0, int c0, int stride, float q, float inv_q, void* stream);
/* Rate-distortion optimised quantisation: the ENCODER modes of the two quantisers above with the symbol chosen
 * between the nearest level s0 = rint(v), v = fp32((y - mu) * inv_q), and s1 = s0 - sign(s0), one level toward zero:
 *   sym = ((float)(cost[idx][s0] - cost[idx][s1]) * k > 1 + 2 sign(s0) (v - s0)) ? s1 : s0,   s0 == 0 stays
 * cost (ntab, width), sizes, offsets: the int32 device tables of lldwt_code_cost with its lookup (a symbol outside its table
 * counts 32 * 2^16); k = rho * 2^-16 with the Lagrangian rho = m / 64, m an integer in [1, 256], in units of q^2 per bit.  idx
 * does not depend on the choice and yhat / level receive sym * q + mu of the chosen symbol, so the decoders (the entry points
 * above with y == null, lldwt_wavefront_apply_q) follow without knowing.  y == null is LLDWT_EINVAL; mu and sigma_out of the
 * wavefront step are outputs of its decoder mode and are not written. */
int lldwt_cgp16_wavefront_step_rdo(const float* plc, float* yhat, const float* y, const void* packed, const float* table63,
                                   int* idx, int* sym, float* mu, float* sigma_out, int64_t planes, int64_t batch, int64_t h,
                                   int64_t w, int groups, int K, uint32_t tap_mask, int t, int64_t ntot, int64_t off, float q,
                                   float inv_q, const int32_t* cost, const int32_t* sizes, const int32_t* offsets, int32_t ntab,
                                   int32_t width, float k, void* stream);
int lldwt_gauss_quantise_rdo(const float* params, const float* y, const float* table63, int32_t* idx, int32_t* sym_out,
                             float* level, int64_t streams, int channels, int64_t h, int64_t w, int64_t H, int64_t W, int r0,
                             int c0, int stride, float q, float inv_q, const int32_t* cost, const int32_t* sizes,
                             const int32_t* offsets, int32_t ntab, int32_t width, float k, void* stream);
/* Region-of-interest coding: the three places where a step is applied, with a step MAP instead of one step.
 * qpairs (units, mh, mw, 2) fp32: per block of 2^shift x 2^shift positions of the level the pair (q, inv_q) of 7.1.6, one map
 * for all planes and channels of a unit -- the image (or tile) z % units of the Z = planes * units tensors (for the wavefront
 * entry points units == batch).  The position (y, x) of the level takes the pair at (y >> shift, x >> shift); the arithmetic
 * per coefficient is that of the entry points above with this pair.  The map must cover the level: mh >= ceil(h / 2^shift) and
 * mw >= ceil(w / 2^shift) of the level's h x w (for lldwt_gauss_quantise_map its H x W), else LLDWT_EINVAL, as is a null or
 * not 8-byte aligned qpairs.  The pairs are device data, which no entry point can check: they are formed in one place on the
 * host, from the integer map, with the rule of a single step.
 * cost == null: the nearest-level quantiser in every mode of the scalar entry point (sizes, offsets, ntab, width, k ignored).
 * cost != null: the encoder with the rule of 7.1.7 and each coefficient's own inv_q; y == null is then LLDWT_EINVAL. */
int lldwt_cgp16_wavefront_step_map(const float* plc, float* yhat, const float* y, const void* packed, const float* table63,
                                   int* idx, int* sym, float* mu, float* sigma_out, int64_t planes, int64_t batch, int64_t h,
                                   int64_t w, int groups, int K, uint32_t tap_mask, int t, int64_t ntot, int64_t off,
                                   const float* qpairs, int64_t mh, int64_t mw, int shift, const int32_t* cost,
                                   const int32_t* sizes, const int32_t* offsets, int32_t ntab, int32_t width, float k,
                                   void* stream);
int lldwt_wavefront_apply_map(const int* sym, const float* mu, float* yhat, int64_t planes, int64_t batch, int64_t h, int64_t w,
                              int groups, int K, int t, int64_t ntot, int64_t off, const float* qpairs, int64_t mh, int64_t mw,
                              int shift, void* stream);
int lldwt_gauss_quantise_map(const float* params, const float* y, const int32_t* sym_in, const float* table63, int32_t* idx,
                             int32_t* sym_out, float* level, int64_t streams, int64_t units, int channels, int64_t h, int64_t w,
                             int64_t H, int64_t W, int r0, int c0, int stride, const float* qpairs, int64_t mh, int64_t mw,
                             int shift, const int32_t* cost, const int32_t* sizes, const int32_t* offsets, int32_t ntab,
                             int32_t width, float k, void* stream);
/* Code length of `streams` streams of n (sym, idx) pairs under quantised tables, for the byte-target search: sums[z] += sum of
 * cost[idx][sym - offsets[idx]] with cost (ntab, width) int32 in units of 2^-16 bit, and esc_cost for a symbol outside
 * [0, sizes[idx] - 2) or an index outside [0, ntab), which escapes[z] counts.  sums and escapes (int64) must be ZERO on entry;
 * integer additions, so the result is exact and independent of their order. */
int lldwt_code_cost(const int32_t* sym, const int32_t* idx, int64_t streams, int64_t n, const int32_t* cost, int32_t ntab,
                    int32_t width, const int32_t* sizes, const int32_t* offsets, int32_t esc_cost, int64_t* sums, int64_t* escapes,
                    void* stream);
/* Real entropy coding of DWTConditioned2EntropyLayerZTBlock (csrc/ztblock.hip; nets: LiftingBasedDWT_net.py:618-624,716-744):
 * (sigma, mu) of ONE polyphase phase k (1 ee, 2 eo, 3 oe, 4 oo) of every plane, image and of the 3 subbands, both heads, in
 * one launch.  parent (planes, batch, 3, h2, w2): the decoded coarser level; level (planes, batch, 3, 2*h2, 2*w2): the
 * decoded finer level, of which only the phases before k are read (strided, in place; may be null for k == 1).
 * packed: planes * 3 * 2 records of lldwt_ztblock_packed_floats() floats, record (plane, subband, head 0 sigma / 1 mu)
 * (ops.ztblock_pack).  params (planes, batch, 6, h2, w2): sigma of subband j on channel 2j, mu on 2j+1.  Exact fp32
 * (v_mfma_f32_16x16x4_f32), every output's reduction order fixed: bitwise deterministic and batch invariant.          */
int64_t lldwt_ztblock_packed_floats(void);
int lldwt_ztblock_phase(const float* parent, const float* level, const float* packed, float* params, int64_t planes,
                        int64_t batch, int64_t h2, int64_t w2, int64_t H, int64_t W, int k, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Real entropy coding (reference: compress_ar / decompress_ar, LiftingBasedDWT_net.py:458-556, on
 * compressai.ans).  HOST functions (csrc/rans.hip): the range-ANS state machine is sequential byte work; the symbols
 * and CDF indexes it consumes are produced on the GPU by the wavefront scheduler of graphs/models/entropy_coding.py.
 *   lldwt_pmf_to_quantized_cdf : compressai `pmf_to_quantized_cdf` -- float pmf (n entries, tail mass last) -> n+1
 *                                cumulative counts at `precision` bits, every symbol with a non-zero frequency.
 *   lldwt_rans_encode          : BufferedRansEncoder.encode_with_indexes + flush (:466,502-505).  cdfs is an
 *                                (ncdf, cdf_stride) int32 table, cdf_sizes[i] = used entries of row i (= pmf length + 2),
 *                                offsets[i] = symbol value of slot 0.  Returns the number of bytes written to `out`
 *                                (a multiple of 4, <= out_cap) or a negative error code.  Out-of-table symbols are
 *                                escaped through the last slot and 4-bit bypass digits.
 *   lldwt_rans_decoder_new / _decode / _free : RansDecoder.set_stream / decode_stream (:516-517,540-546): an opaque
 *                                handle owning a copy of the stream; decode pops n symbols in coding order.        */
int lldwt_pmf_to_quantized_cdf(const float* pmf, int n, int precision, uint32_t* cdf);
int64_t lldwt_rans_encode(const int32_t* symbols, const int32_t* indexes, int64_t n, const int32_t* cdfs, int32_t ncdf,
                          int32_t cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, uint8_t* out,
                          int64_t out_cap);
void* lldwt_rans_decoder_new(const uint8_t* stream, int64_t nbytes);
int lldwt_rans_decode(void* dec, const int32_t* indexes, int64_t n, const int32_t* cdfs, int32_t ncdf, int32_t cdf_stride,
                      const int32_t* cdf_sizes, const int32_t* offsets, int32_t* symbols);
/* The same for nstreams decoders in one call (one wavefront step of every (plane, image) stream): stream k reads its n
 * indexes at indexes + k * stride and writes symbols + k * stride; one table set for all.
 * lldwt_rans_encode_multi: nstreams independent lldwt_rans_encode calls with one table set: stream k codes the n symbols
 *   at symbols + k * stride (indexes likewise) into out + k * out_stride (capacity out_stride bytes), its length goes to
 *   nbytes[k].
 * Both run their streams on a persistent pool of host threads when the call holds at least 4 096 (decode) / 12 288
 * (encode) symbols: min(16, OMP_NUM_THREADS if set, nstreams) threads.  Each stream runs the same state machine as the one-stream call, so bytes and
 * symbols do not depend on the thread count.  On failure the error of the lowest failing stream is reported.
 * lldwt_rans_set_parallel: threads > 0 forces that many threads (at most 16) on every multi-stream call, 1 = sequential;
 *   threads = 0 restores the rule above; min_symbols >= 0 replaces both thresholds, -1 restores them.             */
int lldwt_rans_decode_multi(void* const* decs, int64_t nstreams, const int32_t* indexes, int64_t n, int64_t stride,
                            const int32_t* cdfs, int32_t ncdf, int32_t cdf_stride, const int32_t* cdf_sizes,
                            const int32_t* offsets, int32_t* symbols);
int lldwt_rans_encode_multi(const int32_t* symbols, const int32_t* indexes, int64_t nstreams, int64_t n, int64_t stride,
                            const int32_t* cdfs, int32_t ncdf, int32_t cdf_stride, const int32_t* cdf_sizes,
                            const int32_t* offsets, uint8_t* out, int64_t out_stride, int64_t* nbytes);
int lldwt_rans_set_parallel(int threads, int64_t min_symbols);
void lldwt_rans_decoder_free(void* dec);

/* The interleaved rANS coder "irans32" (csrc/rans_gpu.hip; format: DESIGN.md 7.1.2, definition: tools/irans_ref.py).  Same
 * symbols, order and tables as lldwt_rans_*; a stream of n symbols has lldwt_irans_lanes(n) 32-bit lanes (1..32).
 *   lldwt_irans_encode: nstreams streams, one wave each; stream k codes the n device symbols / indexes at + k * stride into
 *     out + k * out_stride (out_stride >= lldwt_irans_capacity(n)); its bytes END at out + (k + 1) * out_stride and
 *     nbytes[k] (device) is their number, -1 on failure (bad index, no room), which also sets *flag != 0.  rcp: the device
 *     copy of lldwt_irans_rcp_table (65537 u32).  Host-side tables (cdfs, cdf_sizes, offsets) are device arrays here.
 *   lldwt_irans_decode: pops symbols [pos, pos + cnt) of every stream: indexes at indexes + k * idx_stride, symbols to
 *     symbols + k * sym_stride.  state: nstreams * lldwt_irans_state_words() u32, written by the launch with pos == 0 and
 *     carried between launches (queue them in order on one stream).  Stream k's bytes: bytes + byte_offsets[k], of length
 *     byte_lengths[k] (device int64); reads at or past the length return 0 and set *flag.  When pos + cnt == n, every lane
 *     must be back at 2^23 and the cursor at the length, else *flag is set.  lut: lldwt_irans_lut of the tables (device).
 *   lldwt_irans_rcp_table / lldwt_irans_lut: HOST helpers that fill the host arrays the two kernels read.              */
int lldwt_irans_lanes(int64_t n);
int64_t lldwt_irans_capacity(int64_t n);
int lldwt_irans_state_words(void);
int lldwt_irans_rcp_table(uint32_t* rcp);
int lldwt_irans_lut(const int32_t* cdfs, int32_t ncdf, int32_t cdf_stride, const int32_t* cdf_sizes, int32_t* lut);
int lldwt_irans_encode(const int32_t* symbols, const int32_t* indexes, int64_t nstreams, int64_t n, int64_t stride,
                       const int32_t* cdfs, int32_t ncdf, int32_t cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets,
                       const uint32_t* rcp, uint8_t* out, int64_t out_stride, int64_t* nbytes, int32_t* flag, void* stream);
int lldwt_irans_decode(uint32_t* state, const uint8_t* bytes, const int64_t* byte_offsets, const int64_t* byte_lengths,
                       int64_t nstreams, int64_t n, int64_t pos, int64_t cnt, const int32_t* indexes, int64_t idx_stride,
                       int32_t* symbols, int64_t sym_stride, const int32_t* cdfs, int32_t ncdf, int32_t cdf_stride,
                       const int32_t* cdf_sizes, const int32_t* offsets, const int32_t* lut, int32_t* flag, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Rate estimation, fused quantise + likelihood + both LowerBounds + -log2 + sum of bits.
 * Gaussian (compressai GaussianConditional.forward as called at LiftingBasedDWT_net.py:334,345,364,832):
 *   v = mode==0 ? round(x - mu) + mu : x + noise       (noise: U(-.5,.5) tensor or NULL -> eval)
 *   p = Phi((.5-|v-mu|)/max(sigma,0.11)) - Phi((-.5-|v-mu|)/max(sigma,0.11)),  bits = -log2(max(p,1e-9))
 * params: (Z, 2C, h, w) with sigma = channel 2c, mu = channel 2c+1 (:332-333).  x, bits, qout: (Z,C,h,w).
 * qout (optional) receives v (what onlyEZWT hands to the decoder, :832-834).  bits (optional).
 * bit_sum (optional): one device double, accumulated atomically (caller zeroes it).                       */
int lldwt_gauss_rate(const float* x, const float* params, const float* noise, float* bits, float* qout,
                     double* bit_sum, int64_t Z, int C, int64_t hw, void* stream);
/* Backward of lldwt_gauss_rate: gbits = dL/dbits -> dx (Z,C,hw) and dparams (Z,2C,hw) = (dsigma, dmu) interleaved;
 * closed form, both LowerBound pass-through rules (utils/bound_ops.py:26-28) applied.                      */
int lldwt_gauss_rate_bwd(const float* x, const float* params, const float* noise, const float* gbits, float* dx,
                         float* dparams, int64_t Z, int C, int64_t hw, void* stream);
/* quantize(x, mode, means=None): round(x) or x + noise (LiftingBasedDWT_net.py:330,341,352). */
int lldwt_quantize(const float* x, const float* noise, float* q, int64_t n, void* stream);

/* Fused "cgp" parameter network + Gaussian rate of DWTConditioned2EntropyLayerZTsepSubbands
 * (LiftingBasedDWT_net.py:282-289 grouped 1x1 convs c0 -> c1 -> c2 -> c3 -> 2 with LeakyReLU, :361-365 rate).
 * cat: (Z, groups*c0, hw) = the interleaved (plc_g, csc_g) tensor of :357-359; x, noise, bits: (Z, groups, hw);
 * params_out (optional): (Z, 2*groups, hw) receives (sigma, mu) as the reference's out_xo_qnt_mu_sigma.
 * lldwt_cgp_pack: the four conv weights (planes, groups*c_{l+1}, c_l) / biases (planes, groups*c_{l+1}) in PyTorch
 * layout -> packed (planes, lldwt_cgp_packed_floats) in MFMA A-operand lane order.                       */
int64_t lldwt_cgp_packed_floats(int c0, int c1, int c2, int c3, int groups);
int lldwt_cgp_pack(const float* w0, const float* b0, const float* w1, const float* b1, const float* w2,
                   const float* b2, const float* w3, const float* b3, float* packed, int64_t planes, int c0, int c1,
                   int c2, int c3, int groups, void* stream);
int lldwt_cgp_rate(const float* cat, const float* x, const float* noise, const float* packed, float* bits,
                   float* params_out, double* bit_sum, int64_t planes, int64_t batch, int64_t hw, int c0, int c1,
                   int c2, int c3, int groups, void* stream);
/* lldwt_cgp_rate with the masked context conv folded into its first layer (eval).  The csc conv (MaskedConv2d 5x5 type A,
 * LiftingBasedDWT_net.py:275-277,353) feeds cgp layer 0 with no nonlinearity in between, so the host folds
 * W0[:, csc half] . Wcsc (+ bias) into `ntaps` extra input columns of layer 0 -- packed with lldwt_cgp_pack for
 * c0 = cplc + ntaps -- and the kernel gathers those inputs itself: the live taps (tap_mask, KxK) of the quantised
 * subband xq (Z, groups, h, w), zero outside the image.  plc: (Z, groups*cplc, h, w), the tree-context conv's output. */
int lldwt_cgp_rate_ctx(const float* plc, const float* xq, const float* x, const float* noise, const float* packed,
                       float* bits, float* params_out, double* bit_sum, int64_t planes, int64_t batch, int64_t h,
                       int64_t w_, int cplc, int K, uint32_t tap_mask, int c1, int c2, int c3, int groups, void* stream);
/* Training variants of the fused stack.  lldwt_cgp_rate_train: as lldwt_cgp_rate (no bit_sum), and also writes
 * params_out (sigma, mu: (Z, 2*groups, hw)) and the hidden activations after LeakyReLU, h1 (Z, groups*c1, hw),
 * h2 (Z, groups*c2, hw), h3 (Z, groups*c3, hw) -- the layout the unfused 1x1 convs would produce.
 * lldwt_cgp_bwd: backward-data of the four layers in one launch.  dparams (Z, 2*groups, hw) = gradient at (sigma, mu)
 * (lldwt_gauss_rate_bwd) -> d3, d2, d1 = gradients at the PRE-activation outputs of layers 3, 2, 1 (shapes of
 * h3, h2, h1; what lldwt_conv2d_wgrad needs as dy) and dcat (Z, groups*c0, hw).  packed_bwd: the forward weights
 * w0..w3 (PyTorch layout) transposed into MFMA A-operand order by lldwt_cgp_pack_bwd
 * (planes, lldwt_cgp_bwd_packed_floats).  Replaces autograd through LiftingBasedDWT_net.py:282-289,360-365. */
int lldwt_cgp_rate_train(const float* cat, const float* x, const float* noise, const float* packed, float* bits,
                         float* params_out, float* h1, float* h2, float* h3, int64_t planes, int64_t batch, int64_t hw,
                         int c0, int c1, int c2, int c3, int groups, void* stream);
int64_t lldwt_cgp_bwd_packed_floats(int c0, int c1, int c2, int c3, int groups);
int lldwt_cgp_pack_bwd(const float* w0, const float* w1, const float* w2, const float* w3, float* packed_bwd,
                       int64_t planes, int c0, int c1, int c2, int c3, int groups, void* stream);
int lldwt_cgp_bwd(const float* dparams, const float* h1, const float* h2, const float* h3, const float* packed_bwd,
                  float* d1, float* d2, float* d3, float* dcat, int64_t planes, int64_t batch, int64_t hw, int c0, int c1,
                  int c2, int c3, int groups, void* stream);
/* The training stack WITHOUT the concatenated [tree-context channels | gathered taps] input tensor (1.75 GB at the level-0 shape of
 * configs[2], written by a torch.cat and read back; its gradient took the same way back):
 *   lldwt_cgp_rate_train_ctx : lldwt_cgp_rate_train reading its input as lldwt_cgp_rate_ctx does -- plc (Z, groups*cplc, h, w)
 *                              and the live taps of the quantised subband xq (Z, groups, h, w), gathered in the kernel;
 *   lldwt_cgp_bwd_split      : lldwt_cgp_bwd with the input gradient as two tensors, dplc (Z, groups*cplc, hw) and
 *                              dtaps (Z, groups*ntaps, hw) (tap order = ascending live taps of the mask);
 *   lldwt_wgrad1x1_split     : weight gradient of a grouped 1x1 conv whose input rows are [xa rows | xb rows] per group
 *                              (layer 0: xa = plc, xb = the gathered taps), dw (planes, cout, ca + cb), dbias (planes, cout).
 * Autograd of LiftingBasedDWT_net.py:282-289,353-365.                                                                       */
int lldwt_cgp_rate_train_ctx(const float* plc, const float* xq, const float* x, const float* noise, const float* packed,
                             float* bits, float* params_out, float* h1, float* h2, float* h3, int64_t planes, int64_t batch,
                             int64_t h, int64_t w_, int cplc, int K, uint32_t tap_mask, int c1, int c2, int c3, int groups,
                             void* stream);
int lldwt_cgp_bwd_split(const float* dparams, const float* h1, const float* h2, const float* h3, const float* packed_bwd,
                        float* d1, float* d2, float* d3, float* dplc, float* dtaps, int64_t planes, int64_t batch, int64_t hw,
                        int cplc, int ntaps, int c1, int c2, int c3, int groups, void* stream);
int lldwt_wgrad1x1_split(const float* xa, const float* xb, const float* dy, float* dw, float* dbias, int64_t planes,
                         int64_t batch, int64_t hw, int ca, int cb, int cout, int groups, void* stream);

/* Factorized (compressai EntropyBottleneck.forward, call sites LiftingBasedDWT_net.py:225,229,815,818):
 * per channel c of plane p: 5 tiny matrices softplus(_matrix{i}) (1x3,3x3,3x3,3x3,3x1), biases, tanh(_factor).
 * eb: packed per (plane,channel) block of LLDWT_EB_FLOATS floats =
 *   [m0(3) b0(3) f0(3) m1(9) b1(3) f1(3) m2(9) b2(3) f2(3) m3(9) b3(3) f3(3) m4(3) b4(1) median(1)] raw values. */
#define LLDWT_EB_FLOATS 59
int lldwt_factorized_rate(const float* x, const float* eb, const float* noise, float* bits, float* qout,
                          double* bit_sum, int64_t planes, int64_t batch, int C, int64_t hw, void* stream);

/* Eval with the per-offset table precomputed: lldwt_factorized_table writes, for every (plane, channel), the bits of
 * median + o for the integer offsets o = -127 .. 127 (table: planes * C rows of 256 floats) -- the values the kernel of
 * lldwt_factorized_rate builds per workgroup, by the same code; it depends on the parameters only (compressai's update() keeps
 * its quantised CDFs the same way, entropy_models.py:206-240).  lldwt_factorized_rate_tab is the eval form of
 * lldwt_factorized_rate reading that table: identical results, no table build in front of every workgroup's stream. */
int lldwt_factorized_table(const float* eb, float* table, int64_t planes, int C, void* stream);
int lldwt_factorized_rate_tab(const float* x, const float* eb, const float* table, float* bits, float* qout, double* bit_sum,
                              int64_t planes, int64_t batch, int C, int64_t hw, void* stream);

/* Backward of lldwt_factorized_rate (training, v = x + noise): dx (Z,C,hw) and deb (planes,C,59) += gradient wrt the RAW
 * packed parameters (softplus' / tanh' applied; median slot stays 0).  deb is accumulated with atomics: zero it first.
 * noise == NULL (eval): the parameters' gradients at v = round(x - median) + median, where the eval forward evaluates; dx = 0. */
int lldwt_factorized_rate_bwd(const float* x, const float* eb, const float* noise, const float* gbits, float* dx,
                              float* deb, int64_t planes, int64_t batch, int C, int64_t hw, void* stream);

/* sum((a-b)^2) and sum(x) into a double (graphs/losses/rate_dist.py:36-41). */
int lldwt_sq_err_sum(const float* a, const float* b, int64_t n, double* out, void* stream);
int lldwt_sum(const float* x, int64_t n, double* out, void* stream);
/* 1 when the process runs the earlier launches of the small end-of-step work (LLDWT_TAIL=legacy, read when the library loads):
 * the scalar sum kernel; the model then runs the coarsest level's two context stacks layer by layer with lldwt_conv2d instead of
 * lldwt_conv_stack_pair (the entry itself works in either mode). */
int lldwt_tail_legacy(void);
/* out = alpha*a + beta*b elementwise (b optional): gradient glue of the loss (d mse = 2(xhat-x)/N). */
int lldwt_axpby(const float* a, const float* b, float* out, int64_t n, float alpha, float beta, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Fixed CDF 9/7 (bior4.4) DWT, periodization (DWTPytorchWaveletsLayer, lifting_dwt_nets.py:228-231,250,274).
 * Same tensor conventions as lldwt_lifting_forward/inverse.                                                */
/* Level inputs SHORTER than the 10-tap filter (2, 4, 6 or 8 samples, e.g. a 64 x 64 image at 4 levels).  The reference's
 * pytorch_wavelets afb1d / sfb1d fold the linear convolution back once there; these kernels compute the exact periodic
 * transform (= PyWavelets 'periodization', perfect reconstruction).  The two forms differ on such levels and agree from
 * 10 samples up (every BASELINE config: smallest level input 32).  periodic = 0 (default): lldwt_cdf97_* return
 * LLDWT_EINVAL for such a call instead of silently differing from the reference; 1: compute the periodic form.        */
int lldwt_set_cdf97_short_levels(int periodic);
int64_t lldwt_cdf97_ws_bytes(int64_t Z, int64_t H, int64_t W);
/* adj = 0: the transform.  adj = 1: the adjoints for training (bior4.4 is not orthogonal, so the backward pass is NOT the
 * other transform):
 * lldwt_cdf97_inverse(adj=1) maps (g_ll, g_yh) -> g_x   = adjoint of lldwt_cdf97_forward (backward of the analysis);
 * lldwt_cdf97_forward(adj=1) maps g_x -> (g_ll, g_yh)   = adjoint of lldwt_cdf97_inverse (backward of the synthesis). */
int lldwt_cdf97_forward(const float* x, float* ll, float* const* yh, int64_t Z, int64_t H, int64_t W, int levels,
                        int adj, void* ws, int64_t ws_bytes, void* stream);
int lldwt_cdf97_inverse(const float* ll, const float* const* yh, float* x, int64_t Z, int64_t H, int64_t W,
                        int levels, int adj, void* ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * MS-SSIM (pytorch-msssim 0.2.1: data_range 1, 11-tap Gaussian window sigma 1.5 applied "valid", K = (0.01, 0.03), weights
 * (0.0448, 0.2856, 0.3001, 0.2363, 0.1333); the first `scales` weights as they are for scales < 5).  x is the target and y the
 * reconstruction, both (planes, H, W) fp32 with planes = B*C; `offset` is added to both on load (0.5 for RGB kept in [-0.5, 0.5]).
 * Between scales: 2x2 average, stride 2, an odd side padded by one zero on both ends, divisor 4 always.  Every side must be at
 * least 10 * 2^(scales-1) + 1.  One fused launch per scale: no statistic map is written to memory; nothing synchronises.
 *   pyr   lldwt_msssim_ws_floats() floats: the pooled (x, y) pairs of scales 1.. (x then y, each (planes, Hs, Ws)); written by
 *         the forward, read by the backward
 *   sums  (scales, planes, 2) doubles of scratch (sum of cs, sum of l*cs); zeroed by the call
 *   v     (scales, planes): max(spatial mean of cs, 0), of l*cs for the last scale;  m (planes) = prod_s v_s^w_s
 *   coef  (scales, planes): dm/dv_s / N_s for the backward; all zero for a plane in which some v_s is clamped to 0, so that
 *         the gradient there is exactly zero (w v^(w-1) is never evaluated at 0)
 * lldwt_msssim_backward writes grad_y (planes, H, W) = d(gscale * g[0] * sum_planes m) / dy; g is a DEVICE double (null = 1),
 * gpyr is scratch of lldwt_msssim_ws_floats() / 2 floats.  The statistics are recomputed; there is no gradient for x. */
int64_t lldwt_msssim_ws_floats(int64_t planes, int64_t H, int64_t W, int scales);
int lldwt_msssim_forward(const float* x, const float* y, float offset, int64_t planes, int64_t H, int64_t W, int scales,
                         float* pyr, double* sums, double* v, double* m, double* coef, void* stream);
int lldwt_msssim_backward(const float* x, const float* y, float offset, int64_t planes, int64_t H, int64_t W, int scales,
                          const float* pyr, const double* coef, const double* g, double gscale, float* gpyr, float* grad_y,
                          void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Residual layer of the codec (lossless / near-lossless coding over the decoded base image; DESIGN.md 7.1.5, csrc/residual.hip).
 * A unit is the in-image rectangle of one tile of the grid of lldwt_ycc_tiles_to_u8hwc: tile t = (b * ny + ty) * nx + tx of
 * th x tw covers rows [ty*th, min((ty+1)*th, H)) and columns [tx*tw, min((tx+1)*tw, W)).  x, xh and dst are uint8 HWC
 * (B,h,w,3) buffers holding the region (y0, x0, h, w) of every image.  A call handles the n units tiles[0..n) (device int32;
 * null: first .. first+n-1), which must all measure uh x uw and lie inside the region; a unit that does not writes nothing.
 * d: the near-lossless bound in [0, LLDWT_RESID_MAX_NEAR], 0 = lossless; Q = (255 + d) / (2d + 1).  Per pixel and channel c:
 *   symbol   q = sign(r) * ((|r| + d) / (2d + 1)), r = x - xh;   output  clamp(xh + q * (2d + 1), 0, 255), so |out - x| <= d
 *   context  c * 8 + a, a = 0 if g == 0 else min(7, 1 + floor(log2 g)),
 *            g = |xh[y,x+1] - xh[y,x-1]| + |xh[y+1,x] - xh[y-1,x]| with the neighbour coordinates clamped to the unit
 * sym, ctx, idx: (3 n, uh*uw) int32, row 3 j + c = channel c of unit j in raster order (the range coders' layout).
 * hist: (n, 3, 8, 2Q+1) int32 counts of q + Q per context.  scales: (n, 24) uint8, the table index of each context.
 * cs_*: (n) uint64, sum_i (byte_i + 1) * (1 + i mod 65521) mod 2^64 over the unit's bytes in HWC raster order.
 * hist and every cs_* array must be ZERO on entry (the kernels add with integer atomics: the result is order-independent).
 * dst may be xh.  Nothing synchronises. */
#define LLDWT_RESID_MAX_NEAR 32
int lldwt_resid_analyse(const uint8_t* x, const uint8_t* xh, const int32_t* tiles, int64_t first, int64_t n, int64_t B, int64_t H,
                        int64_t W, int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0, int64_t x0, int64_t h, int64_t w,
                        int64_t uh, int64_t uw, int d, int32_t* sym, int32_t* ctx, int32_t* hist, uint64_t* cs_xh, uint64_t* cs_x,
                        void* stream);
int lldwt_resid_contexts(const uint8_t* xh, const int32_t* tiles, int64_t first, int64_t n, int64_t B, int64_t H, int64_t W,
                         int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0, int64_t x0, int64_t h, int64_t w, int64_t uh,
                         int64_t uw, const uint8_t* scales, int32_t* idx, uint64_t* cs_xh, void* stream);
int lldwt_resid_apply(const uint8_t* xh, const int32_t* tiles, int64_t first, int64_t n, int64_t B, int64_t H, int64_t W,
                      int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0, int64_t x0, int64_t h, int64_t w, int64_t uh,
                      int64_t uw, int d, const int32_t* sym, uint8_t* dst, uint64_t* cs_out, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Quality layers of the codec (SNR refinement of the levels that carry a step; DESIGN.md 7.1.10, csrc/layers.hip).
 * Element-wise over a level (streams, channels, h, w) fp32 with its Gaussian parameters (streams, 2 channels, h, w), sigma of
 * channel c on 2c and mu on 2c + 1, and table63 the scale table's first 63 entries (the layout of lldwt_gauss_quantise).
 * A layer takes the level from the step q_prev to q; both come as pairs (q, fp32(1 / q)) formed on the host (the division in
 * double), else LLDWT_EINVAL.  All arithmetic is fp32 with every product rounded before it is added (no fused multiply-add):
 *   idx  = #(table63 < max(sigma * inv_q_prev, 0.11))
 *   m    = rint((v_prev - mu) * inv_q_prev), a = min(|m|, K), sign = m < 0 ? -1 : +1
 *   row  = idx * (K + 1) + a                                   (the table of the coded symbol, K in [1, LLDWT_LAYER_MAX_K])
 *   t    = clamp(rint((y - v_prev) * inv_q), -1, 1), v_out = v_prev + t * q, coded symbol = sign * t
 * lldwt_layer_encode writes sym, row (int32) and v_out; lldwt_layer_rows writes row and sign (int32, +1 / -1) from v_prev and
 * params alone, which a decoder needs before it can pop the symbols; lldwt_layer_apply writes v_out = v_prev + sign * sym * q
 * (a symbol outside {-1, 0, +1} is clamped).  v_out may be v_prev.  One 16-byte access per array and thread where w % 4 == 0
 * and every array is 16-byte aligned, one element per thread otherwise.  streams * channels <= 65535.  Nothing synchronises. */
#define LLDWT_LAYER_MAX_K 255
int lldwt_layer_encode(const float* y, const float* v_prev, const float* params, const float* table63, int32_t* sym, int32_t* row,
                       float* v_out, int64_t streams, int channels, int64_t h, int64_t w, float q_prev, float inv_q_prev, float q,
                       float inv_q, int K, void* stream);
int lldwt_layer_rows(const float* v_prev, const float* params, const float* table63, int32_t* row, int32_t* sign, int64_t streams,
                     int channels, int64_t h, int64_t w, float q_prev, float inv_q_prev, int K, void* stream);
int lldwt_layer_apply(const float* v_prev, const int32_t* sym, const int32_t* sign, float* v_out, int64_t streams, int channels,
                      int64_t h, int64_t w, float q, float inv_q, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Centroid reconstruction of the levels that carry a step (a decoder's choice; DESIGN.md 7.1.13, csrc/recon.hip).
 * Element-wise over a level v (streams, channels, h, w) fp32 with its Gaussian parameters (streams, 2 channels, h, w), sigma of
 * channel c on 2c and mu on 2c + 1 (the layout of lldwt_gauss_quantise), all fp32 with every product rounded:
 *   u   = (v - mu) * inv_q,  a = |u|,  s = max(sigma * inv_q, 0.11)
 *   out = clamp(v - copysign(q * delta(a, s), u), v - q / 2, v + q / 2)
 *   delta(a, s) = a - E[X | a - 1/2 <= X <= a + 1/2], X ~ N(0, s^2), to the tolerance DESIGN.md 7.1.13 states (not to bits)
 * and out = v wherever u, sigma * inv_q or delta is not a finite number.  out may be v.
 * lldwt_gauss_centroid takes the step in force as a pair (q, fp32(1 / q)) formed on the host (the division in double; q in
 * (0, 64]), else LLDWT_EINVAL; lldwt_gauss_centroid_map takes the pair of every element from a step map as
 * lldwt_gauss_quantise_map does: qpairs (units, mh, mw, 2), stream z reads the map of unit z % units and position (i, j) the
 * pair at (i >> shift, j >> shift); the map must cover the h x w level and be 8-byte aligned, else LLDWT_EINVAL.
 * One 16-byte access per array and thread where w % 4 == 0 and every array is 16-byte aligned, one element per thread
 * otherwise.  streams * channels <= 65535.  Nothing synchronises. */
int lldwt_gauss_centroid(const float* params, const float* v, float* out, int64_t streams, int channels, int64_t h, int64_t w,
                         float q, float inv_q, void* stream);
int lldwt_gauss_centroid_map(const float* params, const float* v, float* out, int64_t streams, int64_t units, int channels,
                             int64_t h, int64_t w, const float* qpairs, int64_t mh, int64_t mw, int shift, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Adaptive quantisation: a step map derived from the image (csrc/aq.hip).  Integers only: defined to the bit.
 * lldwt_aq_activity: img (B, H, W, 3) uint8 RGB -> a (B, hb, wb) int32 with hb = ceil(H / 2^L), wb = ceil(W / 2^L), and sums (B)
 * int64, the sum of a over each image (zeroed here, then added to with integer atomics: exact in any order).  Per block of
 * 2^L x 2^L pixels, coordinates clamped to the image:
 *   Y = (77 R + 150 G + 29 B + 128) >> 8
 *   S = sum over the block's 4 x 4 cells of 16 sum(Y^2) - (sum Y)^2,  x = S + (1 << (6 + 2 L))
 *   a = lg(x) = 8 e + #{j in 1..7 : m >= T_j},  e = floor(log2 x),  m = x >> (e - 15) (x << (15 - e) below 2^15),
 *   T = 35734, 38968, 42495, 46341, 50536, 55109, 60097  (T_j the smallest integer with T_j^8 >= 2^(120 + j))
 * One pass over the image; nothing else is written.  L in [2, 8], B <= 65535, hb * wb < 2^22; a 4-byte and sums 8-byte aligned.
 * lldwt_aq_steps: a (B, N) int32 and sums (B) int64 as above, N = hb * wb -> n (B, N) int32, n / 16 the step of each block at the
 * strength m / 16 (m in [1, 32]) around the base step n_q / 16 (n_q in [4, 1024]):
 *   d = clamp(floor((2 m (N a - sums) + 128 N) / (256 N)), -8, 24),  n = clamp((n_q * G(d) + 8) >> 4, 4, 1024)
 * with G(d) = round(16 * 2^(d / 4)), the step grid of a byte target.  N < 2^31; a, n 4-byte and sums 8-byte aligned.
 * Anything else is LLDWT_EINVAL.  Nothing synchronises. */
int lldwt_aq_activity(const uint8_t* img, int32_t* a, int64_t* sums, int64_t B, int64_t H, int64_t W, int L, void* stream);
int lldwt_aq_steps(const int32_t* a, const int64_t* sums, int32_t* n, int64_t B, int64_t N, int m, int n_q, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LLDWT_H */
