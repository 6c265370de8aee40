// depth.hip -- image codec I/O for 9- to 16-bit samples (codec.py depth=) for gfx950.
// The uint8 kernels of ops.hip and chroma.hip are not touched; these are their uint16 siblings on the same tile grid: tile
// t = (b * ny + ty) * nx + tx of th x tw covers rows [ty*th, (ty+1)*th) and columns [tx*tw, (tx+1)*tw), positions past the image
// take the clamped source pixel.  A sample of depth d is v / M with M = 2^d - 1 as an fp32 constant, a true division like the
// / 255.0f of the uint8 kernels; everything after it is their expression, in their order, separately rounded (the file is built
// with -ffp-contract=off like them), so depth 8 on uint16 storage gives their floats and values bit for bit.  An input kernel
// that meets a sample above M sets *flag to 1 with an ordinary store (several threads may, all with the same value).
// All kernels are bandwidth-bound: one pass, one thread per pixel (per chroma sample for the 4:2:0 input), every plane row
// written coalesced.  A row of a uint16 HWC image starts at a multiple of 2 bytes only (6 W is no multiple of 4 for odd W), so
// every sample is loaded and stored as one 16-bit access, which is aligned wherever the row starts.
#include "common.h"
#include <math.h>

namespace lldwt {

constexpr float DP_KR = 0.2126f, DP_KG = 0.7152f, DP_KB = 0.0722f;     // BT.709, as ops.hip and chroma.hip

struct DpYcc {
    float y, cb, cr;
};

// One source pixel -> (Y - 0.5, Cb, Cr): the expressions of k_u8hwc_to_ycc_tiles with M in place of 255.0f.
__device__ __forceinline__ DpYcc px16_to_ycc(const uint16_t* __restrict__ s, float M, uint32_t maxv, int32_t* __restrict__ flag) {
    const uint32_t r0 = s[0], g0 = s[1], b0 = s[2];
    if (r0 > maxv || g0 > maxv || b0 > maxv) *flag = 1;
    const float rr = (float)r0 / M, g = (float)g0 / M, bl = (float)b0 / M;
    const float yy = DP_KR * rr + DP_KG * g + DP_KB * bl;
    DpYcc v;
    v.cb = 0.5f * (bl - yy) / (1.f - DP_KB) + 0.5f;
    v.cr = 0.5f * (rr - yy) / (1.f - DP_KR) + 0.5f;
    v.y = yy - 0.5f;
    return v;
}

// clamp(c, -0.5, 0.5) -> floor((c + 0.5) * M + 0.5): the sample rule of the output kernels (at most M, so it fits 16 bits)
__device__ __forceinline__ uint16_t sample_u16(float c, float M) {
    c = fminf(fmaxf(c, -0.5f), 0.5f);
    return (uint16_t)floorf((c + 0.5f) * M + 0.5f);
}

// (Y - 0.5, Cb, Cr) -> 3 samples of uint16 RGB: the expressions of ops.hip's ycc_vals_u8 without its affine map.
__device__ __forceinline__ void ycc_to_u16(float s0, float cb, float cr, float M, uint16_t* __restrict__ d) {
    const float y = s0 + 0.5f;
    float rr = y + (2.f - 2.f * DP_KR) * (cr - 0.5f);
    float bl = y + (2.f - 2.f * DP_KB) * (cb - 0.5f);
    float g = (y - DP_KR * rr - DP_KB * bl) / DP_KG;
    rr -= 0.5f; g -= 0.5f; bl -= 0.5f;
    d[0] = sample_u16(rr, M);
    d[1] = sample_u16(g, M);
    d[2] = sample_u16(bl, M);
}

// Per-plane affine map of a reduced-resolution decode (ops.hip's LLAffine): s -> (s - b[p]) * inv_a[p].
struct DpAffine {
    float inv_a[3], b[3];
};

// tile number (first + j, or tiles[j]) -> image b and tile origin (oy, ox); false when the index is outside the grid
__device__ __forceinline__ bool dp_tile_origin(int64_t t, int64_t B, int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t& b,
                                               int64_t& oy, int64_t& ox) {
    if (t < 0 || t >= B * ny * nx) return false;
    const uint32_t per = (uint32_t)(ny * nx), b32 = (uint32_t)t / per, r = (uint32_t)t - b32 * per;   // the launcher bounds B*ny*nx
    const uint32_t ty = r / (uint32_t)nx, tx = r - ty * (uint32_t)nx;
    b = b32;
    oy = (int64_t)ty * th;
    ox = (int64_t)tx * tw;
    return true;
}

// The thread of an output kernel -> its slot's image b, its pixel (ly, lx) in the tile and (ry, rx) in the region; false when
// it has nothing to write: the region and in-image tests of k_ycc_tiles_to_u8hwc.  GRID = true: grid (cdiv(tw,256), th, n), one
// thread per tile pixel.  GRID = false: the 1 x 1 grid (tile = image, tiles == NULL): grid (cdiv(w,256), h, n), one thread per
// region pixel.
template <bool GRID>
__device__ __forceinline__ bool dp_out_pixel(const int32_t* __restrict__ tiles, int64_t first, int64_t B, int64_t H, int64_t W,
                                             int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0, int64_t x0, int64_t h,
                                             int64_t w, int64_t& b, int64_t& ly, int64_t& lx, int64_t& ry, int64_t& rx) {
    const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, j = blockIdx.z;
    if (!GRID) {
        if (x >= w) return false;
        b = first + j;
        ry = blockIdx.y;
        rx = x;
        ly = y0 + ry;
        lx = x0 + x;
        return true;
    }
    if (x >= tw) return false;
    int64_t oy, ox;
    if (!dp_tile_origin(tiles ? (int64_t)tiles[j] : first + j, B, th, tw, ny, nx, b, oy, ox)) return false;
    ly = blockIdx.y;
    lx = x;
    const int64_t gy = oy + ly, gx = ox + lx;
    if (gy >= H || gx >= W || gy < y0 || gy >= y0 + h || gx < x0 || gx >= x0 + w) return false;
    ry = gy - y0;
    rx = gx - x0;
    return true;
}

// uint16 HWC RGB -> plane-major (3,n,1,th,tw) YCbCr with Y-0.5 for the tiles first .. first+n-1.  Grid (cdiv(tw,256), th, n): one
// thread per output pixel.  GRID = false: the 1 x 1 grid (tile = image), the untiled codec's path.
template <bool GRID>
__global__ void k_u16hwc_to_ycc_tiles(const uint16_t* __restrict__ src, float* __restrict__ ycc, int64_t B, int64_t H, int64_t W,
                                      int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t first, int64_t n, float M,
                                      uint32_t maxv, int32_t* __restrict__ flag) {
    const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (x >= tw) return;
    const int64_t y = blockIdx.y, j = blockIdx.z;
    int64_t b = first + j, oy = 0, ox = 0;
    if (GRID && !dp_tile_origin(first + j, B, th, tw, ny, nx, b, oy, ox)) return;
    const int64_t gy = oy + y, gx = ox + x;
    const int64_t sy = gy < H ? gy : H - 1, sx = gx < W ? gx : W - 1;
    const DpYcc v = px16_to_ycc(src + ((b * H + sy) * W + sx) * 3, M, maxv, flag);
    const int64_t hw = th * tw, p = y * tw + x;
    ycc[(0 * n + j) * hw + p] = v.y;
    ycc[(1 * n + j) * hw + p] = v.cb;
    ycc[(2 * n + j) * hw + p] = v.cr;
}

// plane-major (3,n,1,th,tw) YCbCr of n tiles -> uint16 HWC RGB of the pixels inside the image and the region, dst (B,h,w,3).
// AFFINE: each plane's sample goes through its map first (a reduced-resolution LL band), as ops.hip's ycc_vals_u8<true>.
template <bool GRID, bool AFFINE>
__global__ void k_ycc_tiles_to_u16hwc(const float* __restrict__ ycc, const int32_t* __restrict__ tiles, int64_t first, int64_t n,
                                      int64_t B, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0,
                                      int64_t x0, int64_t h, int64_t w, uint16_t* __restrict__ dst, DpAffine af, float M) {
    int64_t b, ly, lx, ry, rx;
    if (!dp_out_pixel<GRID>(tiles, first, B, H, W, th, tw, ny, nx, y0, x0, h, w, b, ly, lx, ry, rx)) return;
    const int64_t j = blockIdx.z, hw = th * tw, p = ly * tw + lx;
    float s0 = ycc[(0 * n + j) * hw + p], cb = ycc[(1 * n + j) * hw + p], cr = ycc[(2 * n + j) * hw + p];
    if (AFFINE) {
        s0 = (s0 - af.b[0]) * af.inv_a[0];
        cb = (cb - af.b[1]) * af.inv_a[1];
        cr = (cr - af.b[2]) * af.inv_a[2];
    }
    ycc_to_u16(s0, cb, cr, M, dst + ((b * h + ry) * w + rx) * 3);
}

// uint16 HWC RGB -> luma (1,n,1,th,tw) with Y-0.5 and chroma (2,n,1,th/2,tw/2) (Cb, Cr): k_u8hwc_to_ycc420_tiles on uint16.  Grid
// (cdiv(tw/2,256), th/2, n): one thread per chroma sample; its 2 x 2 pixels are each clamped to the image on their own.
template <bool GRID>
__global__ void k_u16hwc_to_ycc420_tiles(const uint16_t* __restrict__ src, float* __restrict__ luma, float* __restrict__ chroma,
                                         int64_t B, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t ny, int64_t nx,
                                         int64_t first, int64_t n, float M, uint32_t maxv, int32_t* __restrict__ flag) {
    const int64_t twc = tw >> 1, thc = th >> 1;
    const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (x >= twc) return;
    const int64_t i = blockIdx.y, j = blockIdx.z;
    int64_t b = first + j, oy = 0, ox = 0;
    if (GRID && !dp_tile_origin(first + j, B, th, tw, ny, nx, b, oy, ox)) return;
    DpYcc v[2][2];
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const int64_t gy = oy + 2 * i + dy, sy = gy < H ? gy : H - 1;
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int64_t gx = ox + 2 * x + dx, sx = gx < W ? gx : W - 1;
            v[dy][dx] = px16_to_ycc(src + ((b * H + sy) * W + sx) * 3, M, maxv, flag);
        }
    }
    float* l = luma + j * th * tw + (2 * i) * tw + 2 * x;                 // even offset: 8-byte aligned (the launcher checks)
    *reinterpret_cast<float2*>(l) = make_float2(v[0][0].y, v[0][1].y);
    *reinterpret_cast<float2*>(l + tw) = make_float2(v[1][0].y, v[1][1].y);
    const int64_t hwc = thc * twc, p = i * twc + x;
    chroma[(0 * n + j) * hwc + p] = __fmul_rn(__fadd_rn(__fadd_rn(v[0][0].cb, v[0][1].cb), __fadd_rn(v[1][0].cb, v[1][1].cb)), 0.25f);
    chroma[(1 * n + j) * hwc + p] = __fmul_rn(__fadd_rn(__fadd_rn(v[0][0].cr, v[0][1].cr), __fadd_rn(v[1][0].cr, v[1][1].cr)), 0.25f);
}

// The chroma value at tile pixel (y, x) from a chroma plane c of thc x twc: chroma.hip's up420, the same expressions.
template <bool AFFINE>
__device__ __forceinline__ float dp_up420(const float* __restrict__ c, int64_t thc, int64_t twc, int64_t y, int64_t x,
                                          float inv_a, float b) {
    const int64_t cy = y >> 1, cx = x >> 1;
    int64_t my = (y & 1) ? cy + 1 : cy - 1, mx = (x & 1) ? cx + 1 : cx - 1;
    my = my < 0 ? 0 : (my > thc - 1 ? thc - 1 : my);
    mx = mx < 0 ? 0 : (mx > twc - 1 ? twc - 1 : mx);
    float a00 = c[cy * twc + cx], a01 = c[cy * twc + mx], a10 = c[my * twc + cx], a11 = c[my * twc + mx];
    if (AFFINE) {
        a00 = (a00 - b) * inv_a;
        a01 = (a01 - b) * inv_a;
        a10 = (a10 - b) * inv_a;
        a11 = (a11 - b) * inv_a;
    }
    const float t0 = __fadd_rn(__fmul_rn(0.75f, a00), __fmul_rn(0.25f, a01));
    const float t1 = __fadd_rn(__fmul_rn(0.75f, a10), __fmul_rn(0.25f, a11));
    return __fadd_rn(__fmul_rn(0.75f, t0), __fmul_rn(0.25f, t1));
}

// luma (1,n,1,th,tw) and chroma (2,n,1,th/2,tw/2) of n tiles -> uint16 HWC RGB, dst (B,h,w,3): k_ycc420_tiles_to_u8hwc on uint16.
template <bool GRID, bool AFFINE>
__global__ void k_ycc420_tiles_to_u16hwc(const float* __restrict__ luma, const float* __restrict__ chroma,
                                         const int32_t* __restrict__ tiles, int64_t first, int64_t n, int64_t B, int64_t H,
                                         int64_t W, int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0, int64_t x0,
                                         int64_t h, int64_t w, uint16_t* __restrict__ dst, DpAffine af, float M) {
    int64_t b, ly, lx, ry, rx;
    if (!dp_out_pixel<GRID>(tiles, first, B, H, W, th, tw, ny, nx, y0, x0, h, w, b, ly, lx, ry, rx)) return;
    const int64_t j = blockIdx.z, thc = th >> 1, twc = tw >> 1, hwc = thc * twc;
    float s0 = luma[j * th * tw + ly * tw + lx];
    if (AFFINE) s0 = (s0 - af.b[0]) * af.inv_a[0];
    const float cb = dp_up420<AFFINE>(chroma + (0 * n + j) * hwc, thc, twc, ly, lx, af.inv_a[1], af.b[1]);
    const float cr = dp_up420<AFFINE>(chroma + (1 * n + j) * hwc, thc, twc, ly, lx, af.inv_a[2], af.b[2]);
    ycc_to_u16(s0, cb, cr, M, dst + ((b * h + ry) * w + rx) * 3);
}

// 4:0:0 input: uint16 (B,H,W,1) -> y (1,n,1,th,tw), v / M - 0.5f, for the tiles first .. first+n-1.  Grid (cdiv(tw,256), th, n).
template <bool GRID>
__global__ void k_u16hw_to_y_tiles(const uint16_t* __restrict__ src, float* __restrict__ y, int64_t B, int64_t H, int64_t W,
                                   int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t first, int64_t n, float M,
                                   uint32_t maxv, int32_t* __restrict__ flag) {
    const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (x >= tw) return;
    const int64_t ly = blockIdx.y, j = blockIdx.z;
    int64_t b = first + j, oy = 0, ox = 0;
    if (GRID && !dp_tile_origin(first + j, B, th, tw, ny, nx, b, oy, ox)) return;
    const int64_t gy = oy + ly, gx = ox + x;
    const int64_t sy = gy < H ? gy : H - 1, sx = gx < W ? gx : W - 1;
    const uint32_t v = src[(b * H + sy) * W + sx];
    if (v > maxv) *flag = 1;
    y[j * th * tw + ly * tw + x] = (float)v / M - 0.5f;
}

// 4:0:0 output: y (1,n,1,th,tw) -> uint16 (B,h,w,1), floor((clamp(s, -0.5, 0.5) + 0.5) * M + 0.5).  AFFINE: s -> (s - b[0]) *
// inv_a[0] first.
template <bool GRID, bool AFFINE>
__global__ void k_y_tiles_to_u16hw(const float* __restrict__ y, const int32_t* __restrict__ tiles, int64_t first, int64_t n,
                                   int64_t B, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0,
                                   int64_t x0, int64_t h, int64_t w, uint16_t* __restrict__ dst, DpAffine af, float M) {
    int64_t b, ly, lx, ry, rx;
    if (!dp_out_pixel<GRID>(tiles, first, B, H, W, th, tw, ny, nx, y0, x0, h, w, b, ly, lx, ry, rx)) return;
    float s = y[(int64_t)blockIdx.z * th * tw + ly * tw + lx];
    if (AFFINE) s = (s - af.b[0]) * af.inv_a[0];
    dst[(b * h + ry) * w + rx] = sample_u16(s, M);
}

// uint16 HWC image batch -> float NCHW in [0,1], v / M: k_u8hwc_to_f32chw on uint16 (codec.quality).  One thread per pixel.
__global__ void k_u16hwc_to_f32chw(const uint16_t* __restrict__ src, float* __restrict__ dst, int64_t B, int64_t hw, float M,
                                   uint32_t maxv, int32_t* __restrict__ flag) {
    const int64_t n = B * hw;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / hw, p = i - b * hw;
        const uint16_t* s = src + i * 3;
        const uint32_t r0 = s[0], g0 = s[1], b0 = s[2];
        if (r0 > maxv || g0 > maxv || b0 > maxv) *flag = 1;
        dst[(b * 3 + 0) * hw + p] = (float)r0 / M;
        dst[(b * 3 + 1) * hw + p] = (float)g0 / M;
        dst[(b * 3 + 2) * hw + p] = (float)b0 / M;
    }
}

// depth -> M = 2^depth - 1 as a float (exact: at most 16 bits) and as an integer; 8..16 at this level, always uint16 storage
static int depth_ok(const char* who, int depth, float* M, uint32_t* maxv) {
    LLDWT_REQUIRE(depth >= 8 && depth <= 16, "%s: depth %d is outside [8, 16]", who, depth);
    *maxv = (1u << depth) - 1u;
    *M = (float)*maxv;
    return LLDWT_OK;
}

// the argument checks the input entry points share (who: the name their messages carry)
static int dp_tiles_in_ok(const char* who, const void* src, int64_t B, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t ny,
                          int64_t nx, int64_t first, int64_t n, const int32_t* flag) {
    LLDWT_REQUIRE(B > 0 && H > 0 && W > 0 && th > 0 && tw > 0 && ny > 0 && nx > 0, "%s: bad arguments", who);
    LLDWT_REQUIRE(first >= 0 && n > 0 && first + n <= B * ny * nx, "%s: tile range [%lld, %lld) outside the %lld tiles", who,
                  (long long)first, (long long)(first + n), (long long)(B * ny * nx));
    LLDWT_REQUIRE(ny * th >= H && nx * tw >= W, "%s: the grid does not cover the image", who);
    LLDWT_REQUIRE(n <= 65535 && th <= 65535 && tw <= (1ll << 30) && B * ny * nx < (1ll << 31), "%s: grid too large", who);
    LLDWT_REQUIRE(((uintptr_t)src & 1) == 0 && ((uintptr_t)flag & 3) == 0, "%s: src must be 2-byte and flag 4-byte aligned", who);
    return LLDWT_OK;
}

// the argument checks the output entry points share; *grid: whether the tile-grid kernel form runs
static int dp_tiles_out_ok(const char* who, const int32_t* tiles, int64_t first, int64_t n, int64_t B, int64_t H, int64_t W,
                           int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0, int64_t x0, int64_t h, int64_t w,
                           const void* dst, bool* grid) {
    LLDWT_REQUIRE(B > 0 && H > 0 && W > 0 && th > 0 && tw > 0 && ny > 0 && nx > 0 && n > 0, "%s: bad arguments", who);
    LLDWT_REQUIRE(tiles || (first >= 0 && first + n <= B * ny * nx), "%s: tile range outside the grid", who);
    LLDWT_REQUIRE(y0 >= 0 && x0 >= 0 && h > 0 && w > 0 && y0 + h <= H && x0 + w <= W,
                  "%s: region (%lld, %lld, %lld, %lld) outside the %lld x %lld image", who, (long long)y0, (long long)x0,
                  (long long)h, (long long)w, (long long)H, (long long)W);
    LLDWT_REQUIRE(ny * th >= H && nx * tw >= W, "%s: the grid does not cover the image", who);
    *grid = ny * nx > 1 || tiles;
    LLDWT_REQUIRE(n <= 65535 && (*grid ? th : h) <= 65535 && tw <= (1ll << 30) && B * ny * nx < (1ll << 31),
                  "%s: grid too large", who);
    LLDWT_REQUIRE(((uintptr_t)dst & 1) == 0, "%s: dst must be 2-byte aligned", who);
    return LLDWT_OK;
}

// inv_a / b (count host floats each, both NULL: no map) -> af; *on: whether a map was given
static int dp_affine_arg(const char* who, const float* inv_a, const float* b, int count, DpAffine* af, bool* on) {
    LLDWT_REQUIRE(!inv_a == !b, "%s: inv_a and b must be given together", who);
    *on = inv_a != nullptr;
    for (int p = 0; p < 3; ++p) {
        af->inv_a[p] = 1.f;
        af->b[p] = 0.f;
    }
    for (int p = 0; *on && p < count; ++p) {
        LLDWT_REQUIRE(isfinite(inv_a[p]) && inv_a[p] != 0.f && isfinite(b[p]),
                      "%s: plane %d: inv_a = %g, b = %g (inv_a must be finite and non-zero, b finite)", who, p, (double)inv_a[p],
                      (double)b[p]);
        af->inv_a[p] = inv_a[p];
        af->b[p] = b[p];
    }
    return LLDWT_OK;
}

}  // namespace lldwt
using namespace lldwt;

// the four template forms of an output kernel K (GRID, AFFINE), launched on g with the arguments that follow
#define LLDWT_DP_LAUNCH_OUT(K, ...)                                                                       \
    do {                                                                                                  \
        if (grid && on) hipLaunchKernelGGL((K<true, true>), g, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);        \
        else if (grid) hipLaunchKernelGGL((K<true, false>), g, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);        \
        else if (on) hipLaunchKernelGGL((K<false, true>), g, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);          \
        else hipLaunchKernelGGL((K<false, false>), g, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);                 \
    } while (0)

extern "C" int lldwt_u16hwc_to_ycc_tiles(const void* src, float* ycc, int64_t B, int64_t H, int64_t W, int64_t th, int64_t tw,
                                         int64_t ny, int64_t nx, int64_t first, int64_t n, int depth, int32_t* flag,
                                         void* stream) {
    const char* who = "u16hwc_to_ycc_tiles";
    float M;
    uint32_t maxv;
    LLDWT_REQUIRE(src && ycc && flag, "%s: null pointer", who);
    if (const int rc = depth_ok(who, depth, &M, &maxv)) return rc;
    if (const int rc = dp_tiles_in_ok(who, src, B, H, W, th, tw, ny, nx, first, n, flag)) return rc;
    const dim3 g((unsigned)cdiv(tw, 256), (unsigned)th, (unsigned)n);
    const uint16_t* s = (const uint16_t*)src;
    if (ny * nx > 1)
        hipLaunchKernelGGL(k_u16hwc_to_ycc_tiles<true>, g, dim3(256), 0, (hipStream_t)stream, s, ycc, B, H, W, th, tw, ny, nx,
                           first, n, M, maxv, flag);
    else
        hipLaunchKernelGGL(k_u16hwc_to_ycc_tiles<false>, g, dim3(256), 0, (hipStream_t)stream, s, ycc, B, H, W, th, tw, ny, nx,
                           first, n, M, maxv, flag);
    return check_launch(who);
}

extern "C" int lldwt_ycc_tiles_to_u16hwc(const float* ycc, const int32_t* tiles, int64_t first, int64_t n, int64_t B, int64_t H,
                                         int64_t W, int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0, int64_t x0,
                                         int64_t h, int64_t w, const float* inv_a, const float* b, int depth, void* dst,
                                         void* stream) {
    const char* who = "ycc_tiles_to_u16hwc";
    float M;
    uint32_t maxv;
    bool grid, on;
    DpAffine af;
    LLDWT_REQUIRE(ycc && dst, "%s: null pointer", who);
    if (const int rc = depth_ok(who, depth, &M, &maxv)) return rc;
    if (const int rc = dp_tiles_out_ok(who, tiles, first, n, B, H, W, th, tw, ny, nx, y0, x0, h, w, dst, &grid)) return rc;
    if (const int rc = dp_affine_arg(who, inv_a, b, 3, &af, &on)) return rc;
    const dim3 g((unsigned)cdiv(grid ? tw : w, 256), (unsigned)(grid ? th : h), (unsigned)n);
    LLDWT_DP_LAUNCH_OUT(k_ycc_tiles_to_u16hwc, ycc, tiles, first, n, B, H, W, th, tw, ny, nx, y0, x0, h, w, (uint16_t*)dst, af, M);
    return check_launch(who);
}

extern "C" int lldwt_u16hwc_to_ycc420_tiles(const void* src, float* luma, float* chroma, int64_t B, int64_t H, int64_t W,
                                            int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t first, int64_t n, int depth,
                                            int32_t* flag, void* stream) {
    const char* who = "u16hwc_to_ycc420_tiles";
    float M;
    uint32_t maxv;
    LLDWT_REQUIRE(src && luma && chroma && flag, "%s: null pointer", who);
    if (const int rc = depth_ok(who, depth, &M, &maxv)) return rc;
    if (const int rc = dp_tiles_in_ok(who, src, B, H, W, th, tw, ny, nx, first, n, flag)) return rc;
    LLDWT_REQUIRE(th % 2 == 0 && tw % 2 == 0, "%s: a 4:2:0 tile needs even sides (got %lld x %lld)", who, (long long)th,
                  (long long)tw);
    LLDWT_REQUIRE(((uintptr_t)luma & 7) == 0, "%s: luma must be 8-byte aligned", who);
    const dim3 g((unsigned)cdiv(tw / 2, 256), (unsigned)(th / 2), (unsigned)n);
    const uint16_t* s = (const uint16_t*)src;
    if (ny * nx > 1)
        hipLaunchKernelGGL(k_u16hwc_to_ycc420_tiles<true>, g, dim3(256), 0, (hipStream_t)stream, s, luma, chroma, B, H, W, th, tw,
                           ny, nx, first, n, M, maxv, flag);
    else
        hipLaunchKernelGGL(k_u16hwc_to_ycc420_tiles<false>, g, dim3(256), 0, (hipStream_t)stream, s, luma, chroma, B, H, W, th, tw,
                           ny, nx, first, n, M, maxv, flag);
    return check_launch(who);
}

extern "C" int lldwt_ycc420_tiles_to_u16hwc(const float* luma, const float* chroma, const int32_t* tiles, int64_t first, int64_t n,
                                            int64_t B, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t ny, int64_t nx,
                                            int64_t y0, int64_t x0, int64_t h, int64_t w, const float* inv_a, const float* b,
                                            int depth, void* dst, void* stream) {
    const char* who = "ycc420_tiles_to_u16hwc";
    float M;
    uint32_t maxv;
    bool grid, on;
    DpAffine af;
    LLDWT_REQUIRE(luma && chroma && dst, "%s: null pointer", who);
    if (const int rc = depth_ok(who, depth, &M, &maxv)) return rc;
    if (const int rc = dp_tiles_out_ok(who, tiles, first, n, B, H, W, th, tw, ny, nx, y0, x0, h, w, dst, &grid)) return rc;
    LLDWT_REQUIRE(th % 2 == 0 && tw % 2 == 0, "%s: a 4:2:0 tile needs even sides (got %lld x %lld)", who, (long long)th,
                  (long long)tw);
    if (const int rc = dp_affine_arg(who, inv_a, b, 3, &af, &on)) return rc;
    const dim3 g((unsigned)cdiv(grid ? tw : w, 256), (unsigned)(grid ? th : h), (unsigned)n);
    LLDWT_DP_LAUNCH_OUT(k_ycc420_tiles_to_u16hwc, luma, chroma, tiles, first, n, B, H, W, th, tw, ny, nx, y0, x0, h, w,
                        (uint16_t*)dst, af, M);
    return check_launch(who);
}

extern "C" int lldwt_u16hw_to_y_tiles(const void* src, float* y, int64_t B, int64_t H, int64_t W, int64_t th, int64_t tw,
                                      int64_t ny, int64_t nx, int64_t first, int64_t n, int depth, int32_t* flag, void* stream) {
    const char* who = "u16hw_to_y_tiles";
    float M;
    uint32_t maxv;
    LLDWT_REQUIRE(src && y && flag, "%s: null pointer", who);
    if (const int rc = depth_ok(who, depth, &M, &maxv)) return rc;
    if (const int rc = dp_tiles_in_ok(who, src, B, H, W, th, tw, ny, nx, first, n, flag)) return rc;
    const dim3 g((unsigned)cdiv(tw, 256), (unsigned)th, (unsigned)n);
    const uint16_t* s = (const uint16_t*)src;
    if (ny * nx > 1)
        hipLaunchKernelGGL(k_u16hw_to_y_tiles<true>, g, dim3(256), 0, (hipStream_t)stream, s, y, B, H, W, th, tw, ny, nx, first,
                           n, M, maxv, flag);
    else
        hipLaunchKernelGGL(k_u16hw_to_y_tiles<false>, g, dim3(256), 0, (hipStream_t)stream, s, y, B, H, W, th, tw, ny, nx, first,
                           n, M, maxv, flag);
    return check_launch(who);
}

extern "C" int lldwt_y_tiles_to_u16hw(const float* y, const int32_t* tiles, int64_t first, int64_t n, int64_t B, int64_t H,
                                      int64_t W, int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0, int64_t x0, int64_t h,
                                      int64_t w, const float* inv_a, const float* b, int depth, void* dst, void* stream) {
    const char* who = "y_tiles_to_u16hw";
    float M;
    uint32_t maxv;
    bool grid, on;
    DpAffine af;
    LLDWT_REQUIRE(y && dst, "%s: null pointer", who);
    if (const int rc = depth_ok(who, depth, &M, &maxv)) return rc;
    if (const int rc = dp_tiles_out_ok(who, tiles, first, n, B, H, W, th, tw, ny, nx, y0, x0, h, w, dst, &grid)) return rc;
    if (const int rc = dp_affine_arg(who, inv_a, b, 1, &af, &on)) return rc;
    const dim3 g((unsigned)cdiv(grid ? tw : w, 256), (unsigned)(grid ? th : h), (unsigned)n);
    LLDWT_DP_LAUNCH_OUT(k_y_tiles_to_u16hw, y, tiles, first, n, B, H, W, th, tw, ny, nx, y0, x0, h, w, (uint16_t*)dst, af, M);
    return check_launch(who);
}

extern "C" int lldwt_u16hwc_to_f32chw(const void* src, float* dst, int64_t B, int64_t H, int64_t W, int depth, int32_t* flag,
                                      void* stream) {
    const char* who = "u16hwc_to_f32chw";
    float M;
    uint32_t maxv;
    LLDWT_REQUIRE(src && dst && flag && B > 0 && H > 0 && W > 0, "%s: bad arguments", who);
    if (const int rc = depth_ok(who, depth, &M, &maxv)) return rc;
    LLDWT_REQUIRE(((uintptr_t)src & 1) == 0 && ((uintptr_t)flag & 3) == 0, "%s: src must be 2-byte and flag 4-byte aligned", who);
    const int64_t blocks = cdiv(B * H * W, 256);
    hipLaunchKernelGGL(k_u16hwc_to_f32chw, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t*)src, dst, B, H * W, M, maxv, flag);
    return check_launch(who);
}
