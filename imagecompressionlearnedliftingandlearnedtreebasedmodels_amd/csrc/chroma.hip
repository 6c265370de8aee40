// chroma.hip -- image codec I/O for the chroma formats 4:2:0 and 4:0:0 (codec.py chroma=) for gfx950.
// The 4:4:4 kernels of ops.hip (k_u8hwc_to_ycc_tiles, k_ycc_tiles_to_u8hwc) are not touched; these are their siblings on the
// same tile grid: tile t = (b * ny + ty) * nx + tx of th x tw covers rows [ty*th, (ty+1)*th) and columns [tx*tw, (tx+1)*tw),
// positions past the image take the clamped source pixel.  A 4:2:0 tile is a luma plane of th x tw and two chroma planes of
// th/2 x tw/2 (th, tw even); a 4:0:0 tile is one plane.  All four kernels are bandwidth-bound: one pass, every plane row
// written coalesced, the full-size chroma never exists in memory.
#include "common.h"
#include <math.h>

namespace lldwt {

// BT.709, the constants and expressions of ops.hip's colour kernels (the file is compiled with -ffp-contract=off like it)
constexpr float CH_KR = 0.2126f, CH_KG = 0.7152f, CH_KB = 0.0722f;

struct Ycc {
    float y, cb, cr;
};

// One source pixel -> (Y - 0.5, Cb, Cr): the expressions of k_u8hwc_to_ycc_tiles, bit for bit.
__device__ __forceinline__ Ycc px_to_ycc(const uint8_t* __restrict__ s) {
    const float rr = (float)s[0] / 255.0f, g = (float)s[1] / 255.0f, bl = (float)s[2] / 255.0f;
    const float yy = CH_KR * rr + CH_KG * g + CH_KB * bl;
    Ycc v;
    v.cb = 0.5f * (bl - yy) / (1.f - CH_KB) + 0.5f;
    v.cr = 0.5f * (rr - yy) / (1.f - CH_KR) + 0.5f;
    v.y = yy - 0.5f;
    return v;
}

// (Y - 0.5, Cb, Cr) -> 3 bytes of uint8 RGB: the expressions of ops.hip's ycc_vals_u8 without its affine map, bit for bit
// (tests/test_gpu_codec_chroma.py holds the two kernels' bytes to each other).
__device__ __forceinline__ void ycc_to_u8(float s0, float cb, float cr, uint8_t* __restrict__ d) {
    const float y = s0 + 0.5f;
    float rr = y + (2.f - 2.f * CH_KR) * (cr - 0.5f);
    float bl = y + (2.f - 2.f * CH_KB) * (cb - 0.5f);
    float g = (y - CH_KR * rr - CH_KB * bl) / CH_KG;
    rr -= 0.5f; g -= 0.5f; bl -= 0.5f;
    rr = fminf(fmaxf(rr, -0.5f), 0.5f);
    g = fminf(fmaxf(g, -0.5f), 0.5f);
    bl = fminf(fmaxf(bl, -0.5f), 0.5f);
    d[0] = (uint8_t)floorf((rr + 0.5f) * 255.0f + 0.5f);
    d[1] = (uint8_t)floorf((g + 0.5f) * 255.0f + 0.5f);
    d[2] = (uint8_t)floorf((bl + 0.5f) * 255.0f + 0.5f);
}

// Per-plane affine map of a reduced-resolution decode (ops.hip's LLAffine): s -> (s - b[p]) * inv_a[p].  on == 0: none.
struct ChAffine {
    float inv_a[3], b[3];
};

// tile number (first + j, or tiles[j]) -> image b and tile origin (oy, ox); false when the index is outside the grid
__device__ __forceinline__ bool tile_origin(int64_t t, int64_t B, int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t& b,
                                            int64_t& oy, int64_t& ox) {
    if (t < 0 || t >= B * ny * nx) return false;
    const uint32_t per = (uint32_t)(ny * nx), b32 = (uint32_t)t / per, r = (uint32_t)t - b32 * per;   // the launcher bounds B*ny*nx
    const uint32_t ty = r / (uint32_t)nx, tx = r - ty * (uint32_t)nx;
    b = b32;
    oy = (int64_t)ty * th;
    ox = (int64_t)tx * tw;
    return true;
}

// uint8 HWC RGB -> luma (1,n,1,th,tw) with Y-0.5 and chroma (2,n,1,th/2,tw/2) (Cb, Cr) for the tiles first .. first+n-1.
// Grid (cdiv(tw/2,256), th/2, n): one thread per chroma sample (i, x).  It converts its 2 x 2 pixels (each clamped to the image
// on its own, so an odd H or W clamps inside the block), writes the four Y as two float2 (each luma row coalesced) and
// ((c00 + c01) + (c10 + c11)) * 0.25f per chroma plane, every add separately rounded.  GRID = false: the 1 x 1 grid.
template <bool GRID>
__global__ void k_u8hwc_to_ycc420_tiles(const uint8_t* __restrict__ src, float* __restrict__ luma, float* __restrict__ chroma,
                                        int64_t B, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t ny, int64_t nx,
                                        int64_t first, int64_t n) {
    const int64_t twc = tw >> 1, thc = th >> 1;
    const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (x >= twc) return;
    const int64_t i = blockIdx.y, j = blockIdx.z;
    int64_t b = first + j, oy = 0, ox = 0;
    if (GRID && !tile_origin(first + j, B, th, tw, ny, nx, b, oy, ox)) return;
    Ycc v[2][2];
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const int64_t gy = oy + 2 * i + dy, sy = gy < H ? gy : H - 1;
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int64_t gx = ox + 2 * x + dx, sx = gx < W ? gx : W - 1;
            v[dy][dx] = px_to_ycc(src + ((b * H + sy) * W + sx) * 3);
        }
    }
    float* l = luma + j * th * tw + (2 * i) * tw + 2 * x;                 // even offset: 8-byte aligned (the launcher checks)
    *reinterpret_cast<float2*>(l) = make_float2(v[0][0].y, v[0][1].y);
    *reinterpret_cast<float2*>(l + tw) = make_float2(v[1][0].y, v[1][1].y);
    const int64_t hwc = thc * twc, p = i * twc + x;
    chroma[(0 * n + j) * hwc + p] = __fmul_rn(__fadd_rn(__fadd_rn(v[0][0].cb, v[0][1].cb), __fadd_rn(v[1][0].cb, v[1][1].cb)), 0.25f);
    chroma[(1 * n + j) * hwc + p] = __fmul_rn(__fadd_rn(__fadd_rn(v[0][0].cr, v[0][1].cr), __fadd_rn(v[1][0].cr, v[1][1].cr)), 0.25f);
}

// The chroma value at tile pixel (y, x) from a chroma plane c of thc x twc: the bilinear 4:2:0 upsampling of DESIGN.md 7.1.11
// with the co-sited-in-the-middle phase (weights 3/4 and 1/4 toward the nearer and the farther sample), clamped at the tile's
// own plane.  Every product and sum separately rounded.  AFFINE: each sample goes through (s - b) * inv_a first.
template <bool AFFINE>
__device__ __forceinline__ float up420(const float* __restrict__ c, int64_t thc, int64_t twc, int64_t y, int64_t x, float inv_a,
                                       float b) {
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

// luma (1,n,1,th,tw) and chroma (2,n,1,th/2,tw/2) of n tiles (tile of slot j: tiles[j], or first + j when tiles is null) ->
// uint8 HWC RGB of the pixels inside the image and inside the region [y0, y0+h) x [x0, x0+w), written to dst (B,h,w,3) at the
// image of the tile: the region and in-image tests of k_ycc_tiles_to_u8hwc.  One thread per output pixel; the four chroma
// samples it blends are shared with its neighbours through the cache, so the kernel reads 4 + 2 * 4 / 4 bytes per pixel from
// memory.  GRID = true: grid (cdiv(tw,256), th, n).  GRID = false: the 1 x 1 grid (tile = image, tiles == NULL): grid
// (cdiv(w,256), h, n), one thread per region pixel.
template <bool GRID, bool AFFINE>
__global__ void k_ycc420_tiles_to_u8hwc(const float* __restrict__ luma, const float* __restrict__ chroma,
                                        const int32_t* __restrict__ tiles, int64_t first, int64_t n, int64_t B, int64_t H,
                                        int64_t W, int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0, int64_t x0,
                                        int64_t h, int64_t w, uint8_t* __restrict__ dst, ChAffine af) {
    const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, j = blockIdx.z;
    const int64_t thc = th >> 1, twc = tw >> 1, hwc = thc * twc;
    int64_t b, ly, lx, ry, rx;                     // image, pixel in the tile, pixel in the region
    if (!GRID) {
        if (x >= w) return;
        b = first + j;
        ry = blockIdx.y;
        rx = x;
        ly = y0 + ry;
        lx = x0 + x;
    } else {
        if (x >= tw) return;
        int64_t oy, ox;
        if (!tile_origin(tiles ? (int64_t)tiles[j] : first + j, B, th, tw, ny, nx, b, oy, ox)) return;
        ly = blockIdx.y;
        lx = x;
        const int64_t gy = oy + ly, gx = ox + lx;
        if (gy >= H || gx >= W || gy < y0 || gy >= y0 + h || gx < x0 || gx >= x0 + w) return;
        ry = gy - y0;
        rx = gx - x0;
    }
    float s0 = luma[j * th * tw + ly * tw + lx];
    if (AFFINE) s0 = (s0 - af.b[0]) * af.inv_a[0];
    const float cb = up420<AFFINE>(chroma + (0 * n + j) * hwc, thc, twc, ly, lx, af.inv_a[1], af.b[1]);
    const float cr = up420<AFFINE>(chroma + (1 * n + j) * hwc, thc, twc, ly, lx, af.inv_a[2], af.b[2]);
    ycc_to_u8(s0, cb, cr, dst + ((b * h + ry) * w + rx) * 3);
}

// 4:0:0 input: uint8 (B,H,W,1) -> y (1,n,1,th,tw), g / 255.0f - 0.5f, for the tiles first .. first+n-1.  Grid (cdiv(tw,256), th, n).
template <bool GRID>
__global__ void k_u8hw_to_y_tiles(const uint8_t* __restrict__ src, float* __restrict__ y, int64_t B, int64_t H, int64_t W,
                                  int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t first, int64_t n) {
    const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (x >= tw) return;
    const int64_t ly = blockIdx.y, j = blockIdx.z;
    int64_t b = first + j, oy = 0, ox = 0;
    if (GRID && !tile_origin(first + j, B, th, tw, ny, nx, b, oy, ox)) return;
    const int64_t gy = oy + ly, gx = ox + x;
    const int64_t sy = gy < H ? gy : H - 1, sx = gx < W ? gx : W - 1;
    y[j * th * tw + ly * tw + x] = (float)src[(b * H + sy) * W + sx] / 255.0f - 0.5f;
}

// 4:0:0 output: y (1,n,1,th,tw) -> uint8 (B,h,w,1), floor((clamp(s, -0.5, 0.5) + 0.5) * 255 + 0.5), with the tile list, region
// and in-image tests of k_ycc420_tiles_to_u8hwc.  AFFINE: s -> (s - b[0]) * inv_a[0] first.
template <bool GRID, bool AFFINE>
__global__ void k_y_tiles_to_u8hw(const float* __restrict__ y, const int32_t* __restrict__ tiles, int64_t first, int64_t n,
                                  int64_t B, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0,
                                  int64_t x0, int64_t h, int64_t w, uint8_t* __restrict__ dst, ChAffine af) {
    const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, j = blockIdx.z;
    int64_t b, ly, lx, ry, rx;
    if (!GRID) {
        if (x >= w) return;
        b = first + j;
        ry = blockIdx.y;
        rx = x;
        ly = y0 + ry;
        lx = x0 + x;
    } else {
        if (x >= tw) return;
        int64_t oy, ox;
        if (!tile_origin(tiles ? (int64_t)tiles[j] : first + j, B, th, tw, ny, nx, b, oy, ox)) return;
        ly = blockIdx.y;
        lx = x;
        const int64_t gy = oy + ly, gx = ox + lx;
        if (gy >= H || gx >= W || gy < y0 || gy >= y0 + h || gx < x0 || gx >= x0 + w) return;
        ry = gy - y0;
        rx = gx - x0;
    }
    float s = y[j * th * tw + ly * tw + lx];
    if (AFFINE) s = (s - af.b[0]) * af.inv_a[0];
    s = fminf(fmaxf(s, -0.5f), 0.5f);
    dst[(b * h + ry) * w + rx] = (uint8_t)floorf((s + 0.5f) * 255.0f + 0.5f);
}

// the argument checks the two input entry points share (who: the name their messages carry)
static int tiles_in_ok(const char* who, int64_t B, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t ny, int64_t nx,
                       int64_t first, int64_t n) {
    LLDWT_REQUIRE(B > 0 && H > 0 && W > 0 && th > 0 && tw > 0 && ny > 0 && nx > 0, "%s: bad arguments", who);
    LLDWT_REQUIRE(first >= 0 && n > 0 && first + n <= B * ny * nx, "%s: tile range [%lld, %lld) outside the %lld tiles", who,
                  (long long)first, (long long)(first + n), (long long)(B * ny * nx));
    LLDWT_REQUIRE(ny * th >= H && nx * tw >= W, "%s: the grid does not cover the image", who);
    LLDWT_REQUIRE(n <= 65535 && th <= 65535 && tw <= (1ll << 30) && B * ny * nx < (1ll << 31), "%s: grid too large", who);
    return LLDWT_OK;
}

// the argument checks the two output entry points share; *grid: whether the tile-grid kernel form runs
static int tiles_out_ok(const char* who, const int32_t* tiles, int64_t first, int64_t n, int64_t B, int64_t H, int64_t W,
                        int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0, int64_t x0, int64_t h, int64_t w,
                        bool* grid) {
    LLDWT_REQUIRE(B > 0 && H > 0 && W > 0 && th > 0 && tw > 0 && ny > 0 && nx > 0 && n > 0, "%s: bad arguments", who);
    LLDWT_REQUIRE(tiles || (first >= 0 && first + n <= B * ny * nx), "%s: tile range outside the grid", who);
    LLDWT_REQUIRE(y0 >= 0 && x0 >= 0 && h > 0 && w > 0 && y0 + h <= H && x0 + w <= W,
                  "%s: region (%lld, %lld, %lld, %lld) outside the %lld x %lld image", who, (long long)y0, (long long)x0,
                  (long long)h, (long long)w, (long long)H, (long long)W);
    LLDWT_REQUIRE(ny * th >= H && nx * tw >= W, "%s: the grid does not cover the image", who);
    *grid = ny * nx > 1 || tiles;
    LLDWT_REQUIRE(n <= 65535 && (*grid ? th : h) <= 65535 && tw <= (1ll << 30) && B * ny * nx < (1ll << 31),
                  "%s: grid too large", who);
    return LLDWT_OK;
}

// inv_a / b (count host floats each, both NULL: no map) -> af; *on: whether a map was given
static int affine_arg(const char* who, const float* inv_a, const float* b, int count, ChAffine* af, bool* on) {
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

extern "C" int lldwt_u8hwc_to_ycc420_tiles(const uint8_t* src, float* luma, float* chroma, int64_t B, int64_t H, int64_t W,
                                           int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t first, int64_t n,
                                           void* stream) {
    const char* who = "u8hwc_to_ycc420_tiles";
    LLDWT_REQUIRE(src && luma && chroma, "%s: null pointer", who);
    if (const int rc = tiles_in_ok(who, B, H, W, th, tw, ny, nx, first, n)) return rc;
    LLDWT_REQUIRE(th % 2 == 0 && tw % 2 == 0, "%s: a 4:2:0 tile needs even sides (got %lld x %lld)", who, (long long)th,
                  (long long)tw);
    LLDWT_REQUIRE(((uintptr_t)luma & 7) == 0, "%s: luma must be 8-byte aligned", who);
    const dim3 g((unsigned)cdiv(tw / 2, 256), (unsigned)(th / 2), (unsigned)n);
    if (ny * nx > 1)
        hipLaunchKernelGGL(k_u8hwc_to_ycc420_tiles<true>, g, dim3(256), 0, (hipStream_t)stream, src, luma, chroma, B, H, W, th,
                           tw, ny, nx, first, n);
    else
        hipLaunchKernelGGL(k_u8hwc_to_ycc420_tiles<false>, g, dim3(256), 0, (hipStream_t)stream, src, luma, chroma, B, H, W, th,
                           tw, ny, nx, first, n);
    return check_launch(who);
}

extern "C" int lldwt_ycc420_tiles_to_u8hwc(const float* luma, const float* chroma, const int32_t* tiles, int64_t first, int64_t n,
                                           int64_t B, int64_t H, int64_t W, int64_t th, int64_t tw, int64_t ny, int64_t nx,
                                           int64_t y0, int64_t x0, int64_t h, int64_t w, const float* inv_a, const float* b,
                                           uint8_t* dst, void* stream) {
    const char* who = "ycc420_tiles_to_u8hwc";
    LLDWT_REQUIRE(luma && chroma && dst, "%s: null pointer", who);
    bool grid, on;
    ChAffine af;
    if (const int rc = tiles_out_ok(who, tiles, first, n, B, H, W, th, tw, ny, nx, y0, x0, h, w, &grid)) return rc;
    LLDWT_REQUIRE(th % 2 == 0 && tw % 2 == 0, "%s: a 4:2:0 tile needs even sides (got %lld x %lld)", who, (long long)th,
                  (long long)tw);
    if (const int rc = affine_arg(who, inv_a, b, 3, &af, &on)) return rc;
    const dim3 g((unsigned)cdiv(grid ? tw : w, 256), (unsigned)(grid ? th : h), (unsigned)n);
#define LLDWT_CH_LAUNCH(G, A)                                                                                                  \
    hipLaunchKernelGGL((k_ycc420_tiles_to_u8hwc<G, A>), g, dim3(256), 0, (hipStream_t)stream, luma, chroma, tiles, first, n, B, \
                       H, W, th, tw, ny, nx, y0, x0, h, w, dst, af)
    if (grid && on) LLDWT_CH_LAUNCH(true, true);
    else if (grid) LLDWT_CH_LAUNCH(true, false);
    else if (on) LLDWT_CH_LAUNCH(false, true);
    else LLDWT_CH_LAUNCH(false, false);
#undef LLDWT_CH_LAUNCH
    return check_launch(who);
}

extern "C" int lldwt_u8hw_to_y_tiles(const uint8_t* src, float* y, int64_t B, int64_t H, int64_t W, int64_t th, int64_t tw,
                                     int64_t ny, int64_t nx, int64_t first, int64_t n, void* stream) {
    const char* who = "u8hw_to_y_tiles";
    LLDWT_REQUIRE(src && y, "%s: null pointer", who);
    if (const int rc = tiles_in_ok(who, B, H, W, th, tw, ny, nx, first, n)) return rc;
    const dim3 g((unsigned)cdiv(tw, 256), (unsigned)th, (unsigned)n);
    if (ny * nx > 1)
        hipLaunchKernelGGL(k_u8hw_to_y_tiles<true>, g, dim3(256), 0, (hipStream_t)stream, src, y, B, H, W, th, tw, ny, nx, first,
                           n);
    else
        hipLaunchKernelGGL(k_u8hw_to_y_tiles<false>, g, dim3(256), 0, (hipStream_t)stream, src, y, B, H, W, th, tw, ny, nx, first,
                           n);
    return check_launch(who);
}

extern "C" int lldwt_y_tiles_to_u8hw(const float* y, const int32_t* tiles, int64_t first, int64_t n, int64_t B, int64_t H,
                                     int64_t W, int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0, int64_t x0, int64_t h,
                                     int64_t w, const float* inv_a, const float* b, uint8_t* dst, void* stream) {
    const char* who = "y_tiles_to_u8hw";
    LLDWT_REQUIRE(y && dst, "%s: null pointer", who);
    bool grid, on;
    ChAffine af;
    if (const int rc = tiles_out_ok(who, tiles, first, n, B, H, W, th, tw, ny, nx, y0, x0, h, w, &grid)) return rc;
    if (const int rc = affine_arg(who, inv_a, b, 1, &af, &on)) return rc;
    const dim3 g((unsigned)cdiv(grid ? tw : w, 256), (unsigned)(grid ? th : h), (unsigned)n);
#define LLDWT_Y_LAUNCH(G, A)                                                                                                  \
    hipLaunchKernelGGL((k_y_tiles_to_u8hw<G, A>), g, dim3(256), 0, (hipStream_t)stream, y, tiles, first, n, B, H, W, th, tw, ny, \
                       nx, y0, x0, h, w, dst, af)
    if (grid && on) LLDWT_Y_LAUNCH(true, true);
    else if (grid) LLDWT_Y_LAUNCH(true, false);
    else if (on) LLDWT_Y_LAUNCH(false, true);
    else LLDWT_Y_LAUNCH(false, false);
#undef LLDWT_Y_LAUNCH
    return check_launch(who);
}
