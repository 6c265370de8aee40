// residual.hip -- the residual layer of the codec: lossless / near-lossless coding on top of the decoded
// base image.  Three kernels over "units": a unit is the in-image rectangle uh x uw of one tile of the tile grid of ops.hip
// (tile t = (b * ny + ty) * nx + tx covers rows [ty*th, min((ty+1)*th, H)) and columns [tx*tw, min((tx+1)*tw, W)); the
// untiled codec is the 1 x 1 grid).  All image buffers are uint8 HWC (B,h,w,3) holding the region [y0, y0+h) x [x0, x0+w)
// of every image; a launch handles the n units tiles[0..n) (first + j when tiles is null), which must all have the rectangle
// size (uh, uw) and lie inside the region -- a unit that does not writes nothing.
//
// Per pixel and channel c, with d the near-lossless bound (0 = lossless), xh the base reconstruction and x the original:
//   residual symbol   q = sign(r) * ((|r| + d) / (2d + 1)),  r = x - xh,  |q| <= Q = (255 + d) / (2d + 1)
//   context id        c * 8 + a,  a = 0 if g == 0 else min(7, 1 + floor(log2 g)),
//                     g = |xh[y, x+1] - xh[y, x-1]| + |xh[y+1, x] - xh[y-1, x]|, neighbour coordinates clamped to the unit
//   output            clamp(xh + q * (2d + 1), 0, 255)
//   checksum          sum_i (byte_i + 1) * (1 + i mod 65521) mod 2^64 over the unit's bytes in HWC raster order
// Symbols, context ids and table indexes are (3 n_units, uh*uw) int32, stream z = 3 j + c, in raster order over the unit:
// the layout both range coders take.
//
// Launch shape: grid (strips, n), 256 threads; a block walks `rows` consecutive rows of its unit with a flat pixel index,
// so a block covers thousands of pixels whatever the unit's width, and its histogram (LDS) and checksum partials reach
// global memory through a few integer atomics per block -- integer sums, so the result does not depend on their order.
// The kernels move 6 (contexts, apply) to 9 (analyse) bytes of image and 12 to 24 bytes of int32 per pixel and do no
// floating point.  Unit rows start at arbitrary byte offsets of the HWC buffers, so the image bytes are read one at a time
// (a wave's 64 pixels are 192 consecutive bytes); the int32 rows are written one dword per lane, consecutive per stream.
#include "common.h"

using namespace lldwt;

namespace {

constexpr int kThreads = 256;
constexpr int kClasses = 8;
constexpr int kContexts = 3 * kClasses;
constexpr uint32_t kCsMod = 65521u;

struct Geo {
    uint32_t B, H, W, th, tw, ny, nx, y0, x0, h, w, uh, uw, rows;
    int64_t first;
};

// The unit of slot j (block-uniform).  false: the tile is outside the grid, its rectangle is not uh x uw or it is not
// inside the region.  base: byte offset of the unit's first pixel in a (B,h,w,3) region buffer.
__device__ __forceinline__ bool unit_of(const Geo& g, const int32_t* __restrict__ tiles, uint32_t j, int64_t& base) {
    const int64_t t = tiles ? (int64_t)tiles[j] : g.first + (int64_t)j;
    if (t < 0 || t >= (int64_t)g.B * g.ny * g.nx) return false;
    const uint32_t per = g.ny * g.nx, b = (uint32_t)t / per, r = (uint32_t)t - b * per, ty = r / g.nx, tx = r - ty * g.nx;
    const uint32_t uy0 = ty * g.th, ux0 = tx * g.tw;
    if (uy0 >= g.H || ux0 >= g.W) return false;
    const uint32_t uh = min(g.th, g.H - uy0), uw = min(g.tw, g.W - ux0);
    if (uh != g.uh || uw != g.uw) return false;
    if (uy0 < g.y0 || ux0 < g.x0 || uy0 + uh > g.y0 + g.h || ux0 + uw > g.x0 + g.w) return false;
    base = (((int64_t)b * g.h + (uy0 - g.y0)) * g.w + (ux0 - g.x0)) * 3;
    return true;
}

// activity class of channel c at (ly, lx) of the unit at p (row stride rs bytes); neighbours clamped to the unit
__device__ __forceinline__ uint32_t activity(const uint8_t* __restrict__ p, uint32_t rs, uint32_t ly, uint32_t lx, uint32_t uh,
                                             uint32_t uw, uint32_t c) {
    const uint32_t xm = lx ? lx - 1 : 0, xp = lx + 1 < uw ? lx + 1 : uw - 1, ym = ly ? ly - 1 : 0, yp = ly + 1 < uh ? ly + 1 : uh - 1;
    const int dh = (int)p[ly * rs + xp * 3 + c] - (int)p[ly * rs + xm * 3 + c];
    const int dv = (int)p[yp * rs + lx * 3 + c] - (int)p[ym * rs + lx * 3 + c];
    const uint32_t g = (uint32_t)(dh < 0 ? -dh : dh) + (uint32_t)(dv < 0 ? -dv : dv);
    const uint32_t a = 32u - (uint32_t)__clz((int)g);                // 0 for g == 0, else 1 + floor(log2 g)
    return a < kClasses - 1 ? a : kClasses - 1;
}

__device__ __forceinline__ uint64_t cs_term(uint32_t byte, uint32_t i) { return (uint64_t)(byte + 1u) * (uint64_t)(1u + i % kCsMod); }

// block sum of a 64-bit partial -> one atomic add by thread 0 (red: kThreads / 64 words of LDS)
__device__ __forceinline__ void block_add_u64(uint64_t v, uint64_t* red, unsigned long long* dst) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down((unsigned long long)v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t s = 0;
        for (int k = 0; k < kThreads / 64; ++k) s += red[k];
        atomicAdd(dst, (unsigned long long)s);
    }
    __syncthreads();
}

// Encoder.  sym / ctx: (3 n, uh*uw) int32; hist: (n, 3, 8, 2Q+1) int32 and cs_xh / cs_x: (n) u64, all zero on entry.
// Dynamic LDS: 24 * (2Q+1) ints, the block's private histogram.
__global__ __launch_bounds__(kThreads) void k_resid_analyse(const uint8_t* __restrict__ x, const uint8_t* __restrict__ xh,
                                                            const int32_t* __restrict__ tiles, Geo g, uint32_t d, uint32_t Q,
                                                            int32_t* __restrict__ sym, int32_t* __restrict__ ctx,
                                                            int32_t* __restrict__ hist, unsigned long long* cs_xh,
                                                            unsigned long long* cs_x) {
    extern __shared__ int32_t lh[];
    __shared__ uint64_t red[kThreads / 64];
    const uint32_t j = blockIdx.y, bins = 2 * Q + 1, nh = kContexts * bins;
    int64_t base;
    if (!unit_of(g, tiles, j, base)) return;                        // block-uniform
    for (uint32_t i = threadIdx.x; i < nh; i += kThreads) lh[i] = 0;
    __syncthreads();
    const uint32_t r0 = blockIdx.x * g.rows, r1 = min(g.uh, r0 + g.rows), uw = g.uw, rs = g.w * 3, step = 2 * d + 1;
    const uint32_t p0 = r0 * uw, p1 = r1 * uw, npx = g.uh * uw;
    const uint8_t* ph = xh + base;
    const uint8_t* px = x + base;
    int32_t* so = sym + (int64_t)j * 3 * npx;
    int32_t* co = ctx + (int64_t)j * 3 * npx;
    uint64_t sh = 0, sx = 0;
    for (uint32_t p = p0 + threadIdx.x; p < p1; p += kThreads) {
        const uint32_t ly = p / uw, lx = p - ly * uw, o = ly * rs + lx * 3;
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) {
            const uint32_t vh = ph[o + c], vx = px[o + c];
            const uint32_t a = activity(ph, rs, ly, lx, g.uh, uw, c);
            const int r = (int)vx - (int)vh;
            const int m = (int)(((uint32_t)(r < 0 ? -r : r) + d) / step);
            const int q = r < 0 ? -m : m;
            so[c * npx + p] = q;
            co[c * npx + p] = (int32_t)(c * kClasses + a);
            atomicAdd(&lh[(c * kClasses + a) * bins + (uint32_t)(q + (int)Q)], 1);
            sh += cs_term(vh, p * 3 + c);
            sx += cs_term(vx, p * 3 + c);
        }
    }
    __syncthreads();
    int32_t* gh = hist + (int64_t)j * nh;
    for (uint32_t i = threadIdx.x; i < nh; i += kThreads) {
        const int32_t v = lh[i];
        if (v) atomicAdd(&gh[i], v);
    }
    block_add_u64(sh, red, cs_xh + j);
    block_add_u64(sx, red, cs_x + j);
}

// Decoder (and the encoder once the scales are chosen): table index = scales[j][c * 8 + a] -> idx (3 n, uh*uw) int32;
// cs_xh (n) u64, zero on entry.
__global__ __launch_bounds__(kThreads) void k_resid_contexts(const uint8_t* __restrict__ xh, const int32_t* __restrict__ tiles,
                                                             Geo g, const uint8_t* __restrict__ scales, int32_t* __restrict__ idx,
                                                             unsigned long long* cs_xh) {
    __shared__ uint64_t red[kThreads / 64];
    __shared__ int32_t sc[kContexts];
    const uint32_t j = blockIdx.y;
    int64_t base;
    if (!unit_of(g, tiles, j, base)) return;
    if (threadIdx.x < kContexts) sc[threadIdx.x] = scales[(int64_t)j * kContexts + threadIdx.x];
    __syncthreads();
    const uint32_t r0 = blockIdx.x * g.rows, r1 = min(g.uh, r0 + g.rows), uw = g.uw, rs = g.w * 3;
    const uint32_t p0 = r0 * uw, p1 = r1 * uw, npx = g.uh * uw;
    const uint8_t* ph = xh + base;
    int32_t* io = idx + (int64_t)j * 3 * npx;
    uint64_t sh = 0;
    for (uint32_t p = p0 + threadIdx.x; p < p1; p += kThreads) {
        const uint32_t ly = p / uw, lx = p - ly * uw, o = ly * rs + lx * 3;
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) {
            io[c * npx + p] = sc[c * kClasses + activity(ph, rs, ly, lx, g.uh, uw, c)];
            sh += cs_term(ph[o + c], p * 3 + c);
        }
    }
    block_add_u64(sh, red, cs_xh + j);
}

// Decoder: dst = clamp(xh + q * (2d + 1), 0, 255) on the units' pixels (dst: a region buffer like xh, may be xh itself);
// cs_out (n) u64, zero on entry.
__global__ __launch_bounds__(kThreads) void k_resid_apply(const uint8_t* xh, const int32_t* __restrict__ tiles, Geo g, uint32_t d,
                                                          const int32_t* __restrict__ sym, uint8_t* dst,
                                                          unsigned long long* cs_out) {
    __shared__ uint64_t red[kThreads / 64];
    const uint32_t j = blockIdx.y;
    int64_t base;
    if (!unit_of(g, tiles, j, base)) return;
    const uint32_t r0 = blockIdx.x * g.rows, r1 = min(g.uh, r0 + g.rows), uw = g.uw, rs = g.w * 3;
    const uint32_t p0 = r0 * uw, p1 = r1 * uw, npx = g.uh * uw;
    const int step = 2 * (int)d + 1;
    const int32_t* si = sym + (int64_t)j * 3 * npx;
    uint64_t so = 0;
    for (uint32_t p = p0 + threadIdx.x; p < p1; p += kThreads) {
        const uint32_t ly = p / uw, lx = p - ly * uw, o = ly * rs + lx * 3;
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) {
            int q = si[c * npx + p];
            q = q < -255 ? -255 : (q > 255 ? 255 : q);               // a symbol outside [-Q, Q] cannot overflow the sum
            int v = (int)xh[base + o + c] + q * step;
            v = v < 0 ? 0 : (v > 255 ? 255 : v);
            dst[base + o + c] = (uint8_t)v;
            so += cs_term((uint32_t)v, p * 3 + c);
        }
    }
    block_add_u64(so, red, cs_out + j);
}

// the checks all three entry points share, and the launch geometry: strips of `rows` rows with about 16K pixels each
static int resid_geo(const char* who, int64_t first, int64_t n, const int32_t* tiles, int64_t B, int64_t H, int64_t W, int64_t th,
                     int64_t tw, int64_t ny, int64_t nx, int64_t y0, int64_t x0, int64_t h, int64_t w, int64_t uh, int64_t uw,
                     Geo& g, dim3& grid) {
    LLDWT_REQUIRE(B > 0 && H > 0 && W > 0 && th > 0 && tw > 0 && ny > 0 && nx > 0 && n > 0, "%s: bad arguments", who);
    LLDWT_REQUIRE(tiles || (first >= 0 && first + n <= B * ny * nx), "%s: tile range outside the grid", who);
    LLDWT_REQUIRE(y0 >= 0 && x0 >= 0 && h > 0 && w > 0 && y0 + h <= H && x0 + w <= W,
                  "%s: region (%lld, %lld, %lld, %lld) outside the %lld x %lld image", who, (long long)y0, (long long)x0,
                  (long long)h, (long long)w, (long long)H, (long long)W);
    LLDWT_REQUIRE(ny * th >= H && nx * tw >= W, "%s: the grid does not cover the image", who);
    LLDWT_REQUIRE(uh > 0 && uw > 0 && uh <= th && uw <= tw && uh <= h && uw <= w,
                  "%s: unit size %lld x %lld does not fit the %lld x %lld tile and the %lld x %lld region", who, (long long)uh,
                  (long long)uw, (long long)th, (long long)tw, (long long)h, (long long)w);
    LLDWT_REQUIRE(n <= 65535 && H < (1ll << 31) && W < (1ll << 31) && th < (1ll << 31) && tw < (1ll << 31) &&
                  B * ny * nx < (1ll << 31) && uh * w * 3 < (1ll << 31) && uh * uw * 3 < (1ll << 31),
                  "%s: grid too large", who);
    const int64_t want = cdiv(uh * uw, 16384);
    const int64_t strips = want < 1 ? 1 : (want > uh ? uh : want), rows = cdiv(uh, strips);
    g = Geo{(uint32_t)B, (uint32_t)H, (uint32_t)W, (uint32_t)th, (uint32_t)tw, (uint32_t)ny, (uint32_t)nx, (uint32_t)y0,
            (uint32_t)x0, (uint32_t)h, (uint32_t)w, (uint32_t)uh, (uint32_t)uw, (uint32_t)rows, first};
    grid = dim3((unsigned)cdiv(uh, rows), (unsigned)n);
    return LLDWT_OK;
}

}  // namespace

extern "C" int lldwt_resid_analyse(const uint8_t* x, const uint8_t* xh, const int32_t* tiles, int64_t first, int64_t n, int64_t B,
                                   int64_t H, int64_t W, int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0, int64_t x0,
                                   int64_t h, int64_t w, int64_t uh, int64_t uw, int d, int32_t* sym, int32_t* ctx, int32_t* hist,
                                   uint64_t* cs_xh, uint64_t* cs_x, void* stream) {
    LLDWT_REQUIRE(x && xh && sym && ctx && hist && cs_xh && cs_x, "resid_analyse: null pointer");
    LLDWT_REQUIRE(d >= 0 && d <= LLDWT_RESID_MAX_NEAR, "resid_analyse: near-lossless bound %d outside [0, %d]", d,
                  LLDWT_RESID_MAX_NEAR);
    Geo g;
    dim3 grid;
    if (const int rc = resid_geo("resid_analyse", first, n, tiles, B, H, W, th, tw, ny, nx, y0, x0, h, w, uh, uw, g, grid)) return rc;
    const uint32_t Q = (255u + (uint32_t)d) / (2u * (uint32_t)d + 1u);
    hipLaunchKernelGGL(k_resid_analyse, grid, dim3(kThreads), (size_t)kContexts * (2 * Q + 1) * sizeof(int32_t),
                       (hipStream_t)stream, x, xh, tiles, g, (uint32_t)d, Q, sym, ctx, hist, (unsigned long long*)cs_xh,
                       (unsigned long long*)cs_x);
    return check_launch("resid_analyse");
}

extern "C" int lldwt_resid_contexts(const uint8_t* xh, const int32_t* tiles, int64_t first, int64_t n, int64_t B, int64_t H,
                                    int64_t W, int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0, int64_t x0, int64_t h,
                                    int64_t w, int64_t uh, int64_t uw, const uint8_t* scales, int32_t* idx, uint64_t* cs_xh,
                                    void* stream) {
    LLDWT_REQUIRE(xh && scales && idx && cs_xh, "resid_contexts: null pointer");
    Geo g;
    dim3 grid;
    if (const int rc = resid_geo("resid_contexts", first, n, tiles, B, H, W, th, tw, ny, nx, y0, x0, h, w, uh, uw, g, grid)) return rc;
    hipLaunchKernelGGL(k_resid_contexts, grid, dim3(kThreads), 0, (hipStream_t)stream, xh, tiles, g, scales, idx,
                       (unsigned long long*)cs_xh);
    return check_launch("resid_contexts");
}

extern "C" int lldwt_resid_apply(const uint8_t* xh, const int32_t* tiles, int64_t first, int64_t n, int64_t B, int64_t H,
                                 int64_t W, int64_t th, int64_t tw, int64_t ny, int64_t nx, int64_t y0, int64_t x0, int64_t h,
                                 int64_t w, int64_t uh, int64_t uw, int d, const int32_t* sym, uint8_t* dst, uint64_t* cs_out,
                                 void* stream) {
    LLDWT_REQUIRE(xh && sym && dst && cs_out, "resid_apply: null pointer");
    LLDWT_REQUIRE(d >= 0 && d <= LLDWT_RESID_MAX_NEAR, "resid_apply: near-lossless bound %d outside [0, %d]", d,
                  LLDWT_RESID_MAX_NEAR);
    Geo g;
    dim3 grid;
    if (const int rc = resid_geo("resid_apply", first, n, tiles, B, H, W, th, tw, ny, nx, y0, x0, h, w, uh, uw, g, grid)) return rc;
    hipLaunchKernelGGL(k_resid_apply, grid, dim3(kThreads), 0, (hipStream_t)stream, xh, tiles, g, (uint32_t)d, sym, dst,
                       (unsigned long long*)cs_out);
    return check_launch("resid_apply");
}
