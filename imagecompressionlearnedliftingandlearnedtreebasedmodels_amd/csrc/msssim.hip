// msssim.hip -- MS-SSIM (pytorch-msssim 0.2.1: data_range 1, 11-tap Gaussian sigma 1.5, K = (0.01, 0.03)) forward and backward.
//
// Forward, one launch per scale (k_msssim_fwd): a workgroup stages a 32 x 32 output tile plus the 10-pixel halo of x and y in LDS,
// runs the horizontal pass of the five statistics F(x), F(y), F(xx), F(yy), F(xy) into LDS and the vertical pass out of it, forms
// cs and l*cs per pixel and adds their float64 partial sums per plane into a device buffer.  No statistic map goes to HBM.
// k_msssim_pool makes the next scale's x and y (2x2 average, an odd side zero-padded by one on both ends, divisor 4 always);
// k_msssim_finalize turns the sums into v (S,planes), m (planes) and the backward coefficients dm/dv / N_s.
// Backward, one launch per scale from coarse to fine (k_msssim_bwd): the statistics are recomputed on the output tile widened by
// 10, the three per-pixel adjoints A = dL/dF(y), Bq = dL/dF(yy), Cq = dL/dF(xy) are formed in LDS, the transposed window is applied
// (the same correlation on the zero-extended adjoint maps) and grad = Ft(A) + 2 Y Ft(Bq) + X Ft(Cq) + the pool adjoint of the
// coarser scale's gradient is written.  fp32 per pixel, float64 for everything summed over more than a tile.
#include "common.h"

namespace lldwt {
namespace {

constexpr int MS_NT = 256;
constexpr int MS_HALO = 10;                 // window 11
constexpr float MS_C1 = 1e-4f, MS_C2 = 9e-4f;
// g[i] = exp(-(i-5)^2 / 4.5) / sum, evaluated in float64 and rounded once
__device__ __constant__ float MS_G[11] = {0.00102838008447911f, 0.007598758135239185f, 0.03600077212843083f, 0.10936068950970002f,
                                           0.2130055377112537f,  0.26601172486179436f,  0.2130055377112537f,  0.10936068950970002f,
                                           0.03600077212843083f, 0.007598758135239185f, 0.00102838008447911f};
__device__ __constant__ double MS_W[5] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};

// forward tile
constexpr int FW_TW = 32, FW_TH = 32;
constexpr int FW_IW = FW_TW + MS_HALO, FW_IH = FW_TH + MS_HALO;
constexpr int FW_IS = FW_IW + 1;            // odd row stride: the 4-column items of the horizontal pass fall on distinct banks
// backward tile
constexpr int BW_TW = 32, BW_TH = 24;
constexpr int BW_AW = BW_TW + MS_HALO, BW_AH = BW_TH + MS_HALO;            // adjoint tile (statistic pixels)
constexpr int BW_IW = BW_TW + 2 * MS_HALO, BW_IH = BW_TH + 2 * MS_HALO;    // input tile
constexpr int BW_IS = BW_IW + 1;

// per-pixel SSIM terms from the five window means
struct Terms {
    float cs, l, dcs, dl;   // dcs = sxx + syy + C2, dl = mx^2 + my^2 + C1
};
__device__ __forceinline__ Terms ssim_terms(float mx, float my, float exx, float eyy, float exy) {
    const float mxx = mx * mx, myy = my * my, mxy = mx * my;
    const float sxx = exx - mxx, syy = eyy - myy, sxy = exy - mxy;
    Terms t;
    t.dcs = sxx + syy + MS_C2;
    t.cs = (2.f * sxy + MS_C2) / t.dcs;
    t.dl = mxx + myy + MS_C1;
    t.l = (2.f * mxy + MS_C1) / t.dl;
    return t;
}

// stage rows [y0, y0+rows) x cols [x0, x0+cols) of one plane into LDS with `offset` added; zero outside the image
__device__ __forceinline__ void stage_tile(const float* __restrict__ src, float* dst, int y0, int x0, int rows, int cols, int stride,
                                           int H, int W, float offset) {
    for (int i = threadIdx.x; i < rows * cols; i += MS_NT) {
        const int r = i / cols, c = i - r * cols;
        const int gy = y0 + r, gx = x0 + c;
        float v = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = src[(int64_t)gy * W + gx] + offset;
        dst[r * stride + c] = v;
    }
}

// horizontal pass of the five statistics: rows x (ncol = NPER * groups) outputs, NPER adjacent columns per work item
template <int NPER>
__device__ __forceinline__ void hpass5(const float* sx, const float* sy, int in_stride, float* hs, int rows, int ncol) {
    const int groups = ncol / NPER;
    const int plane = rows * ncol;
    for (int it = threadIdx.x; it < rows * groups; it += MS_NT) {
        const int r = it / groups, c0 = (it - r * groups) * NPER;
        float xv[NPER + MS_HALO], yv[NPER + MS_HALO];
#pragma unroll
        for (int k = 0; k < NPER + MS_HALO; ++k) {
            xv[k] = sx[r * in_stride + c0 + k];
            yv[k] = sy[r * in_stride + c0 + k];
        }
#pragma unroll
        for (int j = 0; j < NPER; ++j) {
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
            for (int k = 0; k <= MS_HALO; ++k) {
                const float g = MS_G[k], xx = xv[j + k], yy = yv[j + k];
                a0 = fmaf(g, xx, a0);
                a1 = fmaf(g, yy, a1);
                a2 = fmaf(g, xx * xx, a2);
                a3 = fmaf(g, yy * yy, a3);
                a4 = fmaf(g, xx * yy, a4);
            }
            const int o = r * ncol + c0 + j;
            hs[o] = a0;
            hs[plane + o] = a1;
            hs[2 * plane + o] = a2;
            hs[3 * plane + o] = a3;
            hs[4 * plane + o] = a4;
        }
    }
}

__global__ __launch_bounds__(MS_NT) void k_msssim_fwd(const float* __restrict__ x, const float* __restrict__ y, float offset, int H,
                                                      int W, double* __restrict__ sums) {
    __shared__ float sx[FW_IH * FW_IS], sy[FW_IH * FW_IS];
    __shared__ float hs[5 * FW_IH * FW_TW];
    __shared__ double part[2][MS_NT / 64];
    const int64_t plane = blockIdx.z;
    const int ty0 = blockIdx.y * FW_TH, tx0 = blockIdx.x * FW_TW;
    const int OH = H - MS_HALO, OW = W - MS_HALO;
    const float* xp = x + plane * (int64_t)H * W;
    const float* yp = y + plane * (int64_t)H * W;
    stage_tile(xp, sx, ty0, tx0, FW_IH, FW_IW, FW_IS, H, W, offset);
    stage_tile(yp, sy, ty0, tx0, FW_IH, FW_IW, FW_IS, H, W, offset);
    __syncthreads();
    hpass5<4>(sx, sy, FW_IS, hs, FW_IH, FW_TW);
    __syncthreads();
    double s_cs = 0, s_lcs = 0;
    constexpr int NR = 4, HP = FW_IH * FW_TW;
    for (int it = threadIdx.x; it < (FW_TH / NR) * FW_TW; it += MS_NT) {
        const int c = it % FW_TW, r0 = (it / FW_TW) * NR;
        float acc[5][NR];
#pragma unroll
        for (int s = 0; s < 5; ++s)
#pragma unroll
            for (int j = 0; j < NR; ++j) acc[s][j] = 0.f;
#pragma unroll
        for (int k = 0; k < NR + MS_HALO; ++k) {
            float v[5];
#pragma unroll
            for (int s = 0; s < 5; ++s) v[s] = hs[s * HP + (r0 + k) * FW_TW + c];
#pragma unroll
            for (int j = 0; j < NR; ++j)
                if (k - j >= 0 && k - j <= MS_HALO) {
#pragma unroll
                    for (int s = 0; s < 5; ++s) acc[s][j] = fmaf(MS_G[k - j], v[s], acc[s][j]);
                }
        }
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            if (ty0 + r0 + j < OH && tx0 + c < OW) {
                const Terms t = ssim_terms(acc[0][j], acc[1][j], acc[2][j], acc[3][j], acc[4][j]);
                s_cs += (double)t.cs;
                s_lcs += (double)(t.l * t.cs);
            }
        }
    }
    s_cs = wave_sum(s_cs);
    s_lcs = wave_sum(s_lcs);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
        part[0][wv] = s_cs;
        part[1][wv] = s_lcs;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        double s = 0;
        for (int i = 0; i < MS_NT / 64; ++i) s += part[threadIdx.x][i];
        atomicAdd(sums + plane * 2 + threadIdx.x, s);
    }
}

// next scale of x and y: avg_pool2d(kernel 2, stride 2, padding = side % 2, count_include_pad)
__global__ __launch_bounds__(MS_NT) void k_msssim_pool(const float* __restrict__ x, const float* __restrict__ y, float offset, int H,
                                                       int W, int H2, int W2, float* __restrict__ x2, float* __restrict__ y2,
                                                       int64_t planes) {
    const int64_t n = planes * H2 * W2;
    const int py = H & 1, px = W & 1;
    for (int64_t i = blockIdx.x * (int64_t)MS_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * MS_NT) {
        const int64_t p = i / ((int64_t)H2 * W2);
        const int r = (int)(i - p * H2 * W2);
        const int oy = r / W2, ox = r - oy * W2;
        const float* xs = x + p * (int64_t)H * W;
        const float* ys = y + p * (int64_t)H * W;
        float ax = 0.f, ay = 0.f;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int iy = 2 * oy - py + dy, ix = 2 * ox - px + dx;
                if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
                    ax += xs[(int64_t)iy * W + ix] + offset;
                    ay += ys[(int64_t)iy * W + ix] + offset;
                }
            }
        x2[i] = 0.25f * ax;
        y2[i] = 0.25f * ay;
    }
}

struct ScaleDims {
    int n[5];   // (H-10)*(W-10) per scale
};

// sums (S, planes, 2) -> v (S, planes), m (planes), coef (S, planes) = dm/dv_s / N_s, zero for a plane with a clamped term
__global__ __launch_bounds__(MS_NT) void k_msssim_finalize(const double* __restrict__ sums, ScaleDims dims, int S, int64_t planes,
                                                           double* __restrict__ v, double* __restrict__ m, double* __restrict__ coef) {
    const int64_t p = blockIdx.x * (int64_t)MS_NT + threadIdx.x;
    if (p >= planes) return;
    double vs[5], prod = 1.0;
    bool alive = true;
    for (int s = 0; s < S; ++s) {
        const double mean = sums[((int64_t)s * planes + p) * 2 + (s == S - 1 ? 1 : 0)] / (double)dims.n[s];
        vs[s] = mean > 0.0 ? mean : 0.0;
        alive = alive && mean > 0.0;
        v[(int64_t)s * planes + p] = vs[s];
    }
    if (alive)
        for (int s = 0; s < S; ++s) prod *= pow(vs[s], MS_W[s]);
    else
        prod = 0.0;
    m[p] = prod;
    // w v^(w-1) is never evaluated at 0: a plane with a clamped term has the gradient zero
    for (int s = 0; s < S; ++s) coef[(int64_t)s * planes + p] = alive ? MS_W[s] * prod / vs[s] / (double)dims.n[s] : 0.0;
}

// correlation of `rows` x (ncol + 10) values at `src` (row stride in_stride) with the window along the row; NPER columns per item
template <int NPER>
__device__ __forceinline__ void hpass1(const float* src, int in_stride, float* dst, int rows, int ncol) {
    const int groups = ncol / NPER;
    for (int it = threadIdx.x; it < rows * groups; it += MS_NT) {
        const int r = it / groups, c0 = (it - r * groups) * NPER;
        float v[NPER + MS_HALO];
#pragma unroll
        for (int k = 0; k < NPER + MS_HALO; ++k) v[k] = src[r * in_stride + c0 + k];
#pragma unroll
        for (int j = 0; j < NPER; ++j) {
            float a = 0.f;
#pragma unroll
            for (int k = 0; k <= MS_HALO; ++k) a = fmaf(MS_G[k], v[j + k], a);
            dst[r * ncol + c0 + j] = a;
        }
    }
}

// grad (this scale) = Ft(A) + 2 Y Ft(Bq) + X Ft(Cq) + 1/4 of the coarser scale's gradient at the pixel's pool cell.
// last = 1: the scale whose term is l*cs.  coarse may be null (coarsest scale).  g: the upstream gradient (device, may be null = 1).
__global__ __launch_bounds__(MS_NT) void k_msssim_bwd(const float* __restrict__ x, const float* __restrict__ y, float offset, int H,
                                                      int W, int last, const double* __restrict__ coef, const double* __restrict__ g,
                                                      double gscale, const float* __restrict__ coarse, int H2, int W2,
                                                      float* __restrict__ grad) {
    // in: x and y input tiles, later the three adjoint tiles (3 * 34 * 42 <= 2 * 44 * 53 floats)
    __shared__ float in[2 * BW_IH * BW_IS];
    // hs: the five horizontally filtered statistics (5 * 44 * 42), later the three horizontally filtered adjoints (3 * 34 * 32)
    __shared__ float hs[5 * BW_IH * BW_AW];
    static_assert(3 * BW_AH * BW_AW <= 2 * BW_IH * BW_IS, "adjoint tiles must fit the input tiles");
    static_assert(3 * BW_AH * BW_TW <= 5 * BW_IH * BW_AW, "filtered adjoints must fit the statistics");
    const int64_t plane = blockIdx.z;
    const int gy0 = blockIdx.y * BW_TH, gx0 = blockIdx.x * BW_TW;
    const int OH = H - MS_HALO, OW = W - MS_HALO;
    const float* xp = x + plane * (int64_t)H * W;
    const float* yp = y + plane * (int64_t)H * W;
    float* gp = grad + plane * (int64_t)H * W;
    const float* cp = coarse ? coarse + plane * (int64_t)H2 * W2 : nullptr;
    const int py = H & 1, px = W & 1;
    const float kf = (float)(coef[plane] * (g ? g[0] : 1.0) * gscale);

    if (kf == 0.f) {   // clamped plane (or a zero upstream gradient): only the pool adjoint remains, exactly zero at the finest scale
        for (int i = threadIdx.x; i < BW_TH * BW_TW; i += MS_NT) {
            const int r = i / BW_TW, c = i - r * BW_TW;
            const int gy = gy0 + r, gx = gx0 + c;
            if (gy < H && gx < W) gp[(int64_t)gy * W + gx] = cp ? 0.25f * cp[(int64_t)((gy + py) >> 1) * W2 + ((gx + px) >> 1)] : 0.f;
        }
        return;
    }

    float* sx = in;
    float* sy = in + BW_IH * BW_IS;
    stage_tile(xp, sx, gy0 - MS_HALO, gx0 - MS_HALO, BW_IH, BW_IW, BW_IS, H, W, offset);
    stage_tile(yp, sy, gy0 - MS_HALO, gx0 - MS_HALO, BW_IH, BW_IW, BW_IS, H, W, offset);
    __syncthreads();
    hpass5<3>(sx, sy, BW_IS, hs, BW_IH, BW_AW);
    __syncthreads();
    // vertical pass of the statistics and the per-pixel adjoints, two rows per item; the adjoint tiles overwrite the input tiles
    {
        constexpr int NR = 2, HP = BW_IH * BW_AW, AP = BW_AH * BW_AW;
        for (int it = threadIdx.x; it < (BW_AH / NR) * BW_AW; it += MS_NT) {
            const int c = it % BW_AW, r0 = (it / BW_AW) * NR;
            float acc[5][NR];
#pragma unroll
            for (int s = 0; s < 5; ++s)
#pragma unroll
                for (int j = 0; j < NR; ++j) acc[s][j] = 0.f;
#pragma unroll
            for (int k = 0; k < NR + MS_HALO; ++k) {
                float v[5];
#pragma unroll
                for (int s = 0; s < 5; ++s) v[s] = hs[s * HP + (r0 + k) * BW_AW + c];
#pragma unroll
                for (int j = 0; j < NR; ++j)
                    if (k - j >= 0 && k - j <= MS_HALO) {
#pragma unroll
                        for (int s = 0; s < 5; ++s) acc[s][j] = fmaf(MS_G[k - j], v[s], acc[s][j]);
                    }
            }
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                const int sy_ = gy0 - MS_HALO + r0 + j, sx_ = gx0 - MS_HALO + c;   // statistic pixel of this adjoint
                float A = 0.f, Bq = 0.f, Cq = 0.f;
                if (sy_ >= 0 && sy_ < OH && sx_ >= 0 && sx_ < OW) {
                    const float mx = acc[0][j], my = acc[1][j];
                    const Terms t = ssim_terms(mx, my, acc[2][j], acc[3][j], acc[4][j]);
                    const float fcs = last ? kf * t.l : kf;          // k * df/dcs
                    const float dsxy = fcs * (2.f / t.dcs);          // k * df/dsxy
                    const float dsyy = -fcs * (t.cs / t.dcs);        // k * df/dsyy
                    Cq = dsxy;
                    Bq = dsyy;
                    A = -(dsxy * mx) - 2.f * (dsyy * my);
                    if (last) A += kf * t.cs * ((2.f * mx - 2.f * (t.l * my)) / t.dl);
                }
                const int o = (r0 + j) * BW_AW + c;
                in[o] = A;
                in[AP + o] = Bq;
                in[2 * AP + o] = Cq;
            }
        }
    }
    __syncthreads();
    // transposed window = the same correlation on the zero-extended adjoint maps: horizontal, then vertical
    {
        constexpr int AP = BW_AH * BW_AW, TP = BW_AH * BW_TW;
#pragma unroll
        for (int s = 0; s < 3; ++s) hpass1<4>(in + s * AP, BW_AW, hs + s * TP, BW_AH, BW_TW);
    }
    __syncthreads();
    {
        constexpr int NR = 3, TP = BW_AH * BW_TW;
        for (int it = threadIdx.x; it < (BW_TH / NR) * BW_TW; it += MS_NT) {
            const int c = it % BW_TW, r0 = (it / BW_TW) * NR;
            float acc[3][NR];
#pragma unroll
            for (int s = 0; s < 3; ++s)
#pragma unroll
                for (int j = 0; j < NR; ++j) acc[s][j] = 0.f;
#pragma unroll
            for (int k = 0; k < NR + MS_HALO; ++k) {
                float v[3];
#pragma unroll
                for (int s = 0; s < 3; ++s) v[s] = hs[s * TP + (r0 + k) * BW_TW + c];
#pragma unroll
                for (int j = 0; j < NR; ++j)
                    if (k - j >= 0 && k - j <= MS_HALO) {
#pragma unroll
                        for (int s = 0; s < 3; ++s) acc[s][j] = fmaf(MS_G[k - j], v[s], acc[s][j]);
                    }
            }
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                const int gy = gy0 + r0 + j, gx = gx0 + c;
                if (gy < H && gx < W) {
                    const int64_t o = (int64_t)gy * W + gx;
                    const float X = xp[o] + offset, Y = yp[o] + offset;
                    float gr = acc[0][j] + 2.f * Y * acc[1][j] + X * acc[2][j];
                    if (cp) gr += 0.25f * cp[(int64_t)((gy + py) >> 1) * W2 + ((gx + px) >> 1)];
                    gp[o] = gr;
                }
            }
        }
    }
}

static_assert(FW_TW % 4 == 0 && FW_TH % 4 == 0, "forward items: 4 columns / 4 rows");
static_assert(BW_AW % 3 == 0 && BW_AH % 2 == 0 && BW_TW % 4 == 0 && BW_TH % 3 == 0, "backward items");

inline int64_t pooled(int64_t n) { return n / 2 + (n & 1); }   // floor(n/2) + 1 for odd n, n/2 for even n

int check_dims(const char* what, int64_t planes, int64_t H, int64_t W, int scales) {
    LLDWT_REQUIRE(scales >= 1 && scales <= 5, "%s: scales must be 1..5 (got %d)", what, scales);
    const int64_t min_side = 10 * ((int64_t)1 << (scales - 1)) + 1;
    LLDWT_REQUIRE(planes > 0 && planes <= 65535, "%s: planes must be 1..65535 (got %lld)", what, (long long)planes);
    LLDWT_REQUIRE(H >= min_side && W >= min_side && H <= 32768 && W <= 32768, "%s: sides must be %lld..32768 (got %lld x %lld)", what,
                  (long long)min_side, (long long)H, (long long)W);
    return LLDWT_OK;
}

}  // namespace
}  // namespace lldwt

using namespace lldwt;

extern "C" int64_t lldwt_msssim_ws_floats(int64_t planes, int64_t H, int64_t W, int scales) {
    if (planes <= 0 || H <= 0 || W <= 0 || scales < 1 || scales > 5) return 0;
    int64_t total = 0;
    for (int s = 1; s < scales; ++s) {
        H = pooled(H);
        W = pooled(W);
        total += 2 * planes * H * W;
    }
    return total;
}

extern "C" int lldwt_msssim_forward(const float* x, const float* y, float offset, int64_t planes, int64_t H, int64_t W, int scales,
                                    float* pyr, double* sums, double* v, double* m, double* coef, void* stream) {
    if (int rc = check_dims("msssim_forward", planes, H, W, scales)) return rc;
    LLDWT_REQUIRE(x && y && sums && v && m && coef && (pyr || scales == 1), "msssim_forward: null argument");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(sums, 0, sizeof(double) * 2 * planes * scales, st) != hipSuccess) {
        set_error("msssim_forward: hipMemsetAsync failed");
        return LLDWT_EHIP;
    }
    ScaleDims dims;
    const float* xs = x;
    const float* ys = y;
    float off = offset;
    float* next = pyr;
    int64_t h = H, w = W;
    for (int s = 0; s < scales; ++s) {
        dims.n[s] = (int)((h - MS_HALO) * (w - MS_HALO));
        const dim3 grid((unsigned)cdiv(w - MS_HALO, FW_TW), (unsigned)cdiv(h - MS_HALO, FW_TH), (unsigned)planes);
        hipLaunchKernelGGL(k_msssim_fwd, grid, dim3(MS_NT), 0, st, xs, ys, off, (int)h, (int)w, sums + (int64_t)s * planes * 2);
        if (s + 1 < scales) {
            const int64_t h2 = pooled(h), w2 = pooled(w), n2 = planes * h2 * w2;
            float* x2 = next;
            float* y2 = next + n2;
            const int64_t blocks = cdiv(n2, MS_NT);
            hipLaunchKernelGGL(k_msssim_pool, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(MS_NT), 0, st, xs, ys, off, (int)h,
                               (int)w, (int)h2, (int)w2, x2, y2, planes);
            xs = x2;
            ys = y2;
            off = 0.f;   // the pyramid holds the shifted values
            next += 2 * n2;
            h = h2;
            w = w2;
        }
    }
    hipLaunchKernelGGL(k_msssim_finalize, dim3((unsigned)cdiv(planes, MS_NT)), dim3(MS_NT), 0, st, sums, dims, scales, planes, v, m, coef);
    return check_launch("msssim_forward");
}

extern "C" int lldwt_msssim_backward(const float* x, const float* y, float offset, int64_t planes, int64_t H, int64_t W, int scales,
                                     const float* pyr, const double* coef, const double* g, double gscale, float* gpyr, float* grad_y,
                                     void* stream) {
    if (int rc = check_dims("msssim_backward", planes, H, W, scales)) return rc;
    LLDWT_REQUIRE(x && y && coef && grad_y && ((pyr && gpyr) || scales == 1), "msssim_backward: null argument");
    hipStream_t st = (hipStream_t)stream;
    int64_t hh[5], ww[5];
    const float *xs[5], *ys[5];
    float* gs[5];
    hh[0] = H;
    ww[0] = W;
    xs[0] = x;
    ys[0] = y;
    gs[0] = grad_y;
    const float* p = pyr;
    float* q = gpyr;
    for (int s = 1; s < scales; ++s) {
        hh[s] = pooled(hh[s - 1]);
        ww[s] = pooled(ww[s - 1]);
        const int64_t n = planes * hh[s] * ww[s];
        xs[s] = p;
        ys[s] = p + n;
        p += 2 * n;
        gs[s] = q;
        q += n;
    }
    for (int s = scales - 1; s >= 0; --s) {
        const bool has_coarse = s + 1 < scales;
        const dim3 grid((unsigned)cdiv(ww[s], BW_TW), (unsigned)cdiv(hh[s], BW_TH), (unsigned)planes);
        hipLaunchKernelGGL(k_msssim_bwd, grid, dim3(MS_NT), 0, st, xs[s], ys[s], s == 0 ? offset : 0.f, (int)hh[s], (int)ww[s],
                           s == scales - 1 ? 1 : 0, coef + (int64_t)s * planes, g, gscale, has_coarse ? (const float*)gs[s + 1] : nullptr,
                           has_coarse ? (int)hh[s + 1] : 0, has_coarse ? (int)ww[s + 1] : 0, gs[s]);
    }
    return check_launch("msssim_backward");
}
