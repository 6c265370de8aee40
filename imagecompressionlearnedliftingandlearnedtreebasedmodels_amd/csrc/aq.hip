// aq.hip -- adaptive quantisation: the activity of every block of 2^L x 2^L pixels of a uint8 RGB image and
// the step map that follows from it.  gfx950 only.  Integers throughout, so the result is defined to the bit.
//   Y = (77 R + 150 G + 29 B + 128) >> 8, coordinates clamped to the image (replicate)
//   t = 16 sum(Y^2) - (sum Y)^2 per 4 x 4 cell, S = sum of t over the block's 4^(L-2) cells, x = S + (1 << (6 + 2L))
//   a = lg(x) = 8 floor(log2 x) + #{j in 1..7 : m >= T_j}, m the 16 leading bits of x            (k_aq_activity)
//   d = clamp(floor((2 m (N a - A) + 128 N) / (256 N)), -8, 24), n = clamp((n_q G(d) + 8) >> 4, 4, 1024)      (k_aq_steps)
// k_aq_activity: one pass over the image, nothing but a and the per-image sums A goes to memory.  A lane owns a 4 x 4 cell (48
// bytes, four row reads of 12: three aligned words where W % 4 == 0, bytes otherwise and on the clamped border); the
// min(4^(L-2), 64) cells of a block sit on adjacent lanes, row-major inside the block, and the 64 / 4^(L-2) blocks of a wave
// follow each other in the image's block raster, so a wave's row reads are runs of 12 * 2^(L-2) bytes or more and every byte of
// a touched line is used by that wave.  From L = 6 on a wave owns one block and its lanes walk the block's cells 64 at a time.  The block sum is a butterfly over the block's lanes; the block's first lane writes a and keeps a
// running sum of its a.  A workgroup is four waves of one image (blockIdx.y); an image takes min(cdiv(N, 4 * blocks per wave),
// WG_CAP) workgroups, whose waves stride over the rest, so a small image still spreads over many workgroups and a large one ends
// in at most WG_CAP adds: a second butterfly, four ints through LDS and one barrier give the workgroup's sum, which one thread
// adds to A[image] with one 64-bit integer atomic (exact in any order; atomics on one address are served one after another, one
// per wave made a 2160 x 3840 image wait for 8 100 of them).  Nothing waits on another workgroup.
#include "common.h"

using namespace lldwt;

namespace {

constexpr int NT = 256, WAVE = 64;
constexpr int64_t WG_CAP = 1024;                 // workgroups per image: atomics on one address are served one after another
constexpr int L_MIN = 2, L_MAX = 8, M_MAX = 32;
constexpr int N_MIN = 4, N_MAX = 1024, D_MIN = -8, D_MAX = 24;
// T_j: the smallest integer with T_j^8 >= 2^(120 + j), j = 1 .. 7
__constant__ const uint32_t LG_T[7] = {35734, 38968, 42495, 46341, 50536, 55109, 60097};
// codec.STEP_GRID: round(16 * 2^(k / 4)), k = -8 .. 24
__constant__ const int32_t STEP_GRID[D_MAX - D_MIN + 1] = {4,  5,  6,  7,   8,   10,  11,  13,  16,  19,  23,  27,  32,  38,  45,  54,  64,
                                                          76, 91, 108, 128, 152, 181, 215, 256, 304, 362, 431, 512, 609, 724, 861, 1024};

struct ActivityArgs {
    const uint8_t* img;                          // (B, H, W, 3)
    int32_t* a;                                  // (B, hb, wb)
    unsigned long long* sums;                    // (B), zeroed before the launch
    int H, W, hb, wb, L;
};

__device__ __forceinline__ uint32_t luma(uint32_t r, uint32_t g, uint32_t b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }

// the eighth-octave logarithm of x >= 1
__device__ __forceinline__ int lg8(uint64_t x) {
    const int e = 63 - __builtin_clzll(x);
    const uint32_t m = (uint32_t)(e >= 15 ? x >> (e - 15) : x << (15 - e));
    int f = 0;
#pragma unroll
    for (int j = 0; j < 7; ++j) f += m >= LG_T[j] ? 1 : 0;
    return 8 * e + f;
}

// t of the cell whose first pixel is (y0, x0); y0 < H and x0 < W.  VEC: every row of the batch starts on a 4-byte boundary (W % 4
// == 0 and the batch is aligned), so the 12 bytes of a cell's row inside the image are three aligned words.
template <bool VEC>
__device__ __forceinline__ uint32_t cell_energy(const uint8_t* im, int H, int W, int y0, int x0) {
    uint32_t s1 = 0, s2 = 0;
    const bool words = VEC && x0 + 4 <= W;       // x0 % 4 == 0 then: a clamped x0 = W - 1 is not
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint8_t* row = im + (int64_t)min(y0 + r, H - 1) * W * 3;
        uint8_t px[12];
        if (words) {
            const uint32_t* p = reinterpret_cast<const uint32_t*>(row + (int64_t)x0 * 3);
            const uint32_t w[3] = {p[0], p[1], p[2]};
#pragma unroll
            for (int k = 0; k < 12; ++k) px[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint8_t* p = row + (int64_t)min(x0 + c, W - 1) * 3;
                px[3 * c] = p[0];
                px[3 * c + 1] = p[1];
                px[3 * c + 2] = p[2];
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t y = luma(px[3 * c], px[3 * c + 1], px[3 * c + 2]);
            s1 += y;
            s2 += y * y;
        }
    }
    return 16u * s2 - s1 * s1;
}

template <bool VEC>
__global__ __launch_bounds__(NT) void k_aq_activity(ActivityArgs g) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int side = 1 << (g.L - 2);             // cells along a block's side
    const int cells = side * side;
    const int cl = min(cells, WAVE);             // lanes per block
    const int64_t nblocks = (int64_t)g.hb * g.wb;
    const int64_t nslots = (nblocks + WAVE / cl - 1) / (WAVE / cl);               // a slot: the blocks one wave takes at a time
    const uint8_t* im = g.img + (int64_t)blockIdx.y * g.H * g.W * 3;
    int asum = 0;                                // this lane's a: at most 2^31 / 287 blocks, the entry point's bound
    // the slot index is the same in all lanes of a wave, so every lane stays for the butterflies
    for (int64_t slot = (int64_t)blockIdx.x * (NT / WAVE) + (threadIdx.x >> 6); slot < nslots; slot += (int64_t)gridDim.x * (NT / WAVE)) {
        const int64_t blk = slot * (WAVE / cl) + lane / cl;
        const bool live = blk < nblocks;
        const int by = live ? (int)(blk / g.wb) : 0, bx = live ? (int)(blk - (int64_t)by * g.wb) : 0;
        uint64_t S = 0;
        if (live) {
            for (int i = lane % cl; i < cells; i += cl) {
                // a cell that starts past the image is all replicated border: the cell of the clamped corner pixel
                const int y0 = min((by << g.L) + 4 * (i >> (g.L - 2)), g.H - 1), x0 = min((bx << g.L) + 4 * (i & (side - 1)), g.W - 1);
                S += cell_energy<VEC>(im, g.H, g.W, y0, x0);
            }
        }
        for (int o = cl >> 1; o > 0; o >>= 1) S += __shfl_xor((unsigned long long)S, o, WAVE);
        if (live && lane % cl == 0) {
            const int a = lg8(S + ((uint64_t)1 << (6 + 2 * g.L)));
            g.a[(int64_t)blockIdx.y * nblocks + blk] = a;
            asum += a;
        }
    }
#pragma unroll
    for (int o = WAVE >> 1; o > 0; o >>= 1) asum += __shfl_xor(asum, o, WAVE);
    __shared__ int wave_sum[NT / WAVE];
    if (lane == 0) wave_sum[threadIdx.x >> 6] = asum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
#pragma unroll
        for (int w = 0; w < NT / WAVE; ++w) total += (unsigned long long)wave_sum[w];
        if (total != 0) atomicAdd(g.sums + blockIdx.y, total);
    }
}

struct StepsArgs {
    const int32_t* a;                            // (B, N)
    const int64_t* sums;                         // (B)
    int32_t* n;                                  // (B, N)
    int64_t N;
    int m, n_q;
};

__global__ __launch_bounds__(NT) void k_aq_steps(StepsArgs g) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= g.N) return;
    const int64_t at = (int64_t)blockIdx.y * g.N + i;
    const int64_t num = (int64_t)g.m * (g.N * (int64_t)g.a[at] - g.sums[blockIdx.y]), den = 128 * g.N;
    const int64_t p = 2 * num + den, q = 2 * den;
    int64_t d = p / q;
    if (p % q < 0) --d;                          // floor, not truncation
    d = d < D_MIN ? D_MIN : (d > D_MAX ? D_MAX : d);
    const int n = (g.n_q * STEP_GRID[d - D_MIN] + 8) >> 4;
    g.n[at] = n < N_MIN ? N_MIN : (n > N_MAX ? N_MAX : n);
}

inline bool aligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }

}  // namespace

extern "C" int lldwt_aq_activity(const uint8_t* img, int32_t* a, int64_t* sums, int64_t B, int64_t H, int64_t W, int L, void* stream) {
    LLDWT_REQUIRE(img && a && sums, "aq_activity: null pointer");
    LLDWT_REQUIRE(aligned(a, 4) && aligned(sums, 8), "aq_activity: a must be 4-byte and sums 8-byte aligned");
    LLDWT_REQUIRE(L >= L_MIN && L <= L_MAX, "aq_activity: L = %d is outside [%d, %d]", L, L_MIN, L_MAX);
    LLDWT_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H < ((int64_t)1 << 30) && W < ((int64_t)1 << 30) &&
                      H * W < ((int64_t)1 << 40),
                  "aq_activity: bad sizes (B %lld, H %lld, W %lld)", (long long)B, (long long)H, (long long)W);
    ActivityArgs g;
    g.img = img; g.a = a; g.sums = reinterpret_cast<unsigned long long*>(sums);
    g.H = (int)H; g.W = (int)W; g.L = L;
    g.hb = (int)cdiv(H, (int64_t)1 << L); g.wb = (int)cdiv(W, (int64_t)1 << L);
    const int64_t cells = (int64_t)1 << (2 * (L - 2));
    const int64_t per_wg = (NT / WAVE) * (cells < WAVE ? WAVE / cells : 1);       // blocks of a workgroup
    LLDWT_REQUIRE((int64_t)g.hb * g.wb < ((int64_t)1 << 22), "aq_activity: %lld x %lld blocks are more than one launch takes",
                  (long long)g.hb, (long long)g.wb);
    const int64_t wgs = std::min(cdiv((int64_t)g.hb * g.wb, per_wg), WG_CAP);
    if (hipMemsetAsync(sums, 0, (size_t)B * sizeof(int64_t), (hipStream_t)stream) != hipSuccess) return check_launch("aq_activity");
    const dim3 grid((unsigned)wgs, (unsigned)B);
    if (W % 4 == 0 && aligned(img, 4)) hipLaunchKernelGGL(k_aq_activity<true>, grid, dim3(NT), 0, (hipStream_t)stream, g);
    else hipLaunchKernelGGL(k_aq_activity<false>, grid, dim3(NT), 0, (hipStream_t)stream, g);
    return check_launch("aq_activity");
}

extern "C" int lldwt_aq_steps(const int32_t* a, const int64_t* sums, int32_t* n, int64_t B, int64_t N, int m, int n_q, void* stream) {
    LLDWT_REQUIRE(a && sums && n, "aq_steps: null pointer");
    LLDWT_REQUIRE(aligned(a, 4) && aligned(n, 4) && aligned(sums, 8), "aq_steps: a and n must be 4-byte and sums 8-byte aligned");
    LLDWT_REQUIRE(m >= 1 && m <= M_MAX, "aq_steps: m = %d is outside [1, %d] (aq = m / 16)", m, M_MAX);
    LLDWT_REQUIRE(n_q >= N_MIN && n_q <= N_MAX, "aq_steps: n_q = %d is outside [%d, %d] (step = n_q / 16)", n_q, N_MIN, N_MAX);
    LLDWT_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && N < ((int64_t)1 << 31), "aq_steps: bad sizes (B %lld, N %lld)", (long long)B,
                  (long long)N);
    StepsArgs g;
    g.a = a; g.sums = sums; g.n = n; g.N = N; g.m = m; g.n_q = n_q;
    hipLaunchKernelGGL(k_aq_steps, dim3((unsigned)cdiv(N, NT), (unsigned)B), dim3(NT), 0, (hipStream_t)stream, g);
    return check_launch("aq_steps");
}
