// A loss that trains against folds (DESIGN.md "Fold penalty"): the hinge max(0, margin - det) on the forward-difference Jacobian
// determinant of the transformation a UNet offset field describes at its own size, forward and backward.  Not a call site of the
// reference, whose only regulariser is the first-order smoothness term (smooth.hip), which does not know the determinant's sign.
//   p(h, w) = sample_position(grid_coord<GRID_UNET>(d)), a = p(h, w+1) - p(h, w), b = p(h+1, w) - p(h, w), det = a.x * b.y - b.x * a.y
// through jacobian_tile.h: the bits jacobian_kernel<GRID_UNET, false> (regularity.hip) computes at equal field and output size.  A pixel
// is interior when it has both forward neighbours, M = N (H-1) (W-1);
//   loss = factor / M * sum over the interior pixels of max(0, margin - det),   active[n] = #(det <= margin).
//
// Forward: one workgroup per 64 x 16 tile (resampled_grid.h) writes the positions of the 65 x 17 tile into LDS once and takes the
// differences from there, a lane owning one pixel in each of four rows — jacobian_kernel's shape.  Per-lane partials, the xor tree of
// each wave, the waves in ascending order, one record (sum, count) per workgroup in the caller's workspace; one finish kernel reads
// the records in a fixed order.  No atomics: bitwise repeatable.  A term passes through at most 4 (lane) + 6 (wave) + 3 (workgroup)
// additions in the tile kernel and ceil(records / 256) + 6 + 3 in the finish.
//
// Backward: a pure gather (as smooth_bwd_kernel).  d loss / d det = -factor / M where det < margin and 0 elsewhere, equality included
// (torch's relu).  Texel (h, w) is the p(h, w) of its own pixel, the p(h, w+1) of its left neighbour and the p(h+1, w) of the upper one:
// the workgroup stages the positions of the 66 x 18 tile (a halo of one on every side), each lane re-forms a, b and the active flag of
// those three pixels from LDS — together the 65 x 17 pixels the tile's texels hear from — and writes both channels.  The three terms
// are added in that order.  One launch, no workspace.
#include "common.h"
#include "jacobian_tile.h"

namespace {

constexpr int FOLD_WORDS = 2;                          // a record: the hinge sum (f32), the active count (u32)
constexpr int BT_W = RT_W + 2, BT_H = RT_H + 2;        // the backward tile: a halo of one on every side

template <bool BWD>
__device__ __forceinline__ void stage_positions(float* pos, const float* __restrict__ dN, size_t plane, int x0, int y0, int H, int W, int tid) {
    constexpr int TW = BWD ? BT_W : JT_W, TH = BWD ? BT_H : JT_H, OFF = BWD ? 1 : 0;
    for (int e = tid; e < TH * TW; e += RT_THREADS) {
        const int r = e / TW, c = e - r * TW;
        const int h = y0 + r - OFF, w = x0 + c - OFF;
        if (h < 0 || w < 0 || h >= H || w >= W) continue;
        float px, py;
        unet_position(dN, plane, h, w, H, W, px, py);
        pos[e] = px;
        pos[TH * TW + e] = py;
    }
}

__global__ __launch_bounds__(RT_THREADS) void fold_fwd_kernel(const float* __restrict__ d, float margin, unsigned* __restrict__ partial, int H,
                                                              int W) {
    __shared__ float pos[2 * JT_H * JT_W];                 // p of the 65 x 17 tile: x plane, then y plane
    __shared__ unsigned red[(RT_THREADS / 64) * FOLD_WORDS];
    const int n = blockIdx.z, tid = threadIdx.x;
    const int x0 = blockIdx.x * RT_W, y0 = blockIdx.y * RT_H;
    const size_t plane = (size_t)H * W;
    stage_positions<false>(pos, d + (size_t)n * 2 * plane, plane, x0, y0, H, W, tid);
    __syncthreads();

    float sum = 0.f;
    unsigned cnt = 0u;
    constexpr int ROWS = RT_THREADS / RT_W, RUNS = RT_H / ROWS;      // a lane owns one pixel in each of RUNS rows: a wave = 64 pixels of a row
#pragma unroll
    for (int i = 0; i < RUNS; ++i) {
        const int r = tid / RT_W + ROWS * i, c = tid % RT_W;
        if (y0 + r >= H - 1 || x0 + c >= W - 1) continue;           // not interior
        const float* qx = pos + r * JT_W + c;
        const float* qy = qx + JT_H * JT_W;
        const float det = jac_det(qx[0], qy[0], qx[1], qy[1], qx[JT_W], qy[JT_W]);
        sum += fmaxf(0.f, margin - det);
        if (det <= margin) cnt += 1u;
    }
    // the workgroup's record, in thread 0: the xor tree of each wave, then the waves in ascending order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o, 64);
        cnt += (unsigned)__shfl_xor((int)cnt, o, 64);
    }
    const int lane = tid & 63, wid = tid >> 6;
    if (lane == 0) {
        red[wid * FOLD_WORDS] = __float_as_uint(sum);
        red[wid * FOLD_WORDS + 1] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < RT_THREADS / 64; ++i) {
            sum += __uint_as_float(red[i * FOLD_WORDS]);
            cnt += red[i * FOLD_WORDS + 1];
        }
        unsigned* dst = partial + (((size_t)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * FOLD_WORDS;
        dst[0] = __float_as_uint(sum);
        dst[1] = cnt;
    }
}

// loss[0] (+)= scale * (all records' sums: thread t takes records t, t + 256, ... in ascending order, then the fixed workgroup tree);
// active[n] = the sample's counts (integers: any order gives the same bits; wave k takes samples k, k + 4, ...)
__global__ __launch_bounds__(256) void fold_finish_kernel(const unsigned* __restrict__ partial, int tiles, int N, float scale, int accumulate,
                                                          float* __restrict__ loss, unsigned* __restrict__ active) {
    __shared__ float red[16];
    const long long total = (long long)N * tiles;
    float acc = 0.f;
    for (long long i = threadIdx.x; i < total; i += 256) acc += __uint_as_float(partial[i * FOLD_WORDS]);
    const float t = block_sum(acc, red);
    if (threadIdx.x == 0) loss[0] = (accumulate ? loss[0] : 0.f) + scale * t;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int n0 = 0; n0 < N; n0 += 4) {                     // (uniform trip count: every wave reaches every shuffle)
        const int n = n0 + wid;
        unsigned cnt = 0u;
        if (n < N) {
            const unsigned* p = partial + (size_t)n * tiles * FOLD_WORDS;
            for (int i = lane; i < tiles; i += 64) cnt += p[(size_t)i * FOLD_WORDS + 1];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += (unsigned)__shfl_xor((int)cnt, o, 64);
        if (lane == 0 && n < N) active[n] = cnt;
    }
}

// what pixel (r, c) of the staged 66 x 18 tile (tile-relative, halo included: the pixel at LDS row r + 1, column c + 1) contributes:
// its a and b, and whether its hinge has slope (interior, inside the image, det < margin)
struct FoldPixel {
    float ax, ay, bx, by;
    bool on;
};
__device__ __forceinline__ FoldPixel fold_pixel(const float* pos, int r, int c, int h, int w, int H, int W, float margin) {
    FoldPixel q{0.f, 0.f, 0.f, 0.f, false};
    if (h < 0 || w < 0 || h >= H - 1 || w >= W - 1) return q;      // the pixel does not exist or is not interior: its term is absent
    const float* qx = pos + (r + 1) * BT_W + (c + 1);
    const float* qy = qx + BT_H * BT_W;
    const float ix = qx[0], iy = qy[0];
    q.ax = qx[1] - ix; q.ay = qy[1] - iy;
    q.bx = qx[BT_W] - ix; q.by = qy[BT_W] - iy;
    q.on = jac_det(ix, iy, qx[1], qy[1], qx[BT_W], qy[BT_W]) < margin;
    return q;
}

__global__ __launch_bounds__(RT_THREADS) void fold_bwd_kernel(const float* __restrict__ d, float margin, const float* __restrict__ gscale,
                                                              float scale, float* __restrict__ gd, int accumulate, int H, int W) {
    __shared__ float pos[2 * BT_H * BT_W];                 // p of the 66 x 18 tile: x plane, then y plane
    const int n = blockIdx.z, tid = threadIdx.x;
    const int x0 = blockIdx.x * RT_W, y0 = blockIdx.y * RT_H;
    const size_t plane = (size_t)H * W;
    stage_positions<true>(pos, d + (size_t)n * 2 * plane, plane, x0, y0, H, W, tid);
    __syncthreads();

    const float s = -(gscale[0] * scale);                  // d loss / d det on an active pixel, times the upstream gradient
    const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;      // d p.x / d d0, d p.y / d d1
    float* gN = gd + (size_t)n * 2 * plane;
    constexpr int ROWS = RT_THREADS / RT_W, RUNS = RT_H / ROWS;
#pragma unroll
    for (int i = 0; i < RUNS; ++i) {
        const int r = tid / RT_W + ROWS * i, c = tid % RT_W;
        const int h = y0 + r, w = x0 + c;
        if (h >= H || w >= W) continue;
        const FoldPixel own = fold_pixel(pos, r, c, h, w, H, W, margin);
        const FoldPixel lf = fold_pixel(pos, r, c - 1, h, w - 1, H, W, margin);
        const FoldPixel up = fold_pixel(pos, r - 1, c, h - 1, w, H, W, margin);
        // this texel as p(h, w) of its own pixel, as p(h, w+1) of the left one, as p(h+1, w) of the upper one — in that order
        const float t0 = own.on ? s * (own.ay - own.by) : 0.f, t1 = lf.on ? s * lf.by : 0.f, t2 = up.on ? s * -up.ay : 0.f;
        const float u0 = own.on ? s * (own.bx - own.ax) : 0.f, u1 = lf.on ? s * -lf.bx : 0.f, u2 = up.on ? s * up.ax : 0.f;
        const float g0 = hw * (t0 + t1 + t2), g1 = hh * (u0 + u1 + u2);
        const size_t o = (size_t)h * W + w;
        if (accumulate) { gN[o] += g0; gN[plane + o] += g1; } else { gN[o] = g0; gN[plane + o] = g1; }
    }
}

long long fold_tiles(int H, int W) { return (long long)nemar_cdiv(W, RT_W) * nemar_cdiv(H, RT_H); }

// factor / M as the kernels apply it (0 without an interior pixel: the loss and the gradient are then zeros, written)
float fold_scale(float factor, int N, int H, int W) {
    const double m = (double)N * (H - 1) * (W - 1);
    return m > 0 ? (float)((double)factor / m) : 0.f;
}

bool fold_shape_ok(int N, int H, int W) {
    return N > 0 && H > 0 && W > 0 && N <= 65535 && (long long)H * W < (1ll << 31) && nemar_cdiv(H, RT_H) <= 65535;
}

}  // namespace

NEMAR_API size_t nemar_fold_penalty_workspace(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return sizeof(unsigned) * FOLD_WORDS * (size_t)fold_tiles(H, W) * N;
}

NEMAR_API int nemar_fold_penalty_fwd(const float* d, float margin, float factor, float* loss, int accumulate, unsigned* active,
                                     void* workspace, size_t ws_bytes, int N, int H, int W, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(d && loss && active && workspace, "fold_penalty_fwd: null pointer");
    NEMAR_REQUIRE(((((uintptr_t)d) | ((uintptr_t)loss) | ((uintptr_t)active) | ((uintptr_t)workspace)) & 3) == 0,
                  "fold_penalty_fwd: d, loss, active and workspace must be 4-byte aligned");
    NEMAR_REQUIRE(fold_shape_ok(N, H, W), "fold_penalty_fwd: bad shape N=%d H=%d W=%d", N, H, W);
    NEMAR_REQUIRE(ws_bytes >= nemar_fold_penalty_workspace(N, H, W), "fold_penalty_fwd: workspace %zu < %zu", ws_bytes,
                  nemar_fold_penalty_workspace(N, H, W));
    hipStream_t st = (hipStream_t)stream;
    unsigned* partial = (unsigned*)workspace;
    const dim3 grid(nemar_cdiv(W, RT_W), nemar_cdiv(H, RT_H), N), block(RT_THREADS);
    hipLaunchKernelGGL(fold_fwd_kernel, grid, block, 0, st, d, margin, partial, H, W);
    hipLaunchKernelGGL(fold_finish_kernel, dim3(1), dim3(256), 0, st, (const unsigned*)partial, (int)fold_tiles(H, W), N,
                       fold_scale(factor, N, H, W), accumulate, loss, active);
    NEMAR_CHECK_LAUNCH("fold_penalty_fwd");
    return NEMAR_OK;
}

NEMAR_API int nemar_fold_penalty_bwd(const float* d, float margin, const float* gscale, float factor, float* gd, int accumulate, int N,
                                     int H, int W, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(d && gscale && gd, "fold_penalty_bwd: null pointer");
    NEMAR_REQUIRE(((((uintptr_t)d) | ((uintptr_t)gscale) | ((uintptr_t)gd)) & 3) == 0, "fold_penalty_bwd: d, gscale and gd must be 4-byte aligned");
    NEMAR_REQUIRE(fold_shape_ok(N, H, W), "fold_penalty_bwd: bad shape N=%d H=%d W=%d", N, H, W);
    NEMAR_REQUIRE(gd != d, "fold_penalty_bwd: gd must not be the operand (neighbouring tiles read it)");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(nemar_cdiv(W, RT_W), nemar_cdiv(H, RT_H), N), block(RT_THREADS);
    hipLaunchKernelGGL(fold_bwd_kernel, grid, block, 0, st, d, margin, gscale, fold_scale(factor, N, H, W), gd, accumulate, H, W);
    NEMAR_CHECK_LAUNCH("fold_penalty_bwd");
    return NEMAR_OK;
}
