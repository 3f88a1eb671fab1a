// How regular a registration is (DESIGN.md "Regularity of a registration"): the forward-difference Jacobian determinant of the
// transformation a prediction describes at output size (Ho, Wo), as a map (optional) and as per-sample statistics, in one pass.  Not a
// call site of the reference, which has no evaluation code.  For output pixel (h, w): (gx, gy) = resampled_coord, the normalised
// coordinate nemar_warp_resampled_fwd, nemar_label_overlap and nemar_compose_pred compute; p = sample_position(gx, gy, Wo, Ho), the
// position in pixels of an image of the output's own size (a pure resize has determinant 1); with a = p(h, w+1) - p(h, w) and
// b = p(h+1, w) - p(h, w), det = a.x * b.y - b.x * a.y — registration_error_kernel's expression, in its order.  A pixel is interior when
// it has both forward neighbours; det <= 0 is a fold.
//
// One workgroup per 64 x 16 output tile (resampled_grid.h, as register.hip and compose.hip).  The neighbour of a pixel in the tile's
// last column or row lies in the NEXT tile and must be the bits resampled_coord gives THAT pixel there, or neighbouring tiles would
// disagree.  So the workgroup first writes the positions of a 65 x 17 tile into LDS: its own 64 x 16 pixels through the staged field
// patch, the halo column and row through the un-staged field_at(fN, ...) path — the patch holds copies of the same texels and the
// blend is the same expression, so the value is the one the next tile computes for its own pixel (stage_field's patch covers the
// tile's own pixels only: a 65-pixel row can tap one texel more).  Differences are then taken from LDS, a lane owning one pixel in
// each of four rows.
// Every statistic is accumulated from the very `det` the map gets: counts and stats are the same bits with and without det_out.
// Per-workgroup partials (JAC_WORDS words) go to the workspace and one merge kernel reads them in a fixed order — the scheme of
// registration_error_merge_kernel; no atomics, bitwise repeatable.  A sum passes through at most 4 (lane) + 6 (wave) + 3 (workgroup)
// additions in the tile kernel and ceil(tiles / 256) + 6 + 3 in the merge.
#include <math.h>

#include "common.h"
#include "jacobian_tile.h"

namespace {

constexpr int JAC_WORDS = 8;      // interior (u32), folds (u32), min, max, sum det, sum log det, sum (log det)^2 (f32), one unused

struct JacAcc {
    unsigned interior, folds;
    float mn, mx, sum, slog, slog2;
};
__device__ __forceinline__ JacAcc jac_empty() { return JacAcc{0u, 0u, INFINITY, -INFINITY, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ void jac_merge(JacAcc& a, const JacAcc& b) {
    a.interior += b.interior;
    a.folds += b.folds;
    a.mn = fminf(a.mn, b.mn);
    a.mx = fmaxf(a.mx, b.mx);
    a.sum += b.sum;
    a.slog += b.slog;
    a.slog2 += b.slog2;
}
// the workgroup's totals, valid in thread 0: the xor tree of each wave, then the waves in ascending order (a fixed tree: the same bits on
// every run).  `red` is JAC_WORDS words of LDS per wave
__device__ __forceinline__ JacAcc jac_block(JacAcc a, unsigned* red) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        JacAcc b;
        b.interior = (unsigned)__shfl_xor((int)a.interior, o, 64);
        b.folds = (unsigned)__shfl_xor((int)a.folds, o, 64);
        b.mn = __shfl_xor(a.mn, o, 64);
        b.mx = __shfl_xor(a.mx, o, 64);
        b.sum = __shfl_xor(a.sum, o, 64);
        b.slog = __shfl_xor(a.slog, o, 64);
        b.slog2 = __shfl_xor(a.slog2, o, 64);
        jac_merge(a, b);
    }
    __syncthreads();      // protect `red` from a previous use
    if (lane == 0) {
        unsigned* r = red + wid * JAC_WORDS;
        r[0] = a.interior; r[1] = a.folds; r[2] = __float_as_uint(a.mn); r[3] = __float_as_uint(a.mx);
        r[4] = __float_as_uint(a.sum); r[5] = __float_as_uint(a.slog); r[6] = __float_as_uint(a.slog2);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < nw; ++i) {
            const unsigned* r = red + i * JAC_WORDS;
            jac_merge(a, JacAcc{r[0], r[1], __uint_as_float(r[2]), __uint_as_float(r[3]), __uint_as_float(r[4]), __uint_as_float(r[5]),
                                __uint_as_float(r[6])});
        }
    }
    return a;
}

template <int MODE, bool RESAMPLE>
__global__ __launch_bounds__(RT_THREADS) void jacobian_kernel(const float* __restrict__ pred, float* __restrict__ det_out,
                                                              unsigned* __restrict__ partial, int hf, int wf, int Ho, int Wo, float sh,
                                                              float sw) {
    __shared__ float patch[RESAMPLE ? 2 * RT_PH * RT_PW : 1];
    __shared__ float pos[2 * JT_H * JT_W];                          // p of the 65 x 17 tile: x plane, then y plane
    __shared__ unsigned red[(RT_THREADS / 64) * JAC_WORDS];
    const int n = blockIdx.z, tid = threadIdx.x;
    const int x0 = blockIdx.x * RT_W, y0 = blockIdx.y * RT_H;
    float th[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (MODE == GRID_AFFINE) {
        affine_theta(pred, n, th);
    }
    const size_t plane = (size_t)Ho * Wo;
    const int fplane = RESAMPLE ? hf * wf : 0;
    const float* fN = MODE == GRID_UNET ? pred + (size_t)n * 2 * (RESAMPLE ? (size_t)fplane : plane) : nullptr;

    FieldPatch fp{0, 0, false};
    if (RESAMPLE) {
        fp = stage_field(patch, fN, fplane, x0, y0, hf, wf, Ho, Wo, sh, sw, tid);
        __syncthreads();
    }
    for (int e = tid; e < JT_H * JT_W; e += RT_THREADS) {
        const int r = e / JT_W, c = e - r * JT_W;
        const int h = y0 + r, w = x0 + c;
        if (h >= Ho || w >= Wo) continue;
        // the halo belongs to the next tile, whose patch is another: read the field itself there
        const FieldPatch use{fp.px0, fp.py0, fp.staged && r < RT_H && c < RT_W};
        float gx, gy, px, py;
        resampled_coord<MODE, RESAMPLE>(patch, use, fN, fplane, plane, h, w, hf, wf, Ho, Wo, sh, sw, th, gx, gy);
        sample_position(gx, gy, Wo, Ho, px, py);
        pos[e] = px;
        pos[JT_H * JT_W + e] = py;
    }
    __syncthreads();

    JacAcc acc = jac_empty();
    float* dN = det_out ? det_out + (size_t)n * plane : nullptr;
    constexpr int ROWS = RT_THREADS / RT_W, RUNS = RT_H / ROWS;      // a lane owns one pixel in each of RUNS rows: a wave = 64 pixels of a row
#pragma unroll
    for (int i = 0; i < RUNS; ++i) {
        const int r = tid / RT_W + ROWS * i, c = tid % RT_W;
        const int h = y0 + r, w = x0 + c;
        if (h >= Ho || w >= Wo) continue;
        float det = __uint_as_float(0x7fc00000u);                  // the last row and column have no forward neighbour: a quiet NaN
        if (h < Ho - 1 && w < Wo - 1) {
            const float* qx = pos + r * JT_W + c;
            const float* qy = qx + JT_H * JT_W;
            const float ix = qx[0], iy = qy[0];
            det = jac_det(ix, iy, qx[1], qy[1], qx[JT_W], qy[JT_W]);      // (jacobian_tile.h: shared with fold.hip)
            acc.interior += 1u;
            acc.mn = fminf(acc.mn, det);
            acc.mx = fmaxf(acc.mx, det);
            acc.sum += det;
            if (det <= 0.f) {
                acc.folds += 1u;
            } else if (det > 0.f) {                                 // (a NaN determinant is neither)
                const float l = logf(det);
                acc.slog += l;
                acc.slog2 += l * l;
            }
        }
        if (dN) dN[(size_t)h * Wo + w] = det;
    }
    acc = jac_block(acc, red);
    if (tid == 0) {
        unsigned* dst = partial + (((size_t)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * JAC_WORDS;
        dst[0] = acc.interior; dst[1] = acc.folds; dst[2] = __float_as_uint(acc.mn); dst[3] = __float_as_uint(acc.mx);
        dst[4] = __float_as_uint(acc.sum); dst[5] = __float_as_uint(acc.slog); dst[6] = __float_as_uint(acc.slog2);
    }
}

// counts[n], stats[n] = the sample's partials merged: thread t takes partials t, t + 256, ... in ascending order, then the fixed workgroup tree
__global__ __launch_bounds__(256) void jacobian_merge_kernel(const unsigned* __restrict__ partial, int n_partial, unsigned* __restrict__ counts,
                                                             float* __restrict__ stats) {
    __shared__ unsigned red[(256 / 64) * JAC_WORDS];
    const int n = blockIdx.x;
    const unsigned* p = partial + (size_t)n * n_partial * JAC_WORDS;
    JacAcc acc = jac_empty();
    for (int i = threadIdx.x; i < n_partial; i += blockDim.x) {
        const unsigned* q = p + (size_t)i * JAC_WORDS;
        jac_merge(acc, JacAcc{q[0], q[1], __uint_as_float(q[2]), __uint_as_float(q[3]), __uint_as_float(q[4]), __uint_as_float(q[5]),
                              __uint_as_float(q[6])});
    }
    acc = jac_block(acc, red);
    if (threadIdx.x == 0) {
        counts[n * 2] = acc.interior;
        counts[n * 2 + 1] = acc.folds;
        float* s = stats + n * 5;
        s[0] = acc.mn; s[1] = acc.mx; s[2] = acc.sum; s[3] = acc.slog; s[4] = acc.slog2;
    }
}

long long jac_tiles(int Ho, int Wo) { return (long long)nemar_cdiv(Wo, RT_W) * nemar_cdiv(Ho, RT_H); }

template <int MODE, bool RESAMPLE>
void launch(const float* pred, float* det_out, unsigned* partial, int N, int hf, int wf, int Ho, int Wo, hipStream_t st) {
    const dim3 grid(nemar_cdiv(Wo, RT_W), nemar_cdiv(Ho, RT_H), N), block(RT_THREADS);
    // nemar_bilinear_fwd's scales, of the field to the output size
    hipLaunchKernelGGL((jacobian_kernel<MODE, RESAMPLE>), grid, block, 0, st, pred, det_out, partial, hf, wf, Ho, Wo, (float)hf / (float)Ho,
                       (float)wf / (float)Wo);
}

}  // namespace

NEMAR_API size_t nemar_jacobian_stats_workspace(int N, int Ho, int Wo) {
    if (N <= 0 || Ho <= 0 || Wo <= 0) return 0;
    return sizeof(unsigned) * JAC_WORDS * (size_t)jac_tiles(Ho, Wo) * N;
}

NEMAR_API int nemar_jacobian_stats(const float* pred, int grid_mode, float* det_out, unsigned* counts, float* stats, void* workspace,
                                   size_t ws_bytes, int N, int hf, int wf, int Ho, int Wo, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(pred && counts && stats && workspace, "jacobian_stats: null pointer");
    NEMAR_REQUIRE(((((uintptr_t)pred) | ((uintptr_t)det_out) | ((uintptr_t)counts) | ((uintptr_t)stats) | ((uintptr_t)workspace)) & 3) == 0,
                  "jacobian_stats: pred, det_out, counts, stats and workspace must be 4-byte aligned");
    NEMAR_REQUIRE(grid_mode == GRID_UNET || grid_mode == GRID_AFFINE,
                  "jacobian_stats: grid_mode %d (NEMAR_GRID_UNET or NEMAR_GRID_AFFINE: an explicit grid has no other resolution)", grid_mode);
    NEMAR_REQUIRE(N > 0 && Ho > 0 && Wo > 0, "jacobian_stats: bad shape N=%d size %dx%d", N, Ho, Wo);
    NEMAR_REQUIRE(grid_mode != GRID_UNET || (hf >= 1 && wf >= 1), "jacobian_stats: offset field %d x %d", hf, wf);
    NEMAR_REQUIRE((long long)Ho * Wo < (1ll << 31) && N <= 65535 && nemar_cdiv(Ho, RT_H) <= 65535 &&
                      (grid_mode != GRID_UNET || (long long)hf * wf < (1ll << 30)),
                  "jacobian_stats: plane too large");
    NEMAR_REQUIRE(det_out != pred, "jacobian_stats: det_out must not be the operand (neighbouring tiles read it)");
    NEMAR_REQUIRE(ws_bytes >= nemar_jacobian_stats_workspace(N, Ho, Wo), "jacobian_stats: workspace %zu < %zu", ws_bytes,
                  nemar_jacobian_stats_workspace(N, Ho, Wo));
    hipStream_t st = (hipStream_t)stream;
    unsigned* partial = (unsigned*)workspace;
    if (grid_mode == GRID_AFFINE) launch<GRID_AFFINE, false>(pred, det_out, partial, N, 1, 1, Ho, Wo, st);
    else if (hf != Ho || wf != Wo) launch<GRID_UNET, true>(pred, det_out, partial, N, hf, wf, Ho, Wo, st);
    else launch<GRID_UNET, false>(pred, det_out, partial, N, hf, wf, Ho, Wo, st);
    hipLaunchKernelGGL(jacobian_merge_kernel, dim3(N), dim3(256), 0, st, (const unsigned*)partial, (int)jac_tiles(Ho, Wo), counts, stats);
    NEMAR_CHECK_LAUNCH("jacobian_stats");
    return NEMAR_OK;
}
