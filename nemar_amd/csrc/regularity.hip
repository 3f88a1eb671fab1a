// How regular a registration is (DESIGN.md "Regularity of a registration"): the forward-difference Jacobian determinant of the
// transformation a prediction describes at output size (Ho, Wo), as a map (optional) and as per-sample statistics, in one pass.  Not a
// call site of the reference, which has no evaluation code.  For output pixel (h, w): (gx, gy) = PredView::coord, the normalised
// coordinate nemar_warp_resampled_fwd, nemar_label_overlap and nemar_compose_pred compute; p = sample_position(gx, gy, Wo, Ho), the
// position in pixels of an image of the output's own size (a pure resize has determinant 1); with a = p(h, w+1) - p(h, w) and
// b = p(h+1, w) - p(h, w), det = a.x * b.y - b.x * a.y — registration_error_kernel's expression, in its order.  A pixel is interior when
// it has both forward neighbours; det <= 0 is a fold.
//
// One workgroup per 64 x 16 output tile (resampled_grid.h).  The neighbour of a pixel in the tile's last column or row lies in the
// NEXT tile and must be the bits PredView::coord gives THAT pixel there, or neighbouring tiles would disagree.  So the workgroup
// first writes the positions of a 65 x 17 tile into LDS: its own 64 x 16 pixels through the staged field patch, the halo column and
// row through the un-staged field_at(fN, ...) path — the patch holds copies of the same texels and the blend is the same
// expression, so the value is the one the next tile computes for its own pixel (a staged patch covers the tile's own pixels only: a
// 65-pixel row can tap one texel more).  Differences are then taken from LDS, a lane owning one pixel in each of four rows.
// Every statistic is accumulated from the very `det` the map gets: counts and stats are the same bits with and without det_out.
// One record (JAC_WORDS words) per workgroup goes to the workspace and one merge kernel folds a sample's records (tile_record.h): no
// atomics, bitwise repeatable.  A sum passes through at most 4 (lane) + 6 (wave) + 3 (workgroup) additions in the tile kernel and
// ceil(tiles / 256) + 6 + 3 in the merge.
#include <math.h>

#include "common.h"
#include "jacobian_tile.h"
#include "pred_launch.h"
#include "tile_record.h"

namespace {

constexpr int JAC_WORDS = 8;      // interior (u32), folds (u32), min, max, sum det, sum log det, sum (log det)^2 (f32), one unused

struct JacAcc {
    static constexpr int WORDS = JAC_WORDS;
    unsigned interior, folds;
    float mn, mx, sum, slog, slog2;
    static __device__ __forceinline__ JacAcc empty() { return JacAcc{0u, 0u, INFINITY, -INFINITY, 0.f, 0.f, 0.f}; }
    __device__ __forceinline__ void merge(const JacAcc& b) {
        interior += b.interior;
        folds += b.folds;
        mn = fminf(mn, b.mn);
        mx = fmaxf(mx, b.mx);
        sum += b.sum;
        slog += b.slog;
        slog2 += b.slog2;
    }
    __device__ __forceinline__ JacAcc shfl_xor(int o) const {
        return JacAcc{(unsigned)__shfl_xor((int)interior, o, 64), (unsigned)__shfl_xor((int)folds, o, 64), __shfl_xor(mn, o, 64),
                      __shfl_xor(mx, o, 64), __shfl_xor(sum, o, 64), __shfl_xor(slog, o, 64), __shfl_xor(slog2, o, 64)};
    }
    __device__ __forceinline__ void store(unsigned* r) const {
        r[0] = interior; r[1] = folds; r[2] = __float_as_uint(mn); r[3] = __float_as_uint(mx);
        r[4] = __float_as_uint(sum); r[5] = __float_as_uint(slog); r[6] = __float_as_uint(slog2);
    }
    static __device__ __forceinline__ JacAcc load(const unsigned* r) {
        return JacAcc{r[0], r[1], __uint_as_float(r[2]), __uint_as_float(r[3]), __uint_as_float(r[4]), __uint_as_float(r[5]), __uint_as_float(r[6])};
    }
};

template <int MODE, bool RESAMPLE>
__global__ __launch_bounds__(RT_THREADS) void jacobian_kernel(const float* __restrict__ pred, float* __restrict__ det_out,
                                                              unsigned* __restrict__ partial, int hf, int wf, int Ho, int Wo, float sh,
                                                              float sw) {
    __shared__ float patch[RESAMPLE ? 2 * RT_PH * RT_PW : 1];
    __shared__ float pos[2 * JT_H * JT_W];                          // p of the 65 x 17 tile: x plane, then y plane
    __shared__ unsigned red[(RT_THREADS / 64) * JAC_WORDS];
    const int n = blockIdx.z, tid = threadIdx.x;
    const int x0 = blockIdx.x * RT_W, y0 = blockIdx.y * RT_H;
    const auto pv = pred_view<MODE, RESAMPLE>(pred, n, hf, wf, Ho, Wo, sh, sw);
    const size_t plane = pv.oplane;

    const FieldPatch fp = pv.stage(patch, x0, y0, tid);
    if (RESAMPLE) __syncthreads();
    for (int e = tid; e < JT_H * JT_W; e += RT_THREADS) {
        const int r = e / JT_W, c = e - r * JT_W;
        const int h = y0 + r, w = x0 + c;
        if (h >= Ho || w >= Wo) continue;
        // the halo belongs to the next tile, whose patch is another: read the field itself there, as coord_unstaged does — in ONE call
        // with the patch switched off per lane (nearly every wave holds a halo pixel, and would run the arithmetic of two calls twice)
        const FieldPatch use{fp.px0, fp.py0, fp.staged && r < RT_H && c < RT_W};
        float gx, gy, px, py;
        pv.coord(patch, use, h, w, gx, gy);
        sample_position(gx, gy, Wo, Ho, px, py);
        pos[e] = px;
        pos[JT_H * JT_W + e] = py;
    }
    __syncthreads();

    JacAcc acc = JacAcc::empty();
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
    acc = block_record(acc, red);
    if (tid == 0) acc.store(partial + (((size_t)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * JAC_WORDS);
}

// counts[n], stats[n] = the sample's records merged
__global__ __launch_bounds__(256) void jacobian_merge_kernel(const unsigned* __restrict__ partial, int n_partial, unsigned* __restrict__ counts,
                                                             float* __restrict__ stats) {
    __shared__ unsigned red[(256 / 64) * JAC_WORDS];
    const int n = blockIdx.x;
    const JacAcc acc = merge_records<JacAcc>(partial + (size_t)n * n_partial * JAC_WORDS, n_partial, red);
    if (threadIdx.x == 0) {
        counts[n * 2] = acc.interior;
        counts[n * 2 + 1] = acc.folds;
        float* s = stats + n * 5;
        s[0] = acc.mn; s[1] = acc.mx; s[2] = acc.sum; s[3] = acc.slog; s[4] = acc.slog2;
    }
}

long long jac_tiles(int Ho, int Wo) { return (long long)nemar_cdiv(Wo, RT_W) * nemar_cdiv(Ho, RT_H); }

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
    NEMAR_REQUIRE(N > 0 && Ho > 0 && Wo > 0, "jacobian_stats: bad shape N=%d size %dx%d", N, Ho, Wo);
    NEMAR_REQUIRE_OK(pred_ok("jacobian_stats", "", grid_mode, hf, wf) && tile_grid_ok("jacobian_stats", N, Ho, Wo));
    NEMAR_REQUIRE(det_out != pred, "jacobian_stats: det_out must not be the operand (neighbouring tiles read it)");
    NEMAR_REQUIRE(ws_bytes >= nemar_jacobian_stats_workspace(N, Ho, Wo), "jacobian_stats: workspace %zu < %zu", ws_bytes,
                  nemar_jacobian_stats_workspace(N, Ho, Wo));
    hipStream_t st = (hipStream_t)stream;
    unsigned* partial = (unsigned*)workspace;
    const dim3 grid(nemar_cdiv(Wo, RT_W), nemar_cdiv(Ho, RT_H), N), block(RT_THREADS);
    dispatch_pred(grid_mode, hf, wf, Ho, Wo, [&](auto mode, auto resample, int hf, int wf, float sh, float sw) {
        hipLaunchKernelGGL((jacobian_kernel<decltype(mode)::value, decltype(resample)::value>), grid, block, 0, st, pred, det_out, partial, hf, wf,
                           Ho, Wo, sh, sw);
    });
    hipLaunchKernelGGL(jacobian_merge_kernel, dim3(N), dim3(256), 0, st, (const unsigned*)partial, (int)jac_tiles(Ho, Wo), counts, stats);
    NEMAR_CHECK_LAUNCH("jacobian_stats");
    return NEMAR_OK;
}
