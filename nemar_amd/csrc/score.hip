// Scoring a registration of real data (DESIGN.md "Scoring a registration"): what the NeMAR paper reports (distances between annotated
// point pairs) and what everyone else in registration reports (segmentation overlap, Dice).  Not call sites of the reference, which has
// no evaluation code; both read the transformation exactly as nemar_warp_resampled_fwd (register.hip) applies it.
//
//   nemar_label_overlap   the nearest-sampled warp of a label map and its per-class agreement with the fixed map in ONE pass: the
//                         warped map m(x) is the value nemar_warp_resampled_fwd(NEMAR_SAMPLE_NEAREST) would write — the same tile, the
//                         same field patch, the same rounding, all from resampled_grid.h — and is never written to memory: 4 B/px of
//                         the fixed map are streamed where the warp would store 4 B/px, and the gather is the warp's own.
//   nemar_map_points      S(p), the position the warp samples for an annotated point p between (or beyond) the pixels.
//
// Counting.  A workgroup walks 64 x 16 tiles of one sample (a grid-stride loop over as many workgroups as the chip holds at once, so
// that the histogram is cleared and flushed a few times per sample and not once per tile) and keeps `3 * K` uint32 counters in LDS — inter, moving, fixed per
// class —, which it adds to `counts` with one global integer atomicAdd per NON-ZERO counter at the end.  The counts are integers:
// addition is associative and commutative, so the result does not depend on the order in which lanes, waves or workgroups arrive and is
// bitwise repeatable with no fixed-order merge and no workspace (unlike the float sums of nemar_registration_error).
// Label maps are piecewise constant, and a wave covers 64 consecutive pixels of one row, so most waves hit ONE counter: the lanes
// that share the key of the wave's first counting lane are counted by a ballot and added once (one ds_add of the popcount), the rest —
// none inside a segment, a few across a boundary — add for themselves.  tools/microbench_score.py times this against per-lane adds
// (nemar_tune(45, 1), measurement build) on blocky, single-class and per-pixel-random maps: tools/profiles/label_overlap.txt.
#include "common.h"
#include "label_class.h"
#include "pred_launch.h"
#include "wave_count.h"

namespace {

// (MAX_CLASSES, class_of: label_class.h — 3 * 1024 counters = 12 KiB of LDS beside the 9.3 KiB field patch)

// KCAP: the histogram's capacity in classes (K <= KCAP) — 256 (3 KiB + the 9.3 KiB patch: eight workgroups fit a CU's LDS) or 1024
// (21.3 KiB: seven)
template <int MODE, bool RESAMPLE, int KCAP>
__global__ __launch_bounds__(RT_THREADS) void label_overlap_kernel(const float* __restrict__ lm, const float* __restrict__ lf,
                                                                   const float* __restrict__ pred, unsigned* __restrict__ counts, int K,
                                                                   int Hs, int Ws, int hf, int wf, int Ho, int Wo, float sh, float sw,
                                                                   int tiles_x, int tiles, int per_lane) {
    struct Lds {
        unsigned hist[3 * KCAP];                                  // [0,K) inter, [K,2K) moving, [2K,3K) fixed
        float patch[RESAMPLE ? 2 * RT_PH * RT_PW : 1];
    };
    __shared__ Lds lds;
    unsigned* hist = lds.hist;
    float* patch = lds.patch;
    const int n = blockIdx.y, tid = threadIdx.x;
    const auto pv = pred_view<MODE, RESAMPLE>(pred, n, hf, wf, Ho, Wo, sh, sw);
    const float* lmN = lm + (size_t)n * Hs * Ws;
    const float* lfN = lf + (size_t)n * pv.oplane;

    for (int e = tid; e < 3 * K; e += RT_THREADS) hist[e] = 0u;
    __syncthreads();

    constexpr int ROWS = RT_THREADS / RT_W, RUNS = RT_H / ROWS;    // a lane owns one pixel in each of RUNS rows: a wave = 64 pixels of a row
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {         // (the same trip count in every lane of the workgroup)
        const int tyi = t / tiles_x;
        const int x0 = (t - tyi * tiles_x) * RT_W, y0 = tyi * RT_H;
        if (RESAMPLE) __syncthreads();                            // the previous tile's readers are done with the patch
        const FieldPatch fp = pv.stage(patch, x0, y0, tid);
        if (RESAMPLE) __syncthreads();
#pragma unroll
        for (int i = 0; i < RUNS; ++i) {
            const int h = y0 + tid / RT_W + ROWS * i, w = x0 + tid % RT_W;
            const bool inside = h < Ho && w < Wo;                 // (no early exit: the whole wave reaches the ballots)
            int km = -1, kf = -1;
            if (inside) {
                float gx, gy;
                pv.coord(patch, fp, h, w, gx, gy);
                const Taps tp = taps_at<SAMPLE_NEAREST>(gx, gy, Ws, Hs);
                km = class_of(sample_at<SAMPLE_NEAREST>(lmN, tp), K);
                kf = class_of(lfN[(size_t)h * Wo + w], K);
            }
            wave_count(hist, km == kf ? km : -1, per_lane);
            wave_count(hist + K, km, per_lane);
            wave_count(hist + 2 * K, kf, per_lane);
        }
    }
    __syncthreads();
    unsigned* cN = counts + (size_t)n * K * 3;                    // [K,3]: inter, moving, fixed
    for (int e = tid; e < 3 * K; e += RT_THREADS) {
        const unsigned v = hist[e];
        const int which = e / K, k = e - which * K;
        if (v) atomicAdd(&cN[k * 3 + which], v);
    }
}

__global__ __launch_bounds__(64) void map_points_kernel(const float* __restrict__ pts, const float* __restrict__ pred, int mode,
                                                        float* __restrict__ out, int P, int Hs, int Ws, int hf, int wf, int Ho, int Wo,
                                                        float sh, float sw) {
    const int n = blockIdx.y, i = blockIdx.x * 64 + threadIdx.x;
    if (i >= P) return;
    const size_t o = ((size_t)n * P + i) * 2;
    const float qx = pts[o], qy = pts[o + 1];
    const bool missing = qx != qx || qy != qy;                     // a NaN coordinate: a missing annotation
    const float px = missing ? 0.f : qx, py = missing ? 0.f : qy;
    float gx, gy;
    if (mode == GRID_UNET) {
        // the offsets at the point: the align_corners=False resize of `pred` evaluated at a continuous coordinate (resampled_grid.h)
        grid_at<GRID_UNET>(pred + (size_t)n * 2 * hf * wf, hf, wf, sh, sw, nullptr, px, py, Ho, Wo, gx, gy);
    } else {
        float th[6];
        affine_theta(pred, n, th);
        grid_at<GRID_AFFINE>(nullptr, hf, wf, sh, sw, th, px, py, Ho, Wo, gx, gy);
    }
    float ix, iy;
    sample_position(gx, gy, Ws, Hs, ix, iy);
    const float nan = __uint_as_float(0x7fc00000u);
    out[o] = missing ? nan : ix;
    out[o + 1] = missing ? nan : iy;
}

}  // namespace

// nemar_tune(45, 1) (measurement build): every lane adds for itself; 0 (default, and the product): wave-aggregated adds
NEMAR_SWITCH(int, g_overlap_per_lane, 0);

namespace {

template <int MODE, bool RESAMPLE>
void launch_overlap(const float* lm, const float* lf, const float* pred, unsigned* counts, int N, int K, int Hs, int Ws, int hf, int wf, int Ho,
                    int Wo, float sh, float sw, hipStream_t st) {
    const int tiles_x = nemar_cdiv(Wo, RT_W), tiles = tiles_x * nemar_cdiv(Ho, RT_H);
    // every workgroup clears and flushes its own 3K counters (LDS: 8 workgroups per CU with the small histogram, 6 with the large)
    const dim3 grid(resident_groups(N, K <= 256 ? 8 : 6, tiles), N), block(RT_THREADS);
    if (K <= 256)
        hipLaunchKernelGGL((label_overlap_kernel<MODE, RESAMPLE, 256>), grid, block, 0, st, lm, lf, pred, counts, K, Hs, Ws, hf, wf, Ho, Wo, sh, sw, tiles_x,
                           tiles, (int)g_overlap_per_lane);
    else
        hipLaunchKernelGGL((label_overlap_kernel<MODE, RESAMPLE, MAX_CLASSES>), grid, block, 0, st, lm, lf, pred, counts, K, Hs, Ws, hf, wf, Ho, Wo, sh, sw,
                           tiles_x, tiles, (int)g_overlap_per_lane);
}

}  // namespace

NEMAR_API int nemar_label_overlap(const float* labels_moving, const float* labels_fixed, const float* pred, int grid_mode, unsigned* counts,
                                  int N, int K, int Hs, int Ws, int hf, int wf, int Ho, int Wo, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(labels_moving && labels_fixed && pred && counts, "label_overlap: null pointer");
    NEMAR_REQUIRE(((((uintptr_t)labels_moving) | ((uintptr_t)labels_fixed) | ((uintptr_t)pred) | ((uintptr_t)counts)) & 3) == 0,
                  "label_overlap: labels_moving, labels_fixed, pred and counts must be 4-byte aligned");
    NEMAR_REQUIRE(N > 0 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0, "label_overlap: bad shape N=%d source %dx%d output %dx%d", N, Hs, Ws, Ho, Wo);
    NEMAR_REQUIRE(K >= 1 && K <= MAX_CLASSES, "label_overlap: %d classes (1 .. %d)", K, MAX_CLASSES);
    NEMAR_REQUIRE((long long)Hs * Ws < (1ll << 31), "label_overlap: source plane too large");
    NEMAR_REQUIRE_OK(pred_ok("label_overlap", "", grid_mode, hf, wf) && tile_grid_ok("label_overlap", N, Ho, Wo));
    hipStream_t st = (hipStream_t)stream;
    NEMAR_HIP_CALL(hipMemsetAsync(counts, 0, (size_t)N * K * 3 * sizeof(unsigned), st));
    dispatch_pred(grid_mode, hf, wf, Ho, Wo, [&](auto mode, auto resample, int hf, int wf, float sh, float sw) {
        launch_overlap<decltype(mode)::value, decltype(resample)::value>(labels_moving, labels_fixed, pred, counts, N, K, Hs, Ws, hf, wf, Ho, Wo,
                                                                         sh, sw, st);
    });
    NEMAR_CHECK_LAUNCH("label_overlap");
    return NEMAR_OK;
}

NEMAR_API int nemar_map_points(const float* pts, const float* pred, int grid_mode, float* out, int N, int P, int Hs, int Ws, int hf, int wf,
                               int Ho, int Wo, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(pts && pred && out, "map_points: null pointer");
    NEMAR_REQUIRE(((((uintptr_t)pts) | ((uintptr_t)pred) | ((uintptr_t)out)) & 3) == 0, "map_points: pts, pred and out must be 4-byte aligned");
    NEMAR_REQUIRE(N > 0 && N <= 65535 && P > 0 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0, "map_points: bad shape N=%d P=%d source %dx%d output %dx%d",
                  N, P, Hs, Ws, Ho, Wo);
    // (no tile grid: a point needs no output plane, and (Ho, Wo) may be any size)
    NEMAR_REQUIRE_OK(pred_ok("map_points", "", grid_mode, hf, wf));
    if (grid_mode != GRID_UNET) hf = wf = 1;
    hipLaunchKernelGGL(map_points_kernel, dim3(nemar_cdiv(P, 64), N), dim3(64), 0, (hipStream_t)stream, pts, pred, grid_mode, out, P, Hs, Ws, hf, wf,
                       Ho, Wo, (float)hf / (float)Ho, (float)wf / (float)Wo);
    NEMAR_CHECK_LAUNCH("map_points");
    return NEMAR_OK;
}
