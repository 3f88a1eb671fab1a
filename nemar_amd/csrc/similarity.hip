// Scoring a registration WITHOUT annotations (DESIGN.md "Intensity agreement of a registration"): how well the intensities of the
// registered moving image agree with the fixed image — the joint histogram behind mutual information (across modalities) and the five
// moments behind NCC / MSE / MAE (within one).  Not a call site of the reference, which has no evaluation code; the transformation is
// read exactly as nemar_warp_resampled_fwd (register.hip) applies it.
//
//   nemar_joint_histogram   the bilinear warp of the moving image, its channel mean a(x), the fixed image's channel mean b(x), the
//                           bins x bins table of (bin(a), bin(b)) and the moments of (a, b) in ONE pass: the warped image is the value
//                           nemar_warp_resampled_fwd(NEMAR_SAMPLE_BILINEAR) would write — the same tile, the same field patch, the same
//                           taps, all from resampled_grid.h — and is never written to memory; the fixed image is streamed beside the gather.
//
// A pixel counts iff the NEAREST texel of its sampling position lies inside the source (taps_at<SAMPLE_NEAREST>.ok: the region where
// nemar_label_overlap's warped map is not padding) and neither a nor b is NaN.
//
// Counting.  A workgroup walks 64 x 16 tiles of one sample in a grid-stride loop over as many workgroups as the chip holds at once
// (pred_launch.h: resident_groups), keeps the bins x bins uint32 table in LDS — cleared once, flushed once, with one global
// integer atomicAdd per NON-ZERO counter.  Integer addition has no order: bitwise repeatable.  Into the LDS table every lane adds for
// itself (one ds_add per counted pixel).  Adding the lanes that share the wave's first cell once, by a ballot (wave_count.h, what
// nemar_label_overlap does; nemar_tune(46, 0), measurement build) was nowhere faster beyond the spread on smooth, blocky or
// per-pixel-random images and 0 - 3 % slower at 2048^2 — a 64-pixel run of an image spreads over a few of the bins x bins cells
// where a label map hits one counter, and the ballots cost more than the adds they save: tools/microbench_similarity.py,
// tools/profiles/joint_histogram.txt.
// Moments.  No atomics: six per-lane float accumulators, one record per workgroup in the workspace, one merge kernel that folds a
// sample's records (tile_record.h).  With G workgroups per sample (G = min(tiles, what the chip holds / N)) and T = ceil(tiles / G)
// tiles per workgroup a sum passes through at most
//   4 T (lane) + 6 (wave) + 3 (workgroup)   additions in the tile kernel and   ceil(G / 256) + 6 + 3   in the merge:
//   D = 4 T + ceil(G / 256) + 18.
#include <math.h>

#include "common.h"
#include "pred_launch.h"
#include "tile_record.h"
#include "wave_count.h"

namespace {

constexpr int MAX_BINS = 64;            // 64 * 64 counters = 16 KiB of LDS beside the 9.3 KiB field patch
constexpr int MAX_CHANNELS = 64;
constexpr int SIM_WORDS = 8;            // sum a, sum b, sum a^2, sum b^2, sum ab, sum |a - b|, two unused
constexpr int SIM_SUMS = 6;

struct SimAcc {
    static constexpr int WORDS = SIM_WORDS;
    float s[SIM_SUMS];
    static __device__ __forceinline__ SimAcc empty() { return SimAcc{{0.f, 0.f, 0.f, 0.f, 0.f, 0.f}}; }
    __device__ __forceinline__ void merge(const SimAcc& b) {
#pragma unroll
        for (int k = 0; k < SIM_SUMS; ++k) s[k] += b.s[k];
    }
    __device__ __forceinline__ SimAcc shfl_xor(int o) const {
        SimAcc b;
#pragma unroll
        for (int k = 0; k < SIM_SUMS; ++k) b.s[k] = __shfl_xor(s[k], o, 64);
        return b;
    }
    __device__ __forceinline__ void store(unsigned* r) const {
#pragma unroll
        for (int k = 0; k < SIM_SUMS; ++k) r[k] = __float_as_uint(s[k]);
    }
    static __device__ __forceinline__ SimAcc load(const unsigned* r) {
        SimAcc b;
#pragma unroll
        for (int k = 0; k < SIM_SUMS; ++k) b.s[k] = __uint_as_float(r[k]);
        return b;
    }
};

// the bin of a value that is not NaN: clamp((int)floorf((v - lo) * scale), 0, bins - 1), clamped before the conversion (+-Inf, and values
// whose bin no int holds, go to the end bins)
__device__ __forceinline__ int bin_of(float v, float lo, float scale, int bins) {
    return (int)fminf(fmaxf(floorf((v - lo) * scale), 0.f), (float)(bins - 1));
}

struct SimRange {
    float lo_m, scale_m, lo_f, scale_f;      // scale = bins / (hi - lo)
};

// BCAP: the table's capacity in bins per side (bins <= BCAP) — 32 (4 KiB + the 9.3 KiB patch: eight workgroups fit a CU) or 64 (25.8 KiB: six)
template <int MODE, bool RESAMPLE, int BCAP>
__global__ __launch_bounds__(RT_THREADS) void joint_histogram_kernel(const float* __restrict__ moving, const float* __restrict__ fixed,
                                                                     const float* __restrict__ pred, unsigned* __restrict__ counts,
                                                                     float* __restrict__ partial, int Cm, int Cf, int bins, SimRange rg,
                                                                     int Hs, int Ws, int hf, int wf, int Ho, int Wo, float sh, float sw,
                                                                     int tiles_x, int tiles, int per_lane) {
    struct Lds {
        unsigned hist[BCAP * BCAP];                               // [moving bin][fixed bin], rows `bins` apart
        float patch[RESAMPLE ? 2 * RT_PH * RT_PW : 1];
        unsigned red[(RT_THREADS / 64) * SIM_WORDS];
    };
    __shared__ Lds lds;
    unsigned* hist = lds.hist;
    float* patch = lds.patch;
    const int n = blockIdx.y, tid = threadIdx.x;
    const auto pv = pred_view<MODE, RESAMPLE>(pred, n, hf, wf, Ho, Wo, sh, sw);
    const size_t splane = (size_t)Hs * Ws, oplane = pv.oplane;
    const float* mN = moving + (size_t)n * Cm * splane;
    const float* bN = fixed + (size_t)n * Cf * oplane;
    const float inv_cm = 1.f / (float)Cm, inv_cf = 1.f / (float)Cf;
    const int cells = bins * bins;

    for (int e = tid; e < cells; e += RT_THREADS) hist[e] = 0u;
    __syncthreads();

    SimAcc acc = SimAcc::empty();
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
            int key = -1;                                         // (no early exit: the whole wave reaches the ballots)
            if (h < Ho && w < Wo) {
                float gx, gy;
                pv.coord(patch, fp, h, w, gx, gy);
                const bool near_inside = taps_at<SAMPLE_NEAREST>(gx, gy, Ws, Hs).ok != 0u;
                const Taps tp = taps_at<SAMPLE_BILINEAR>(gx, gy, Ws, Hs);
                float sa = 0.f, sb = 0.f;
                for (int c = 0; c < Cm; ++c) sa += sample_at<SAMPLE_BILINEAR>(mN + (size_t)c * splane, tp);
                const size_t o = (size_t)h * Wo + w;
                for (int c = 0; c < Cf; ++c) sb += bN[(size_t)c * oplane + o];
                const float a = sa * inv_cm, b = sb * inv_cf;
                if (near_inside && a == a && b == b) {
                    key = bin_of(a, rg.lo_m, rg.scale_m, bins) * bins + bin_of(b, rg.lo_f, rg.scale_f, bins);
                    acc.s[0] += a;
                    acc.s[1] += b;
                    acc.s[2] += a * a;
                    acc.s[3] += b * b;
                    acc.s[4] += a * b;
                    acc.s[5] += fabsf(a - b);
                }
            }
            wave_count(hist, key, per_lane);
        }
    }
    __syncthreads();
    unsigned* cN = counts + (size_t)n * cells;
    for (int e = tid; e < cells; e += RT_THREADS) {
        const unsigned v = hist[e];
        if (v) atomicAdd(&cN[e], v);
    }
    if (partial) {                                                // (a launch argument: the same in every lane)
        acc = block_record(acc, lds.red);
        if (tid == 0) acc.store((unsigned*)partial + ((size_t)n * gridDim.x + blockIdx.x) * SIM_WORDS);
    }
}

// moments[n] = the sample's records merged
__global__ __launch_bounds__(256) void joint_moments_merge_kernel(const float* __restrict__ partial, int n_partial, float* __restrict__ moments) {
    __shared__ unsigned red[(256 / 64) * SIM_WORDS];
    const int n = blockIdx.x;
    const SimAcc acc = merge_records<SimAcc>((const unsigned*)partial + (size_t)n * n_partial * SIM_WORDS, n_partial, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < SIM_SUMS; ++k) moments[n * SIM_SUMS + k] = acc.s[k];
    }
}

// workgroups per sample: every workgroup clears and flushes its own table (LDS: 8 workgroups per CU with the small table, 6 with the large)
int sim_groups(int N, int bins, int Ho, int Wo) {
    return resident_groups(N, bins <= 32 ? 8 : 6, (long long)nemar_cdiv(Wo, RT_W) * nemar_cdiv(Ho, RT_H));
}

}  // namespace

// 1 (default, and the product): every lane adds for itself; nemar_tune(46, 0) (measurement build): wave-aggregated adds
NEMAR_SWITCH(int, g_histogram_per_lane, 1);

namespace {

template <int MODE, bool RESAMPLE>
void launch_histogram(const float* moving, const float* fixed, const float* pred, unsigned* counts, float* partial, int N, int Cm, int Cf, int bins,
                      SimRange rg, int Hs, int Ws, int hf, int wf, int Ho, int Wo, float sh, float sw, hipStream_t st) {
    const int tiles_x = nemar_cdiv(Wo, RT_W), tiles = tiles_x * nemar_cdiv(Ho, RT_H);
    const dim3 grid(sim_groups(N, bins, Ho, Wo), N), block(RT_THREADS);
    if (bins <= 32)
        hipLaunchKernelGGL((joint_histogram_kernel<MODE, RESAMPLE, 32>), grid, block, 0, st, moving, fixed, pred, counts, partial, Cm, Cf, bins, rg, Hs,
                           Ws, hf, wf, Ho, Wo, sh, sw, tiles_x, tiles, (int)g_histogram_per_lane);
    else
        hipLaunchKernelGGL((joint_histogram_kernel<MODE, RESAMPLE, MAX_BINS>), grid, block, 0, st, moving, fixed, pred, counts, partial, Cm, Cf, bins, rg,
                           Hs, Ws, hf, wf, Ho, Wo, sh, sw, tiles_x, tiles, (int)g_histogram_per_lane);
}

}  // namespace

// (the largest table: the size does not depend on `bins`, which the query does not take)
NEMAR_API size_t nemar_joint_histogram_workspace(int N, int Ho, int Wo) {
    if (N <= 0 || Ho <= 0 || Wo <= 0) return 0;
    return sizeof(float) * SIM_WORDS * (size_t)sim_groups(N, 2, Ho, Wo) * N;
}

NEMAR_API int nemar_joint_histogram(const float* moving, const float* fixed, const float* pred, int grid_mode, unsigned* counts, float* moments,
                                    void* workspace, size_t ws_bytes, int N, int Cm, int Cf, int bins, float lo_m, float hi_m, float lo_f,
                                    float hi_f, int Hs, int Ws, int hf, int wf, int Ho, int Wo, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(moving && fixed && pred && counts, "joint_histogram: null pointer");
    NEMAR_REQUIRE(!moments || workspace, "joint_histogram: moments need a workspace");
    NEMAR_REQUIRE(((((uintptr_t)moving) | ((uintptr_t)fixed) | ((uintptr_t)pred) | ((uintptr_t)counts) | ((uintptr_t)moments) |
                    (moments ? (uintptr_t)workspace : 0)) & 3) == 0,
                  "joint_histogram: moving, fixed, pred, counts, moments and workspace must be 4-byte aligned");
    NEMAR_REQUIRE(N > 0 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0, "joint_histogram: bad shape N=%d source %dx%d output %dx%d", N, Hs, Ws, Ho, Wo);
    NEMAR_REQUIRE(bins >= 2 && bins <= MAX_BINS, "joint_histogram: %d bins (2 .. %d)", bins, MAX_BINS);
    NEMAR_REQUIRE(Cm >= 1 && Cm <= MAX_CHANNELS && Cf >= 1 && Cf <= MAX_CHANNELS, "joint_histogram: %d and %d channels (1 .. %d)", Cm, Cf, MAX_CHANNELS);
    NEMAR_REQUIRE(hi_m > lo_m && hi_f > lo_f, "joint_histogram: empty range [%g, %g] or [%g, %g]", (double)lo_m, (double)hi_m, (double)lo_f, (double)hi_f);
    const SimRange rg{lo_m, (float)bins / (hi_m - lo_m), lo_f, (float)bins / (hi_f - lo_f)};
    NEMAR_REQUIRE(isfinite(lo_m) && isfinite(lo_f) && isfinite(rg.scale_m) && isfinite(rg.scale_f) && rg.scale_m > 0.f && rg.scale_f > 0.f,
                  "joint_histogram: range [%g, %g] or [%g, %g] has no finite bin width", (double)lo_m, (double)hi_m, (double)lo_f, (double)hi_f);
    NEMAR_REQUIRE((long long)Hs * Ws < (1ll << 31), "joint_histogram: source plane too large");
    NEMAR_REQUIRE_OK(pred_ok("joint_histogram", "", grid_mode, hf, wf) && tile_grid_ok("joint_histogram", N, Ho, Wo));
    NEMAR_REQUIRE(!moments || ws_bytes >= nemar_joint_histogram_workspace(N, Ho, Wo), "joint_histogram: workspace %zu < %zu", ws_bytes,
                  nemar_joint_histogram_workspace(N, Ho, Wo));
    hipStream_t st = (hipStream_t)stream;
    float* partial = moments ? (float*)workspace : nullptr;
    NEMAR_HIP_CALL(hipMemsetAsync(counts, 0, (size_t)N * bins * bins * sizeof(unsigned), st));
    dispatch_pred(grid_mode, hf, wf, Ho, Wo, [&](auto mode, auto resample, int hf, int wf, float sh, float sw) {
        launch_histogram<decltype(mode)::value, decltype(resample)::value>(moving, fixed, pred, counts, partial, N, Cm, Cf, bins, rg, Hs, Ws, hf, wf,
                                                                           Ho, Wo, sh, sw, st);
    });
    if (moments)
        hipLaunchKernelGGL(joint_moments_merge_kernel, dim3(N), dim3(256), 0, st, (const float*)partial, sim_groups(N, bins, Ho, Wo), moments);
    NEMAR_CHECK_LAUNCH("joint_histogram");
    return NEMAR_OK;
}
