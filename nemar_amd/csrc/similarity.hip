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
// Counting.  nemar_label_overlap's structure (score.hip): a workgroup walks 64 x 16 tiles of one sample in a grid-stride loop over as
// many workgroups as the chip holds at once, keeps the bins x bins uint32 table in LDS — cleared once, flushed once, with one global
// integer atomicAdd per NON-ZERO counter.  Integer addition has no order: bitwise repeatable.  Into the LDS table every lane adds for
// itself (one ds_add per counted pixel).  Adding the lanes that share the wave's first cell once, by a ballot (wave_count.h, what
// nemar_label_overlap does; nemar_tune(46, 0), measurement build) was nowhere faster beyond the spread on smooth, blocky or
// per-pixel-random images and 0 - 3 % slower at 2048^2 — a 64-pixel run of an image spreads over a few of the bins x bins cells
// where a label map hits one counter, and the ballots cost more than the adds they save: tools/microbench_similarity.py,
// tools/profiles/joint_histogram.txt.
// Moments.  regularity.hip's scheme, no atomics: six per-lane float accumulators, the xor tree of each wave, the waves in ascending
// order, one record per workgroup in the workspace, one merge kernel that reads the records in a fixed order.  With G workgroups per
// sample (G = min(tiles, what the chip holds / N)) and T = ceil(tiles / G) tiles per workgroup a sum passes through at most
//   4 T (lane) + 6 (wave) + 3 (workgroup)   additions in the tile kernel and   ceil(G / 256) + 6 + 3   in the merge:
//   D = 4 T + ceil(G / 256) + 18.
#include <math.h>

#include "common.h"
#include "resampled_grid.h"
#include "wave_count.h"

namespace {

constexpr int MAX_BINS = 64;            // 64 * 64 counters = 16 KiB of LDS beside the 9.3 KiB field patch
constexpr int MAX_CHANNELS = 64;
constexpr int SIM_WORDS = 8;            // sum a, sum b, sum a^2, sum b^2, sum ab, sum |a - b|, two unused
constexpr int SIM_SUMS = 6;

struct SimAcc {
    float s[SIM_SUMS];
};
__device__ __forceinline__ void sim_merge(SimAcc& a, const SimAcc& b) {
#pragma unroll
    for (int k = 0; k < SIM_SUMS; ++k) a.s[k] += b.s[k];
}
// the workgroup's totals, valid in thread 0: the xor tree of each wave, then the waves in ascending order (a fixed tree: the same bits on
// every run).  `red` is SIM_WORDS words of LDS per wave
__device__ __forceinline__ SimAcc sim_block(SimAcc a, float* red) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        SimAcc b;
#pragma unroll
        for (int k = 0; k < SIM_SUMS; ++k) b.s[k] = __shfl_xor(a.s[k], o, 64);
        sim_merge(a, b);
    }
    __syncthreads();      // protect `red` from a previous use
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < SIM_SUMS; ++k) red[wid * SIM_WORDS + k] = a.s[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < nw; ++i) {
            SimAcc b;
#pragma unroll
            for (int k = 0; k < SIM_SUMS; ++k) b.s[k] = red[i * SIM_WORDS + k];
            sim_merge(a, b);
        }
    }
    return a;
}

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
        float red[(RT_THREADS / 64) * SIM_WORDS];
    };
    __shared__ Lds lds;
    unsigned* hist = lds.hist;
    float* patch = lds.patch;
    const int n = blockIdx.y, tid = threadIdx.x;
    float th[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (MODE == GRID_AFFINE) {
        affine_theta(pred, n, th);
    }
    const size_t splane = (size_t)Hs * Ws, oplane = (size_t)Ho * Wo;
    const int fplane = RESAMPLE ? hf * wf : 0;
    const float* mN = moving + (size_t)n * Cm * splane;
    const float* bN = fixed + (size_t)n * Cf * oplane;
    const float* fN = MODE == GRID_UNET ? pred + (size_t)n * 2 * (RESAMPLE ? (size_t)fplane : oplane) : nullptr;
    const float inv_cm = 1.f / (float)Cm, inv_cf = 1.f / (float)Cf;
    const int cells = bins * bins;

    for (int e = tid; e < cells; e += RT_THREADS) hist[e] = 0u;
    __syncthreads();

    SimAcc acc;
#pragma unroll
    for (int k = 0; k < SIM_SUMS; ++k) acc.s[k] = 0.f;
    constexpr int ROWS = RT_THREADS / RT_W, RUNS = RT_H / ROWS;    // a lane owns one pixel in each of RUNS rows: a wave = 64 pixels of a row
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {         // (the same trip count in every lane of the workgroup)
        const int tyi = t / tiles_x;
        const int x0 = (t - tyi * tiles_x) * RT_W, y0 = tyi * RT_H;
        FieldPatch fp{0, 0, false};
        if (RESAMPLE) {
            __syncthreads();                                      // the previous tile's readers are done with the patch
            fp = stage_field(patch, fN, fplane, x0, y0, hf, wf, Ho, Wo, sh, sw, tid);
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < RUNS; ++i) {
            const int h = y0 + tid / RT_W + ROWS * i, w = x0 + tid % RT_W;
            int key = -1;                                         // (no early exit: the whole wave reaches the ballots)
            if (h < Ho && w < Wo) {
                float gx, gy;
                resampled_coord<MODE, RESAMPLE>(patch, fp, fN, fplane, oplane, h, w, hf, wf, Ho, Wo, sh, sw, th, gx, gy);
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
        acc = sim_block(acc, lds.red);
        if (tid == 0) {
            float* dst = partial + ((size_t)n * gridDim.x + blockIdx.x) * SIM_WORDS;
#pragma unroll
            for (int k = 0; k < SIM_SUMS; ++k) dst[k] = acc.s[k];
        }
    }
}

// moments[n] = the sample's records merged: thread t takes records t, t + 256, ... in ascending order, then the fixed workgroup tree
__global__ __launch_bounds__(256) void joint_moments_merge_kernel(const float* __restrict__ partial, int n_partial, float* __restrict__ moments) {
    __shared__ float red[(256 / 64) * SIM_WORDS];
    const int n = blockIdx.x;
    const float* p = partial + (size_t)n * n_partial * SIM_WORDS;
    SimAcc acc;
#pragma unroll
    for (int k = 0; k < SIM_SUMS; ++k) acc.s[k] = 0.f;
    for (int i = threadIdx.x; i < n_partial; i += blockDim.x) {
        SimAcc b;
#pragma unroll
        for (int k = 0; k < SIM_SUMS; ++k) b.s[k] = p[(size_t)i * SIM_WORDS + k];
        sim_merge(acc, b);
    }
    acc = sim_block(acc, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < SIM_SUMS; ++k) moments[n * SIM_SUMS + k] = acc.s[k];
    }
}

// workgroups per sample: every workgroup clears and flushes its own table and walks an equal share of the tiles, so the grid is what the
// chip holds AT ONCE and no more (score.hip: 256 CUs x the workgroups whose LDS fits a CU)
int sim_groups(int N, int bins, int Ho, int Wo) {
    const long long tiles = (long long)nemar_cdiv(Wo, RT_W) * nemar_cdiv(Ho, RT_H);
    const int resident = 256 * (bins <= 32 ? 8 : 6);
    const int share = resident / N > 0 ? resident / N : 1;
    return tiles < share ? (int)tiles : share;
}

}  // namespace

// 1 (default, and the product): every lane adds for itself; nemar_tune(46, 0) (measurement build): wave-aggregated adds
NEMAR_SWITCH(int, g_histogram_per_lane, 1);

namespace {

template <int MODE, bool RESAMPLE>
void launch_histogram(const float* moving, const float* fixed, const float* pred, unsigned* counts, float* partial, int N, int Cm, int Cf, int bins,
                      SimRange rg, int Hs, int Ws, int hf, int wf, int Ho, int Wo, hipStream_t st) {
    const int tiles_x = nemar_cdiv(Wo, RT_W), tiles = tiles_x * nemar_cdiv(Ho, RT_H);
    const dim3 grid(sim_groups(N, bins, Ho, Wo), N), block(RT_THREADS);
    const float sh = (float)hf / (float)Ho, sw = (float)wf / (float)Wo;           // nemar_bilinear_fwd's scales
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
    NEMAR_REQUIRE(grid_mode == GRID_UNET || grid_mode == GRID_AFFINE,
                  "joint_histogram: grid_mode %d (NEMAR_GRID_UNET or NEMAR_GRID_AFFINE: an explicit grid has no other resolution)", grid_mode);
    NEMAR_REQUIRE(N > 0 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0, "joint_histogram: bad shape N=%d source %dx%d output %dx%d", N, Hs, Ws, Ho, Wo);
    NEMAR_REQUIRE(bins >= 2 && bins <= MAX_BINS, "joint_histogram: %d bins (2 .. %d)", bins, MAX_BINS);
    NEMAR_REQUIRE(Cm >= 1 && Cm <= MAX_CHANNELS && Cf >= 1 && Cf <= MAX_CHANNELS, "joint_histogram: %d and %d channels (1 .. %d)", Cm, Cf, MAX_CHANNELS);
    NEMAR_REQUIRE(hi_m > lo_m && hi_f > lo_f, "joint_histogram: empty range [%g, %g] or [%g, %g]", (double)lo_m, (double)hi_m, (double)lo_f, (double)hi_f);
    const SimRange rg{lo_m, (float)bins / (hi_m - lo_m), lo_f, (float)bins / (hi_f - lo_f)};
    NEMAR_REQUIRE(isfinite(lo_m) && isfinite(lo_f) && isfinite(rg.scale_m) && isfinite(rg.scale_f) && rg.scale_m > 0.f && rg.scale_f > 0.f,
                  "joint_histogram: range [%g, %g] or [%g, %g] has no finite bin width", (double)lo_m, (double)hi_m, (double)lo_f, (double)hi_f);
    NEMAR_REQUIRE(grid_mode != GRID_UNET || (hf >= 1 && wf >= 1), "joint_histogram: offset field %d x %d", hf, wf);
    NEMAR_REQUIRE((long long)Hs * Ws < (1ll << 31) && (long long)Ho * Wo < (1ll << 31) && N <= 65535 &&
                      (grid_mode != GRID_UNET || (long long)hf * wf < (1ll << 30)),
                  "joint_histogram: plane too large");
    NEMAR_REQUIRE(!moments || ws_bytes >= nemar_joint_histogram_workspace(N, Ho, Wo), "joint_histogram: workspace %zu < %zu", ws_bytes,
                  nemar_joint_histogram_workspace(N, Ho, Wo));
    hipStream_t st = (hipStream_t)stream;
    float* partial = moments ? (float*)workspace : nullptr;
    NEMAR_HIP_CALL(hipMemsetAsync(counts, 0, (size_t)N * bins * bins * sizeof(unsigned), st));
    if (grid_mode == GRID_UNET) {
        if (hf != Ho || wf != Wo) launch_histogram<GRID_UNET, true>(moving, fixed, pred, counts, partial, N, Cm, Cf, bins, rg, Hs, Ws, hf, wf, Ho, Wo, st);
        else launch_histogram<GRID_UNET, false>(moving, fixed, pred, counts, partial, N, Cm, Cf, bins, rg, Hs, Ws, hf, wf, Ho, Wo, st);
    } else {
        launch_histogram<GRID_AFFINE, false>(moving, fixed, pred, counts, partial, N, Cm, Cf, bins, rg, Hs, Ws, 1, 1, Ho, Wo, st);
    }
    if (moments)
        hipLaunchKernelGGL(joint_moments_merge_kernel, dim3(N), dim3(256), 0, st, (const float*)partial, sim_groups(N, bins, Ho, Wo), moments);
    NEMAR_CHECK_LAUNCH("joint_histogram");
    return NEMAR_OK;
}
