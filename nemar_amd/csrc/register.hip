// Registration at any resolution: the STN's prediction applied to an image of another size in ONE pass (DESIGN.md "Registration at
// native size").  Not a call site of the reference, which only ever warps at the network's own size; it composes two that are:
//   F.interpolate(offsets, (Ho, Wo), 'bilinear', align_corners=False)          reference models/stn/unet_stn.py:139-141,165-166
//   F.grid_sample(img, identity + offsets, <mode>, 'zeros', align_corners=False) reference models/stn/unet_stn.py:167-174
//   F.affine_grid(theta, size) + F.grid_sample                                   reference models/stn/affine_stn.py:122,128
// The sampling grid is in normalised coordinates, so a prediction made at hf x wf describes the same transformation at Ho x Wo.
// nemar_bilinear_fwd + nemar_grid_sample_fwd would write the resized 2-channel field to HBM and read it straight back:
// 4 * (2C + 4) B/px against 4 * 2C B/px here (40 against 24 at C = 3), where the coarse field is interpolated in registers.
//
// One workgroup per 64 x 16 output tile.  The coarse-field taps of a tile span at most (64 wf/Wo + 2) x (16 hf/Ho + 2) texels: with
// wf <= Wo and hf <= Ho they fit a 66 x 18 x 2 LDS patch (9.3 KiB), staged through registers with 4-byte loads — `pred` needs no
// 16-byte alignment on that route; a tile whose taps do not fit (a field being DOWN-sampled) reads them from global memory.  The
// sampling position is computed once per pixel and reused for every channel.  A lane owns ONE pixel in each of four rows of the tile, so
// that every gather and every store instruction of a wave covers whole cache lines.  The other shape — 4 consecutive pixels of one row
// per lane, 16-byte stores where Wo % 4 == 0 and `out` is 16-byte aligned — is in the measurement build only (nemar_tune(44, 1)):
// tools/microbench_register.py times the two side by side and profiles/register_fullres.txt holds the result, 16-byte stores take 27 % to
// 37 % longer, as in warp.hip's forward kernel (profiles/r4_gs_fwd_vec.txt).  No pointer needs more than 4-byte alignment.
//
// Arithmetic is shared, not restated: grid and position from warp_grid.h, the resize taps and their sum from resize_taps.h, the
// prediction's view, the tile's field patch and the texels a pixel reads from resampled_grid.h, the four-corner blend in the
// expression order of warp.hip's grid_sample_fwd_kernel.  With -ffp-contract=off the bilinear result equals the composed path's bit
// for bit (tests/register_cases.py).
#include "common.h"
#include "pred_launch.h"

namespace {

// VEC: pixels of one row a lane owns per run — 1 (the product: four runs, in four rows of the tile) or 4 (measurement build: one run)
template <int MODE, int SAMPLE, int VEC, bool RESAMPLE>
__global__ __launch_bounds__(RT_THREADS) void warp_resampled_kernel(const float* __restrict__ in, const float* __restrict__ pred,
                                                                    float* __restrict__ out, int C, int Hs, int Ws, int hf, int wf,
                                                                    int Ho, int Wo, float sh, float sw) {
    __shared__ float patch[RESAMPLE ? 2 * RT_PH * RT_PW : 1];
    const int n = blockIdx.z, tid = threadIdx.x;
    const int x0 = blockIdx.x * RT_W, y0 = blockIdx.y * RT_H;
    const auto pv = pred_view<MODE, RESAMPLE>(pred, n, hf, wf, Ho, Wo, sh, sw);
    const size_t splane = (size_t)Hs * Ws, oplane = pv.oplane;
    const float* inN = in + (size_t)n * C * splane;
    float* outN = out + (size_t)n * C * oplane;

    const FieldPatch fp = pv.stage(patch, x0, y0, tid);
    if (RESAMPLE) __syncthreads();

    constexpr int LPR = RT_W / VEC, ROWS = RT_THREADS / LPR, RUNS = RT_H / ROWS;      // lanes per tile row, rows per pass, passes
#pragma unroll
    for (int i = 0; i < RUNS; ++i) {
        const int h = y0 + tid / LPR + ROWS * i, w0 = x0 + (tid % LPR) * VEC;
        if (h >= Ho || w0 >= Wo) continue;                 // (VEC 4 only with Wo % 4 == 0: a run is inside the row or outside it)
        Taps t[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const int w = w0 + v;
            float gx, gy;
            pv.coord(patch, fp, h, w, gx, gy);
            t[v] = taps_at<SAMPLE>(gx, gy, Ws, Hs);
        }
        float* q = outN + (size_t)h * Wo + w0;
        for (int c = 0; c < C; ++c) {
            const float* p = inN + (size_t)c * splane;
            float r[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) r[v] = sample_at<SAMPLE>(p, t[v]);
            if constexpr (VEC == 4) {
                *reinterpret_cast<float4*>(q + (size_t)c * oplane) = make_float4(r[0], r[1], r[2], r[3]);
            } else {
                q[(size_t)c * oplane] = r[0];
            }
        }
    }
}

}  // namespace

// nemar_tune(44, 1) (measurement build): 4 consecutive pixels per lane and 16-byte stores where the output allows; 0 (default, and the
// product): one pixel per lane
NEMAR_SWITCH(int, g_register_vec4, 0);

namespace {

template <int MODE, int SAMPLE, bool RESAMPLE>
void launch(const float* in, const float* pred, float* out, int N, int C, int Hs, int Ws, int hf, int wf, int Ho, int Wo, float sh, float sw,
            hipStream_t st) {
    const dim3 grid(nemar_cdiv(Wo, RT_W), nemar_cdiv(Ho, RT_H), N), block(RT_THREADS);
    NEMAR_AB_ONLY(if (g_register_vec4 && (Wo & 3) == 0 && (((uintptr_t)out) & 15) == 0)
        hipLaunchKernelGGL((warp_resampled_kernel<MODE, SAMPLE, 4, RESAMPLE>), grid, block, 0, st, in, pred, out, C, Hs, Ws, hf, wf, Ho, Wo, sh, sw);
    else)
        hipLaunchKernelGGL((warp_resampled_kernel<MODE, SAMPLE, 1, RESAMPLE>), grid, block, 0, st, in, pred, out, C, Hs, Ws, hf, wf, Ho, Wo, sh, sw);
}

}  // namespace

NEMAR_API int nemar_warp_resampled_fwd(const float* in, const float* pred, int grid_mode, int sample_mode, float* out, int N, int C,
                                       int Hs, int Ws, int hf, int wf, int Ho, int Wo, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(in && pred && out, "warp_resampled_fwd: null pointer");
    NEMAR_REQUIRE(((((uintptr_t)in) | ((uintptr_t)pred) | ((uintptr_t)out)) & 3) == 0,
                  "warp_resampled_fwd: in, pred and out must be 4-byte aligned");
    NEMAR_REQUIRE(sample_mode == SAMPLE_BILINEAR || sample_mode == SAMPLE_NEAREST, "warp_resampled_fwd: unknown sample_mode %d", sample_mode);
    NEMAR_REQUIRE(N > 0 && C > 0 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0, "warp_resampled_fwd: bad shape N=%d C=%d source %dx%d output %dx%d", N,
                  C, Hs, Ws, Ho, Wo);
    NEMAR_REQUIRE((long long)Hs * Ws < (1ll << 31), "warp_resampled_fwd: source plane too large");
    NEMAR_REQUIRE_OK(pred_ok("warp_resampled_fwd", "", grid_mode, hf, wf) && tile_grid_ok("warp_resampled_fwd", N, Ho, Wo));
    hipStream_t st = (hipStream_t)stream;
    dispatch_pred(grid_mode, hf, wf, Ho, Wo, [&](auto mode, auto resample, int hf, int wf, float sh, float sw) {
        constexpr int MODE = decltype(mode)::value;
        constexpr bool RESAMPLE = decltype(resample)::value;
        if (sample_mode == SAMPLE_NEAREST) launch<MODE, SAMPLE_NEAREST, RESAMPLE>(in, pred, out, N, C, Hs, Ws, hf, wf, Ho, Wo, sh, sw, st);
        else launch<MODE, SAMPLE_BILINEAR, RESAMPLE>(in, pred, out, N, C, Hs, Ws, hf, wf, Ho, Wo, sh, sw, st);
    });
    NEMAR_CHECK_LAUNCH("warp_resampled_fwd");
    return NEMAR_OK;
}
