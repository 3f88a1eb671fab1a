// Composing two predictions (DESIGN.md "Composing predictions; cascaded registration"): ONE prediction that samples where two would in
// sequence.  Not a call site of the reference, which applies one prediction only.  `first` (P1) is applied to the image first,
// A1(x) = A(S1(x)); `second` (P2) to the result, A2(x) = A1(S2(x)) = A(S1(S2(x))).  At the composition size (H, W) the kernel writes the
// NEMAR_GRID_UNET offset field of x -> S1(S2(x)): for every output pixel the normalised coordinate P2 gives it (resampled_coord: exactly
// what nemar_warp_resampled_fwd computes at output size (H, W)), the pixel position p that coordinate samples in the intermediate image
// (sample_position), the CONTINUOUS extension of P1's grid at p (grid_at: exactly what nemar_map_points evaluates), minus the identity.
// Everything downstream — nemar_warp_resampled_fwd, nemar_label_overlap, nemar_map_points — then reads the composite as it reads
// any UNet prediction, and an image is interpolated ONCE where two warps in sequence would blur it twice (and round class ids twice).
//
// One workgroup per 64 x 16 output tile, a lane owns one pixel in each of four rows (resampled_grid.h, as register.hip).  `second` is
// read where the pixel is: its coarse patch is staged in LDS by stage_field (global fallback when it is being down-sampled).  `first` is
// gathered from global memory at the data-dependent p: four texels per channel, 16 B/px of loads that hit L2 — a network-size field is
// at most 512 KB per sample — against 8 B/px of stores.
// Optional fused warp: with `img` the kernel also writes img warped bilinearly by the composite, bit for bit what
// nemar_warp_resampled_fwd(img, out_field, NEMAR_GRID_UNET, NEMAR_SAMPLE_BILINEAR) writes at equal sizes: the coordinate is rebuilt as
// linspace + the STORED offset (not the gx1 it was subtracted from: (gx1 - l) + l is not gx1 in fp32) and blended by taps_at /
// sample_at.  That is the moving image of the next cascade pass, produced while the position is in registers: the field is not read
// back (8 B/px) and one launch is saved (tools/cascade_record.py times the two forms).
// Plain fp32, no atomics, built without contraction like its neighbours: bitwise repeatable.
#include "common.h"
#include "resampled_grid.h"

namespace {

template <int M1, int M2, bool RESAMPLE2>
__global__ __launch_bounds__(RT_THREADS) void compose_kernel(const float* __restrict__ first, const float* __restrict__ second,
                                                             float* __restrict__ out_field, const float* __restrict__ img,
                                                             float* __restrict__ out_img, int C, int h1, int w1, int h2, int w2, int H,
                                                             int W, float sh1, float sw1, float sh2, float sw2) {
    __shared__ float patch[RESAMPLE2 ? 2 * RT_PH * RT_PW : 1];
    const int n = blockIdx.z, tid = threadIdx.x;
    const int x0 = blockIdx.x * RT_W, y0 = blockIdx.y * RT_H;
    float th1[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, th2[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (M1 == GRID_AFFINE) {
        affine_theta(first, n, th1);
    }
    if (M2 == GRID_AFFINE) {
        affine_theta(second, n, th2);
    }
    const size_t plane = (size_t)H * W;
    const int fplane2 = RESAMPLE2 ? h2 * w2 : 0;
    const float* f1N = M1 == GRID_UNET ? first + (size_t)n * 2 * h1 * w1 : nullptr;
    const float* f2N = M2 == GRID_UNET ? second + (size_t)n * 2 * (RESAMPLE2 ? (size_t)fplane2 : plane) : nullptr;
    float* oN = out_field + (size_t)n * 2 * plane;
    const float* inN = img ? img + (size_t)n * C * plane : nullptr;
    float* outN = img ? out_img + (size_t)n * C * plane : nullptr;

    FieldPatch fp{0, 0, false};
    if (RESAMPLE2) {
        fp = stage_field(patch, f2N, fplane2, x0, y0, h2, w2, H, W, sh2, sw2, tid);
        __syncthreads();
    }

    constexpr int ROWS = RT_THREADS / RT_W, RUNS = RT_H / ROWS;      // a lane owns one pixel in each of RUNS rows: a wave = 64 pixels of a row
#pragma unroll
    for (int i = 0; i < RUNS; ++i) {
        const int h = y0 + tid / RT_W + ROWS * i, w = x0 + tid % RT_W;
        if (h >= H || w >= W) continue;
        float gx2, gy2, px, py, gx1, gy1;
        resampled_coord<M2, RESAMPLE2>(patch, fp, f2N, fplane2, plane, h, w, h2, w2, H, W, sh2, sw2, th2, gx2, gy2);
        sample_position(gx2, gy2, W, H, px, py);                    // where P2 reads the intermediate image, which has the output's size
        grid_at<M1>(f1N, h1, w1, sh1, sw1, th1, px, py, H, W, gx1, gy1);
        const float lx = linspace_m1_p1(w, W), ly = linspace_m1_p1(h, H);
        const float dx = gx1 - lx, dy = gy1 - ly;
        const size_t o = (size_t)h * W + w;
        oN[o] = dx;
        oN[plane + o] = dy;
        if (img) {                                                 // (the same in every lane of the grid)
            const Taps t = taps_at<SAMPLE_BILINEAR>(lx + dx, ly + dy, W, H);
            for (int c = 0; c < C; ++c) outN[(size_t)c * plane + o] = sample_at<SAMPLE_BILINEAR>(inN + (size_t)c * plane, t);
        }
    }
}

template <int M1, int M2, bool RESAMPLE2>
void launch_route(const float* first, int h1, int w1, const float* second, int h2, int w2, float* out_field, const float* img, float* out_img,
                  int C, int N, int H, int W, hipStream_t st) {
    const dim3 grid(nemar_cdiv(W, RT_W), nemar_cdiv(H, RT_H), N), block(RT_THREADS);
    // nemar_bilinear_fwd's scales, of both fields to the composition size
    hipLaunchKernelGGL((compose_kernel<M1, M2, RESAMPLE2>), grid, block, 0, st, first, second, out_field, img, out_img, C, h1, w1, h2, w2, H, W,
                       (float)h1 / (float)H, (float)w1 / (float)W, (float)h2 / (float)H, (float)w2 / (float)W);
}

template <int M1>
void launch(const float* first, int h1, int w1, const float* second, int second_mode, int h2, int w2, float* out_field, const float* img,
            float* out_img, int C, int N, int H, int W, hipStream_t st) {
    if (second_mode == GRID_AFFINE) launch_route<M1, GRID_AFFINE, false>(first, h1, w1, second, 1, 1, out_field, img, out_img, C, N, H, W, st);
    else if (h2 != H || w2 != W) launch_route<M1, GRID_UNET, true>(first, h1, w1, second, h2, w2, out_field, img, out_img, C, N, H, W, st);
    else launch_route<M1, GRID_UNET, false>(first, h1, w1, second, h2, w2, out_field, img, out_img, C, N, H, W, st);
}

}  // namespace

NEMAR_API int nemar_compose_pred(const float* first, int first_mode, int h1, int w1, const float* second, int second_mode, int h2, int w2,
                                 float* out_field, const float* img, float* out_img, int C, int N, int H, int W, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(first && second && out_field, "compose_pred: null pointer");
    NEMAR_REQUIRE((img == nullptr) == (out_img == nullptr), "compose_pred: img and out_img come together (the fused warp) or not at all");
    NEMAR_REQUIRE(((((uintptr_t)first) | ((uintptr_t)second) | ((uintptr_t)out_field) | ((uintptr_t)img) | ((uintptr_t)out_img)) & 3) == 0,
                  "compose_pred: first, second, out_field, img and out_img must be 4-byte aligned");
    NEMAR_REQUIRE((first_mode == GRID_UNET || first_mode == GRID_AFFINE) && (second_mode == GRID_UNET || second_mode == GRID_AFFINE),
                  "compose_pred: grid modes %d, %d (NEMAR_GRID_UNET or NEMAR_GRID_AFFINE: an explicit grid has no other resolution)", first_mode,
                  second_mode);
    NEMAR_REQUIRE(N > 0 && H > 0 && W > 0 && (!img || C > 0), "compose_pred: bad shape N=%d C=%d size %dx%d", N, C, H, W);
    NEMAR_REQUIRE(first_mode != GRID_UNET || (h1 >= 1 && w1 >= 1), "compose_pred: first offset field %d x %d", h1, w1);
    NEMAR_REQUIRE(second_mode != GRID_UNET || (h2 >= 1 && w2 >= 1), "compose_pred: second offset field %d x %d", h2, w2);
    NEMAR_REQUIRE((long long)H * W < (1ll << 31) && N <= 65535 && nemar_cdiv(H, RT_H) <= 65535 &&
                      (first_mode != GRID_UNET || (long long)h1 * w1 < (1ll << 30)) && (second_mode != GRID_UNET || (long long)h2 * w2 < (1ll << 30)),
                  "compose_pred: plane too large");
    NEMAR_REQUIRE(out_field != first && out_field != second, "compose_pred: out_field must not be an operand (the kernel gathers from them)");
    NEMAR_REQUIRE(!img || (out_img != img && (const float*)out_img != first && (const float*)out_img != second && out_img != out_field),
                  "compose_pred: out_img must not be an operand or out_field");
    hipStream_t st = (hipStream_t)stream;
    if (first_mode != GRID_UNET) h1 = w1 = 1;
    if (first_mode == GRID_UNET) launch<GRID_UNET>(first, h1, w1, second, second_mode, h2, w2, out_field, img, out_img, C, N, H, W, st);
    else launch<GRID_AFFINE>(first, h1, w1, second, second_mode, h2, w2, out_field, img, out_img, C, N, H, W, st);
    NEMAR_CHECK_LAUNCH("compose_pred");
    return NEMAR_OK;
}
