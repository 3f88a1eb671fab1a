// Composing two predictions (DESIGN.md "Composing predictions; cascaded registration"): ONE prediction that samples where two would in
// sequence.  Not a call site of the reference, which applies one prediction only.  `first` (P1) is applied to the image first,
// A1(x) = A(S1(x)); `second` (P2) to the result, A2(x) = A1(S2(x)) = A(S1(S2(x))).  At the composition size (H, W) the kernel writes the
// NEMAR_GRID_UNET offset field of x -> S1(S2(x)): for every output pixel the normalised coordinate P2 gives it (PredView::coord: exactly
// what nemar_warp_resampled_fwd computes at output size (H, W)), the pixel position p that coordinate samples in the intermediate image
// (sample_position), the CONTINUOUS extension of P1's grid at p (grid_at: exactly what nemar_map_points evaluates), minus the identity.
// Everything downstream — nemar_warp_resampled_fwd, nemar_label_overlap, nemar_map_points — then reads the composite as it reads
// any UNet prediction, and an image is interpolated ONCE where two warps in sequence would blur it twice (and round class ids twice).
//
// One workgroup per 64 x 16 output tile, a lane owns one pixel in each of four rows (resampled_grid.h).  `second` is read where the
// pixel is, through its PredView: the coarse patch staged in LDS (global fallback when it is being down-sampled).  `first` is
// gathered from global memory at the data-dependent p: four texels per channel, 16 B/px of loads that hit L2 — a network-size field is
// at most 512 KB per sample — against 8 B/px of stores.
// Optional fused warp: with `img` the kernel also writes img warped bilinearly by the composite, bit for bit what
// nemar_warp_resampled_fwd(img, out_field, NEMAR_GRID_UNET, NEMAR_SAMPLE_BILINEAR) writes at equal sizes: the coordinate is rebuilt as
// linspace + the STORED offset (not the gx1 it was subtracted from: (gx1 - l) + l is not gx1 in fp32) and blended by taps_at /
// sample_at.  That is the moving image of the next cascade pass, produced while the position is in registers: the field is not read
// back (8 B/px) and one launch is saved (tools/cascade_record.py times the two forms).
// Plain fp32, no atomics, built without contraction like its neighbours: bitwise repeatable.
#include "common.h"
#include "pred_launch.h"

namespace {

template <int M1, int M2, bool RESAMPLE2>
__global__ __launch_bounds__(RT_THREADS) void compose_kernel(const float* __restrict__ first, const float* __restrict__ second,
                                                             float* __restrict__ out_field, const float* __restrict__ img,
                                                             float* __restrict__ out_img, int C, int h1, int w1, int h2, int w2, int H,
                                                             int W, float sh1, float sw1, float sh2, float sw2) {
    __shared__ float patch[RESAMPLE2 ? 2 * RT_PH * RT_PW : 1];
    const int n = blockIdx.z, tid = threadIdx.x;
    const int x0 = blockIdx.x * RT_W, y0 = blockIdx.y * RT_H;
    float th1[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (M1 == GRID_AFFINE) {
        affine_theta(first, n, th1);
    }
    const auto p2 = pred_view<M2, RESAMPLE2>(second, n, h2, w2, H, W, sh2, sw2);
    const size_t plane = p2.oplane;
    const float* f1N = M1 == GRID_UNET ? first + (size_t)n * 2 * h1 * w1 : nullptr;
    float* oN = out_field + (size_t)n * 2 * plane;
    const float* inN = img ? img + (size_t)n * C * plane : nullptr;
    float* outN = img ? out_img + (size_t)n * C * plane : nullptr;

    const FieldPatch fp = p2.stage(patch, x0, y0, tid);
    if (RESAMPLE2) __syncthreads();

    constexpr int ROWS = RT_THREADS / RT_W, RUNS = RT_H / ROWS;      // a lane owns one pixel in each of RUNS rows: a wave = 64 pixels of a row
#pragma unroll
    for (int i = 0; i < RUNS; ++i) {
        const int h = y0 + tid / RT_W + ROWS * i, w = x0 + tid % RT_W;
        if (h >= H || w >= W) continue;
        float gx2, gy2, px, py, gx1, gy1;
        p2.coord(patch, fp, h, w, gx2, gy2);
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

}  // namespace

NEMAR_API int nemar_compose_pred(const float* first, int first_mode, int h1, int w1, const float* second, int second_mode, int h2, int w2,
                                 float* out_field, const float* img, float* out_img, int C, int N, int H, int W, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(first && second && out_field, "compose_pred: null pointer");
    NEMAR_REQUIRE((img == nullptr) == (out_img == nullptr), "compose_pred: img and out_img come together (the fused warp) or not at all");
    NEMAR_REQUIRE(((((uintptr_t)first) | ((uintptr_t)second) | ((uintptr_t)out_field) | ((uintptr_t)img) | ((uintptr_t)out_img)) & 3) == 0,
                  "compose_pred: first, second, out_field, img and out_img must be 4-byte aligned");
    NEMAR_REQUIRE(N > 0 && H > 0 && W > 0 && (!img || C > 0), "compose_pred: bad shape N=%d C=%d size %dx%d", N, C, H, W);
    NEMAR_REQUIRE_OK(pred_ok("compose_pred", "first ", first_mode, h1, w1) && pred_ok("compose_pred", "second ", second_mode, h2, w2) &&
                     tile_grid_ok("compose_pred", N, H, W));
    NEMAR_REQUIRE(out_field != first && out_field != second, "compose_pred: out_field must not be an operand (the kernel gathers from them)");
    NEMAR_REQUIRE(!img || (out_img != img && (const float*)out_img != first && (const float*)out_img != second && out_img != out_field),
                  "compose_pred: out_img must not be an operand or out_field");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(nemar_cdiv(W, RT_W), nemar_cdiv(H, RT_H), N), block(RT_THREADS);
    // (`first` is read at data-dependent positions by grid_at, resampled or not: its route's second constant is not used)
    dispatch_pred(first_mode, h1, w1, H, W, [&](auto m1, auto, int h1, int w1, float sh1, float sw1) {
        dispatch_pred(second_mode, h2, w2, H, W, [&](auto m2, auto resample2, int h2, int w2, float sh2, float sw2) {
            hipLaunchKernelGGL((compose_kernel<decltype(m1)::value, decltype(m2)::value, decltype(resample2)::value>), grid, block, 0, st, first,
                               second, out_field, img, out_img, C, h1, w1, h2, w2, H, W, sh1, sw1, sh2, sw2);
        });
    });
    NEMAR_CHECK_LAUNCH("compose_pred");
    return NEMAR_OK;
}
