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
//
// Backward (nemar_compose_pred_bwd, DESIGN.md "Training the cascade"; the definition is in include/nemar_hip.h): training size only, a
// UNet operand is AT the composition size.  out_c(x) = grid_at<M1>(first, p(x))_c - linspace_c(x), p(x) = sample_position(coord<M2>(second, x)):
//   towards first, UNET    the four bilinear weights of tap1d_at(p) times gout_c(x), scattered into first's texels.  `second` moves p by an
//                          unbounded amount, so this cannot be a gather over a fixed window, and fp32 atomics would depend on arrival
//                          order: 64-bit FIXED-POINT integer atomics into the zeroed accumulator [N][H*W][2], as nemar_svf_step_bwd
//                          (fixed_scatter.h: the scale from a device-side max of |gout|), then compose_bwd_fold_kernel rescales, writes or
//                          accumulates gfirst and returns the accumulator to all-zero;
//   towards first, AFFINE  the six sums of gout_x (xb(p), yb(p), 1), gout_y (xb(p), yb(p), 1): one record per 64 x 16 tile, merged in a fixed
//                          order by epe_bwd_affine_merge_kernel (pred_grad.h);
//   towards second         only the position path: gp_a(x) = sum_c gout_c(x) d grid_at_c / d p_a — UNET first: the slope of the identity's
//                          extension (linspace_at) plus the bilinear slope of first's 2 x 2 cell, zero along an axis where tap1d_at clamped
//                          the position; AFFINE first: theta's 2 x 2 part times affine_base_at's slope — times d p / d coord = W/2, H/2.
//                          A UNET second receives it at its own pixel (a coalesced store of the tile kernel, no atomics); an AFFINE second
//                          as six sums of gp (xb(x), yb(x), 1): tile records and the same merge.
// A pixel whose position is not finite contributes exactly 0 to both gradients.  Positions are clamped in float before the integer
// conversion (tap1d_at), so no input value can index outside a plane.  Nothing synchronises with the host: capturable into the step graph.
#include "common.h"
#include "fixed_scatter.h"
#include "pred_grad.h"
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

// ---- backward ------------------------------------------------------------------------------------------------------------------
// did tap1d_at clamp the source coordinate of position d (the same expression)?  The bilinear slope along that axis is then zero
__device__ __forceinline__ bool tap1d_clamped(float d, int n_in, float scale) {
    const float s = (d + 0.5f) * scale - 0.5f;
    return s < 0.f || s > (float)(n_in - 1);
}
__device__ __forceinline__ float linspace_slope(int n) { return n <= 1 ? 0.f : 2.f / (float)(n - 1); }

// The 64 x 16 tile of the forward.  want_first / want_second: which gradients the call asked for (the same in every lane of the grid);
// the arithmetic of one does not depend on the other.
//   M1 UNET:   acc = the fixed-point accumulator [N][H*W][2], partial / partials / fix its scale (fixed_scatter.h)
//   M1 AFFINE: rec1 = the tile's six-word record towards first
//   M2 UNET:   gsecond written or accumulated at the pixel
//   M2 AFFINE: rec2 = the tile's six-word record towards second
// `one`: the 1.0f that epe_bwd_affine_merge_kernel takes as its gscale, left behind the records
template <int M1, int M2>
__global__ __launch_bounds__(RT_THREADS) void compose_bwd_kernel(const float* __restrict__ first, const float* __restrict__ second,
                                                                 const float* __restrict__ gout, long long* __restrict__ acc,
                                                                 const unsigned* __restrict__ partial, int partials, int fix,
                                                                 float* __restrict__ rec1, float* __restrict__ gsecond, int accumulate2,
                                                                 float* __restrict__ rec2, float* __restrict__ one, int want_first,
                                                                 int want_second, int H, int W) {
    __shared__ unsigned redu[4];
    __shared__ float red[16];
    const int n = blockIdx.z, tid = threadIdx.x;
    const int x0 = blockIdx.x * RT_W, y0 = blockIdx.y * RT_H;
    float th1[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (M1 == GRID_AFFINE) {
        affine_theta(first, n, th1);
    }
    const auto p2 = pred_view<M2, false>(second, n, H, W, H, W, 1.f, 1.f);
    const size_t plane = p2.oplane;
    const float* f1N = M1 == GRID_UNET ? first + (size_t)n * 2 * plane : nullptr;
    const float* gN = gout + (size_t)n * 2 * plane;
    unsigned long long* aN = M1 == GRID_UNET ? reinterpret_cast<unsigned long long*>(acc) + (size_t)n * 2 * plane : nullptr;
    float* g2N = M2 == GRID_UNET && want_second ? gsecond + (size_t)n * 2 * plane : nullptr;
    float scale = 0.f;
    if (M1 == GRID_UNET && want_first) scale = svf_pow2(fix - svf_exponent(partial, partials, redu));      // products with it are exact
    const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
    const float sx = linspace_slope(W), sy = linspace_slope(H);                 // d linspace_at / d p
    const float bx = 2.f / (float)W, by = 2.f / (float)H;                       // d affine_base_at / d p

    float a1[EPE_WORDS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, a2[EPE_WORDS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    constexpr int ROWS = RT_THREADS / RT_W, RUNS = RT_H / ROWS;      // the forward's shape: one pixel in each of four rows per lane
#pragma unroll
    for (int i = 0; i < RUNS; ++i) {
        const int h = y0 + tid / RT_W + ROWS * i, w = x0 + tid % RT_W;
        if (h >= H || w >= W) continue;
        float gx2, gy2, px, py;
        p2.coord_unstaged(h, w, gx2, gy2);
        sample_position(gx2, gy2, W, H, px, py);
        const bool finite = fabsf(px) <= 3.402823466e+38f && fabsf(py) <= 3.402823466e+38f;      // (false for a NaN)
        const size_t o = (size_t)h * W + w;
        const float g0 = gN[o], g1 = gN[plane + o];
        float gpx = 0.f, gpy = 0.f;                                  // d <gout, out> / d p of this pixel
        if (M1 == GRID_UNET) {
            const Tap1D ty = tap1d_at(py, H, 1.f), tx = tap1d_at(px, W, 1.f);      // (clamped in float: inside the plane whatever p is)
            const size_t tex[4] = {(size_t)ty.i0 * W + tx.i0, (size_t)ty.i0 * W + tx.i1, (size_t)ty.i1 * W + tx.i0, (size_t)ty.i1 * W + tx.i1};
            if (want_first && finite) {
                const float wk[4] = {tx.l0 * ty.l0, tx.l1 * ty.l0, tx.l0 * ty.l1, tx.l1 * ty.l1};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (wk[k] == 0.f) continue;          // (also the coinciding tap of the last column / row)
                    atomicAdd(aN + 2 * tex[k], (unsigned long long)__float2ll_rn((wk[k] * g0) * scale));
                    atomicAdd(aN + 2 * tex[k] + 1, (unsigned long long)__float2ll_rn((wk[k] * g1) * scale));
                }
            }
            if (want_second) {
                const float* c0 = f1N;
                const float* c1 = f1N + plane;
                const bool cx = tap1d_clamped(px, W, 1.f), cy = tap1d_clamped(py, H, 1.f);
                const float a = c0[tex[0]], b = c0[tex[1]], c = c0[tex[2]], d = c0[tex[3]];
                const float e = c1[tex[0]], f = c1[tex[1]], g = c1[tex[2]], k = c1[tex[3]];
                // d bilinear_ch / d p.x, d p.y: zero along an axis whose position was clamped
                const float dx0 = cx ? 0.f : ty.l0 * (b - a) + ty.l1 * (d - c);
                const float dx1 = cx ? 0.f : ty.l0 * (f - e) + ty.l1 * (k - g);
                const float dy0 = cy ? 0.f : tx.l0 * (c - a) + tx.l1 * (d - b);
                const float dy1 = cy ? 0.f : tx.l0 * (g - e) + tx.l1 * (k - f);
                gpx = g0 * (sx + dx0) + g1 * dx1;
                gpy = g0 * dy0 + g1 * (sy + dy1);
            }
        } else {
            if (want_first) {
                const float xb = affine_base_at(px, W), yb = affine_base_at(py, H);
                a1[0] += finite ? g0 * xb : 0.f; a1[1] += finite ? g0 * yb : 0.f; a1[2] += finite ? g0 : 0.f;
                a1[3] += finite ? g1 * xb : 0.f; a1[4] += finite ? g1 * yb : 0.f; a1[5] += finite ? g1 : 0.f;
            }
            if (want_second) {
                gpx = (g0 * th1[0] + g1 * th1[3]) * bx;
                gpy = (g0 * th1[1] + g1 * th1[4]) * by;
            }
        }
        if (want_second) {
            const float dvx = finite ? gpx * hw : 0.f, dvy = finite ? gpy * hh : 0.f;      // d p / d coord
            if (M2 == GRID_UNET) {
                if (accumulate2) { g2N[o] += dvx; g2N[plane + o] += dvy; } else { g2N[o] = dvx; g2N[plane + o] = dvy; }
            } else {
                const float xb = affine_base(w, W), yb = affine_base(h, H);
                a2[0] += dvx * xb; a2[1] += dvx * yb; a2[2] += dvx;
                a2[3] += dvy * xb; a2[4] += dvy * yb; a2[5] += dvy;
            }
        }
    }

    const size_t tile = (size_t)n * gridDim.y * gridDim.x + (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (M1 == GRID_AFFINE && want_first) {
#pragma unroll
        for (int c = 0; c < EPE_WORDS; ++c) {
            const float t = block_sum(a1[c], red);
            if (tid == 0) rec1[tile * EPE_WORDS + c] = t;
        }
    }
    if (M2 == GRID_AFFINE && want_second) {
#pragma unroll
        for (int c = 0; c < EPE_WORDS; ++c) {
            const float t = block_sum(a2[c], red);
            if (tid == 0) rec2[tile * EPE_WORDS + c] = t;
        }
    }
    if (tid == 0 && tile == 0) one[0] = 1.f;
}

// the same tile: the accumulator / scale into gfirst (or added to it, rounded once); the accumulator goes back to all-zero
__global__ __launch_bounds__(RT_THREADS) void compose_bwd_fold_kernel(float* __restrict__ gfirst, int accumulate, long long* __restrict__ acc,
                                                                      const unsigned* __restrict__ partial, int partials, int fix, int H,
                                                                      int W) {
    __shared__ unsigned redu[4];
    const int n = blockIdx.z, tid = threadIdx.x;
    const int x0 = blockIdx.x * RT_W, y0 = blockIdx.y * RT_H;
    const size_t plane = (size_t)H * W;
    float* gN = gfirst + (size_t)n * 2 * plane;
    long long* aN = acc + (size_t)n * 2 * plane;
    const float unscale = svf_pow2(svf_exponent(partial, partials, redu) - fix);
    constexpr int ROWS = RT_THREADS / RT_W, RUNS = RT_H / ROWS;
#pragma unroll
    for (int i = 0; i < RUNS; ++i) {
        const int h = y0 + tid / RT_W + ROWS * i, w = x0 + tid % RT_W;
        if (h >= H || w >= W) continue;
        const size_t o = (size_t)h * W + w;
        const long long i0 = aN[2 * o], i1 = aN[2 * o + 1];
        if (i0 != 0) aN[2 * o] = 0;
        if (i1 != 0) aN[2 * o + 1] = 0;
        const float r0 = (float)i0 * unscale, r1 = (float)i1 * unscale;
        if (accumulate) { gN[o] += r0; gN[plane + o] += r1; } else { gN[o] = r0; gN[plane + o] = r1; }
    }
}

// the workspace: [ accumulator (UNET first; zero on entry and on return) | partial words | records towards first | towards second | 1.0f ]
struct ComposeBwdWs {
    size_t zeroed, partial, rec1, rec2, one, total;
};
ComposeBwdWs compose_bwd_ws(int first_mode, int second_mode, int N, int H, int W) {
    ComposeBwdWs l{};
    if (N <= 0 || H <= 0 || W <= 0) return l;
    const size_t tiles = (size_t)nemar_cdiv(W, RT_W) * nemar_cdiv(H, RT_H) * N;
    l.zeroed = first_mode == GRID_UNET ? sizeof(long long) * 2 * (size_t)N * H * W : 0;
    l.partial = l.zeroed;
    l.rec1 = l.partial + sizeof(unsigned) * SVF_MAX_PARTIALS;
    l.rec2 = l.rec1 + (first_mode == GRID_AFFINE ? sizeof(float) * tiles * EPE_WORDS : 0);
    l.one = l.rec2 + (second_mode == GRID_AFFINE ? sizeof(float) * tiles * EPE_WORDS : 0);
    l.total = l.one + 2 * sizeof(float);      // (a multiple of 8 bytes)
    return l;
}

}  // namespace

NEMAR_API size_t nemar_compose_pred_bwd_zeroed_bytes(int first_mode, int second_mode, int N, int H, int W) {
    return compose_bwd_ws(first_mode, second_mode, N, H, W).zeroed;
}
NEMAR_API size_t nemar_compose_pred_bwd_workspace(int first_mode, int second_mode, int N, int H, int W) {
    return compose_bwd_ws(first_mode, second_mode, N, H, W).total;
}

NEMAR_API int nemar_compose_pred_bwd(const float* first, int first_mode, int h1, int w1, const float* second, int second_mode, int h2, int w2,
                                     const float* gout, float* gfirst, int accumulate_first, float* gsecond, int accumulate_second,
                                     void* workspace, size_t ws_bytes, int N, int H, int W, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(first && second && gout && workspace, "compose_pred_bwd: null pointer");
    NEMAR_REQUIRE(gfirst || gsecond, "compose_pred_bwd: neither gfirst nor gsecond (nothing to compute)");
    NEMAR_REQUIRE(aligned4(first, second, gout, gfirst, gsecond) && (((uintptr_t)workspace) & 7) == 0,
                  "compose_pred_bwd: first, second, gout, gfirst and gsecond must be 4-byte aligned, workspace 8-byte aligned");
    NEMAR_REQUIRE(N > 0 && H > 0 && W > 0, "compose_pred_bwd: bad shape N=%d size %dx%d", N, H, W);
    NEMAR_REQUIRE_OK(pred_ok("compose_pred_bwd", "first ", first_mode, h1, w1) && pred_ok("compose_pred_bwd", "second ", second_mode, h2, w2) &&
                     tile_grid_ok("compose_pred_bwd", N, H, W));
    NEMAR_REQUIRE(first_mode != GRID_UNET || (h1 == H && w1 == W),
                  "compose_pred_bwd: first field %d x %d is resampled to %d x %d (no backward: a UNet operand must be at the composition size)", h1,
                  w1, H, W);
    NEMAR_REQUIRE(second_mode != GRID_UNET || (h2 == H && w2 == W),
                  "compose_pred_bwd: second field %d x %d is resampled to %d x %d (no backward: a UNet operand must be at the composition size)", h2,
                  w2, H, W);
    NEMAR_REQUIRE(!gfirst || (gfirst != first && gfirst != second && gfirst != gout), "compose_pred_bwd: gfirst must not be an operand");
    NEMAR_REQUIRE(!gsecond || (gsecond != first && gsecond != second && gsecond != gout && gsecond != gfirst),
                  "compose_pred_bwd: gsecond must not be an operand or gfirst");
    const ComposeBwdWs l = compose_bwd_ws(first_mode, second_mode, N, H, W);
    NEMAR_REQUIRE(ws_bytes >= l.total, "compose_pred_bwd: workspace %zu < %zu", ws_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    long long* acc = (long long*)ws;
    unsigned* partial = (unsigned*)(ws + l.partial);
    float *rec1 = (float*)(ws + l.rec1), *rec2 = (float*)(ws + l.rec2), *one = (float*)(ws + l.one);
    const int partials = svf_partials(N, H, W), fix = svf_fix_bits(H, W);
    const int tiles_x = nemar_cdiv(W, RT_W), tiles_y = nemar_cdiv(H, RT_H);
    const dim3 grid(tiles_x, tiles_y, N), block(RT_THREADS);
    const bool scatter = gfirst && first_mode == GRID_UNET;
    if (scatter) hipLaunchKernelGGL(svf_max_kernel, dim3(partials), dim3(256), 0, st, gout, (long long)N * 2 * H * W, partial);
    dispatch_pred(first_mode, H, W, H, W, [&](auto m1, auto, int, int, float, float) {
        dispatch_pred(second_mode, H, W, H, W, [&](auto m2, auto, int, int, float, float) {
            hipLaunchKernelGGL((compose_bwd_kernel<decltype(m1)::value, decltype(m2)::value>), grid, block, 0, st, first, second, gout, acc,
                               (const unsigned*)partial, partials, fix, rec1, gsecond, accumulate_second, rec2, one, gfirst ? 1 : 0,
                               gsecond ? 1 : 0, H, W);
        });
    });
    if (scatter)
        hipLaunchKernelGGL(compose_bwd_fold_kernel, grid, block, 0, st, gfirst, accumulate_first, acc, (const unsigned*)partial, partials, fix, H, W);
    if (gfirst && first_mode == GRID_AFFINE)
        hipLaunchKernelGGL(epe_bwd_affine_merge_kernel, dim3(N), dim3(256), 0, st, (const float*)rec1, tiles_x * tiles_y, (const float*)one, 1.f,
                           gfirst, accumulate_first);
    if (gsecond && second_mode == GRID_AFFINE)
        hipLaunchKernelGGL(epe_bwd_affine_merge_kernel, dim3(N), dim3(256), 0, st, (const float*)rec2, tiles_x * tiles_y, (const float*)one, 1.f,
                           gsecond, accumulate_second);
    NEMAR_CHECK_LAUNCH("compose_pred_bwd");
    return NEMAR_OK;
}

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
