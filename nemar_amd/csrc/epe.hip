// A loss that trains against a known misalignment (DESIGN.md "EPE loss"): the registration-error meter's residual (deform.hip) made
// differentiable.  Not a call site of the reference, which has no ground-truth field.  With S(x) = (ix, iy) the position the warp samples
// for output pixel x = (w, h) (warp_grid.h: the bits of nemar_grid_sample_fwd and nemar_registration_error) and g the ground-truth field
// in pixels, read bilinearly at S with the position clamped into the image (clamped_bilerp.h: the meter's read),
//   r = S + g(S) - x,   rho = sqrt(r.x^2 + r.y^2 + eps^2)   (Charbonnier; eps = 0 is the meter's |r|)
//   loss = factor / (N H W) * sum over ALL pixels of rho      (a sample that left the image is not excused: the clamped read extends g by
//                                                              its border value and the residual grows with the distance)
// Both entry points are gathers: a pixel's gradient is with respect to its own sampling position.
//
// Forward: registration_error_kernel's shape — 256-thread workgroups, a grid-stride loop, for UNet offsets 4 pixels per lane with 16-byte
// loads of the prediction when the row length is a multiple of 4 and the tensor is 16-byte aligned (the same 4 pixels by 4-byte loads
// when it is not: the sum's order, and so its bits, do not depend on the alignment), one pixel per lane at any other width; g is read by
// the gather alone.  Per-lane partial, the xor tree of each wave, the waves in ascending order, one float per workgroup in the
// caller's workspace; one merge workgroup reads them in a fixed order.  No atomics: bitwise repeatable.  A term passes through at most
// VEC x (loop trips) additions in its lane, 6 in the wave and 4 across the waves, then ceil(partials / 256) + 6 + 4 in the merge.
//
// Backward: u = r / rho; the derivative of the bilinear read is the slope of the cell floor() chose,
//   dg/dix = (1 - ty) (g01 - g00) + ty (g11 - g10), exactly 0 where ix < 0 or ix > W-1 (the clamp), likewise in y;
//   Dx = u.x (1 + dx g_x) + u.y dx g_y,   Dy = u.x dy g_x + u.y (1 + dy g_y),   k = gscale[0] * factor / (N H W).
// UNet: gpred[n,0,h,w] (+)= k (W/2) Dx, gpred[n,1,h,w] (+)= k (H/2) Dy — one launch, 16-byte stores on the vector route, no workspace.
// Affine: gpred[n,0..5] (+)= k * sum_{h,w} [(W/2) Dx (xb, yb, 1), (H/2) Dy (xb, yb, 1)] — one 6-vector per workgroup in the workspace,
// one merge workgroup per sample reads them in a fixed order.
#include <float.h>

#include "clamped_bilerp.h"
#include "common.h"
#include "pred_grad.h"
#include "warp_grid.h"

namespace {

struct EpeTerm {
    float rho, dx, dy;
};
// one pixel's term at sampling position (ix, iy): rho, and with GRAD the derivative (Dx, Dy) of rho with respect to (ix, iy)
template <bool GRAD>
__device__ __forceinline__ EpeTerm epe_term(const float* __restrict__ gN, size_t plane, float ix, float iy, int h, int w, int H, int W,
                                            float eps2) {
    const Corner k = clamp_locate(ix, iy, W, H);
    const int o00 = k.ya * W + k.xa, o01 = k.ya * W + k.xb, o10 = k.yb * W + k.xa, o11 = k.yb * W + k.xb;
    const float a0 = gN[o00], b0 = gN[o01], c0 = gN[o10], d0 = gN[o11];
    const float a1 = gN[plane + o00], b1 = gN[plane + o01], c1 = gN[plane + o10], d1 = gN[plane + o11];
    const float rx = (ix - (float)w) + bilerp(a0, b0, c0, d0, k.tx, k.ty), ry = (iy - (float)h) + bilerp(a1, b1, c1, d1, k.tx, k.ty);
    EpeTerm t;
    t.rho = sqrtf(rx * rx + ry * ry + eps2);
    t.dx = 0.f;
    t.dy = 0.f;
    if (GRAD) {
        const float ux = rx / t.rho, uy = ry / t.rho;
        // the clamp stops the read's dependence on the position (a NaN position compares false: slope 0, the NaN arrives through u)
        const bool inx = ix >= 0.f && ix <= (float)(W - 1), iny = iy >= 0.f && iy <= (float)(H - 1);
        const float ex = 1.f - k.tx, ey = 1.f - k.ty;
        const float gxx = inx ? ey * (b0 - a0) + k.ty * (d0 - c0) : 0.f, gyx = inx ? ey * (b1 - a1) + k.ty * (d1 - c1) : 0.f;      // d g_x, g_y / d ix
        const float gxy = iny ? ex * (c0 - a0) + k.tx * (d0 - b0) : 0.f, gyy = iny ? ex * (c1 - a1) + k.tx * (d1 - b1) : 0.f;      // d g_x, g_y / d iy
        t.dx = ux * (1.f + gxx) + uy * gyx;
        t.dy = ux * gxy + uy * (1.f + gyy);
    }
    return t;
}

// A lane owns VEC consecutive pixels of a row whenever the row length allows it, aligned or not (WIDE: 16-byte loads): which pixels a
// lane sums does not depend on where the tensors lie, so neither do the loss's bits.
template <int MODE, int VEC, bool WIDE>
__global__ __launch_bounds__(256) void epe_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ g, float eps2,
                                                      float* __restrict__ partial, int H, int W) {
    __shared__ float red[16];
    const int n = blockIdx.y;
    float th[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (MODE == GRID_AFFINE) affine_theta(pred, n, th);
    const size_t plane = (size_t)H * W;
    const float* gN = g + (size_t)n * 2 * plane;
    const float* dN = MODE == GRID_UNET ? pred + (size_t)n * 2 * plane : nullptr;
    float acc = 0.f;
    const unsigned wq = W / VEC, items = (unsigned)H * wq;      // (H * W < 2^31 and the stride is < 2^20: no wrap)
    for (unsigned it = blockIdx.x * blockDim.x + threadIdx.x; it < items; it += gridDim.x * blockDim.x) {
        const int h = (int)(it / wq);
        const int w0 = (int)(it - (unsigned)h * wq) * VEC;
        float ax[VEC], ay[VEC];
        load_run<MODE, VEC, WIDE>(dN, plane, (size_t)h * W + w0, ax, ay);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            float ix, iy;
            warp_position<MODE>(ax[v], ay[v], h, w0 + v, H, W, th, ix, iy);
            acc += epe_term<false>(gN, plane, ix, iy, h, w0 + v, H, W, eps2).rho;
        }
    }
    const float t = block_sum(acc, red);
    if (threadIdx.x == 0) partial[(size_t)n * gridDim.x + blockIdx.x] = t;
}

// loss[0] (+)= scale * (all partials: thread t takes partials t, t + 256, ... in ascending order, then the fixed workgroup tree)
__global__ __launch_bounds__(256) void epe_fwd_merge_kernel(const float* __restrict__ partial, int count, float scale, int accumulate,
                                                            float* __restrict__ loss) {
    __shared__ float red[16];
    float acc = 0.f;
    for (int i = threadIdx.x; i < count; i += 256) acc += partial[i];
    const float t = block_sum(acc, red);
    if (threadIdx.x == 0) loss[0] = (accumulate ? loss[0] : 0.f) + scale * t;
}

template <int VEC>
__global__ __launch_bounds__(256) void epe_bwd_unet_kernel(const float* __restrict__ pred, const float* __restrict__ g, float eps2,
                                                           const float* __restrict__ gscale, float scale, float* __restrict__ gpred,
                                                           int accumulate, int H, int W) {
    const int n = blockIdx.y;
    const size_t plane = (size_t)H * W;
    const float* gN = g + (size_t)n * 2 * plane;
    const float* dN = pred + (size_t)n * 2 * plane;
    float* qN = gpred + (size_t)n * 2 * plane;
    const float k = gscale[0] * scale;
    const float kx = k * (0.5f * (float)W), ky = k * (0.5f * (float)H);      // d ix / d offset x = W / 2, d iy / d offset y = H / 2
    const unsigned wq = W / VEC, items = (unsigned)H * wq;
    for (unsigned it = blockIdx.x * blockDim.x + threadIdx.x; it < items; it += gridDim.x * blockDim.x) {
        const int h = (int)(it / wq);
        const int w0 = (int)(it - (unsigned)h * wq) * VEC;
        const size_t o = (size_t)h * W + w0;
        float ax[VEC], ay[VEC], ox[VEC], oy[VEC];
        load_run<GRID_UNET, VEC, true>(dN, plane, o, ax, ay);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            float ix, iy;
            warp_position<GRID_UNET>(ax[v], ay[v], h, w0 + v, H, W, nullptr, ix, iy);
            const EpeTerm t = epe_term<true>(gN, plane, ix, iy, h, w0 + v, H, W, eps2);
            ox[v] = kx * t.dx;
            oy[v] = ky * t.dy;
        }
        float* q = qN + o;
        if (VEC == 4) {
            float4 a = make_float4(ox[0], ox[1], ox[2], ox[3]), c = make_float4(oy[0], oy[1], oy[2], oy[3]);
            if (accumulate) {
                const float4 pa = *reinterpret_cast<const float4*>(q), pc = *reinterpret_cast<const float4*>(q + plane);
                a.x += pa.x; a.y += pa.y; a.z += pa.z; a.w += pa.w;
                c.x += pc.x; c.y += pc.y; c.z += pc.z; c.w += pc.w;
            }
            *reinterpret_cast<float4*>(q) = a;
            *reinterpret_cast<float4*>(q + plane) = c;
        } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                if (accumulate) { q[v] += ox[v]; q[plane + v] += oy[v]; } else { q[v] = ox[v]; q[plane + v] = oy[v]; }
            }
        }
    }
}

// the workgroup's six sums of (W/2) Dx (xb, yb, 1), (H/2) Dy (xb, yb, 1) -> its record
__global__ __launch_bounds__(256) void epe_bwd_affine_kernel(const float* __restrict__ pred, const float* __restrict__ g, float eps2,
                                                             float* __restrict__ partial, int H, int W) {
    __shared__ float red[16];
    const int n = blockIdx.y;
    float th[6];
    affine_theta(pred, n, th);
    const size_t plane = (size_t)H * W;
    const float* gN = g + (size_t)n * 2 * plane;
    const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
    float acc[EPE_WORDS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const unsigned items = (unsigned)H * (unsigned)W;
    for (unsigned it = blockIdx.x * blockDim.x + threadIdx.x; it < items; it += gridDim.x * blockDim.x) {
        const int h = (int)(it / (unsigned)W);
        const int w = (int)(it - (unsigned)h * (unsigned)W);
        float ix, iy;
        warp_position<GRID_AFFINE>(0.f, 0.f, h, w, H, W, th, ix, iy);
        const EpeTerm t = epe_term<true>(gN, plane, ix, iy, h, w, H, W, eps2);
        const float xb = affine_base(w, W), yb = affine_base(h, H);
        const float cx = hw * t.dx, cy = hh * t.dy;
        acc[0] += cx * xb; acc[1] += cx * yb; acc[2] += cx;
        acc[3] += cy * xb; acc[4] += cy * yb; acc[5] += cy;
    }
    float* dst = partial + ((size_t)n * gridDim.x + blockIdx.x) * EPE_WORDS;
#pragma unroll
    for (int c = 0; c < EPE_WORDS; ++c) {
        const float t = block_sum(acc[c], red);
        if (threadIdx.x == 0) dst[c] = t;
    }
}

// (the launch shape is the meter's: reg_blocks, clamped_bilerp.h; load_run, the affine merge, aligned4 and epe_shape_ok: pred_grad.h)
// factor / (N H W) as the kernels apply it
float epe_scale(float factor, int N, int H, int W) { return (float)((double)factor / ((double)N * H * W)); }

}  // namespace

NEMAR_API size_t nemar_epe_loss_workspace(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return sizeof(float) * EPE_WORDS * (size_t)reg_blocks(N, (long long)H * W) * N;
}

NEMAR_API int nemar_epe_loss_fwd(const float* pred, int grid_mode, const float* g, float eps, float factor, float* loss, int accumulate,
                                 void* workspace, size_t ws_bytes, int N, int H, int W, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(pred && g && loss && workspace, "epe_loss_fwd: null pointer");
    NEMAR_REQUIRE(aligned4(pred, g, loss, workspace), "epe_loss_fwd: pred, g, loss and workspace must be 4-byte aligned");
    NEMAR_REQUIRE(grid_mode == GRID_UNET || grid_mode == GRID_AFFINE, "epe_loss_fwd: grid_mode %d (NEMAR_GRID_UNET or NEMAR_GRID_AFFINE)",
                  grid_mode);
    NEMAR_REQUIRE(epe_shape_ok(N, H, W), "epe_loss_fwd: bad shape N=%d H=%d W=%d", N, H, W);
    NEMAR_REQUIRE(eps >= 0.f && eps <= FLT_MAX, "epe_loss_fwd: eps %g (finite, >= 0)", (double)eps);
    NEMAR_REQUIRE(ws_bytes >= nemar_epe_loss_workspace(N, H, W), "epe_loss_fwd: workspace %zu < %zu", ws_bytes,
                  nemar_epe_loss_workspace(N, H, W));
    hipStream_t st = (hipStream_t)stream;
    float* partial = (float*)workspace;
    const bool runs = grid_mode == GRID_UNET && (W & 3) == 0, wide = runs && aligned16(pred);
    const int gx = reg_blocks(N, (long long)H * (runs ? W / 4 : W));             // (<= the workspace query's count)
    const dim3 grid(gx, N), block(256);
    const float eps2 = eps * eps;
    if (grid_mode == GRID_AFFINE) hipLaunchKernelGGL((epe_fwd_kernel<GRID_AFFINE, 1, false>), grid, block, 0, st, pred, g, eps2, partial, H, W);
    else if (wide) hipLaunchKernelGGL((epe_fwd_kernel<GRID_UNET, 4, true>), grid, block, 0, st, pred, g, eps2, partial, H, W);
    else if (runs) hipLaunchKernelGGL((epe_fwd_kernel<GRID_UNET, 4, false>), grid, block, 0, st, pred, g, eps2, partial, H, W);
    else hipLaunchKernelGGL((epe_fwd_kernel<GRID_UNET, 1, false>), grid, block, 0, st, pred, g, eps2, partial, H, W);
    hipLaunchKernelGGL(epe_fwd_merge_kernel, dim3(1), dim3(256), 0, st, (const float*)partial, gx * N, epe_scale(factor, N, H, W), accumulate,
                       loss);
    NEMAR_CHECK_LAUNCH("epe_loss_fwd");
    return NEMAR_OK;
}

NEMAR_API int nemar_epe_loss_bwd(const float* pred, int grid_mode, const float* g, float eps, const float* gscale, float factor, float* gpred,
                                 int accumulate, void* workspace, size_t ws_bytes, int N, int H, int W, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(pred && g && gscale && gpred && workspace, "epe_loss_bwd: null pointer");
    NEMAR_REQUIRE(aligned4(pred, g, gscale, gpred, workspace), "epe_loss_bwd: pred, g, gscale, gpred and workspace must be 4-byte aligned");
    NEMAR_REQUIRE(grid_mode == GRID_UNET || grid_mode == GRID_AFFINE, "epe_loss_bwd: grid_mode %d (NEMAR_GRID_UNET or NEMAR_GRID_AFFINE)",
                  grid_mode);
    NEMAR_REQUIRE(epe_shape_ok(N, H, W), "epe_loss_bwd: bad shape N=%d H=%d W=%d", N, H, W);
    NEMAR_REQUIRE(eps >= 0.f && eps <= FLT_MAX, "epe_loss_bwd: eps %g (finite, >= 0)", (double)eps);
    NEMAR_REQUIRE(ws_bytes >= nemar_epe_loss_workspace(N, H, W), "epe_loss_bwd: workspace %zu < %zu", ws_bytes,
                  nemar_epe_loss_workspace(N, H, W));
    NEMAR_REQUIRE(gpred != pred, "epe_loss_bwd: gpred must not be the prediction");
    hipStream_t st = (hipStream_t)stream;
    const float eps2 = eps * eps, scale = epe_scale(factor, N, H, W);
    if (grid_mode == GRID_UNET) {
        const bool vec = (W & 3) == 0 && aligned16(pred, gpred);
        const dim3 grid(reg_blocks(N, (long long)H * (vec ? W / 4 : W)), N), block(256);
        if (vec) hipLaunchKernelGGL(epe_bwd_unet_kernel<4>, grid, block, 0, st, pred, g, eps2, gscale, scale, gpred, accumulate, H, W);
        else hipLaunchKernelGGL(epe_bwd_unet_kernel<1>, grid, block, 0, st, pred, g, eps2, gscale, scale, gpred, accumulate, H, W);
    } else {
        float* partial = (float*)workspace;
        const int gx = reg_blocks(N, (long long)H * W);
        hipLaunchKernelGGL(epe_bwd_affine_kernel, dim3(gx, N), dim3(256), 0, st, pred, g, eps2, partial, H, W);
        hipLaunchKernelGGL(epe_bwd_affine_merge_kernel, dim3(N), dim3(256), 0, st, (const float*)partial, gx, gscale, scale, gpred, accumulate);
    }
    NEMAR_CHECK_LAUNCH("epe_loss_bwd");
    return NEMAR_OK;
}
