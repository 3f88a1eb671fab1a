// Integrating a stationary velocity field by scaling and squaring (DESIGN.md "Diffeomorphic UNet STN"): one squaring step
//   a = s * u,   p(h, w) = (clamp(w + a0 * W/2, 0, W-1), clamp(h + a1 * H/2, 0, H-1)),   out = a + bilinear(a, p)
// on a displacement field u [N,2,H,W] in the units of NEMAR_GRID_UNET offsets, forward and backward (the definition is in
// include/nemar_hip.h).  Not a call site of the reference, whose UNet STN warps with the network's output as it is.  The identity of the
// integration is a TRUE identity — align_corners=True texel centres, a zero field samples its own texel — not the slight zoom of
// linspace(-1, 1) under align_corners=False, which stays where it is: in the final warp only.  K squarings would
// apply that zoom 2^K times.  Outside the image the border texel: the flow does not collapse at the border as it would under zero padding.
//
// Forward: one workgroup per 64 x 16 tile (resampled_grid.h), a lane owns one pixel in each of four rows, as compose_kernel.  The loads
// and stores at the pixel are coalesced (8 B/px each way); the four texels per channel are gathered at the data-dependent p: 32 B/px of
// loads that hit L2 — a network-size field is at most 512 KB per sample.  Positions are clamped in float BEFORE the integer conversion:
// fmaxf / fminf also tame NaN and +-inf, so no input value can index outside the plane.
//
// Backward: d out / d u has three parts, each times s — the direct term gout(x); the image path, w_k(x') gout(x') scattered into the four
// corners of every p(x'); the position path at the texel itself, sum_ch gout_ch(x) d bilinear_ch / d p_c (W/2 or H/2), zero along an axis
// whose raw position was clamped.  The last steps of a chain move tens of pixels, so the image path cannot be a gather over a fixed
// window; fp32 atomics would make it depend on arrival order.  It is scattered with 64-bit FIXED-POINT integer atomics — integer addition
// is associative: bitwise repeatable, whatever the field — as far_scatter_kernel / far_fold_kernel (warp.hip) do for the far pixels of
// the warp's gradient:
//   svf_max_kernel       per-workgroup max |gout| (bit patterns) into the workspace's partial words: found on the device, no host read;
//   svf_scatter_kernel   the 64 x 16 tile: the pixel's u and gout (coalesced), its p and weights, 8 atomics into the accumulator
//                        [N][H*W][2] (both channels of a texel side by side: a wave's 64 pixels of a row land on 1 KB where the field
//                        is smooth), contributions scaled by 2^(FIX - e), max |gout| < 2^e;
//   svf_fold_kernel      the same tile: direct + position term of its own pixel (gathers a's corners as the forward does), + accumulator
//                        / scale, times s, into gu (or added to it, rounded once); the accumulator goes back to all-zero.
// FIX = 40 bits below the largest gradient while the plane has fewer than 2^22 pixels, 62 - ceil(log2(H W)) beyond: even if every pixel of
// a plane lands on one border texel the 64-bit sum cannot overflow.  Nothing synchronises with the host: capturable into the step graph.
// Plain fp32 apart from that accumulator, built without contraction like its neighbours.
#include "common.h"
#include "fixed_scatter.h"
#include "pred_launch.h"

namespace {

// where pixel (h, w) with scaled displacement (a0, a1) samples: the top-left texel (x0, y0) of its 2 x 2 patch, the other corner clamped
// into the plane (x1 == x0 at the last column: its weight is then 0), the fractional position, whether the raw position was clamped
struct SvfPos {
    int x0, y0, x1, y1;
    float tx, ty;
    bool cx, cy;
};
__device__ __forceinline__ SvfPos svf_locate(float a0, float a1, int h, int w, int H, int W, float hw, float hh) {
    const float rx = (float)w + a0 * hw, ry = (float)h + a1 * hh;
    const float mx = (float)(W - 1), my = (float)(H - 1);
    const float px = fminf(fmaxf(rx, 0.f), mx), py = fminf(fmaxf(ry, 0.f), my);      // (NaN -> 0: fmaxf returns the other operand)
    SvfPos q;
    q.x0 = (int)px; q.y0 = (int)py;                                                  // 0 <= p: the conversion is the floor
    q.x1 = min(q.x0 + 1, W - 1); q.y1 = min(q.y0 + 1, H - 1);
    q.tx = px - (float)q.x0; q.ty = py - (float)q.y0;
    q.cx = rx < 0.f || rx > mx; q.cy = ry < 0.f || ry > my;
    return q;
}

// a = s * u at the four corners of one channel
struct SvfCorners {
    float v00, v01, v10, v11;
};
__device__ __forceinline__ SvfCorners svf_corners(const float* __restrict__ p, const SvfPos& q, int W, float s) {
    const size_t r0 = (size_t)q.y0 * W, r1 = (size_t)q.y1 * W;
    return SvfCorners{s * p[r0 + q.x0], s * p[r0 + q.x1], s * p[r1 + q.x0], s * p[r1 + q.x1]};
}

__global__ __launch_bounds__(RT_THREADS) void svf_step_fwd_kernel(const float* __restrict__ u, float s, float* __restrict__ out, int H, int W) {
    const int n = blockIdx.z, tid = threadIdx.x;
    const int x0 = blockIdx.x * RT_W, y0 = blockIdx.y * RT_H;
    const size_t plane = (size_t)H * W;
    const float* uN = u + (size_t)n * 2 * plane;
    float* oN = out + (size_t)n * 2 * plane;
    const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
    constexpr int ROWS = RT_THREADS / RT_W, RUNS = RT_H / ROWS;      // a lane owns one pixel in each of RUNS rows: a wave = 64 pixels of a row
#pragma unroll
    for (int i = 0; i < RUNS; ++i) {
        const int h = y0 + tid / RT_W + ROWS * i, w = x0 + tid % RT_W;
        if (h >= H || w >= W) continue;
        const size_t o = (size_t)h * W + w;
        const float a0 = s * uN[o], a1 = s * uN[plane + o];
        const SvfPos q = svf_locate(a0, a1, h, w, H, W, hw, hh);
        const float ex = 1.f - q.tx, ey = 1.f - q.ty;
        const float wnw = ex * ey, wne = q.tx * ey, wsw = ex * q.ty, wse = q.tx * q.ty;
        const SvfCorners c0 = svf_corners(uN, q, W, s), c1 = svf_corners(uN + plane, q, W, s);
        oN[o] = a0 + (c0.v00 * wnw + c0.v01 * wne + c0.v10 * wsw + c0.v11 * wse);
        oN[plane + o] = a1 + (c1.v00 * wnw + c1.v01 * wne + c1.v10 * wsw + c1.v11 * wse);
    }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
// (the scale of the fixed-point scatter — svf_max_kernel, svf_exponent, svf_pow2, svf_fix_bits — is in fixed_scatter.h)
__global__ __launch_bounds__(RT_THREADS) void svf_scatter_kernel(const float* __restrict__ u, float s, const float* __restrict__ gout,
                                                                 long long* __restrict__ acc, const unsigned* __restrict__ partial,
                                                                 int partials, int fix, int H, int W) {
    __shared__ unsigned red[4];
    const int n = blockIdx.z, tid = threadIdx.x;
    const int x0 = blockIdx.x * RT_W, y0 = blockIdx.y * RT_H;
    const size_t plane = (size_t)H * W;
    const float* uN = u + (size_t)n * 2 * plane;
    const float* gN = gout + (size_t)n * 2 * plane;
    unsigned long long* aN = reinterpret_cast<unsigned long long*>(acc) + (size_t)n * 2 * plane;
    const float scale = svf_pow2(fix - svf_exponent(partial, partials, red));      // products with it are exact
    const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
    constexpr int ROWS = RT_THREADS / RT_W, RUNS = RT_H / ROWS;
#pragma unroll
    for (int i = 0; i < RUNS; ++i) {
        const int h = y0 + tid / RT_W + ROWS * i, w = x0 + tid % RT_W;
        if (h >= H || w >= W) continue;
        const size_t o = (size_t)h * W + w;
        const SvfPos q = svf_locate(s * uN[o], s * uN[plane + o], h, w, H, W, hw, hh);
        const float g0 = gN[o], g1 = gN[plane + o];
        const float ex = 1.f - q.tx, ey = 1.f - q.ty;
        const float wk[4] = {ex * ey, q.tx * ey, ex * q.ty, q.tx * q.ty};
        const size_t tex[4] = {(size_t)q.y0 * W + q.x0, (size_t)q.y0 * W + q.x1, (size_t)q.y1 * W + q.x0, (size_t)q.y1 * W + q.x1};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (wk[k] == 0.f) continue;          // (also the clamped corner of the last column / row)
            atomicAdd(aN + 2 * tex[k], (unsigned long long)__float2ll_rn((wk[k] * g0) * scale));
            atomicAdd(aN + 2 * tex[k] + 1, (unsigned long long)__float2ll_rn((wk[k] * g1) * scale));
        }
    }
}

__global__ __launch_bounds__(RT_THREADS) void svf_fold_kernel(const float* __restrict__ u, float s, const float* __restrict__ gout,
                                                              float* __restrict__ gu, int accumulate, long long* __restrict__ acc,
                                                              const unsigned* __restrict__ partial, int partials, int fix, int H, int W) {
    __shared__ unsigned red[4];
    const int n = blockIdx.z, tid = threadIdx.x;
    const int x0 = blockIdx.x * RT_W, y0 = blockIdx.y * RT_H;
    const size_t plane = (size_t)H * W;
    const float* uN = u + (size_t)n * 2 * plane;
    const float* gN = gout + (size_t)n * 2 * plane;
    float* guN = gu + (size_t)n * 2 * plane;
    long long* aN = acc + (size_t)n * 2 * plane;
    const float unscale = svf_pow2(svf_exponent(partial, partials, red) - fix);
    const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
    constexpr int ROWS = RT_THREADS / RT_W, RUNS = RT_H / ROWS;
#pragma unroll
    for (int i = 0; i < RUNS; ++i) {
        const int h = y0 + tid / RT_W + ROWS * i, w = x0 + tid % RT_W;
        if (h >= H || w >= W) continue;
        const size_t o = (size_t)h * W + w;
        const SvfPos q = svf_locate(s * uN[o], s * uN[plane + o], h, w, H, W, hw, hh);
        const float g0 = gN[o], g1 = gN[plane + o];
        const SvfCorners c0 = svf_corners(uN, q, W, s), c1 = svf_corners(uN + plane, q, W, s);
        const float ex = 1.f - q.tx, ey = 1.f - q.ty;
        // d bilinear_ch / d p.x, d p.y: zero along an axis whose raw position was clamped
        const float dx0 = q.cx ? 0.f : ey * (c0.v01 - c0.v00) + q.ty * (c0.v11 - c0.v10);
        const float dx1 = q.cx ? 0.f : ey * (c1.v01 - c1.v00) + q.ty * (c1.v11 - c1.v10);
        const float dy0 = q.cy ? 0.f : ex * (c0.v10 - c0.v00) + q.tx * (c0.v11 - c0.v01);
        const float dy1 = q.cy ? 0.f : ex * (c1.v10 - c1.v00) + q.tx * (c1.v11 - c1.v01);
        const float t0 = g0 + hw * (g0 * dx0 + g1 * dx1);           // direct + position term
        const float t1 = g1 + hh * (g0 * dy0 + g1 * dy1);
        const long long i0 = aN[2 * o], i1 = aN[2 * o + 1];
        if (i0 != 0) aN[2 * o] = 0;
        if (i1 != 0) aN[2 * o + 1] = 0;
        const float r0 = s * (t0 + (float)i0 * unscale), r1 = s * (t1 + (float)i1 * unscale);
        if (accumulate) { guN[o] += r0; guN[plane + o] += r1; } else { guN[o] = r0; guN[plane + o] = r1; }
    }
}

bool svf_shape_ok(int N, int H, int W) {
    return N > 0 && H > 0 && W > 0 && N <= 65535 && (long long)H * W < (1ll << 31) && nemar_cdiv(H, RT_H) <= 65535;
}
}  // namespace

NEMAR_API int nemar_svf_step_fwd(const float* u, float scale, float* out, int N, int H, int W, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(u && out, "svf_step_fwd: null pointer");
    NEMAR_REQUIRE(((((uintptr_t)u) | ((uintptr_t)out)) & 3) == 0, "svf_step_fwd: u and out must be 4-byte aligned");
    NEMAR_REQUIRE(svf_shape_ok(N, H, W), "svf_step_fwd: bad shape N=%d H=%d W=%d", N, H, W);
    NEMAR_REQUIRE(out != u, "svf_step_fwd: out must not be the operand (the kernel gathers from it)");
    const dim3 grid(nemar_cdiv(W, RT_W), nemar_cdiv(H, RT_H), N), block(RT_THREADS);
    hipLaunchKernelGGL(svf_step_fwd_kernel, grid, block, 0, (hipStream_t)stream, u, scale, out, H, W);
    NEMAR_CHECK_LAUNCH("svf_step_fwd");
    return NEMAR_OK;
}

NEMAR_API size_t nemar_svf_step_bwd_zeroed_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return sizeof(long long) * 2 * (size_t)N * H * W;
}
NEMAR_API size_t nemar_svf_step_bwd_workspace(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return nemar_svf_step_bwd_zeroed_bytes(N, H, W) + sizeof(unsigned) * SVF_MAX_PARTIALS;
}

NEMAR_API int nemar_svf_step_bwd(const float* u, float scale, const float* gout, float* gu, int accumulate, void* workspace, size_t ws_bytes,
                                 int N, int H, int W, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(u && gout && gu && workspace, "svf_step_bwd: null pointer");
    NEMAR_REQUIRE(((((uintptr_t)u) | ((uintptr_t)gout) | ((uintptr_t)gu)) & 3) == 0 && (((uintptr_t)workspace) & 7) == 0,
                  "svf_step_bwd: u, gout and gu must be 4-byte aligned, workspace 8-byte aligned");
    NEMAR_REQUIRE(svf_shape_ok(N, H, W), "svf_step_bwd: bad shape N=%d H=%d W=%d", N, H, W);
    NEMAR_REQUIRE(gu != u && gu != gout, "svf_step_bwd: gu must not be an operand");
    NEMAR_REQUIRE(ws_bytes >= nemar_svf_step_bwd_workspace(N, H, W), "svf_step_bwd: workspace %zu < %zu", ws_bytes,
                  nemar_svf_step_bwd_workspace(N, H, W));
    hipStream_t st = (hipStream_t)stream;
    long long* acc = (long long*)workspace;
    unsigned* partial = (unsigned*)((char*)workspace + nemar_svf_step_bwd_zeroed_bytes(N, H, W));
    const int partials = svf_partials(N, H, W), fix = svf_fix_bits(H, W);
    const dim3 grid(nemar_cdiv(W, RT_W), nemar_cdiv(H, RT_H), N), block(RT_THREADS);
    hipLaunchKernelGGL(svf_max_kernel, dim3(partials), dim3(256), 0, st, gout, (long long)N * 2 * H * W, partial);
    hipLaunchKernelGGL(svf_scatter_kernel, grid, block, 0, st, u, scale, gout, acc, (const unsigned*)partial, partials, fix, H, W);
    hipLaunchKernelGGL(svf_fold_kernel, grid, block, 0, st, u, scale, gout, gu, accumulate, acc, (const unsigned*)partial, partials, fix, H, W);
    NEMAR_CHECK_LAUNCH("svf_step_bwd");
    return NEMAR_OK;
}
