// A loss that trains against label overlap (DESIGN.md "Soft-Dice loss"): the Dice that nemar_label_overlap (score.hip) reports, made
// differentiable by warping the moving label map bilinearly instead of nearest.  Not a call site of the reference, which has no labels.
//
// Definition.  lm [N,H,W] the moving label map and lf [N,H,W] the fixed one, float class ids read by class_of (label_class.h: k iff the
// value == (float)k for an integer 0 <= k < K; anything else is no class); pred the prediction at that same size, NEMAR_GRID_UNET offsets
// [N,2,H,W] or NEMAR_GRID_AFFINE dtheta [N,6].  For output pixel x, S(x) = (ix, iy) is the position the warp samples (warp_grid.h: the bits of
// nemar_grid_sample_fwd), and the 2 x 2 cell and (tx, ty) are locate()'s — the image warp's own rule, ZEROS padding: a corner outside the
// image belongs to no class.
//   p_k(x) = sum of the bilinear weights of the in-image corners whose class is k,     f_k(x) = [class_of(lf[x]) == k]
//   per sample and class   I = sum_x p_k f_k,   M = sum_x p_k,   F = sum_x f_k
//   dice = (2 I + eps) / (M + F + eps),   eps > 0 in pixels
//   loss = factor / (N Kc) * sum_n sum_{k >= k0} (1 - dice),   k0 = 0 or 1 (1: background excluded), Kc = K - k0
// A class absent from both maps has dice 1 and gradient 0; the denominator N Kc does not depend on the data.
// A pixel whose ix or iy is not finite contributes NOTHING to I and M and gets gradient 0 (its f_k still counts): the float is tested before
// it is quantised, because an integer sum cannot carry a NaN — unlike the EPE loss (epe.hip), which is NaN where it hears from one.
// Every corner address is clamped into the map, whatever the position holds.
//
// Forward sums (nemar_dice_sums): sums [N,K,3] uint64 = I and M in fixed point with DICE_FIX_BITS fractional bits, F a plain pixel count.
// Every corner weight is rounded ONCE (__float2ll_rn of weight * 2^DICE_FIX_BITS, as integrate.hip quantises) and added as an integer.
// Range: a weight is a product of two floats in [0, 1], so its quantised value is <= 2^30; a pixel adds four of them whose weights sum to
// 1 within four half-unit roundings, < 2^30 + 2 + a few float ulps of 2^30 < 2^31; a sample has H W < 2^31 pixels: every counter stays
// below 2^62 < 2^63.  Integer addition is associative and commutative, so the sums do not depend on the order in which lanes, waves and
// workgroups arrive: bitwise repeatable with no fixed-order merge, whichever route (16-byte or 4-byte loads) a call takes.
// The shape is label_overlap_kernel's: a workgroup grid-strides over 64 x 16 tiles of one sample, keeps its 3 K counters in LDS (64-bit for
// I and M), clears them once and flushes the non-zero ones with one global 64-bit integer atomicAdd each at the end.  The four corners of
// a pixel are folded by class first (label maps are piecewise constant: inside a segment a pixel makes one LDS add to M and one to I, not
// four each), and a corner of weight 0 is not added; F is counted by wave_count (wave_count.h), as the score counts.
//
// Finalising (nemar_dice_loss_fwd = the sums + one launch of one workgroup): the N K triples are converted in double, the 1 - dice terms
// are added in a fixed order, and the backward's coefficient table coef [N,K,2] float is written: with D = M + F + eps, c = factor / (N Kc)
//   a = -2 c / D,   b = c (2 I + eps) / D^2   (both 0 for k < k0),   so that dL/dp_k(x) = a f_k(x) + b.
//
// Backward (nemar_dice_loss_bwd), a gather that does not repeat the sums: per pixel the four corners give q_c = a[k_c] [k_c == kf] + b[k_c]
// (0 for a corner outside the image or of no class), and the slope of the cell floor() chose, as in epe.hip:
//   dL/dix = (1 - ty) (q01 - q00) + ty (q11 - q10),   dL/diy = (1 - tx) (q10 - q00) + tx (q11 - q01).
// The sample's coef rows are staged in LDS (<= 8 KiB).
// UNet: gpred[n,0,h,w] (+)= gscale[0] (W/2) dL/dix, gpred[n,1,h,w] (+)= gscale[0] (H/2) dL/diy — one launch, 16-byte stores on the vector route.
// Affine: the six sums per workgroup go to the workspace and are merged per sample in a fixed order (pred_grad.h: the EPE loss's merge).
// No float atomics anywhere.
#include <float.h>

#include "common.h"
#include "label_class.h"
#include "pred_grad.h"
#include "pred_launch.h"
#include "wave_count.h"

namespace {

constexpr int DICE_FIX_BITS = 30;
constexpr float DICE_FIX_ONE = (float)(1 << DICE_FIX_BITS);
constexpr int DICE_TW = 64, DICE_TH = 16;      // a tile: label_overlap_kernel's

// the cell of output pixel (h, w): locate()'s corner and fractions, and the classes of its four corners in lm (-1: outside the image, no
// class, or a position that is not finite).  k[0..3]: (y0, x0), (y0, x0+1), (y0+1, x0), (y0+1, x0+1)
struct DiceCell {
    float tx, ty;
    int k[4];
};
template <int MODE>
__device__ __forceinline__ DiceCell dice_cell(const float* __restrict__ lmN, float sx, float sy, int h, int w, int H, int W, int K,
                                              const float* th) {
    float gx, gy, ix, iy;
    grid_coord<MODE>(RegSrc{sx, sy}, h, w, H, W, th, gx, gy);
    sample_position(gx, gy, W, H, ix, iy);                                  // (warp_position's bits)
    const bool finite = fabsf(ix) <= FLT_MAX && fabsf(iy) <= FLT_MAX;       // (a NaN compares false)
    const Sample s = locate(gx, gy, W, H);                                  // (a NaN position: x0 = -2, every corner outside)
    const bool xa = s.x0 >= 0 && s.x0 < W, xb = s.x0 + 1 >= 0 && s.x0 + 1 < W;
    const bool ya = s.y0 >= 0 && s.y0 < H, yb = s.y0 + 1 >= 0 && s.y0 + 1 < H;
    const int cxa = min(max(s.x0, 0), W - 1), cxb = min(max(s.x0 + 1, 0), W - 1);
    const int cya = min(max(s.y0, 0), H - 1), cyb = min(max(s.y0 + 1, 0), H - 1);
    const float v00 = lmN[cya * W + cxa], v01 = lmN[cya * W + cxb], v10 = lmN[cyb * W + cxa], v11 = lmN[cyb * W + cxb];
    DiceCell c;
    c.tx = finite ? s.tx : 0.f;
    c.ty = finite ? s.ty : 0.f;
    c.k[0] = finite && xa && ya ? class_of(v00, K) : -1;
    c.k[1] = finite && xb && ya ? class_of(v01, K) : -1;
    c.k[2] = finite && xa && yb ? class_of(v10, K) : -1;
    c.k[3] = finite && xb && yb ? class_of(v11, K) : -1;
    return c;
}

// the fixed map's VEC values at offset o (16-byte load when VEC == 4: the vector route is taken only for aligned tensors)
template <int VEC>
__device__ __forceinline__ void load_fixed(const float* __restrict__ lfN, size_t o, float* fv) {
    if (VEC == 4) {
        const float4 a = *reinterpret_cast<const float4*>(lfN + o);
        fv[0] = a.x; fv[1] = a.y; fv[2] = a.z; fv[3] = a.w;
    } else {
#pragma unroll
        for (int v = 0; v < VEC; ++v) fv[v] = lfN[o + v];
    }
}

// KCAP: the tables' capacity in classes (K <= KCAP) — 256 (5 KiB of LDS) or 1024 (20 KiB: eight workgroups still fit a CU's 160 KiB)
template <int MODE, int VEC, int KCAP>
__global__ __launch_bounds__(256) void dice_sums_kernel(const float* __restrict__ pred, const float* __restrict__ lm,
                                                        const float* __restrict__ lf, unsigned long long* __restrict__ sums, int K, int H,
                                                        int W, int tiles_x, int tiles) {
    __shared__ unsigned long long hI[KCAP], hM[KCAP];
    __shared__ unsigned hF[KCAP];
    const int n = blockIdx.y, tid = threadIdx.x;
    float th[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (MODE == GRID_AFFINE) affine_theta(pred, n, th);
    const size_t plane = (size_t)H * W;
    const float* lmN = lm + (size_t)n * plane;
    const float* lfN = lf + (size_t)n * plane;
    const float* dN = MODE == GRID_UNET ? pred + (size_t)n * 2 * plane : nullptr;

    for (int e = tid; e < K; e += 256) { hI[e] = 0ull; hM[e] = 0ull; hF[e] = 0u; }
    __syncthreads();

    constexpr int RUNS_X = DICE_TW / VEC, ROWS = 256 / RUNS_X, TRIPS = DICE_TH / ROWS;      // a lane owns VEC consecutive pixels of a row
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {         // (the same trip count in every lane of the workgroup)
        const int tyi = t / tiles_x;
        const int x0 = (t - tyi * tiles_x) * DICE_TW, y0 = tyi * DICE_TH;
#pragma unroll
        for (int i = 0; i < TRIPS; ++i) {
            const int h = y0 + tid / RUNS_X + ROWS * i, w0 = x0 + (tid % RUNS_X) * VEC;
            const bool inside = h < H && w0 < W;                  // (VEC == 4 only when W % 4 == 0: a run is inside or outside as a whole;
                                                                  //  no early exit: the whole wave reaches wave_count's ballots)
            float ax[VEC], ay[VEC], fv[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) { ax[v] = 0.f; ay[v] = 0.f; fv[v] = -1.f; }
            if (inside) {
                const size_t o = (size_t)h * W + w0;
                load_run<MODE, VEC, true>(dN, plane, o, ax, ay);
                load_fixed<VEC>(lfN, o, fv);
            }
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const int kf = inside ? class_of(fv[v], K) : -1;
                if (inside) {
                    DiceCell c = dice_cell<MODE>(lmN, ax[v], ay[v], h, w0 + v, H, W, K, th);
                    const float ex = 1.f - c.tx, ey = 1.f - c.ty;
                    long long q[4] = {__float2ll_rn((ex * ey) * DICE_FIX_ONE), __float2ll_rn((c.tx * ey) * DICE_FIX_ONE),
                                      __float2ll_rn((ex * c.ty) * DICE_FIX_ONE), __float2ll_rn((c.tx * c.ty) * DICE_FIX_ONE)};
                    // corners of one class are added once (integers: the sum is the same)
#pragma unroll
                    for (int a = 1; a < 4; ++a) {
#pragma unroll
                        for (int b = 0; b < a; ++b) {
                            if (c.k[a] >= 0 && c.k[a] == c.k[b]) { q[b] += q[a]; c.k[a] = -1; }
                        }
                    }
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        if (c.k[a] >= 0 && q[a] != 0) {
                            atomicAdd(&hM[c.k[a]], (unsigned long long)q[a]);
                            if (c.k[a] == kf) atomicAdd(&hI[c.k[a]], (unsigned long long)q[a]);
                        }
                    }
                }
                wave_count(hF, kf, 0);
            }
        }
    }
    __syncthreads();
    unsigned long long* sN = sums + (size_t)n * K * 3;            // [K,3]: I, M, F
    for (int e = tid; e < K; e += 256) {
        const unsigned long long vi = hI[e], vm = hM[e], vf = hF[e];
        if (vi) atomicAdd(&sN[e * 3], vi);
        if (vm) atomicAdd(&sN[e * 3 + 1], vm);
        if (vf) atomicAdd(&sN[e * 3 + 2], vf);
    }
}

// one workgroup: loss[0] (+)= c * sum over (n, k >= k0) of (1 - dice) — thread t takes triples t, t + 256, ... in ascending order (in
// double), then the fixed workgroup tree —, and coef[n,k] = (a, b)
__global__ __launch_bounds__(256) void dice_finalize_kernel(const unsigned long long* __restrict__ sums, int NK, int K, int k0, double eps,
                                                            double c, float* __restrict__ coef, float* __restrict__ loss, int accumulate) {
    __shared__ float red[16];
    const double unit = 1.0 / (double)(1ll << DICE_FIX_BITS);
    double acc = 0.0;
    for (int i = threadIdx.x; i < NK; i += 256) {
        const int k = i % K;
        const double I = (double)sums[(size_t)i * 3] * unit, M = (double)sums[(size_t)i * 3 + 1] * unit, F = (double)sums[(size_t)i * 3 + 2];
        const double D = M + F + eps, num = 2.0 * I + eps;
        const bool on = k >= k0;
        coef[(size_t)i * 2] = on ? (float)(-2.0 * c / D) : 0.f;
        coef[(size_t)i * 2 + 1] = on ? (float)(c * num / (D * D)) : 0.f;
        if (on) acc += 1.0 - num / D;
    }
    const float t = block_sum((float)acc, red);
    if (threadIdx.x == 0) loss[0] = (accumulate ? loss[0] : 0.f) + (float)c * t;
}

// the sample's coef rows -> LDS
__device__ __forceinline__ void stage_coef(float* cf, const float* __restrict__ coef, int n, int K) {
    for (int e = threadIdx.x; e < 2 * K; e += 256) cf[e] = coef[(size_t)n * K * 2 + e];
    __syncthreads();
}

// (dL/dix, dL/diy) of one pixel whose fixed class is kf
__device__ __forceinline__ void dice_slopes(const DiceCell& c, int kf, const float* cf, float& dx, float& dy) {
    float q[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int k = c.k[a], kk = k >= 0 ? k : 0;
        const float qa = (k == kf ? cf[2 * kk] : 0.f) + cf[2 * kk + 1];
        q[a] = k >= 0 ? qa : 0.f;
    }
    dx = (1.f - c.ty) * (q[1] - q[0]) + c.ty * (q[3] - q[2]);
    dy = (1.f - c.tx) * (q[2] - q[0]) + c.tx * (q[3] - q[1]);
}

template <int VEC>
__global__ __launch_bounds__(256) void dice_bwd_unet_kernel(const float* __restrict__ pred, const float* __restrict__ lm,
                                                            const float* __restrict__ lf, const float* __restrict__ coef,
                                                            const float* __restrict__ gscale, float* __restrict__ gpred, int accumulate,
                                                            int K, int H, int W) {
    __shared__ float cf[2 * MAX_CLASSES];
    const int n = blockIdx.y;
    stage_coef(cf, coef, n, K);
    const size_t plane = (size_t)H * W;
    const float* lmN = lm + (size_t)n * plane;
    const float* lfN = lf + (size_t)n * plane;
    const float* dN = pred + (size_t)n * 2 * plane;
    float* qN = gpred + (size_t)n * 2 * plane;
    const float k = gscale[0];
    const float kx = k * (0.5f * (float)W), ky = k * (0.5f * (float)H);      // d ix / d offset x = W / 2, d iy / d offset y = H / 2
    const unsigned wq = W / VEC, items = (unsigned)H * wq;      // (H * W < 2^31 and the stride is < 2^20: no wrap)
    for (unsigned it = blockIdx.x * blockDim.x + threadIdx.x; it < items; it += gridDim.x * blockDim.x) {
        const int h = (int)(it / wq);
        const int w0 = (int)(it - (unsigned)h * wq) * VEC;
        const size_t o = (size_t)h * W + w0;
        float ax[VEC], ay[VEC], fv[VEC], ox[VEC], oy[VEC];
        load_run<GRID_UNET, VEC, true>(dN, plane, o, ax, ay);
        load_fixed<VEC>(lfN, o, fv);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const DiceCell c = dice_cell<GRID_UNET>(lmN, ax[v], ay[v], h, w0 + v, H, W, K, nullptr);
            float dx, dy;
            dice_slopes(c, class_of(fv[v], K), cf, dx, dy);
            ox[v] = kx * dx;
            oy[v] = ky * dy;
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

// the workgroup's six sums of (W/2) dL/dix (xb, yb, 1), (H/2) dL/diy (xb, yb, 1) -> its record (epe_bwd_affine_kernel's shape)
__global__ __launch_bounds__(256) void dice_bwd_affine_kernel(const float* __restrict__ pred, const float* __restrict__ lm,
                                                              const float* __restrict__ lf, const float* __restrict__ coef,
                                                              float* __restrict__ partial, int K, int H, int W) {
    __shared__ float cf[2 * MAX_CLASSES];
    __shared__ float red[16];
    const int n = blockIdx.y;
    stage_coef(cf, coef, n, K);
    float th[6];
    affine_theta(pred, n, th);
    const size_t plane = (size_t)H * W;
    const float* lmN = lm + (size_t)n * plane;
    const float* lfN = lf + (size_t)n * plane;
    const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
    float acc[EPE_WORDS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const unsigned items = (unsigned)H * (unsigned)W;
    for (unsigned it = blockIdx.x * blockDim.x + threadIdx.x; it < items; it += gridDim.x * blockDim.x) {
        const int h = (int)(it / (unsigned)W);
        const int w = (int)(it - (unsigned)h * (unsigned)W);
        const DiceCell c = dice_cell<GRID_AFFINE>(lmN, 0.f, 0.f, h, w, H, W, K, th);
        float dx, dy;
        dice_slopes(c, class_of(lfN[it], K), cf, dx, dy);
        const float xb = affine_base(w, W), yb = affine_base(h, H);
        const float cx = hw * dx, cy = hh * dy;
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

template <int MODE, int VEC>
void launch_sums(const float* pred, const float* lm, const float* lf, unsigned long long* sums, int N, int K, int H, int W, hipStream_t st) {
    const int tiles_x = nemar_cdiv(W, DICE_TW), tiles = tiles_x * nemar_cdiv(H, DICE_TH);
    // every workgroup clears and flushes its own 3 K counters: what the chip holds at once and no more (eight workgroups of four waves
    // per CU with either table)
    const dim3 grid(resident_groups(N, 8, tiles), N), block(256);
    if (K <= 256) hipLaunchKernelGGL((dice_sums_kernel<MODE, VEC, 256>), grid, block, 0, st, pred, lm, lf, sums, K, H, W, tiles_x, tiles);
    else hipLaunchKernelGGL((dice_sums_kernel<MODE, VEC, MAX_CLASSES>), grid, block, 0, st, pred, lm, lf, sums, K, H, W, tiles_x, tiles);
}

// what nemar_dice_sums and nemar_dice_loss_fwd share: the checks, the clear and the launch
int dice_sums(const char* entry, const float* pred, int grid_mode, const float* lm, const float* lf, unsigned long long* sums, int N, int K,
              int H, int W, hipStream_t st) {
    NEMAR_REQUIRE(pred && lm && lf && sums, "%s: null pointer", entry);
    NEMAR_REQUIRE(aligned4(pred, lm, lf, sums) && ((uintptr_t)sums & 7) == 0,
                  "%s: pred, labels_moving and labels_fixed must be 4-byte aligned, sums 8-byte aligned", entry);
    NEMAR_REQUIRE(grid_mode == GRID_UNET || grid_mode == GRID_AFFINE, "%s: grid_mode %d (NEMAR_GRID_UNET or NEMAR_GRID_AFFINE)", entry, grid_mode);
    NEMAR_REQUIRE(K >= 1 && K <= MAX_CLASSES, "%s: %d classes (1 .. %d)", entry, K, MAX_CLASSES);
    NEMAR_REQUIRE(epe_shape_ok(N, H, W), "%s: bad shape N=%d H=%d W=%d", entry, N, H, W);
    NEMAR_HIP_CALL(hipMemsetAsync(sums, 0, (size_t)N * K * 3 * sizeof(unsigned long long), st));
    if (grid_mode == GRID_AFFINE) launch_sums<GRID_AFFINE, 1>(pred, lm, lf, sums, N, K, H, W, st);
    else if ((W & 3) == 0 && aligned16(pred, lf)) launch_sums<GRID_UNET, 4>(pred, lm, lf, sums, N, K, H, W, st);
    else launch_sums<GRID_UNET, 1>(pred, lm, lf, sums, N, K, H, W, st);
    return NEMAR_OK;
}

}  // namespace

NEMAR_API size_t nemar_dice_loss_workspace(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return sizeof(float) * EPE_WORDS * (size_t)reg_blocks(N, (long long)H * W) * N;
}

NEMAR_API int nemar_dice_sums(const float* pred, int grid_mode, const float* labels_moving, const float* labels_fixed,
                              unsigned long long* sums, int N, int K, int H, int W, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    const int rc = dice_sums("dice_sums", pred, grid_mode, labels_moving, labels_fixed, sums, N, K, H, W, (hipStream_t)stream);
    if (rc != NEMAR_OK) return rc;
    NEMAR_CHECK_LAUNCH("dice_sums");
    return NEMAR_OK;
}

NEMAR_API int nemar_dice_loss_fwd(const float* pred, int grid_mode, const float* labels_moving, const float* labels_fixed, int K, int k0,
                                  float eps, float factor, float* loss, int accumulate, unsigned long long* sums, float* coef, int N, int H,
                                  int W, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(loss && coef, "dice_loss_fwd: null pointer");
    NEMAR_REQUIRE(aligned4(loss, coef, nullptr, nullptr), "dice_loss_fwd: loss and coef must be 4-byte aligned");
    NEMAR_REQUIRE(K >= 1 && K <= MAX_CLASSES, "dice_loss_fwd: %d classes (1 .. %d)", K, MAX_CLASSES);
    NEMAR_REQUIRE((k0 == 0 || k0 == 1) && k0 < K, "dice_loss_fwd: first class %d (0 or 1, below the %d classes)", k0, K);
    NEMAR_REQUIRE(eps > 0.f && eps <= FLT_MAX, "dice_loss_fwd: eps %g (finite, > 0)", (double)eps);
    hipStream_t st = (hipStream_t)stream;
    const int rc = dice_sums("dice_loss_fwd", pred, grid_mode, labels_moving, labels_fixed, sums, N, K, H, W, st);
    if (rc != NEMAR_OK) return rc;
    hipLaunchKernelGGL(dice_finalize_kernel, dim3(1), dim3(256), 0, st, (const unsigned long long*)sums, N * K, K, k0, (double)eps,
                       (double)factor / ((double)N * (K - k0)), coef, loss, accumulate);
    NEMAR_CHECK_LAUNCH("dice_loss_fwd");
    return NEMAR_OK;
}

NEMAR_API int nemar_dice_loss_bwd(const float* pred, int grid_mode, const float* labels_moving, const float* labels_fixed, const float* coef,
                                  int K, const float* gscale, float* gpred, int accumulate, void* workspace, size_t ws_bytes, int N, int H,
                                  int W, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(pred && labels_moving && labels_fixed && coef && gscale && gpred && workspace, "dice_loss_bwd: null pointer");
    NEMAR_REQUIRE(aligned4(pred, labels_moving, labels_fixed, coef, gscale) && aligned4(gpred, workspace, nullptr, nullptr),
                  "dice_loss_bwd: pred, labels_moving, labels_fixed, coef, gscale, gpred and workspace must be 4-byte aligned");
    NEMAR_REQUIRE(grid_mode == GRID_UNET || grid_mode == GRID_AFFINE, "dice_loss_bwd: grid_mode %d (NEMAR_GRID_UNET or NEMAR_GRID_AFFINE)",
                  grid_mode);
    NEMAR_REQUIRE(K >= 1 && K <= MAX_CLASSES, "dice_loss_bwd: %d classes (1 .. %d)", K, MAX_CLASSES);
    NEMAR_REQUIRE(epe_shape_ok(N, H, W), "dice_loss_bwd: bad shape N=%d H=%d W=%d", N, H, W);
    NEMAR_REQUIRE(ws_bytes >= nemar_dice_loss_workspace(N, H, W), "dice_loss_bwd: workspace %zu < %zu", ws_bytes,
                  nemar_dice_loss_workspace(N, H, W));
    NEMAR_REQUIRE(gpred != pred, "dice_loss_bwd: gpred must not be the prediction");
    hipStream_t st = (hipStream_t)stream;
    if (grid_mode == GRID_UNET) {
        const bool vec = (W & 3) == 0 && aligned16(pred, gpred, labels_fixed);
        const dim3 grid(reg_blocks(N, (long long)H * (vec ? W / 4 : W)), N), block(256);
        if (vec) hipLaunchKernelGGL(dice_bwd_unet_kernel<4>, grid, block, 0, st, pred, labels_moving, labels_fixed, coef, gscale, gpred, accumulate, K, H, W);
        else hipLaunchKernelGGL(dice_bwd_unet_kernel<1>, grid, block, 0, st, pred, labels_moving, labels_fixed, coef, gscale, gpred, accumulate, K, H, W);
    } else {
        float* partial = (float*)workspace;
        const int gx = reg_blocks(N, (long long)H * W);
        hipLaunchKernelGGL(dice_bwd_affine_kernel, dim3(gx, N), dim3(256), 0, st, pred, labels_moving, labels_fixed, coef, partial, K, H, W);
        hipLaunchKernelGGL(epe_bwd_affine_merge_kernel, dim3(N), dim3(256), 0, st, (const float*)partial, gx, gscale, 1.f, gpred, accumulate);
    }
    NEMAR_CHECK_LAUNCH("dice_loss_bwd");
    return NEMAR_OK;
}
