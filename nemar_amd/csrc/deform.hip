// Known-misalignment training pairs and the registration-error meter (DESIGN.md "Known misalignment").  Not in the reference, whose
// loaders serve the misaligned pairs of its data sets as they are: here the input pipeline deforms modality A by a seeded smooth
// transformation whose field travels with the batch, and the meter reports how far the STN's prediction is from undoing it.
//
// Conventions: pixel coordinates q = (x, y), integer values at pixel centres, origin at the top-left pixel of the output crop
// [Hc, Wc].  A ground-truth field g is [B,2,Hc,Wc] fp32 IN PIXELS, channel 0 = x (the UNet STN's channel order); the deformed image
// is A'(q) = A_crop(q + g(q)).
//   nemar_deform_field                 g from per-sample parameters: affine about the crop centre + cubic B-spline lattice
//   nemar_crop_flip_deform_normalize   nemar_crop_flip_normalize sampling bilinearly at q + g(q), border-clamped
//   nemar_crop_flip_deform_labels      its label twin: the same window, flip and positions, nearest sampling, class ids copied
//   nemar_registration_error           residual r(x) = S(x) + g(S(x)) - x of the warp's own sampling position S(x) (warp_grid.h)
//
// All three are HBM-bound streaming kernels (8 B/px written; 8 + 4C B/px + gathers; 16 B/px read): one lane owns VEC consecutive
// pixels of a row — 16-byte loads / stores when the row length is a multiple of 4 and the tensors are 16-byte aligned, one pixel
// per lane otherwise.  No floating-point atomics: the meter's sums are per-workgroup partials merged in a fixed order, so every
// result is bitwise repeatable.
#include "common.h"
#include "clamped_bilerp.h"
#include "warp_grid.h"

namespace {

// ---- (a) ground-truth field --------------------------------------------------------------------------------------------------
// uniform cubic B-spline basis on one segment, t in [0, 1]: a partition of unity, C2 across segments
__device__ __forceinline__ void bspline_weights(float t, float w[4]) {
    const float t2 = t * t, t3 = t2 * t, u = 1.f - t;
    w[0] = (u * u * u) * (1.f / 6.f);
    w[1] = (3.f * t3 - 6.f * t2 + 4.f) * (1.f / 6.f);
    w[2] = (-3.f * t3 + 3.f * t2 + 3.f * t + 1.f) * (1.f / 6.f);
    w[3] = t3 * (1.f / 6.f);
}
// segment and basis of pixel i of `size` on a lattice of `gn` control points: the gn - 3 segments span [0, size - 1], so the four
// control points of every pixel are inside the lattice.  (i * (gn - 3) is exact; one rounding in the quotient.)
__device__ __forceinline__ int lattice_segment(int i, int size, int gn, float w[4]) {
    const float u = size > 1 ? (float)(i * (gn - 3)) / (float)(size - 1) : 0.f;
    const int j = min((int)u, gn - 4);
    bspline_weights(u - (float)j, w);
    return j;
}

// params [B, 6 + 2 gh gw]: a11 a12 tx a21 a22 ty, then the lattice [2, gh, gw] (displacements in pixels; gh = gw = 0: none).
// g(q) = (M - I)(q - c) + t + spline(q), c = the crop centre: the centred form keeps every product small.
template <int VEC>
__global__ __launch_bounds__(256) void deform_field_kernel(const float* __restrict__ params, float* __restrict__ g, int Hc, int Wc,
                                                           int gh, int gw) {
    const int n = blockIdx.y;
    const float* p = params + (size_t)n * (6 + 2 * gh * gw);
    const float m00 = p[0] - 1.f, m01 = p[1], tx = p[2], m10 = p[3], m11 = p[4] - 1.f, ty = p[5];
    const float* lat = p + 6;
    const float cx = 0.5f * (float)(Wc - 1), cy = 0.5f * (float)(Hc - 1);
    const size_t plane = (size_t)Hc * Wc;
    float* gN = g + (size_t)n * 2 * plane;
    const int wq = Wc / VEC, items = Hc * wq;
    for (int it = blockIdx.x * blockDim.x + threadIdx.x; it < items; it += gridDim.x * blockDim.x) {
        const int h = it / wq;
        const int w0 = (it - h * wq) * VEC;
        const float dy = (float)h - cy;
        float wy[4] = {0.f, 0.f, 0.f, 0.f};
        const int jy = gh ? lattice_segment(h, Hc, gh, wy) : 0;
        float ox[VEC], oy[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const float dx = (float)(w0 + v) - cx;
            ox[v] = m00 * dx + m01 * dy + tx;
            oy[v] = m10 * dx + m11 * dy + ty;
            if (gh) {
                float wx[4];
                const int jx = lattice_segment(w0 + v, Wc, gw, wx);
                float e[2];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const float* q = lat + (size_t)c * gh * gw + (size_t)jy * gw + jx;
                    float acc = 0.f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float* r = q + j * gw;
                        acc += wy[j] * (((wx[0] * r[0] + wx[1] * r[1]) + wx[2] * r[2]) + wx[3] * r[3]);
                    }
                    e[c] = acc;
                }
                ox[v] += e[0];
                oy[v] += e[1];
            }
        }
        float* q = gN + (size_t)h * Wc + w0;
        if (VEC == 4) {
            *reinterpret_cast<float4*>(q) = make_float4(ox[0], ox[1], ox[2], ox[3]);
            *reinterpret_cast<float4*>(q + plane) = make_float4(oy[0], oy[1], oy[2], oy[3]);
        } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) { q[v] = ox[v]; q[plane + v] = oy[v]; }
        }
    }
}

// (the bilinear read with border clamp that the sampler and the meter share — clamp_locate, bilerp — and warp_position: clamped_bilerp.h)

// ---- (b) crop + flip + deform + normalise ------------------------------------------------------------------------------------------
// y[b][c][q] = (F_b(q + g_b(q)) * scale - 0.5) / 0.5, F_b = the cropped-and-flipped image of crop_flip_normalize_kernel read bilinearly
// with the position clamped to the crop window.  With g == 0 the weights are (1, 0, 0, 0) and the value is the texel's own: the output
// is crop_flip_normalize_kernel's bit for bit.  The crop window (device data) is clamped into the pool: every address is in bounds.
template <int VEC>
__global__ __launch_bounds__(256) void crop_flip_deform_normalize_kernel(const float* __restrict__ pool, const int* __restrict__ params,
                                                                         const float* __restrict__ g, float* __restrict__ y, int M, int C,
                                                                         int H, int W, int Hc, int Wc, float scale) {
    const int b = blockIdx.y;
    const int4 pr = reinterpret_cast<const int4*>(params)[b];
    const int idx = min(max(pr.x, 0), M - 1), y0 = min(max(pr.y, 0), H - Hc), x0 = min(max(pr.z, 0), W - Wc);
    const bool flip = pr.w != 0;
    const size_t cplane = (size_t)Hc * Wc, pplane = (size_t)H * W;
    const float* gN = g + (size_t)b * 2 * cplane;
    float* yN = y + (size_t)b * C * cplane;
    const float* src = pool + (size_t)idx * C * pplane + (size_t)y0 * W;     // row y0 of channel 0
    const int wq = Wc / VEC, items = Hc * wq;
    for (int it = blockIdx.x * blockDim.x + threadIdx.x; it < items; it += gridDim.x * blockDim.x) {
        const int h = it / wq;
        const int w0 = (it - h * wq) * VEC;
        const size_t o = (size_t)h * Wc + w0;
        float gx[VEC], gy[VEC];
        if (VEC == 4) {
            const float4 a = *reinterpret_cast<const float4*>(gN + o), c = *reinterpret_cast<const float4*>(gN + cplane + o);
            gx[0] = a.x; gx[1] = a.y; gx[2] = a.z; gx[3] = a.w;
            gy[0] = c.x; gy[1] = c.y; gy[2] = c.z; gy[3] = c.w;
        } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) { gx[v] = gN[o + v]; gy[v] = gN[cplane + o + v]; }
        }
        int o00[VEC], o01[VEC], o10[VEC], o11[VEC];
        float tx[VEC], ty[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const Corner k = clamp_locate((float)(w0 + v) + gx[v], (float)h + gy[v], Wc, Hc);
            const int sa = flip ? x0 + Wc - 1 - k.xa : x0 + k.xa, sb = flip ? x0 + Wc - 1 - k.xb : x0 + k.xb;
            o00[v] = k.ya * W + sa; o01[v] = k.ya * W + sb; o10[v] = k.yb * W + sa; o11[v] = k.yb * W + sb;
            tx[v] = k.tx; ty[v] = k.ty;
        }
        for (int c = 0; c < C; ++c) {
            const float* p = src + (size_t)c * pplane;
            float r[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const float t = bilerp(p[o00[v]], p[o01[v]], p[o10[v]], p[o11[v]], tx[v], ty[v]);
                r[v] = (t * scale - 0.5f) / 0.5f;
            }
            float* q = yN + (size_t)c * cplane + o;
            if (VEC == 4) {
                *reinterpret_cast<float4*>(q) = make_float4(r[0], r[1], r[2], r[3]);
            } else {
#pragma unroll
                for (int v = 0; v < VEC; ++v) q[v] = r[v];
            }
        }
    }
}

// ---- (b') crop + flip + deform of a label map ------------------------------------------------------------------------------------------
// The label twin of crop_flip_deform_normalize_kernel: pool [M,1,H,W] float class ids, the same crop window and flip, the same positions
// q + g(q) clamped to the crop window — read by NEAREST sampling, round half to even (rintf: the rounding of taps_at<SAMPLE_NEAREST>,
// resampled_grid.h), and copied: a class id is never blended and never normalised.  DEFORM false (g == NULL): the plain crop / flip copy,
// which g == 0 gives too (rintf of an integer is the integer).  fmaxf / fminf drop a NaN: every address is in the crop window.
template <int VEC, bool DEFORM>
__global__ __launch_bounds__(256) void crop_flip_deform_labels_kernel(const float* __restrict__ pool, const int* __restrict__ params,
                                                                      const float* __restrict__ g, float* __restrict__ y, int M, int H, int W,
                                                                      int Hc, int Wc) {
    const int b = blockIdx.y;
    const int4 pr = reinterpret_cast<const int4*>(params)[b];
    const int idx = min(max(pr.x, 0), M - 1), y0 = min(max(pr.y, 0), H - Hc), x0 = min(max(pr.z, 0), W - Wc);
    const bool flip = pr.w != 0;
    const size_t cplane = (size_t)Hc * Wc, pplane = (size_t)H * W;
    const float* gN = DEFORM ? g + (size_t)b * 2 * cplane : nullptr;
    float* yN = y + (size_t)b * cplane;
    const float* src = pool + (size_t)idx * pplane + (size_t)y0 * W;     // row y0 of the map
    const int wq = Wc / VEC, items = Hc * wq;
    for (int it = blockIdx.x * blockDim.x + threadIdx.x; it < items; it += gridDim.x * blockDim.x) {
        const int h = it / wq;
        const int w0 = (it - h * wq) * VEC;
        const size_t o = (size_t)h * Wc + w0;
        float gx[VEC], gy[VEC], r[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) { gx[v] = 0.f; gy[v] = 0.f; }
        if (DEFORM) {
            if (VEC == 4) {
                const float4 a = *reinterpret_cast<const float4*>(gN + o), c = *reinterpret_cast<const float4*>(gN + cplane + o);
                gx[0] = a.x; gx[1] = a.y; gx[2] = a.z; gx[3] = a.w;
                gy[0] = c.x; gy[1] = c.y; gy[2] = c.z; gy[3] = c.w;
            } else {
#pragma unroll
                for (int v = 0; v < VEC; ++v) { gx[v] = gN[o + v]; gy[v] = gN[cplane + o + v]; }
            }
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const float cx = fminf(fmaxf((float)(w0 + v) + gx[v], 0.f), (float)(Wc - 1)), cy = fminf(fmaxf((float)h + gy[v], 0.f), (float)(Hc - 1));
            const int xn = (int)rintf(cx), yn = (int)rintf(cy);
            r[v] = src[yn * W + (flip ? x0 + Wc - 1 - xn : x0 + xn)];
        }
        float* q = yN + o;
        if (VEC == 4) {
            *reinterpret_cast<float4*>(q) = make_float4(r[0], r[1], r[2], r[3]);
        } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) q[v] = r[v];
        }
    }
}

// ---- (c) registration-error meter ----------------------------------------------------------------------------------------------------
// Per workgroup one partial of REG_WORDS 32-bit words: valid count (u32), sum |r| (f32), max |r| (f32), sum |g(x)| (f32), fold count (u32),
// interior count (u32), two unused.  Counts stay integers until the merge writes them as floats (exact up to 2^24 pixels per sample).
constexpr int REG_WORDS = 8;

__device__ __forceinline__ unsigned block_sum_u(unsigned v, unsigned* red) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    unsigned t = 0;
    for (int i = 0; i < nw; ++i) t += red[i];
    return t;
}
__device__ __forceinline__ float block_max(float v, float* red) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_max(v);
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    float t = red[0];
    for (int i = 1; i < nw; ++i) t = fmaxf(t, red[i]);
    return t;
}

struct RegAcc {
    unsigned valid, fold, interior;
    float sum_r, max_r, sum_g;
};
// the workgroup's totals -> words (thread 0 stores; the tree is fixed, so the bits are the same on every run)
__device__ __forceinline__ void reg_block_store(const RegAcc& a, unsigned* __restrict__ dst, float* red, unsigned* redu, bool as_float) {
    const unsigned valid = block_sum_u(a.valid, redu), fold = block_sum_u(a.fold, redu), interior = block_sum_u(a.interior, redu);
    const float sum_r = block_sum(a.sum_r, red), sum_g = block_sum(a.sum_g, red), max_r = block_max(a.max_r, red);
    if (threadIdx.x == 0) {
        if (as_float) {                 // out [N,6]
            float* o = reinterpret_cast<float*>(dst);
            o[0] = (float)valid; o[1] = sum_r; o[2] = max_r; o[3] = sum_g; o[4] = (float)fold; o[5] = (float)interior;
        } else {
            dst[0] = valid; dst[1] = __float_as_uint(sum_r); dst[2] = __float_as_uint(max_r); dst[3] = __float_as_uint(sum_g);
            dst[4] = fold; dst[5] = interior;
        }
    }
}

template <int MODE, int VEC>
__global__ __launch_bounds__(256) void registration_error_kernel(const float* __restrict__ pred, const float* __restrict__ g,
                                                                 unsigned* __restrict__ partial, int H, int W) {
    __shared__ float red[16];
    __shared__ unsigned redu[16];
    const int n = blockIdx.y;
    float th[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (MODE == GRID_AFFINE) {
        affine_theta(pred, n, th);
    }
    const size_t plane = (size_t)H * W;
    const float* gN = g + (size_t)n * 2 * plane;
    const float* dN = MODE == GRID_UNET ? pred + (size_t)n * 2 * plane : nullptr;
    RegAcc acc = {0u, 0u, 0u, 0.f, 0.f, 0.f};
    const int wq = W / VEC, items = H * wq;
    for (int it = blockIdx.x * blockDim.x + threadIdx.x; it < items; it += gridDim.x * blockDim.x) {
        const int h = it / wq;
        const int w0 = (it - h * wq) * VEC;
        const size_t o = (size_t)h * W + w0;
        const bool below = h + 1 < H, right = w0 + VEC < W;      // the row below / the pixel right of this lane's run exist
        // grid_src values of the run, its right neighbour, and the run one row below (UNET: the offsets; AFFINE: none)
        float ax[VEC + 1], ay[VEC + 1], bx[VEC], by[VEC];
#pragma unroll
        for (int v = 0; v <= VEC; ++v) { ax[v] = 0.f; ay[v] = 0.f; }
#pragma unroll
        for (int v = 0; v < VEC; ++v) { bx[v] = 0.f; by[v] = 0.f; }
        float g0[VEC], g1[VEC];
        if (VEC == 4) {
            const float4 a = *reinterpret_cast<const float4*>(gN + o), c = *reinterpret_cast<const float4*>(gN + plane + o);
            g0[0] = a.x; g0[1] = a.y; g0[2] = a.z; g0[3] = a.w;
            g1[0] = c.x; g1[1] = c.y; g1[2] = c.z; g1[3] = c.w;
        } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) { g0[v] = gN[o + v]; g1[v] = gN[plane + o + v]; }
        }
        if (MODE == GRID_UNET) {
            const size_t ob = below ? o + W : o;                 // (no row below: re-read the own row, never used)
            if (VEC == 4) {
                const float4 a = *reinterpret_cast<const float4*>(dN + o), c = *reinterpret_cast<const float4*>(dN + plane + o);
                const float4 e = *reinterpret_cast<const float4*>(dN + ob), f = *reinterpret_cast<const float4*>(dN + plane + ob);
                ax[0] = a.x; ax[1] = a.y; ax[2] = a.z; ax[3] = a.w;
                ay[0] = c.x; ay[1] = c.y; ay[2] = c.z; ay[3] = c.w;
                bx[0] = e.x; bx[1] = e.y; bx[2] = e.z; bx[3] = e.w;
                by[0] = f.x; by[1] = f.y; by[2] = f.z; by[3] = f.w;
            } else {
#pragma unroll
                for (int v = 0; v < VEC; ++v) { ax[v] = dN[o + v]; ay[v] = dN[plane + o + v]; bx[v] = dN[ob + v]; by[v] = dN[plane + ob + v]; }
            }
            const size_t orr = right ? o + VEC : o;
            ax[VEC] = dN[orr];
            ay[VEC] = dN[plane + orr];
        }
        // sampled positions: the run and its right neighbour (row h), the run one row below
        float sx[VEC + 1], sy[VEC + 1], tx[VEC], ty[VEC];
#pragma unroll
        for (int v = 0; v <= VEC; ++v) warp_position<MODE>(ax[v], ay[v], h, w0 + v, H, W, th, sx[v], sy[v]);
#pragma unroll
        for (int v = 0; v < VEC; ++v) warp_position<MODE>(bx[v], by[v], h + 1, w0 + v, H, W, th, tx[v], ty[v]);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const float ix = sx[v], iy = sy[v];
            const bool valid = ix >= 0.f && ix <= (float)(W - 1) && iy >= 0.f && iy <= (float)(H - 1);
            // g at S(x): bilinear, addresses clamped so that the loads are unconditional
            const Corner k = clamp_locate(ix, iy, W, H);
            const int o00 = k.ya * W + k.xa, o01 = k.ya * W + k.xb, o10 = k.yb * W + k.xa, o11 = k.yb * W + k.xb;
            const float gsx = bilerp(gN[o00], gN[o01], gN[o10], gN[o11], k.tx, k.ty);
            const float gsy = bilerp(gN[plane + o00], gN[plane + o01], gN[plane + o10], gN[plane + o11], k.tx, k.ty);
            const float rx = (ix - (float)(w0 + v)) + gsx, ry = (iy - (float)h) + gsy;       // r = S + g(S) - x
            const float rn = sqrtf(rx * rx + ry * ry);
            if (valid) {
                acc.valid += 1u;
                acc.sum_r += rn;
                acc.max_r = fmaxf(acc.max_r, rn);
            }
            acc.sum_g += sqrtf(g0[v] * g0[v] + g1[v] * g1[v]);
            if (below && (v + 1 < VEC || right)) {
                // Jacobian of x -> S(x) by forward differences; a non-positive determinant is a fold
                const float det = (sx[v + 1] - ix) * (ty[v] - iy) - (tx[v] - ix) * (sy[v + 1] - iy);
                acc.interior += 1u;
                if (det <= 0.f) acc.fold += 1u;
            }
        }
    }
    reg_block_store(acc, partial + ((size_t)n * gridDim.x + blockIdx.x) * REG_WORDS, red, redu, false);
}

// out[n] = the sample's partials merged: thread t takes partials t, t + 256, ... in ascending order, then the fixed workgroup tree
__global__ __launch_bounds__(256) void registration_error_merge_kernel(const unsigned* __restrict__ partial, int n_partial, float* __restrict__ out) {
    __shared__ float red[16];
    __shared__ unsigned redu[16];
    const int n = blockIdx.x;
    const unsigned* p = partial + (size_t)n * n_partial * REG_WORDS;
    RegAcc acc = {0u, 0u, 0u, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < n_partial; i += blockDim.x) {
        const unsigned* q = p + (size_t)i * REG_WORDS;
        acc.valid += q[0];
        acc.sum_r += __uint_as_float(q[1]);
        acc.max_r = fmaxf(acc.max_r, __uint_as_float(q[2]));
        acc.sum_g += __uint_as_float(q[3]);
        acc.fold += q[4];
        acc.interior += q[5];
    }
    reg_block_store(acc, reinterpret_cast<unsigned*>(out + (size_t)n * 6), red, redu, true);
}

// (reg_blocks, aligned16: clamped_bilerp.h)

}  // namespace

NEMAR_API int nemar_deform_field(const float* params, float* g, int B, int Hc, int Wc, int gh, int gw, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(params && g, "deform_field: null pointer");
    NEMAR_REQUIRE(B > 0 && B <= 65535 && Hc > 0 && Wc > 0 && Hc <= 32768 && Wc <= 32768, "deform_field: bad shape B=%d Hc=%d Wc=%d", B, Hc, Wc);
    NEMAR_REQUIRE((gh == 0 && gw == 0) || (gh >= 4 && gw >= 4 && gh <= 4096 && gw <= 4096),
                  "deform_field: lattice %d x %d (a cubic B-spline needs at least 4 x 4 control points; 0 x 0 = none)", gh, gw);
    const bool vec = (Wc & 3) == 0 && aligned16(g);
    const long long items = (long long)Hc * (vec ? Wc / 4 : Wc);
    dim3 grid(reg_blocks(B, items), B), block(256);
    if (vec) hipLaunchKernelGGL((deform_field_kernel<4>), grid, block, 0, (hipStream_t)stream, params, g, Hc, Wc, gh, gw);
    else hipLaunchKernelGGL((deform_field_kernel<1>), grid, block, 0, (hipStream_t)stream, params, g, Hc, Wc, gh, gw);
    NEMAR_CHECK_LAUNCH("deform_field");
    return NEMAR_OK;
}

NEMAR_API int nemar_crop_flip_deform_normalize(const float* pool, const int* params, const float* g, float* y, int M, int B, int C, int H,
                                               int W, int Hc, int Wc, float scale, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(pool && params && g && y, "crop_flip_deform_normalize: null pointer");
    NEMAR_REQUIRE(M > 0 && B > 0 && B <= 65535 && C > 0 && Hc > 0 && Wc > 0 && Hc <= H && Wc <= W && (long long)H * W < (1ll << 31),
                  "crop_flip_deform_normalize: bad arguments");
    NEMAR_REQUIRE((((uintptr_t)params) & 15) == 0, "crop_flip_deform_normalize: params must be 16-byte aligned");
    const bool vec = (Wc & 3) == 0 && aligned16(g, y);
    const long long items = (long long)Hc * (vec ? Wc / 4 : Wc);
    dim3 grid(reg_blocks(B, items), B), block(256);
    if (vec)
        hipLaunchKernelGGL((crop_flip_deform_normalize_kernel<4>), grid, block, 0, (hipStream_t)stream, pool, params, g, y, M, C, H, W, Hc, Wc,
                           scale);
    else
        hipLaunchKernelGGL((crop_flip_deform_normalize_kernel<1>), grid, block, 0, (hipStream_t)stream, pool, params, g, y, M, C, H, W, Hc, Wc,
                           scale);
    NEMAR_CHECK_LAUNCH("crop_flip_deform_normalize");
    return NEMAR_OK;
}

NEMAR_API int nemar_crop_flip_deform_labels(const float* pool, const int* params, const float* g, float* y, int M, int B, int H, int W,
                                            int Hc, int Wc, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(pool && params && y, "crop_flip_deform_labels: null pointer");
    NEMAR_REQUIRE(M > 0 && B > 0 && B <= 65535 && Hc > 0 && Wc > 0 && Hc <= H && Wc <= W && (long long)H * W < (1ll << 31),
                  "crop_flip_deform_labels: bad arguments");
    NEMAR_REQUIRE((((uintptr_t)params) & 15) == 0, "crop_flip_deform_labels: params must be 16-byte aligned");
    NEMAR_REQUIRE(((((uintptr_t)pool) | ((uintptr_t)g) | ((uintptr_t)y)) & 3) == 0, "crop_flip_deform_labels: pool, g and y must be 4-byte aligned");
    const bool vec = (Wc & 3) == 0 && aligned16(g, y);
    const long long items = (long long)Hc * (vec ? Wc / 4 : Wc);
    const dim3 grid(reg_blocks(B, items), B), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (g && vec) hipLaunchKernelGGL((crop_flip_deform_labels_kernel<4, true>), grid, block, 0, st, pool, params, g, y, M, H, W, Hc, Wc);
    else if (g) hipLaunchKernelGGL((crop_flip_deform_labels_kernel<1, true>), grid, block, 0, st, pool, params, g, y, M, H, W, Hc, Wc);
    else if (vec) hipLaunchKernelGGL((crop_flip_deform_labels_kernel<4, false>), grid, block, 0, st, pool, params, g, y, M, H, W, Hc, Wc);
    else hipLaunchKernelGGL((crop_flip_deform_labels_kernel<1, false>), grid, block, 0, st, pool, params, g, y, M, H, W, Hc, Wc);
    NEMAR_CHECK_LAUNCH("crop_flip_deform_labels");
    return NEMAR_OK;
}

NEMAR_API size_t nemar_registration_error_workspace(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return sizeof(unsigned) * REG_WORDS * (size_t)reg_blocks(N, (long long)H * W) * N;
}

NEMAR_API int nemar_registration_error(const float* pred, int grid_mode, const float* g, float* out, void* workspace, size_t ws_bytes, int N,
                                       int H, int W, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(pred && g && out && workspace, "registration_error: null pointer");
    NEMAR_REQUIRE(grid_mode == GRID_UNET || grid_mode == GRID_AFFINE, "registration_error: grid_mode %d (NEMAR_GRID_UNET or NEMAR_GRID_AFFINE)",
                  grid_mode);
    NEMAR_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && (long long)H * W < (1ll << 31), "registration_error: bad shape N=%d H=%d W=%d", N, H, W);
    NEMAR_REQUIRE(ws_bytes >= nemar_registration_error_workspace(N, H, W) && (((uintptr_t)workspace) & 3) == 0,
                  "registration_error: workspace %zu < %zu", ws_bytes, nemar_registration_error_workspace(N, H, W));
    hipStream_t st = (hipStream_t)stream;
    unsigned* partial = (unsigned*)workspace;
    const bool vec = grid_mode == GRID_UNET && (W & 3) == 0 && aligned16(pred, g);
    const int gx = reg_blocks(N, (long long)H * (vec ? W / 4 : W));             // (<= the workspace query's count)
    dim3 grid(gx, N), block(256);
    if (grid_mode == GRID_AFFINE) hipLaunchKernelGGL((registration_error_kernel<GRID_AFFINE, 1>), grid, block, 0, st, pred, g, partial, H, W);
    else if (vec) hipLaunchKernelGGL((registration_error_kernel<GRID_UNET, 4>), grid, block, 0, st, pred, g, partial, H, W);
    else hipLaunchKernelGGL((registration_error_kernel<GRID_UNET, 1>), grid, block, 0, st, pred, g, partial, H, W);
    hipLaunchKernelGGL(registration_error_merge_kernel, dim3(N), dim3(256), 0, st, (const unsigned*)partial, gx, out);
    NEMAR_CHECK_LAUNCH("registration_error");
    return NEMAR_OK;
}
