// Where the warp kernels sample: the (never materialised) sampling grid of nemar_grid_sample_fwd/bwd and the pixel position it
// unnormalises to.  Shared by warp.hip (the warp itself) and deform.hip (the registration-error meter, which measures the SAME
// positions against a known ground-truth field) — one statement of the arithmetic, so the two cannot drift apart.
#pragma once
#include "common.h"

namespace {

constexpr int GRID_EXPLICIT = 0;  // grid [N,Ho,Wo,2]  (x,y) interleaved, normalised coords
constexpr int GRID_UNET = 1;      // offsets [N,2,Ho,Wo] planar; + linspace(-1,1) identity (ch0 = x)
constexpr int GRID_AFFINE = 2;    // dtheta [N,6]; theta = dtheta + [1,0,0,0,1,0]; affine_grid(align_corners=False)

// torch.linspace(-1, 1, n)[i] in fp32: fused multiply-add from the nearer end (ATen RangeFactories
// symmetric form; bit-exact against torch CPU, see tests/test_oracle_torch.py).  linspace_at is its continuous extension
// -1 + 2p/(n-1) (score.hip: annotated points between pixels), the same expression — at an integer p the same bits
__device__ __forceinline__ float linspace_at(float p, int n) {
    if (n <= 1) return -1.f;
    const float step = 2.f / (float)(n - 1);
    return (2.f * p < (float)(n - 1)) ? fmaf(step, p, -1.f) : fmaf(-step, (float)(n - 1) - p, 1.f);
}
__device__ __forceinline__ float linspace_m1_p1(int i, int n) {
    if (n <= 1) return -1.f;
    const float step = 2.f / (float)(n - 1);
    return (i < n / 2) ? fmaf(step, (float)i, -1.f) : fmaf(-step, (float)(n - 1 - i), 1.f);
}
// affine_grid base coordinate, align_corners=False: (2i+1)/n - 1 (affine_base_at: at a continuous coordinate)
__device__ __forceinline__ float affine_base_at(float p, int n) { return (2.f * p + 1.f) / (float)n - 1.f; }
__device__ __forceinline__ float affine_base(int i, int n) { return affine_base_at((float)i, n); }

// theta = dtheta + identity of sample n (reference models/stn/affine_stn.py:96,122)
__device__ __forceinline__ void affine_theta(const float* gsrc, int n, float* th) {
#pragma unroll
    for (int i = 0; i < 6; ++i) th[i] = gsrc[n * 6 + i] + ((i == 0 || i == 4) ? 1.f : 0.f);
}

// normalised grid coordinate of output pixel (h, w).  `src` supplies the pixel's two grid_src values — x() and y() — from wherever the
// caller holds them (GridSrc below: global memory; deform.hip: registers filled by 16-byte loads): the grid itself (EXPLICIT), the offsets
// added to the reference's linspace identity (UNET), or nothing — theta alone (AFFINE)
template <int MODE, class Src>
__device__ __forceinline__ void grid_coord(const Src& src, int h, int w, int Ho, int Wo, const float* th, float& gx, float& gy) {
    if (MODE == GRID_EXPLICIT) {
        gx = src.x();
        gy = src.y();
    } else if (MODE == GRID_UNET) {
        gx = linspace_m1_p1(w, Wo) + src.x();
        gy = linspace_m1_p1(h, Ho) + src.y();
    } else {
        const float xb = affine_base(w, Wo), yb = affine_base(h, Ho);
        gx = th[0] * xb + th[1] * yb + th[2];
        gy = th[3] * xb + th[4] * yb + th[5];
    }
}
// the two values of pixel (h, w) of sample n in grid_src itself
template <int MODE>
struct GridSrc {
    const float* p;
    size_t step;        // from the x value to the y value
    __device__ __forceinline__ GridSrc(const float* gsrc, int n, int h, int w, int Ho, int Wo) : p(gsrc), step(0) {
        if (MODE == GRID_EXPLICIT) {
            p = gsrc + (((size_t)n * Ho + h) * Wo + w) * 2;
            step = 1;
        } else if (MODE == GRID_UNET) {
            const size_t plane = (size_t)Ho * Wo;
            p = gsrc + (size_t)n * 2 * plane + (size_t)h * Wo + w;
            step = plane;
        }
    }
    __device__ __forceinline__ float x() const { return p[0]; }
    __device__ __forceinline__ float y() const { return p[step]; }
};
// the two grid_src values of a pixel held in registers (deform.hip: filled by 16-byte loads; register.hip: interpolated from a coarse field)
struct RegSrc {
    float sx, sy;
    __device__ __forceinline__ float x() const { return sx; }
    __device__ __forceinline__ float y() const { return sy; }
};

template <int MODE>
__device__ __forceinline__ void make_grid(const float* __restrict__ gsrc, int n, int h, int w, int Ho, int Wo,
                                          const float* th, float& gx, float& gy) {
    grid_coord<MODE>(GridSrc<MODE>(gsrc, n, h, w, Ho, Wo), h, w, Ho, Wo, th, gx, gy);
}

// the pixel position (integer values at pixel centres) a normalised coordinate samples — unnormalise, align_corners=False:
// ((g + 1) * size - 1) / 2
__device__ __forceinline__ void sample_position(float gx, float gy, int W, int H, float& ix, float& iy) {
    ix = ((gx + 1.f) * (float)W - 1.f) * 0.5f;
    iy = ((gy + 1.f) * (float)H - 1.f) * 0.5f;
}

// the top-left corner of the 2 x 2 patch a normalised coordinate samples bilinearly, and the fractional position inside it
struct Sample {
    int x0, y0;
    float tx, ty;  // ix - x0, iy - y0
};
__device__ __forceinline__ Sample locate(float gx, float gy, int W, int H) {
    float ix, iy;
    sample_position(gx, gy, W, H, ix, iy);
    const float fx = floorf(ix), fy = floorf(iy);
    Sample s;
    // clamp far-out-of-range coordinates before the int conversion (all four corners are OOB anyway)
    s.x0 = (int)fminf(fmaxf(fx, -2.f), (float)W + 1.f);
    s.y0 = (int)fminf(fmaxf(fy, -2.f), (float)H + 1.f);
    s.tx = ix - fx;
    s.ty = iy - fy;
    return s;
}

}  // namespace
