// Bilinear resize, align_corners=False: the source index / weight pair of one axis and the order of the four-tap sum.  Shared by
// pointwise.hip (nemar_bilinear_fwd/bwd, which materialise the resized tensor) and register.hip (nemar_warp_resampled_fwd, which
// interpolates a coarse offset field in registers) — one statement of the arithmetic, so that the fused warp equals the composed
// resize + warp bit for bit.
#pragma once
#include "common.h"

namespace {

struct Tap1D { int i0, i1; float l0, l1; };
// the pair of a source coordinate s >= 0: i0 = floor(s); i1 = min(i0 + 1, in - 1)
__device__ __forceinline__ Tap1D tap1d_from(float s, int n_in) {
    Tap1D t;
    t.i0 = min((int)s, n_in - 1);
    t.i1 = min(t.i0 + 1, n_in - 1);
    t.l1 = s - (float)t.i0;
    t.l0 = 1.f - t.l1;
    return t;
}
__device__ __forceinline__ Tap1D tap1d(int d, int n_in, float scale) {
    // s = max((d + 0.5) * in/out - 0.5, 0)
    float s = ((float)d + 0.5f) * scale - 0.5f;
    s = s < 0.f ? 0.f : s;
    return tap1d_from(s, n_in);
}
// the same pair at a CONTINUOUS output coordinate d (score.hip, nemar_map_points: annotated points lie between pixels and may lie beyond
// the border): the source coordinate clamped to [0, in - 1] on both sides, so that a point outside the image takes the border texel
__device__ __forceinline__ Tap1D tap1d_at(float d, int n_in, float scale) {
    const float s = (d + 0.5f) * scale - 0.5f;
    return tap1d_from(fminf(fmaxf(s, 0.f), (float)(n_in - 1)), n_in);
}

// the four taps (row i0: a, b; row i1: c, d) blended: rows first, then the two rows
__device__ __forceinline__ float resize_blend(float a, float b, float c, float d, const Tap1D& tw, const Tap1D& th) {
    const float top = a * tw.l0 + b * tw.l1;
    const float bot = c * tw.l0 + d * tw.l1;
    return top * th.l0 + bot * th.l1;
}

}  // namespace
