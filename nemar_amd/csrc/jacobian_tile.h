// The forward-difference Jacobian determinant of a prediction's transformation, for every kernel that must compute THOSE bits:
// regularity.hip (nemar_jacobian_stats: the map and its statistics) and fold.hip (nemar_fold_penalty_fwd / _bwd: the hinge on the same
// determinant, and its gradient) — one statement of the arithmetic on top of resampled_grid.h, so that the fold count a user reads and
// the fold penalty a user trains against cannot drift apart.
#pragma once
#include "resampled_grid.h"

namespace {

constexpr int JT_W = RT_W + 1, JT_H = RT_H + 1;      // the 64 x 16 tile with the halo column and row of its forward neighbours

// det = a.x * b.y - b.x * a.y with a = p(h, w+1) - p(h, w) and b = p(h+1, w) - p(h, w): (ix, iy) the pixel's own position, (rx, ry)
// its right neighbour's, (dx, dy) the lower one's — registration_error_kernel's expression, in its order
__device__ __forceinline__ float jac_det(float ix, float iy, float rx, float ry, float dx, float dy) {
    return (rx - ix) * (dy - iy) - (dx - ix) * (ry - iy);
}

// p(h, w) of a UNet offset field fN [2,H,W] taken at its own size: the position in pixels that grid_coord<GRID_UNET> + sample_position
// give the pixel — the call jacobian_kernel<GRID_UNET, false> makes
__device__ __forceinline__ void unet_position(const float* __restrict__ fN, size_t plane, int h, int w, int H, int W, float& px, float& py) {
    float gx, gy;
    pred_view<GRID_UNET, false>(fN, 0, H, W, H, W, 1.f, 1.f).coord_unstaged(h, w, gx, gy);
    sample_position(gx, gy, W, H, px, py);
}

}  // namespace
