// Reading a ground-truth field at the position the warp samples: the bilinear read with the position clamped into the image, and the
// warp's sampling position from grid_src values held in registers.  Shared by deform.hip (the deforming sampler and the
// registration-error meter) and epe.hip (the loss that trains against the meter's residual) — one statement of the arithmetic, so the
// number that is watched and the number that is trained against cannot drift apart.
#pragma once
#include "common.h"
#include "warp_grid.h"

namespace {

struct Corner {
    int xa, xb, ya, yb;      // the two columns / rows, inside [0, W-1] / [0, H-1]
    float tx, ty;
};
// position (px, py) clamped into [0, W-1] x [0, H-1] (fmaxf / fminf drop a NaN: the address stays inside whatever the field holds)
__device__ __forceinline__ Corner clamp_locate(float px, float py, int W, int H) {
    const float cx = fminf(fmaxf(px, 0.f), (float)(W - 1)), cy = fminf(fmaxf(py, 0.f), (float)(H - 1));
    const float fx = floorf(cx), fy = floorf(cy);
    Corner k;
    k.xa = (int)fx; k.ya = (int)fy;
    k.xb = min(k.xa + 1, W - 1); k.yb = min(k.ya + 1, H - 1);
    k.tx = cx - fx; k.ty = cy - fy;
    return k;
}
__device__ __forceinline__ float bilerp(float a, float b, float c, float d, float tx, float ty) {
    const float ex = 1.f - tx, ey = 1.f - ty;
    return a * (ex * ey) + b * (tx * ey) + c * (ex * ty) + d * (tx * ty);
}

// x -> S(x): the pixel position the warp kernel samples for grid_src values (sx, sy) held in registers, at output pixel (h, w)
// (RegSrc: warp_grid.h)
template <int MODE>
__device__ __forceinline__ void warp_position(float sx, float sy, int h, int w, int H, int W, const float* th, float& ix, float& iy) {
    float gx, gy;
    grid_coord<MODE>(RegSrc{sx, sy}, h, w, H, W, th, gx, gy);
    sample_position(gx, gy, W, H, ix, iy);
}

// The launch shape of the streaming kernels that read such a field — workgroups of 256 per sample: enough to cover the sample one item
// per lane, at most 256 CUs x 8 over the batch (the kernels grid-stride the rest)
inline int reg_blocks(int N, long long items) {
    int gx = nemar_cdiv(items, 256);
    const int cap = nemar_cdiv(256 * 8, N);
    if (gx > cap) gx = cap;
    return gx < 1 ? 1 : gx;
}

inline bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

}  // namespace
