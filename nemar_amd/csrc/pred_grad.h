// What the losses on a prediction at its own size share (epe.hip: the EPE loss; dice.hip: the soft-Dice loss): how a lane loads its run
// of UNet offsets, the fixed-order merge of the per-workgroup records of an affine gradient, and what both refuse.
#pragma once
#include "clamped_bilerp.h"
#include "common.h"
#include "warp_grid.h"

namespace {

constexpr int EPE_WORDS = 6;        // an affine backward record: the six sums of one workgroup

// the grid_src values of the VEC pixels at offset o of sample plane pair dN (UNET: the offsets, by 16-byte loads when WIDE; AFFINE: none,
// theta alone)
template <int MODE, int VEC, bool WIDE>
__device__ __forceinline__ void load_run(const float* __restrict__ dN, size_t plane, size_t o, float* ax, float* ay) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) { ax[v] = 0.f; ay[v] = 0.f; }
    if (MODE != GRID_UNET) return;
    if (VEC == 4 && WIDE) {
        const float4 a = *reinterpret_cast<const float4*>(dN + o), c = *reinterpret_cast<const float4*>(dN + plane + o);
        ax[0] = a.x; ax[1] = a.y; ax[2] = a.z; ax[3] = a.w;
        ay[0] = c.x; ay[1] = c.y; ay[2] = c.z; ay[3] = c.w;
    } else {
#pragma unroll
        for (int v = 0; v < VEC; ++v) { ax[v] = dN[o + v]; ay[v] = dN[plane + o + v]; }
    }
}

// gpred[n, c] (+)= k * (the sample's records: thread t takes records t, t + 256, ... in ascending order, then the fixed workgroup tree)
__global__ __launch_bounds__(256) void epe_bwd_affine_merge_kernel(const float* __restrict__ partial, int n_partial,
                                                                   const float* __restrict__ gscale, float scale, float* __restrict__ gpred,
                                                                   int accumulate) {
    __shared__ float red[16];
    const int n = blockIdx.x;
    const float* p = partial + (size_t)n * n_partial * EPE_WORDS;
    const float k = gscale[0] * scale;
#pragma unroll
    for (int c = 0; c < EPE_WORDS; ++c) {
        float acc = 0.f;
        for (int i = threadIdx.x; i < n_partial; i += 256) acc += p[(size_t)i * EPE_WORDS + c];
        const float t = block_sum(acc, red);
        if (threadIdx.x == 0) gpred[n * 6 + c] = (accumulate ? gpred[n * 6 + c] : 0.f) + k * t;
    }
}

inline bool aligned4(const void* a, const void* b, const void* c, const void* d, const void* e = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e) & 3) == 0;
}

inline bool epe_shape_ok(int N, int H, int W) { return N > 0 && H > 0 && W > 0 && N <= 65535 && (long long)H * W < (1ll << 31); }

}  // namespace
