// The scale of a 64-bit FIXED-POINT scatter, for the gradients whose contributions land at data-dependent texels any distance away
// (integrate.hip: nemar_svf_step_bwd's image path; compose.hip: nemar_compose_pred_bwd towards a UNet `first`).  Integer addition is
// associative, so 64-bit integer atomics give the same bits whatever the arrival order; what the integers mean is fixed per call, on the
// device, from the largest |gout|:
//   svf_max_kernel   per-workgroup max |gout| (bit patterns) into the workspace's partial words: no host read;
//   svf_exponent     e with max |gout| < 2^e from those words, in every thread of a 256-thread workgroup;
//   svf_pow2         2^e as a float: contributions are scaled by 2^(fix - e) on the way in and 2^(e - fix) on the way out, exactly;
//   svf_fix_bits     fix = 40 bits below the largest gradient while the plane has fewer than 2^22 pixels, 62 - ceil(log2(H W)) beyond: even
//                    if every pixel of a plane lands on one texel the 64-bit sum cannot overflow.
// One statement of the rule, so that the two users cannot drift apart.
#pragma once
#include "common.h"

namespace {

constexpr int SVF_FIX_BITS = 40;
constexpr int SVF_MAX_PARTIALS = 256;      // workgroups of svf_max_kernel = partial words in the workspace (one per thread of a consumer)

// max over the call of the bit patterns of |gout| (a NaN counts as larger than every float: the scale then is the smallest one)
__global__ __launch_bounds__(256) void svf_max_kernel(const float* __restrict__ gout, long long total, unsigned* __restrict__ partial) {
    __shared__ unsigned red[4];
    unsigned m = 0u;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256)
        m = max(m, __float_as_uint(gout[i]) & 0x7fffffffu);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = max(max(red[0], red[1]), max(red[2], red[3]));
}

// e with max |gout| < 2^e, from the partial words, in every thread of a 256-thread workgroup (clamped: 2^(fix - e) must be a float)
__device__ __forceinline__ int svf_exponent(const unsigned* __restrict__ partial, int partials, unsigned* red) {
    unsigned m = (int)threadIdx.x < partials ? partial[threadIdx.x] : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = max(max(red[0], red[1]), max(red[2], red[3]));
    return max((int)((m >> 23) & 255u) - 126, -80);
}
__device__ __forceinline__ float svf_pow2(int e) { return __uint_as_float((unsigned)(127 + e) << 23); }      // -126 <= e <= 127

// the partial words a call over N x 2 x H x W gradient values fills
inline int svf_partials(int N, int H, int W) {
    const long long blocks = nemar_cdiv((long long)N * 2 * H * W, 1024);
    return (int)(blocks < SVF_MAX_PARTIALS ? blocks : SVF_MAX_PARTIALS);
}
// fixed-point bits below 2^e: H W contributions of less than 2^(fix + 1) each stay below 2^63
inline int svf_fix_bits(int H, int W) {
    int lg = 0;
    while ((1ll << lg) < (long long)H * W) ++lg;
    return 62 - lg < SVF_FIX_BITS ? 62 - lg : SVF_FIX_BITS;
}

}  // namespace
