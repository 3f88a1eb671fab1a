// BatchNorm2d(C, affine=True, track_running_stats=True), forward (training / eval) and backward, with the following ReLU /
// LeakyReLU, Dropout and the ResnetBlock residual add fused in.
//
// Replaces nn.BatchNorm2d at reference models/networks.py:22 (norm_layer of ResnetGenerator :351,358,373, ResnetBlock :426,439,
// UnetSkipConnectionBlock :517,519, NLayerDiscriminator :584,592, PixelDiscriminator :626) with `--norm batch`.
//   train fwd:  mean, var = biased statistics over (N, H, W) of a SEGMENT of the batch;  scale = gamma * rstd
//               y = [residual +] dropout(act((x - mean) * scale + beta));  running = (1 - momentum) running + momentum (mean | unbiased var)
//   eval fwd:   the same with the running statistics (left untouched)
//   bwd:        z = (x - mean) * scale + beta (recomputed; NOT x * scale + (beta - mean * scale): three roundings the size of mean * scale), g = gy [* mask / (1 - p)] * act'(z), xhat = (x - mean) * rstd
//               dgamma += sum g xhat, dbeta += sum g;  gx = gamma rstd (g - sum g / M - xhat sum(g xhat) / M)   (eval: gx = gamma rstd g)
//
// Segments: the N samples form S equal segments (the model's batched passes: T over [a ; R(a)], D over [real ; fakes]); statistics,
// running-stat updates and the backward sums are per (segment, channel), the updates applied in segment order — what S separate calls
// of the reference's layer compute.
//
// HBM-bound.  A PIECE is up to 1024 contiguous elements of one (n, c) plane, one wave per piece (16 values per lane in registers, 16-byte
// accesses where H*W % 4 == 0); four pieces per 256-thread workgroup.  A piece never spans planes, so on small maps most lanes of a wave
// idle: a 2x2 plane keeps 1 lane of 64 busy, an 8x8 plane 16 (the U-Net's inner levels, D's last layers).  Those layers are a few KB
// to a few hundred KB; a mapping that packs several planes into one wave is left for when their time shows in a profile.
// Training forward and backward are three launches each, the eval forward one (the apply pass):
//   1. partials per piece (forward: mean and M2 by the exact two-pass form in registers; backward: sum g, sum g xhat);
//   2. one workgroup per channel merges its pieces per segment in a FIXED order (mean = sum cnt_i mean_i / M, then
//      M2 = sum M2_i + cnt_i (mean_i - mean)^2: the exact parallel-variance combination) and writes the saved statistics, the running
//      statistics and the counter (forward) or the gradient sums and dgamma / dbeta (backward);
//   3. apply: every element once more.
// No floating-point atomics anywhere: every reduction has a fixed order, results are bitwise reproducible.
#include "common.h"
#include "max_words.h"

extern const unsigned* g_dropout_base;          // pointwise.hip (nemar_set_dropout_base)

namespace {

constexpr int ACT_NONE = 0, ACT_RELU = 1, ACT_LRELU = 2;
constexpr int PIECE = 1024;              // elements per piece = 64 lanes x 16
constexpr int WAVES = 4;                 // pieces per workgroup

typedef float f32x4b __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bn_act(float v, int act, float slope) {
    if (act == ACT_RELU) return fmaxf(v, 0.f);
    if (act == ACT_LRELU) return v > 0.f ? v : v * slope;
    return v;
}
__device__ __forceinline__ float bn_act_d(float z, int act, float slope) {
    if (act == ACT_RELU) return z > 0.f ? 1.f : 0.f;
    if (act == ACT_LRELU) return z > 0.f ? 1.f : slope;
    return 1.f;
}

// Philox4x32-10 exactly as pointwise.hip's dropout_kernel draws it (counter = float4 index over the [N,C,H,W] tensor)
__device__ __forceinline__ void bn_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned* out) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

struct BnDrop {
    int on;
    unsigned thresh;       // keep when the random word >= thresh (pointwise.hip's rule)
    float scale;           // 1 / (1 - p)
    unsigned seed_lo, seed_hi, offset;
    const unsigned* obase;
};

// keep factor of the four elements of global float4 index q
__device__ __forceinline__ void bn_mask4(const BnDrop& d, unsigned off, long long q, float* m) {
    unsigned r[4];
    bn_philox((unsigned)q, (unsigned)(q >> 32), off, 0u, d.seed_lo, d.seed_hi, r);
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = r[j] >= d.thresh ? 1.f : 0.f;
}

// The 16 values of a lane: element e = k * 256 + lane * 4 + j of the piece (k, j < 4).  VEC: one 16-byte access per k (the piece length
// is then a multiple of 4); otherwise four guarded scalar accesses.  Lanes past the piece's end read nothing and hold zeros.
template <bool VEC>
__device__ __forceinline__ void bn_load(const float* __restrict__ p, int len, int lane, float (&v)[4][4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int e0 = k * 256 + lane * 4;
        if (VEC) {
            if (e0 < len) {
                const f32x4b t = *reinterpret_cast<const f32x4b*>(p + e0);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[k][j] = t[j];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[k][j] = 0.f;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[k][j] = e0 + j < len ? p[e0 + j] : 0.f;
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void bn_store(float* __restrict__ p, int len, int lane, const float (&v)[4][4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int e0 = k * 256 + lane * 4;
        if (VEC) {
            if (e0 < len) *reinterpret_cast<f32x4b*>(p + e0) = f32x4b{v[k][0], v[k][1], v[k][2], v[k][3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e0 + j < len) p[e0 + j] = v[k][j];
        }
    }
}

// the dropout keep factors (1 / 0) of the lane's 16 elements; `gbase` = global element index of the piece's first element
template <bool VEC>
__device__ __forceinline__ void bn_masks(const BnDrop& d, long long gbase, int len, int lane, float (&m)[4][4]) {
    const unsigned off = d.offset + (d.obase ? *d.obase : 0u);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int e0 = k * 256 + lane * 4;
        if (VEC) {
            // (gbase and e0 are multiples of 4: one counter per float4, as nemar_dropout)
            if (e0 < len) bn_mask4(d, off, (gbase + e0) >> 2, m[k]);
            else m[k][0] = m[k][1] = m[k][2] = m[k][3] = 0.f;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (e0 + j < len) {
                    const long long i = gbase + e0 + j;
                    float t[4];
                    bn_mask4(d, off, i >> 2, t);
                    m[k][j] = t[i & 3];
                } else {
                    m[k][j] = 0.f;
                }
            }
        }
    }
}

struct BnShape {
    int N, C, HW, S, P;          // P = pieces per plane
};

__device__ __forceinline__ int piece_len(const BnShape& sh, int p) { return min(PIECE, sh.HW - p * PIECE); }

// (mean, rstd) of (segment s, channel c): the saved statistics [2, S, C] of a training pass, or the running statistics (var -> rstd)
__device__ __forceinline__ void bn_stats(const float* mean_src, const float* var_src, int from_var, float eps, int S, int C, int s, int c,
                                         float& mean, float& rstd) {
    if (from_var) {
        mean = mean_src[c];
        rstd = 1.f / sqrtf(var_src[c] + eps);
    } else {
        mean = mean_src[s * C + c];
        rstd = mean_src[S * C + s * C + c];
    }
}

// ---- forward launch 1: (mean, M2) of every piece ---------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void bn_fwd_partials_kernel(const float* __restrict__ x, float* __restrict__ part, BnShape sh) {
    const int lane = threadIdx.x & 63;
    const long long piece = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    const long long pieces = (long long)sh.N * sh.C * sh.P;
    if (piece >= pieces) return;                     // (whole waves; wave collectives only below)
    const long long plane = piece / sh.P;
    const int p = (int)(piece - plane * sh.P);
    const int len = piece_len(sh, p);
    float v[4][4];
    bn_load<VEC>(x + plane * sh.HW + (long long)p * PIECE, len, lane, v);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) s += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
    const float m0 = wave_sum(s) / (float)len;
    float q = 0.f, e = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float d = k * 256 + lane * 4 + j < len ? v[k][j] - m0 : 0.f;
            e += d;
            q += d * d;
        }
    }
    // (the sum of the deviations takes the rounding of m0 — an ulp of a mean far from zero — out of the mean and of M2)
    const float c = wave_sum(e) / (float)len;
    q = fmaxf(wave_sum(q) - (float)len * (c * c), 0.f);
    if (lane == 0) {
        part[2 * piece] = m0 + c;
        part[2 * piece + 1] = q;
    }
}

// ---- forward launch 2: one workgroup per channel, the S segments in order --------------------------------------------------------
__global__ __launch_bounds__(256) void bn_fwd_merge_kernel(const float* __restrict__ part, float* __restrict__ saved,
                                                           float* __restrict__ running_mean, float* __restrict__ running_var,
                                                           long long* __restrict__ counter, BnShape sh, float eps, float momentum) {
    __shared__ float red[16];
    const int c = blockIdx.x;
    const int Ns = sh.N / sh.S;
    const int items = Ns * sh.P;
    const float M = (float)Ns * (float)sh.HW;
    for (int s = 0; s < sh.S; ++s) {
        float a = 0.f;
        for (int i = threadIdx.x; i < items; i += 256) {
            const int n = s * Ns + i / sh.P, p = i % sh.P;
            const long long piece = ((long long)n * sh.C + c) * sh.P + p;
            a += (float)piece_len(sh, p) * part[2 * piece];
        }
        const float m0 = block_sum(a, red) / M;
        // (... and once more as deviations from m0: what is left of the error is an ulp of the pieces' spread, not of their size)
        float e = 0.f;
        for (int i = threadIdx.x; i < items; i += 256) {
            const int n = s * Ns + i / sh.P, p = i % sh.P;
            const long long piece = ((long long)n * sh.C + c) * sh.P + p;
            e += (float)piece_len(sh, p) * (part[2 * piece] - m0);
        }
        const float mean = m0 + block_sum(e, red) / M;
        float b = 0.f;
        for (int i = threadIdx.x; i < items; i += 256) {
            const int n = s * Ns + i / sh.P, p = i % sh.P;
            const long long piece = ((long long)n * sh.C + c) * sh.P + p;
            const float d = part[2 * piece] - mean;
            b += part[2 * piece + 1] + (float)piece_len(sh, p) * (d * d);
        }
        const float m2 = block_sum(b, red);
        if (threadIdx.x == 0) {
            const float var = m2 / M;
            saved[s * sh.C + c] = mean;
            saved[sh.S * sh.C + s * sh.C + c] = 1.f / sqrtf(var + eps);
            if (running_mean) {
                // (PyTorch's order: running * (1 - momentum) + momentum * statistic; the unbiased variance M2 / (M - 1))
                running_mean[c] = running_mean[c] * (1.f - momentum) + momentum * mean;
                running_var[c] = running_var[c] * (1.f - momentum) + momentum * (m2 / (M - 1.f));
            }
        }
    }
    if (counter && c == 0 && threadIdx.x == 0) counter[0] = counter[0] + (long long)sh.S;
}

// per-workgroup maximum -> its partial word of sample blockIdx.y (max_words.h layout; a finalize launch follows)
__device__ __forceinline__ void bn_publish_max(unsigned m, unsigned* maxw, unsigned* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = max(max(red[0], red[1]), max(red[2], red[3]));
        maxw[gridDim.y + (size_t)blockIdx.y * gridDim.x + blockIdx.x] = m;
    }
}

__device__ __forceinline__ unsigned bn_finite_mag(float v) {
    const unsigned u = __builtin_bit_cast(unsigned, v) & 0x7fffffffu;
    return u < 0x7f800000u ? u : 0u;
}

// ---- forward launch 3 (training and eval): y = [residual +] dropout(act((x - mean) * scale + beta)) -------------------------------------
// grid (ceil(C * P / 4), N): the four waves of a workgroup take four consecutive pieces of sample blockIdx.y
template <bool VEC>
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ residual, float* __restrict__ y,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ mean_src, const float* __restrict__ var_src, int from_var,
                                                       float* __restrict__ saved_out, BnShape sh, float eps, int act, float slope,
                                                       BnDrop drop, unsigned* maxw) {
    __shared__ unsigned red[4];
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.y;
    const int lp = blockIdx.x * WAVES + (threadIdx.x >> 6);
    unsigned omax = 0;
    if (lp < sh.C * sh.P) {
        const int c = lp / sh.P, p = lp - c * sh.P;
        const int s = n / (sh.N / sh.S);
        float mean, rstd;
        bn_stats(mean_src, var_src, from_var, eps, sh.S, sh.C, s, c, mean, rstd);
        const float scale = gamma[c] * rstd;
        const float shift = beta[c];
        if (saved_out && n == 0 && p == 0 && lane == 0) {      // (eval: the statistics the backward pass uses)
            saved_out[c] = mean;
            saved_out[sh.C + c] = rstd;
        }
        const int len = piece_len(sh, p);
        const long long gbase = ((long long)n * sh.C + c) * sh.HW + (long long)p * PIECE;
        float v[4][4];
        bn_load<VEC>(x + gbase, len, lane, v);
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[k][j] = bn_act((v[k][j] - mean) * scale + shift, act, slope);
        if (drop.on) {
            float m[4][4];
            bn_masks<VEC>(drop, gbase, len, lane, m);
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (k * 256 + lane * 4 + j < len) v[k][j] = m[k][j] != 0.f ? v[k][j] * drop.scale : 0.f;
        }
        if (residual) {
            float r[4][4];
            bn_load<VEC>(residual + gbase, len, lane, r);
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) v[k][j] += r[k][j];
        }
        bn_store<VEC>(y + gbase, len, lane, v);
        if (maxw) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (k * 256 + lane * 4 + j < len) omax = max(omax, bn_finite_mag(v[k][j]));
        }
    }
    if (maxw) bn_publish_max(omax, maxw, red);
}

// g = gy [* mask / (1 - p)] * act'((x - mean) * scale + beta) and xhat of the lane's 16 elements (zeros past the piece's end)
template <bool VEC>
__device__ __forceinline__ void bn_bwd_load(const float* __restrict__ x, const float* __restrict__ gy, long long gbase, int len, int lane,
                                            float mean, float rstd, float scale, float shift, int act, float slope, const BnDrop& drop,
                                            float (&g)[4][4], float (&xh)[4][4]) {
    bn_load<VEC>(x + gbase, len, lane, xh);
    bn_load<VEC>(gy + gbase, len, lane, g);
    float m[4][4];
    if (drop.on) bn_masks<VEC>(drop, gbase, len, lane, m);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool on = k * 256 + lane * 4 + j < len;
            const float xv = xh[k][j];
            float t = g[k][j];
            if (drop.on) t = m[k][j] != 0.f ? t * drop.scale : 0.f;
            t = t * bn_act_d((xv - mean) * scale + shift, act, slope);
            g[k][j] = on ? t : 0.f;
            xh[k][j] = on ? (xv - mean) * rstd : 0.f;
        }
    }
}

// ---- backward launch 1: (sum g, sum g xhat) of every piece ---------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void bn_bwd_partials_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              const float* __restrict__ stats, float* __restrict__ part, BnShape sh,
                                                              int act, float slope, BnDrop drop) {
    const int lane = threadIdx.x & 63;
    const long long piece = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    const long long pieces = (long long)sh.N * sh.C * sh.P;
    if (piece >= pieces) return;
    const long long plane = piece / sh.P;
    const int p = (int)(piece - plane * sh.P);
    const int n = (int)(plane / sh.C), c = (int)(plane - (long long)n * sh.C);
    const int s = n / (sh.N / sh.S);
    float mean, rstd;
    bn_stats(stats, nullptr, 0, 0.f, sh.S, sh.C, s, c, mean, rstd);
    const float scale = gamma[c] * rstd;
    const float shift = beta[c];
    const int len = piece_len(sh, p);
    float g[4][4], xh[4][4];
    bn_bwd_load<VEC>(x, gy, plane * sh.HW + (long long)p * PIECE, len, lane, mean, rstd, scale, shift, act, slope, drop, g, xh);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s1 += g[k][j];
            s2 += g[k][j] * xh[k][j];
        }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) {
        part[2 * piece] = s1;
        part[2 * piece + 1] = s2;
    }
}

// ---- backward launch 2: one workgroup per channel: per-segment sums (-> sums[S, C, 2]) and dgamma / dbeta accumulated -----------------
__global__ __launch_bounds__(256) void bn_bwd_merge_kernel(const float* __restrict__ part, float* __restrict__ sums, float* __restrict__ gw,
                                                           float* __restrict__ gb, BnShape sh) {
    __shared__ float red[16];
    const int c = blockIdx.x;
    const int Ns = sh.N / sh.S;
    const int items = Ns * sh.P;
    float tw = 0.f, tb = 0.f;
    for (int s = 0; s < sh.S; ++s) {
        float a = 0.f, b = 0.f;
        for (int i = threadIdx.x; i < items; i += 256) {
            const int n = s * Ns + i / sh.P, p = i % sh.P;
            const long long piece = ((long long)n * sh.C + c) * sh.P + p;
            a += part[2 * piece];
            b += part[2 * piece + 1];
        }
        a = block_sum(a, red);
        b = block_sum(b, red);
        tb += a;
        tw += b;
        if (threadIdx.x == 0) {
            sums[2 * (s * sh.C + c)] = a;
            sums[2 * (s * sh.C + c) + 1] = b;
        }
    }
    if (threadIdx.x == 0) {
        if (gw) gw[c] = gw[c] + tw;
        if (gb) gb[c] = gb[c] + tb;
    }
}

// ---- backward launch 3: gx ---------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ gx,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const float* __restrict__ stats, const float* __restrict__ sums, int training,
                                                           BnShape sh, int act, float slope, BnDrop drop) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.y;
    const int lp = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (lp >= sh.C * sh.P) return;
    const int c = lp / sh.P, p = lp - c * sh.P;
    const int s = n / (sh.N / sh.S);
    float mean, rstd;
    bn_stats(stats, nullptr, 0, 0.f, sh.S, sh.C, s, c, mean, rstd);
    const float scale = gamma[c] * rstd;
    const float shift = beta[c];
    const float M = (float)(sh.N / sh.S) * (float)sh.HW;
    const float m1 = training ? sums[2 * (s * sh.C + c)] / M : 0.f;
    const float m2 = training ? sums[2 * (s * sh.C + c) + 1] / M : 0.f;
    const int len = piece_len(sh, p);
    const long long gbase = ((long long)n * sh.C + c) * sh.HW + (long long)p * PIECE;
    float g[4][4], xh[4][4];
    bn_bwd_load<VEC>(x, gy, gbase, len, lane, mean, rstd, scale, shift, act, slope, drop, g, xh);
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) g[k][j] = scale * (g[k][j] - m1 - xh[k][j] * m2);
    bn_store<VEC>(gx + gbase, len, lane, g);
}

BnDrop make_drop(float p, unsigned long long seed, unsigned offset) {
    BnDrop d;
    d.on = p > 0.f ? 1 : 0;
    const double t = (double)p * 4294967296.0;
    d.thresh = t >= 4294967295.0 ? 4294967295u : (unsigned)t;
    d.scale = p > 0.f ? 1.f / (1.f - p) : 1.f;
    d.seed_lo = (unsigned)(seed & 0xffffffffu);
    d.seed_hi = (unsigned)(seed >> 32);
    d.offset = offset;
    d.obase = g_dropout_base;
    return d;
}

BnShape make_shape(int N, int C, int HW, int S) {
    BnShape sh;
    sh.N = N; sh.C = C; sh.HW = HW; sh.S = S;
    sh.P = (HW + PIECE - 1) / PIECE;
    return sh;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

size_t partial_floats(const BnShape& sh) { return (size_t)sh.N * sh.C * sh.P * 2; }

int check_common(const float* x, const float* y, const float* gamma, const float* beta, int N, int C, int HW, int S, int act, float p,
                 const char* what) {
    NEMAR_REQUIRE(x && y && gamma && beta, "%s: null pointer", what);
    NEMAR_REQUIRE(N > 0 && C > 0 && HW > 0 && N <= 65535, "%s: bad shape N=%d C=%d HW=%d", what, N, C, HW);
    NEMAR_REQUIRE(S >= 1 && N % S == 0, "%s: %d segments do not divide the batch of %d", what, S, N);
    NEMAR_REQUIRE(act == ACT_NONE || act == ACT_RELU || act == ACT_LRELU, "%s: unsupported act %d", what, act);
    NEMAR_REQUIRE(p >= 0.f && p < 1.f, "%s: bad dropout p", what);
    return NEMAR_OK;
}

int launch_apply(const float* x, const float* residual, float* y, const float* gamma, const float* beta, const float* mean_src,
                 const float* var_src, int from_var, float* saved_out, const BnShape& sh, float eps, int act, float slope, const BnDrop& drop,
                 void* max_words, hipStream_t st) {
    const int gx = nemar_cdiv((long long)sh.C * sh.P, WAVES);
    unsigned* maxw = (unsigned*)max_words;
    NEMAR_REQUIRE(!maxw || gx <= NEMAR_MAX_PARTIALS, "batchnorm: %d workgroups per sample exceed the max-word partials", gx);
    const bool vec = sh.HW % 4 == 0 && aligned16(x) && aligned16(y) && aligned16(residual);
    dim3 grid(gx, sh.N);
    if (vec)
        hipLaunchKernelGGL((bn_apply_kernel<true>), grid, dim3(256), 0, st, x, residual, y, gamma, beta, mean_src, var_src, from_var, saved_out,
                           sh, eps, act, slope, drop, maxw);
    else
        hipLaunchKernelGGL((bn_apply_kernel<false>), grid, dim3(256), 0, st, x, residual, y, gamma, beta, mean_src, var_src, from_var, saved_out,
                           sh, eps, act, slope, drop, maxw);
    if (maxw) max_words_finalize(maxw, sh.N, gx, st);
    return NEMAR_OK;
}

}  // namespace

NEMAR_API size_t nemar_batchnorm_workspace(int N, int C, int HW, int segments) {
    if (N <= 0 || C <= 0 || HW <= 0 || segments <= 0) return 0;
    const BnShape sh = make_shape(N, C, HW, segments);
    return (partial_floats(sh) + (size_t)segments * C * 2) * sizeof(float);
}

NEMAR_API int nemar_batchnorm_fwd_train(const float* x, const float* residual, float* y, const float* weight, const float* bias,
                                        float* running_mean, float* running_var, long long* num_batches_tracked, float* saved,
                                        int N, int C, int HW, int segments, float eps, float momentum, int act, float slope,
                                        float dropout_p, unsigned long long seed, unsigned offset, void* max_words,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    const int rc = check_common(x, y, weight, bias, N, C, HW, segments, act, dropout_p, "batchnorm_fwd_train");
    if (rc != NEMAR_OK) return rc;
    NEMAR_REQUIRE(saved, "batchnorm_fwd_train: null saved statistics");
    NEMAR_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "batchnorm_fwd_train: running_mean and running_var go together");
    NEMAR_REQUIRE((long long)(N / segments) * HW > 1, "batchnorm_fwd_train: expected more than 1 value per channel when training");
    const BnShape sh = make_shape(N, C, HW, segments);
    NEMAR_REQUIRE(workspace && workspace_bytes >= nemar_batchnorm_workspace(N, C, HW, segments), "batchnorm_fwd_train: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)workspace;
    const long long pieces = (long long)N * C * sh.P;
    const dim3 pgrid(nemar_cdiv(pieces, WAVES));
    if (HW % 4 == 0 && aligned16(x))
        hipLaunchKernelGGL((bn_fwd_partials_kernel<true>), pgrid, dim3(256), 0, st, x, part, sh);
    else
        hipLaunchKernelGGL((bn_fwd_partials_kernel<false>), pgrid, dim3(256), 0, st, x, part, sh);
    hipLaunchKernelGGL(bn_fwd_merge_kernel, dim3(C), dim3(256), 0, st, part, saved, running_mean, running_var, num_batches_tracked, sh, eps,
                       momentum);
    const int rc2 = launch_apply(x, residual, y, weight, bias, saved, nullptr, 0, nullptr, sh, eps, act, slope,
                                 make_drop(dropout_p, seed, offset), max_words, st);
    if (rc2 != NEMAR_OK) return rc2;
    NEMAR_CHECK_LAUNCH("batchnorm_fwd_train");
    return NEMAR_OK;
}

NEMAR_API int nemar_batchnorm_fwd_eval(const float* x, const float* residual, float* y, const float* weight, const float* bias,
                                       const float* running_mean, const float* running_var, float* saved, int N, int C, int HW, float eps,
                                       int act, float slope, float dropout_p, unsigned long long seed, unsigned offset, void* max_words,
                                       void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    const int rc = check_common(x, y, weight, bias, N, C, HW, 1, act, dropout_p, "batchnorm_fwd_eval");
    if (rc != NEMAR_OK) return rc;
    NEMAR_REQUIRE(running_mean && running_var, "batchnorm_fwd_eval: null running statistics");
    const BnShape sh = make_shape(N, C, HW, 1);
    const int rc2 = launch_apply(x, residual, y, weight, bias, running_mean, running_var, 1, saved, sh, eps, act, slope,
                                 make_drop(dropout_p, seed, offset), max_words, (hipStream_t)stream);
    if (rc2 != NEMAR_OK) return rc2;
    NEMAR_CHECK_LAUNCH("batchnorm_fwd_eval");
    return NEMAR_OK;
}

NEMAR_API int nemar_batchnorm_bwd(const float* x, const float* gy, float* gx, const float* weight, const float* bias, const float* saved,
                                  float* grad_weight, float* grad_bias, int N, int C, int HW, int segments, int training, int act,
                                  float slope, float dropout_p, unsigned long long seed, unsigned offset, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    const int rc = check_common(x, gy, weight, bias, N, C, HW, segments, act, dropout_p, "batchnorm_bwd");
    if (rc != NEMAR_OK) return rc;
    NEMAR_REQUIRE(saved, "batchnorm_bwd: null saved statistics");
    NEMAR_REQUIRE(training || segments == 1, "batchnorm_bwd: eval-mode statistics have one segment");
    const BnShape sh = make_shape(N, C, HW, segments);
    NEMAR_REQUIRE(workspace && workspace_bytes >= nemar_batchnorm_workspace(N, C, HW, segments), "batchnorm_bwd: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)workspace;
    float* sums = part + partial_floats(sh);
    const BnDrop drop = make_drop(dropout_p, seed, offset);
    const bool vec = HW % 4 == 0 && aligned16(x) && aligned16(gy) && aligned16(gx);
    const long long pieces = (long long)N * C * sh.P;
    const bool need_sums = training || grad_weight || grad_bias;
    if (need_sums) {
        const dim3 pgrid(nemar_cdiv(pieces, WAVES));
        if (vec)
            hipLaunchKernelGGL((bn_bwd_partials_kernel<true>), pgrid, dim3(256), 0, st, x, gy, weight, bias, saved, part, sh, act, slope, drop);
        else
            hipLaunchKernelGGL((bn_bwd_partials_kernel<false>), pgrid, dim3(256), 0, st, x, gy, weight, bias, saved, part, sh, act, slope, drop);
        hipLaunchKernelGGL(bn_bwd_merge_kernel, dim3(C), dim3(256), 0, st, part, sums, grad_weight, grad_bias, sh);
    }
    if (gx) {
        const dim3 grid(nemar_cdiv((long long)C * sh.P, WAVES), N);
        if (vec)
            hipLaunchKernelGGL((bn_bwd_apply_kernel<true>), grid, dim3(256), 0, st, x, gy, gx, weight, bias, saved, sums, training, sh, act,
                               slope, drop);
        else
            hipLaunchKernelGGL((bn_bwd_apply_kernel<false>), grid, dim3(256), 0, st, x, gy, gx, weight, bias, saved, sums, training, sh, act,
                               slope, drop);
    }
    NEMAR_CHECK_LAUNCH("batchnorm_bwd");
    return NEMAR_OK;
}
