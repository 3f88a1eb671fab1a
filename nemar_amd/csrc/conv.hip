// K1 + K2 + K4 + K8: the convolution operators — entry points, launches, and the kernels that live here.
//
// Replaces nn.Conv2d / nn.ConvTranspose2d (+ the ReflectionPad2d in front of them and the torch.cat that feeds them) at reference
// models/networks.py:349-377,418-439,576-597 and models/stn/layers.py:85, models/stn/unet_stn.py:80,97, models/stn/affine_stn.py:69-72,79 —
// forward, data gradient and weight gradient.  nn.Linear of the affine head is the 1x1 case on a 1x1 image.
//
// Each operator is: validate -> plan (conv_route.h: which kernel family serves the call, with which workspace layout; the table is DESIGN.md
// 4a) -> workspace check -> switch on the plan, where each case only fills parameters and launches.  The host-side size queries at the end of
// the file ask the same plans with the canonical call-time facts.  Kernels here: the first-generation weight gradient (wgrad_kernel: what
// conv_wgrad.hip does not take), the passes around the exact-fp32 reflect data gradient, bias gradients, and the 7x7 many -> few passes.
#define NEMAR_CONV_HIP
#include "common.h"
#include "conv_exact.h"
#include "conv_call.h"
#include "conv_route.h"
#include "pack_plan.h"

#ifdef NEMAR_AB
extern int g_split16_ring3;                      // conv_split16.hip
extern int g_split16_ksplit_cap;
extern int g_narrow_fwd4;                        // conv_narrow.hip
extern int g_wg_xreg;                            // conv_split16_wgrad.hip
extern int g_register_vec4;                      // register.hip
extern int g_overlap_per_lane;                   // score.hip
extern int g_histogram_per_lane;                 // similarity.hip
void nemar_norm_planes_debug(int bits);          // norm_planes.hip: ablation bits of the fused producer (measurement only)
#endif

// conv_narrow.hip: VALU + LDS-halo kernels for layers with <= 4 output channels
int nemar_narrow_fwd(const float* x, const float* w, const float* bias, float* y, int N, int C, int H, int W, int K, int R,
                     int pad, int border, int act, float slope, float* part, size_t part_floats, hipStream_t st);
int nemar_narrow_wgrad(const float* x, const float* gy, float* gw, int N, int C, int H, int W, int K, int R, int pad,
                       int border, float* part, hipStream_t st);
// conv_wgrad.hip: wave-specialised weight gradient for wide layers
void nemar_wgrad2_launch(const float* x0, int C0, const float* x1, int C1, const float* gy, float* gw, float* gb, int N,
                         int H, int W, int K, int OH, int OW, int R, int S, int stride, int pad, int pad_mode,
                         int target_blocks, bool vec_ok, int dbg, float* part, hipStream_t st);
// reduce.hip: dst (+)= sum of `splits` slabs in split order (the deterministic second stage of every split reduction)
void nemar_sum_partials_pair(const float* part_a, long long stride_a, int splits_a, float* dst_a, long long n_a,
                             const float* part_b, long long stride_b, int splits_b, float* dst_b, long long n_b, bool accumulate, hipStream_t st);
void nemar_sum_partials_fold(const float* part, long long stride, int splits, float* gx, long long planes, int H, int W, int pad,
                             const float* addend, hipStream_t st);
void nemar_sum_partials(const float* part, long long stride, int splits, float* dst, long long n, bool accumulate,
                        hipStream_t st);

namespace {

// which kernel family served the last conv call of this thread (nemar_last_route; tests and tools): conv_route.h ROUTE_*
static thread_local int g_last_route = 0;
static thread_local int g_last_gy_planes = 0;     // did the last nemar_conv2d_bwd_data_ex call of this thread fill gy_planes_out? (nemar_last_gy_planes)
static NEMAR_SWITCH(int, g_config_epoch, 0);      // A/B build: bumped by every nemar_tune (routes and packed-weight formats may have changed)

// ---- weight gradient ----------------------------------------------------------------------------------------
struct WgradParams {
    const float* src0; const float* src1; int C0, C1, Hs, Ws;
    const float* gy; int K, OH, OW;
    float* gw; int J;  // J = Cs * R * S columns, j = c*R*S + r*S + s (the tensor's own memory order)
    float* gb;         // optional [K]: += sum_pixels gy (bias gradient), folded into the A-tile loads of column-tile 0
    float* part;       // [splits][K*J] slabs then [splits][K] bias slabs (nullptr: fp32 atomics into gw / gb)
    float* partb;
    int N, P, sy, sx, R, S, pad, border;
    int pix_per_split;
    int dbg;   // ablation (nemar_tune key 2): 1 = skip staging loads, 2 = skip MFMAs, 8 = skip the atomic epilogue
    FastDiv fd_ohw, fd_ow;
};

template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(256) void wgrad_kernel(WgradParams p) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    constexpr int LDA = BM + 1, LDB = BN + 1;  // odd stride: conflict-free transposing stores
    constexpr int ACOLS = BM / 8, BCOLS = BN / 8;
    __shared__ float As[2][WBK][LDA];
    __shared__ float Bs[2][WBK][LDB];
    __shared__ int s_jc[BN];   // source channel of column j (or -1: out of range)
    __shared__ int s_jt[BN];   // packed (dy << 16) | (dx & 0xffff)

    const int tid = threadIdx.x;
    const int m0 = blockIdx.x * BM;
    const int j0 = blockIdx.y * BN;
    const int RS = p.R * p.S;
    const int HW = p.Hs * p.Ws, OHW = p.OH * p.OW;
    for (int i = tid; i < BN; i += 256) {
        const int j = j0 + i;
        int c = -1, tp = 0;
        if (j < p.J) {
            c = j / RS;
            const int t = j - c * RS;
            const int r = t / p.S, s = t - r * p.S;
            tp = ((r - p.pad) << 16) | ((s - p.pad) & 0xffff);
        }
        s_jc[i] = c;
        s_jt[i] = tp;
    }
    const int pbeg = blockIdx.z * p.pix_per_split;
    const int pend = min(p.P, pbeg + p.pix_per_split);
    const int prow = tid & 31, cgrp = tid >> 5;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    __syncthreads();

    float ra[ACOLS], rb[BCOLS];
    float bsum[ACOLS];
#pragma unroll
    for (int i = 0; i < ACOLS; ++i) bsum[i] = 0.f;
    const bool do_bias = p.gb != nullptr && blockIdx.y == 0;
    auto load_stage = [&](int pb) {
        const int pix = pb + prow;
        const bool pv = pix < pend;
        const unsigned upix = pv ? (unsigned)pix : 0u;
        const unsigned n = fd_div(upix, p.fd_ohw);
        const unsigned rem = upix - n * (unsigned)OHW;
        const unsigned oy = fd_div(rem, p.fd_ow);
        const unsigned ox = rem - oy * (unsigned)p.OW;
        const float* g = p.gy + (size_t)n * p.K * OHW + rem;
#pragma unroll
        for (int i = 0; i < ACOLS; ++i) {
            const int m = m0 + cgrp + 8 * i;
            ra[i] = (pv && m < p.K) ? g[(size_t)m * OHW] : 0.f;
            bsum[i] += ra[i];
        }
        const int by = (int)oy * p.sy, bx = (int)ox * p.sx;
        const float* s0n = p.src0 + (size_t)n * p.C0 * HW;
        const float* s1n = p.C1 ? p.src1 + (size_t)n * p.C1 * HW : p.src0;
#pragma unroll
        for (int i = 0; i < BCOLS; ++i) {
            const int col = cgrp + 8 * i;
            const int c = s_jc[col];
            const int tp = s_jt[col];
            float v = 0.f;
            if (pv && c >= 0) {
                int y = by + (tp >> 16), x = bx + (int)(short)(tp & 0xffff);
                bool inb = true;
                if (p.border == BORDER_REFLECT) {
                    y = reflect(y, p.Hs);
                    x = reflect(x, p.Ws);
                } else {
                    inb = (unsigned)y < (unsigned)p.Hs && (unsigned)x < (unsigned)p.Ws;
                }
                if (inb) {
                    const float* base = (c < p.C0) ? s0n + (size_t)c * HW : s1n + (size_t)(c - p.C0) * HW;
                    v = base[y * p.Ws + x];
                }
            }
            rb[i] = v;
        }
    };
    auto store_stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < ACOLS; ++i) As[buf][prow][cgrp + 8 * i] = ra[i];
#pragma unroll
        for (int i = 0; i < BCOLS; ++i) Bs[buf][prow][cgrp + 8 * i] = rb[i];
    };

    const int wid = tid >> 6, lane = tid & 63;
    const int wm = wid / WN, wn = wid - wm * WN;
    const int l31 = lane & 31, lhi = lane >> 5;
    const int nk = (pend - pbeg + WBK - 1) / WBK;
    if (nk > 0) {
        load_stage(pbeg);
        store_stage(0);
    }
    __syncthreads();
    for (int ks = 0; ks < nk; ++ks) {
        const int buf = ks & 1;
        if (ks + 1 < nk && !(p.dbg & 1)) load_stage(pbeg + (ks + 1) * WBK);
        if (!(p.dbg & 2))
#pragma unroll
        for (int k2 = 0; k2 < WBK / 2; ++k2) {
            const int kr = 2 * k2 + lhi;
            float a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = As[buf][kr][(wm * TM + i) * 32 + l31];
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = Bs[buf][kr][(wn * TN + j) * 32 + l31];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (ks + 1 < nk) store_stage(buf ^ 1);
        __syncthreads();
    }
    if (nk <= 0 || (p.dbg & 8)) return;
    float* const gw = p.part ? p.part + (size_t)blockIdx.z * ((size_t)p.K * p.J) : p.gw;
    if (do_bias) {
        // this thread summed gy over its pixel rows for channels cgrp + 8i; fold the 32 pixel lanes of each half-wave
        float* const gb = p.part ? p.partb + (size_t)blockIdx.z * p.K : p.gb;
#pragma unroll
        for (int i = 0; i < ACOLS; ++i) {
            float v = bsum[i];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            const int m = m0 + cgrp + 8 * i;
            if (prow == 0 && m < p.K) {
                if (p.part) gb[m] = v;
                else atomicAdd(gb + m, v);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int jj = j0 + (wn * TN + j) * 32 + l31;
        if (jj >= p.J) continue;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                if (m < p.K) {
                    if (p.part) gw[(size_t)m * p.J + jj] = acc[i][j][r];
                    else atomicAdd(gw + (size_t)m * p.J + jj, acc[i][j][r]);
                }
            }
    }
}

// Reflect data gradient, 3x3 / pad 1, without a ring launch.  The gradient of reflect-pad + conv w.r.t. texel (h,w) is the
// zero-padded data gradient plus, for the texels one step inside the border, the gradient of the padded texel they were
// mirrored to:  gx[1][w] gets  w[r=0] * gy[0]  on top of  w[r=0] * gy[2]  — i.e. tap dy = +1 must read gy[2] + gy[0] at output
// row 1 (and tap dy = -1 reads gy[H-3] + gy[H-1] at row H-2; columns likewise for dx = +-1 at columns 1 / W-2).  Those sums
// depend on the tap, so they cannot live in gy itself; they are pre-folded into two small side buffers that the loader lanes of
// igemm_ws2_kernel read INSTEAD of gy when their (tap, row / column group) is one of the special ones:
//   rows [v][d][n][k][xs]    v = 0: rows 2 + 0 (top), 1: rows H-3 + H-1 (bottom);  d = dx + 1 selects the column fold baked
//                            into that row: d = 2 adds texel 0 to texel 2, d = 0 adds texel W-1 to texel W-3
//   cols [e][n][k][y][j]     e = 0 (dx = +1): source columns 1..4 of row y with column 0 added to column 2;
//                            e = 1 (dx = -1): source columns W-5..W-2 with column W-1 added to column W-3
// (one 16-byte group = what the first / last 4-pixel output group of a row loads for that tap).
__global__ __launch_bounds__(256) void reflect_aux_kernel(const float* __restrict__ gy, float* __restrict__ rows,
                                                          float* __restrict__ cols, int N, int K, int H, int W) {
    const long long nrow = 6ll * N * K * W, ncol = 8ll * N * K * H;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < nrow + ncol;
         idx += (long long)gridDim.x * blockDim.x) {
        if (idx < nrow) {
            const int xs = (int)(idx % W);
            long long t = idx / W;
            const int k = (int)(t % K); t /= K;
            const int n = (int)(t % N);
            const int vd = (int)(t / N), v = vd / 3, d = vd - 3 * v;
            const float* g = gy + ((size_t)n * K + k) * H * W;
            const float* ra = g + (size_t)(v == 0 ? 2 : H - 3) * W;
            const float* rb = g + (size_t)(v == 0 ? 0 : H - 1) * W;
            float val = ra[xs] + rb[xs];
            if (d == 2 && xs == 2) val += ra[0] + rb[0];
            if (d == 0 && xs == W - 3) val += ra[W - 1] + rb[W - 1];
            rows[idx] = val;
        } else {
            const long long c = idx - nrow;
            const int j = (int)(c & 3);
            long long t = c >> 2;
            const int y = (int)(t % H); t /= H;
            const int k = (int)(t % K); t /= K;
            const int n = (int)(t % N);
            const int e = (int)(t / N);
            const float* r = gy + (((size_t)n * K + k) * H + y) * W;
            float val;
            if (e == 0) val = r[1 + j] + (j == 1 ? r[0] : 0.f);
            else val = r[W - 5 + j] + (j == 2 ? r[W - 1] : 0.f);
            cols[c] = val;
        }
    }
}

// Inverse of decode_ring: padded position (py, px) of the border ring -> index in the compact ring layout.
__device__ __forceinline__ unsigned encode_ring(unsigned rp, unsigned H, unsigned W, unsigned py, unsigned px) {
    const unsigned Wp = W + 2 * rp, band = rp * Wp;
    if (py < rp) return py * Wp + px;
    if (py >= H + rp) return band + (py - H - rp) * Wp + px;
    return 2 * band + (py - rp) * (2 * rp) + (px < rp ? px : px - W);
}

// gx[n,c,ty,tx] += sum of the ring texels that mirror onto (ty,tx), in a fixed order (gather: one thread per affected texel,
// no atomics).  Affected texels: rows 1..pad and H-1-pad..H-2 (whole rows), and columns 1..pad, W-1-pad..W-2 of every row.
// The launch enumerates, per (n,c) plane, `nrows` listed rows x W columns, then H rows x `ncols` listed columns (a texel of
// the second part that lies in a listed row was handled by the first part and is skipped).
struct RingBand { int nrows, ncols; int rows[8], cols[8]; };
__global__ __launch_bounds__(256) void ring_gather_kernel(const float* __restrict__ ring, float* __restrict__ gx, int H, int W,
                                                          int pad, int ring_len, RingBand band, long long planes) {
    const int per_plane = band.nrows * W + H * band.ncols;
    const long long total = planes * per_plane;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const long long nc = idx / per_plane;
        int e = (int)(idx - nc * per_plane), ty, tx;
        if (e < band.nrows * W) {
            ty = band.rows[e / W];
            tx = e % W;
        } else {
            e -= band.nrows * W;
            ty = e / band.ncols;
            tx = band.cols[e % band.ncols];
            bool listed = false;
            for (int i = 0; i < band.nrows; ++i) listed = listed || band.rows[i] == ty;
            if (listed) continue;
        }
        // padded rows / columns that mirror onto ty / tx (interior candidate first)
        int ys[3], xs[3], ny = 0, nx = 0;
        ys[ny++] = ty + pad;
        if (ty >= 1 && ty <= pad) ys[ny++] = pad - ty;
        if (ty <= H - 2 && ty >= H - 1 - pad) ys[ny++] = 2 * (H - 1) - ty + pad;
        xs[nx++] = tx + pad;
        if (tx >= 1 && tx <= pad) xs[nx++] = pad - tx;
        if (tx <= W - 2 && tx >= W - 1 - pad) xs[nx++] = 2 * (W - 1) - tx + pad;
        const float* r = ring + nc * ring_len;
        float sum = 0.f;
        for (int a = 0; a < ny; ++a)
            for (int b = 0; b < nx; ++b)
                if (a | b) sum += r[encode_ring((unsigned)pad, (unsigned)H, (unsigned)W, (unsigned)ys[a], (unsigned)xs[b])];
        gx[nc * (long long)H * W + (long long)ty * W + tx] += sum;
    }
}

// w2[c][k][r][s] = w[k][c][R-1-r][S-1-s]: the data gradient of a stride-1 convolution is the correlation of gy with
// these weights (and padding R-1-pad), which lets a layer with <= 4 INPUT channels use the narrow forward kernel
__global__ __launch_bounds__(256) void flip_transpose_kernel(const float* __restrict__ w, float* __restrict__ w2, int K,
                                                             int C, int R, int S) {
    const int total = K * C * R * S;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int s = idx % S, r = (idx / S) % R, k = (idx / (S * R)) % K, c = idx / (S * R * K);
        w2[idx] = w[(((size_t)k * C + c) * R + (R - 1 - r)) * S + (S - 1 - s)];
    }
}

// ... as a job of a weight-pack plan (pack_plan.h)
struct FlipTArgs {
    const float* w; float* w2;
    int K, C, R, S;
    int gx, gy;
};
__device__ __forceinline__ void flipt_body(const FlipTArgs& a, int bx, int, int gx) {
    const int total = a.K * a.C * a.R * a.S;
    for (int idx = bx * 256 + threadIdx.x; idx < total; idx += gx * 256) {
        const int s = idx % a.S, r = (idx / a.S) % a.R, k = (idx / (a.S * a.R)) % a.K, c = idx / (a.S * a.R * a.K);
        a.w2[idx] = a.w[(((size_t)k * a.C + c) * a.R + (a.R - 1 - r)) * a.S + (a.S - 1 - s)];
    }
}
NEMAR_PACK_MULTI(flipt_multi_kernel, FlipTArgs, flipt_body, 256)
void flipt_multi(const void* jobs, int njobs, int gx, int gy, hipStream_t st) {
    hipLaunchKernelGGL(flipt_multi_kernel, dim3(gx, gy, njobs), dim3(256), 0, st, (const FlipTArgs*)jobs);
}
struct RegFlipT {
    RegFlipT() { nemar_pack_register(PACK_FAM_FLIPT, sizeof(FlipTArgs), flipt_multi); }
} g_reg_flipt;

// round-1 form (nemar_tune(14, 0)): one atomic per workgroup
__global__ __launch_bounds__(256) void bias_grad_atomic_kernel(const float* __restrict__ g, float* __restrict__ gb, int N, int C,
                                                               int HW, int chunk) {
    __shared__ float red[16];
    const int c = blockIdx.x, n = blockIdx.y;
    const int beg = blockIdx.z * chunk, end = min(HW, beg + chunk);
    const float* q = g + ((size_t)n * C + c) * HW;
    float acc = 0.f;
    for (int i = beg + threadIdx.x; i < end; i += blockDim.x) acc += q[i];
    const float t = block_sum(acc, red);
    if (threadIdx.x == 0) atomicAdd(gb + c, t);
}

// part[(n * chunks + z) * C + c] = sum of g[n,c, chunk z of the plane]; grid (C, N, chunks): fixed tree per workgroup, one
// plain store; nemar_sum_partials adds the N * chunks slabs into gb in order (bitwise reproducible bias gradient)
__global__ __launch_bounds__(256) void bias_grad_kernel(const float* __restrict__ g, float* __restrict__ part, int N, int C,
                                                        int HW, int chunk) {
    __shared__ float red[16];
    const int c = blockIdx.x, n = blockIdx.y;
    const int beg = blockIdx.z * chunk, end = min(HW, beg + chunk);
    const float* q = g + ((size_t)n * C + c) * HW;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if ((((uintptr_t)(q + beg)) & 15) == 0) {
        // 16-byte loads, four independent sums, two loads in flight per thread (the one-dword-one-accumulator loop ran at 1.7 TB/s)
        const float4* q4 = reinterpret_cast<const float4*>(q + beg);
        const int n4 = (end - beg) >> 2;
        int i = threadIdx.x;
        for (; i + 256 < n4; i += 512) {
            const float4 u = q4[i], v = q4[i + 256];
            a0 += u.x + v.x; a1 += u.y + v.y; a2 += u.z + v.z; a3 += u.w + v.w;
        }
        if (i < n4) { const float4 u = q4[i]; a0 += u.x; a1 += u.y; a2 += u.z; a3 += u.w; }
        for (int k = beg + (n4 << 2) + threadIdx.x; k < end; k += 256) a0 += q[k];
    } else {
        for (int i = beg + threadIdx.x; i < end; i += blockDim.x) a0 += q[i];
    }
    const float t = block_sum((a0 + a1) + (a2 + a3), red);
    if (threadIdx.x == 0) part[((size_t)n * gridDim.z + blockIdx.z) * C + c] = t;
}

// gb[C] += sum over N and the plane of g [N,C,HW]: through the partial sums of bias_grad_kernel at `part`, or (no slabs) by atomics — the
// bias gradient of every route whose kernels leave gb alone, and nemar_bias_grad
void bias_grad_slabs(const float* g, float* gb, float* part, int N, int C, int HW, hipStream_t st) {
    const int chunks = nemar_cdiv(HW, BIAS_CHUNK);
    if (!part) { hipLaunchKernelGGL(bias_grad_atomic_kernel, dim3(C, N, chunks), dim3(256), 0, st, g, gb, N, C, HW, BIAS_CHUNK); return; }
    hipLaunchKernelGGL(bias_grad_kernel, dim3(C, N, chunks), dim3(256), 0, st, g, part, N, C, HW, BIAS_CHUNK);
    nemar_sum_partials(part, C, N * chunks, gb, C, true, st);
}

// gx[n,c,h,w] = sum of the padded-domain gradient gp over every padded position that mirrors onto (h,w)
// (+ addend[n,c,h,w] where given: the skip gradient of a ResnetBlock rides in the pass that writes the data gradient of its first convolution)
__global__ __launch_bounds__(256) void reflect_fold_kernel(const float* __restrict__ gp, float* __restrict__ gx, int H,
                                                           int W, int pad, long long total, const float* __restrict__ addend) {
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int w = (int)(idx % W);
        const long long t = idx / W;
        const int h = (int)(t % H);
        const long long nc = t / H;
        const float* q = gp + nc * (long long)Hp * Wp;
        // padded rows that map to h: h+pad always; pad-h if 1<=h<=pad; 2(H-1)-h+pad if H-1-pad<=h<=H-2 (columns likewise).  No index
        // lists in private arrays (dynamically indexed ones live in scratch memory): up to three rows x three columns, spelled out
        const int y0 = h + pad, x0 = w + pad;
        const int y1 = (h >= 1 && h <= pad) ? pad - h : -1, y2 = (h <= H - 2 && h >= H - 1 - pad) ? 2 * (H - 1) - h + pad : -1;
        const int x1 = (w >= 1 && w <= pad) ? pad - w : -1, x2 = (w <= W - 2 && w >= W - 1 - pad) ? 2 * (W - 1) - w + pad : -1;
        auto rowsum = [&](int y) {
            const float* r = q + (long long)y * Wp;
            float v = r[x0];
            if (x1 >= 0) v += r[x1];
            if (x2 >= 0) v += r[x2];
            return v;
        };
        float s = rowsum(y0);
        if (y1 >= 0) s += rowsum(y1);
        if (y2 >= 0) s += rowsum(y2);
        gx[idx] = addend ? s + addend[idx] : s;
    }
}
// ... for pad == 1 and rows of whole 4-float runs: a lane owns 4 consecutive texels of one row (unit = plane, row, run: row_unit, common.h).
// The interior is a copy (+ addend) of padded[h + 1][w + 1 ..]: one 16-byte load at a 4-byte aligned address, one 16-byte store.  Only
// rows 1 and H - 2 have a mirror row (padded rows 0 and H + 1), only texels 1 and W - 2 of a row a mirror column (padded columns 0 and
// W + 1): the first and the last run of a row load those two words, rows 1 and H - 2 the mirror row's 16 bytes as well — every load of a
// unit before the first use.  The sums are reflect_fold_kernel's: rows own, upper mirror, lower mirror; within a row own, left, right; the addend last.
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));      // 16-byte load at a 4-byte-aligned address
template <bool ADD>
__global__ __launch_bounds__(256) void reflect_fold_rows_kernel(const float* __restrict__ gp, float* __restrict__ gx, int H, int W,
                                                                unsigned units, const float* __restrict__ addend) {
    const int Hp = H + 2, Wp = W + 2;
    const unsigned runs = (unsigned)W >> 2;
    for (unsigned u = blockIdx.x * 256 + threadIdx.x; u < units; u += gridDim.x * 256) {
        int j, h;
        size_t nc;
        row_unit(u, runs, H, j, h, nc);
        const bool up = h == 1, dn = h == H - 2, le = j == 0, ri = j == (int)runs - 1;
        const float* q = gp + nc * Hp * Wp;
        const float* r0 = q + (size_t)(h + 1) * Wp;
        const float* r1 = up ? q : r0;                              // padded row 0 mirrors onto row 1
        const float* r2 = dn ? q + (size_t)(H + 1) * Wp : r0;       // padded row H + 1 onto row H - 2
        const int x0 = 4 * j + 1;
        const size_t o = (nc * H + h) * W + 4 * j;
        const f32x4u v0 = *reinterpret_cast<const f32x4u*>(r0 + x0);
        f32x4u v1 = v0, v2 = v0;
        float l0 = 0.f, l1 = 0.f, l2 = 0.f, e0 = 0.f, e1 = 0.f, e2 = 0.f;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (up) v1 = *reinterpret_cast<const f32x4u*>(r1 + x0);
        if (dn) v2 = *reinterpret_cast<const f32x4u*>(r2 + x0);
        if (le) { l0 = r0[0]; l1 = r1[0]; l2 = r2[0]; }
        if (ri) { e0 = r0[W + 1]; e1 = r1[W + 1]; e2 = r2[W + 1]; }
        if (ADD) a = *reinterpret_cast<const float4*>(addend + o);
        // texel 1 of the run is w == 1 in the first run, texel 2 is w == W - 2 in the last
        float s0 = v0.x, s1 = v0.y, s2 = v0.z, s3 = v0.w;
        if (le) s1 += l0;
        if (ri) s2 += e0;
        if (up) {
            float t1 = v1.y, t2 = v1.z;
            if (le) t1 += l1;
            if (ri) t2 += e1;
            s0 += v1.x; s1 += t1; s2 += t2; s3 += v1.w;
        }
        if (dn) {
            float t1 = v2.y, t2 = v2.z;
            if (le) t1 += l2;
            if (ri) t2 += e2;
            s0 += v2.x; s1 += t1; s2 += t2; s3 += v2.w;
        }
        *reinterpret_cast<float4*>(gx + o) = ADD ? make_float4(s0 + a.x, s1 + a.y, s2 + a.z, s3 + a.w) : make_float4(s0, s1, s2, s3);
    }
}
// the padded domain's gradient folded onto the image (+ addend)
void fold_padded(const float* padded, float* gx, int H, int W, int pad, long long total, const float* addend, hipStream_t st) {
    if (g_pointwise_rows && pad == 1 && (W & 3) == 0 && total / 4 < (1ll << 31) &&
        (((uintptr_t)padded) & 3) == 0 && ((((uintptr_t)gx) | ((uintptr_t)addend)) & 15) == 0) {
        const dim3 grid(nemar_stream_grid(total / 4, 256)), block(256);
        if (addend) hipLaunchKernelGGL((reflect_fold_rows_kernel<true>), grid, block, 0, st, padded, gx, H, W, (unsigned)(total / 4), addend);
        else hipLaunchKernelGGL((reflect_fold_rows_kernel<false>), grid, block, 0, st, padded, gx, H, W, (unsigned)(total / 4), addend);
        return;
    }
    hipLaunchKernelGGL(reflect_fold_kernel, dim3(nemar_stream_grid(total, 256)), dim3(256), 0, st, padded, gx, H, W, pad, total, addend);
}

// ---- 7x7 / pad-3 layers with <= 4 channels on the OUTPUT side: the launches of the many -> few form (conv_route.h K7MfPlan) ----------
__global__ __launch_bounds__(256) void k7_mf_weights_kernel(const float* __restrict__ w, float* __restrict__ wt, int Ks, int Cb, int dgrad) {
    // wt[(ks * 8 + dx)][cb][dy]: forward w[ks][cb][dy][dx] (w = [Ks][Cb][7][7]); data gradient w[cb][ks][6 - dy][6 - dx] (w = [Cb][Ks][7][7])
    const int total = 32 * Cb * 7;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int dy = i % 7, cb = (i / 7) % Cb, m = i / (7 * Cb), ks = m >> 3, dx = m & 7;
        float v = 0.f;
        if (ks < Ks && dx < 7)
            v = dgrad ? w[(((size_t)cb * Ks + ks) * 7 + (6 - dy)) * 7 + (6 - dx)] : w[(((size_t)ks * Cb + cb) * 7 + dy) * 7 + dx];
        wt[i] = v;
    }
}
struct K7MfWtArgs {
    const float* w; float* wt;
    int Ks, Cb, dgrad;
    int gx, gy;
};
__device__ __forceinline__ void k7_mf_wt_body(const K7MfWtArgs& a, int bx, int, int gx) {
    const int total = 32 * a.Cb * 7;
    for (int i = bx * 256 + threadIdx.x; i < total; i += gx * 256) {
        const int dy = i % 7, cb = (i / 7) % a.Cb, m = i / (7 * a.Cb), ks = m >> 3, dx = m & 7;
        float v = 0.f;
        if (ks < a.Ks && dx < 7)
            v = a.dgrad ? a.w[(((size_t)cb * a.Ks + ks) * 7 + (6 - dy)) * 7 + (6 - dx)] : a.w[(((size_t)ks * a.Cb + cb) * 7 + dy) * 7 + dx];
        a.wt[i] = v;
    }
}
NEMAR_PACK_MULTI(k7_mf_wt_multi_kernel, K7MfWtArgs, k7_mf_wt_body, 256)
void k7_mf_wt_multi(const void* jobs, int njobs, int gx, int gy, hipStream_t st) {
    hipLaunchKernelGGL(k7_mf_wt_multi_kernel, dim3(gx, gy, njobs), dim3(256), 0, st, (const K7MfWtArgs*)jobs);
}
struct RegK7MfWt {
    RegK7MfWt() { nemar_pack_register(PACK_FAM_PRE, sizeof(K7MfWtArgs), k7_mf_wt_multi); }
} g_reg_k7_mf_wt;

// out[n][k][y][x] = act(bias[k] + sum over the P positions (Y, X) that belong to (y, x) of sum_dx P[n][k * 8 + dx][Y][X + dx]).
// fold == 0: (Y, X) = (y, x).  fold == 1 (reflect-padded data gradient, P on the padded domain): every padded position that mirrors onto
// (y, x): rows y + 3, 3 - y (1 <= y <= 3), 2 (H - 1) - y + 3 (H - 4 <= y <= H - 2), columns likewise — fixed order, no atomics.
__global__ __launch_bounds__(256) void k7_mf_sum_kernel(const float* __restrict__ P, const float* __restrict__ bias, float* __restrict__ out,
                                                        int Ks, int H, int W, int PH, int PW, int fold, int act, float slope, long long total) {
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int x = (int)(idx % W);
        long long t = idx / W;
        const int y = (int)(t % H);
        t /= H;
        const int k = (int)(t % Ks);
        const long long n = t / Ks;
        const float* Pk = P + ((size_t)n * 32 + (size_t)k * 8) * PH * PW;
        const size_t pplane = (size_t)PH * PW;
        auto at = [&](int Y, int X) {
            const float* r = Pk + (size_t)Y * PW + X;
            float s = 0.f;
#pragma unroll
            for (int dx = 0; dx < 7; ++dx) s += r[(size_t)dx * pplane + dx];
            return s;
        };
        float v;
        if (!fold) {
            v = at(y, x);
        } else {
            const int y0 = y + 3, x0 = x + 3;
            const int y1 = (y >= 1 && y <= 3) ? 3 - y : -1, y2 = (y <= H - 2 && y >= H - 4) ? 2 * (H - 1) - y + 3 : -1;
            const int x1 = (x >= 1 && x <= 3) ? 3 - x : -1, x2 = (x <= W - 2 && x >= W - 4) ? 2 * (W - 1) - x + 3 : -1;
            auto row = [&](int Y) {
                float s = at(Y, x0);
                if (x1 >= 0) s += at(Y, x1);
                if (x2 >= 0) s += at(Y, x2);
                return s;
            };
            v = row(y0);
            if (y1 >= 0) v += row(y1);
            if (y2 >= 0) v += row(y2);
        }
        if (bias) v += bias[k];
        out[idx] = apply_act(v, act, slope);
    }
}

// src -> out through the three launches (weights re-arranged + packed first unless prepacked)
void k7_mf_run(const K7MfPlan& m_, const float* src, const float* w, int Ks, int Cb, int dgrad, const float* bias, float* out, int N, int H, int W,
               int fold, int act, float slope, float* wsf, int prepacked, hipStream_t st) {
    K7MfPlan m = m_;
    float* wt = wsf + m.wt_off;
    void* packed = wsf + m.pack_off;
    float* P = wsf + m.p_off;
    if (!prepacked) {
        K7MfWtArgs a{w, wt, Ks, Cb, dgrad, nemar_stream_grid(32 * Cb * 7, 256), 1};
        if (nemar_pack_recording()) nemar_pack_record_job(PACK_FAM_PRE, &a, a.gx, 1);
        hipLaunchKernelGGL(k7_mf_weights_kernel, dim3(a.gx), dim3(256), 0, st, w, wt, Ks, Cb, dgrad);
        nemar_s16g_pack(m.q, m.pl, wt, (long long)Cb * 7, 7, packed, st);
    }
    m.q.src0 = src; m.q.src1 = nullptr; m.q.dst0 = P; m.q.dst1 = nullptr; m.q.bias = nullptr; m.q.dbg = 0; m.q.tl = nullptr;
    nemar_s16g_conv(m.q, m.pl, packed, st);
    const long long total = (long long)N * Ks * H * W;
    hipLaunchKernelGGL(k7_mf_sum_kernel, dim3(nemar_stream_grid(total, 256)), dim3(256), 0, st, (const float*)P, bias, out, Ks, H, W, m.PH, m.PW, fold,
                       act, slope, total);
}

// copy of gy with OHv >= OH rows per plane, (OHv * OW) % 4 == 0, zero-filled below row OH (conv_route.h padded_rows)
__global__ __launch_bounds__(256) void pad_planes_kernel(const float* __restrict__ src, float* __restrict__ dst, int plane,
                                                         int plane_padded, long long total) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const long long pl = idx / plane_padded;
        const int r = (int)(idx - pl * plane_padded);
        dst[idx] = r < plane ? src[pl * plane + r] : 0.f;
    }
}

}  // namespace

// the call-time facts every operator has
static ConvFacts facts_of(const ConvCall& call, const float* bias, int act, float slope) {
    ConvFacts f;
    f.bias = bias != nullptr; f.act = act; f.slope = slope; f.scratch_bytes = call.scratch ? call.scratch_bytes : 0;
    return f;
}

NEMAR_API size_t nemar_conv2d_fwd_workspace(int N, int H, int W, int K, int C, int R, int S, int stride, int pad) {
    if (N <= 0 || H <= 0 || W <= 0 || K <= 0 || C <= 0 || R <= 0 || S <= 0 || stride < 1) return 0;
    return sizeof(float) * plan_fwd({N, C, 0, H, W, K, R, S, stride, pad, BORDER_ZERO}, ConvFacts::canonical()).total;
}

// Honours call.scratch, .src_max and .src_planes (the wide route)
static int conv2d_fwd(ConvCall& call, const float* x0, int C0, const float* x1, int C1, const float* w, const float* bias,
                      float* y, int N, int H, int W, int K, int R, int S, int stride, int pad, int pad_mode,
                      int act, float slope, void* workspace, size_t ws_bytes, int prepacked, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(x0 && w && y && workspace, "conv2d_fwd: null pointer");
    NEMAR_REQUIRE(C0 > 0 && C1 >= 0 && (C1 == 0 || x1), "conv2d_fwd: bad channel split %d+%d", C0, C1);
    NEMAR_REQUIRE(N > 0 && H > 0 && W > 0 && K > 0 && R > 0 && S > 0 && R * S <= MAX_TAPS, "conv2d_fwd: bad shape");
    NEMAR_REQUIRE(stride >= 1 && pad >= 0 && pad < 32768, "conv2d_fwd: bad stride/pad");
    NEMAR_REQUIRE(pad_mode == BORDER_ZERO || (pad_mode == BORDER_REFLECT && pad < H && pad < W),
                  "conv2d_fwd: reflect pad %d needs pad < H,W (%d,%d)", pad, H, W);
    const int C = C0 + C1;
    const int OH = (H + 2 * pad - R) / stride + 1, OW = (W + 2 * pad - S) / stride + 1;
    NEMAR_REQUIRE(OH > 0 && OW > 0, "conv2d_fwd: empty output");
    NEMAR_REQUIRE((long long)N * OH * OW < (1ll << 31) && (long long)C * H * W < (1ll << 31) && (long long)C * R * S < (1 << 20),
                  "conv2d_fwd: problem too large for 32-bit tile indexing");
    ConvFacts f = facts_of(call, bias, act, slope);
    FwdPlan P = plan_fwd({N, C0, C1, H, W, K, R, S, stride, pad, pad_mode}, f);
    if (ws_bytes < sizeof(float) * P.total) {
        nemar_set_error("conv2d_fwd: workspace %zu < %zu", ws_bytes, sizeof(float) * P.total);
        return NEMAR_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const char* what = "conv2d_fwd";
    g_last_route = P.route;
    switch (P.route) {
    case ROUTE_K7:
        if (P.sub == FwdPlan::K7_MANY_FEW) {
            k7_mf_run(P.k7, x0, w, K, C, 0, bias, y, N, H, W, 0, act, slope, (float*)workspace, prepacked, st);
            what = "conv2d_fwd (7x7 many -> few, 16-bit pipe)";
        } else {
            if (!prepacked) nemar_k7_fm_pack(w, (long long)C * 49, 49, 0, K, C, workspace, st);
            nemar_k7_fm_conv(x0, C, H, W, 3, pad_mode == BORDER_REFLECT, workspace, bias, y, K, N, H, W, act, slope, 0, st);
            what = "conv2d_fwd (7x7, 16-bit pipe)";
        }
        break;
    case ROUTE_NARROW:
        // (the weights are read in place: the packed-weight workspace is the slab space of the channel-split mode, see nemar_narrow_fwd)
        nemar_narrow_fwd(x0, w, bias, y, N, C, H, W, K, R, pad, pad_mode, act, slope,
                         g_deterministic ? (float*)workspace : nullptr, ws_bytes / sizeof(float), st);
        what = "conv2d_fwd (narrow)";
        break;
    case ROUTE_SPLIT16: {
        const int mode = pad_mode == BORDER_REFLECT ? SPLIT16_REFLECT : SPLIT16_ZERO;
        if (!prepacked) nemar_split16_pack(w, workspace, K, C, R, 0, g_split16_variant, st);
        nemar_split16_conv(x0, workspace, bias, y, N, H, W, K, C, R, 1, H, W, OH, OW, mode, call.scratch, g_xcd_map, g_split16_variant,
                           g_tl, nullptr, call.src_max, call.src_planes, call.src_planes_kind, nullptr, nullptr, st);
        what = "conv2d_fwd (split-16)";
        break;
    }
    case ROUTE_S16G: {
        S16gProblem& q = P.q;
        q.src0 = x0; q.src1 = x1; q.dst0 = y; q.dst1 = nullptr; q.bias = bias; q.dbg = g_dbg; q.tl = g_tl;
        if (!prepacked) nemar_s16g_pack(q, P.pl, w, (long long)C * R * S, (long long)R * S, workspace, st);
        nemar_s16g_conv(q, P.pl, workspace, st);
        what = "conv2d_fwd (16-bit pipe, in-kernel split)";
        break;
    }
    default: {
        IgemmParams p;
        fwd_taps(p.taps, R, S, pad);
        if (!prepacked) launch_pack(w, (float*)workspace, K, C, C * R * S, R * S, p.taps, st);
        p.src0 = x0; p.src1 = x1; p.C0 = C0; p.C1 = C1; p.Hs = H; p.Ws = W;
        p.wp = (const float*)workspace; p.M = K; p.Mpad = igemm_mpad(K); p.Kred = C * R * S;
        p.zero = p.wp + packed_core_floats(K, C * R * S);
        p.dbg = g_dbg; p.tl = g_tl;
        p.ring_p = 0; p.ring_H = 0; p.ring_W = 0; p.ksplit = 1; p.part = nullptr; p.part_stride = 0;
        p.rf = 0; p.rf_row = nullptr; p.rf_col = nullptr; p.xcd = 0;
        p.bias = bias;
        p.dst0 = y; p.dst1 = nullptr; p.M0 = K;
        p.OH = OH; p.OW = OW; p.OHf = OH; p.OWf = OW; p.osy = 1; p.ooy = 0; p.osx = 1; p.oox = 0;
        p.N = N; p.P = N * OH * OW;
        p.sy = stride; p.sx = stride; p.border = pad_mode; p.act = act; p.slope = slope; p.pad = pad;
        p.fd_ohw = make_fastdiv(OH * OW); p.fd_ow = make_fastdiv(OW); p.fd_cs = make_fastdiv(C);
        if (P.sub != FwdPlan::PLAIN) {      // slab 0 carries the bias; an activation follows the sum (ReLU / LeakyReLU)
            p.ksplit = P.ksplit;
            p.part = (float*)workspace + P.slab_off;
            p.part_stride = (long long)N * K * OH * OW;
            p.act = ACT_NONE;
        }
        launch_igemm(p, st);
        if (P.sub == FwdPlan::SPLIT_ACT) nemar_sum_partials_act(p.part, p.part_stride, p.ksplit, y, p.part_stride, act == ACT_RELU ? 1 : 2, slope, st);
        else if (P.sub == FwdPlan::SPLIT) nemar_sum_partials(p.part, p.part_stride, p.ksplit, y, p.part_stride, false, st);
    }
    }
    NEMAR_CHECK_LAUNCH(what);
    return NEMAR_OK;
}

// Data gradient of the conv above: gy [N,K,OH,OW] -> gx [N,C,H,W] (split over gx0[C0] | gx1[C1]; gx0 may be NULL to
// skip its channels).  With bias/act it is also the FORWARD of nn.ConvTranspose2d(K -> C) whose weight is w[K][C][R][S].
NEMAR_API size_t nemar_conv2d_bwd_data_workspace(int N, int C, int H, int W, int K, int R, int S, int stride, int pad, int pad_mode) {
    if (N <= 0 || C <= 0 || K <= 0 || R <= 0 || S <= 0 || stride < 1) return 0;
    return sizeof(float) * plan_dgrad({N, C, 0, H, W, K, R, S, stride, pad, pad_mode}, ConvFacts::canonical()).total;
}

// Honours call.scratch, .src_max, .src_planes, .gy_planes_out, .addend and .out_max; sets .gy_planes_written, .epilogue_fused, .addend_done
static int conv2d_bwd_data(ConvCall& call, const float* gy, const float* w, const float* bias, int act, float slope,
                           float* gx0, int C0, float* gx1, int C1, int N, int H, int W, int K, int OH, int OW,
                           int R, int S, int stride, int pad, int pad_mode, void* workspace, size_t ws_bytes,
                           int prepacked, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(gy && w && workspace && (gx0 || gx1), "conv2d_bwd_data: null pointer");
    NEMAR_REQUIRE(C0 >= 0 && C1 >= 0 && C0 + C1 > 0 && (C1 == 0 || gx1), "conv2d_bwd_data: bad channel split");
    NEMAR_REQUIRE(N > 0 && H > 0 && W > 0 && K > 0 && OH > 0 && OW > 0 && R * S <= MAX_TAPS && R > 0 && S > 0,
                  "conv2d_bwd_data: bad shape");
    NEMAR_REQUIRE(stride >= 1 && stride <= 4 && pad >= 0, "conv2d_bwd_data: bad stride/pad");
    NEMAR_REQUIRE((H + 2 * pad - R) / stride + 1 == OH && (W + 2 * pad - S) / stride + 1 == OW,
                  "conv2d_bwd_data: gy %dx%d inconsistent with x %dx%d k%d s%d p%d", OH, OW, H, W, R, stride, pad);
    const int C = C0 + C1;
    const bool refl = pad_mode == BORDER_REFLECT && pad > 0;
    NEMAR_REQUIRE(pad_mode != BORDER_REFLECT || (pad < H && pad < W), "conv2d_bwd_data: reflect pad too large");
    NEMAR_REQUIRE(!refl || (!bias && act == ACT_NONE && gx1 == nullptr),
                  "conv2d_bwd_data: reflect mode supports a single destination without bias/activation");
    NEMAR_REQUIRE(!refl || stride > 1 || pad <= 4, "conv2d_bwd_data: reflect pad %d > 4 unsupported", pad);
    ConvFacts f = facts_of(call, bias, act, slope);
    f.gx0 = gx0 != nullptr; f.gx1 = gx1 != nullptr;
    f.gy_planes_bytes = call.gy_planes_out ? call.gy_planes_bytes : 0;
    DgradPlan L = plan_dgrad({N, C0, C1, H, W, K, R, S, stride, pad, pad_mode}, f);
    if (ws_bytes < sizeof(float) * L.total) {
        nemar_set_error("conv2d_bwd_data: workspace %zu < %zu", ws_bytes, sizeof(float) * L.total);
        return NEMAR_EWORKSPACE;
    }
    NEMAR_REQUIRE((long long)N * (H + 2 * pad) * (W + 2 * pad) < (1ll << 31) && (long long)K * OH * OW < (1ll << 31) && (long long)K * R * S < (1 << 20),
                  "conv2d_bwd_data: problem too large for 32-bit tile indexing");
    hipStream_t st = (hipStream_t)stream;
    float* wsf = (float*)workspace;
    const long long total = (long long)N * C * H * W;
    const int mskip = L.mskip;        // skipping the first C0 channels when gx0 == NULL: start the M range at C0
    const char* what = "conv2d_bwd_data";
    g_last_route = L.route;
    switch (L.sub) {
    case DgradPlan::K7_MANY_FEW:
        k7_mf_run(L.k7, gy, w, C, K, 1, nullptr, gx0, N, H, W, L.k7_fold, ACT_NONE, 0.f, wsf, prepacked, st);
        what = "conv2d_bwd_data (7x7 many -> few, 16-bit pipe)";
        break;
    case DgradPlan::K7_FEW_MANY:
        if (!prepacked) nemar_k7_fm_pack(w, 49, (long long)C * 49, 1, C, K, workspace, st);
        if (L.k7_fold == 2) {             // reflect: on the padded (H + 6) x (W + 6) domain (gy through a 6-texel zero border), then the fold
            float* padded = wsf + ((nemar_k7_fm_pack_floats(C) + 3) & ~(size_t)3);
            nemar_k7_fm_conv(gy, K, OH, OW, 6, 0, workspace, nullptr, padded, C, N, H + 6, W + 6, ACT_NONE, 0.f, 0, st);
            fold_padded(padded, gx0, H, W, pad, total, nullptr, st);
        } else {                          // (k7_fold == 1: mirrored contributions accumulated in the kernel: no padded tensor, no fold pass)
            nemar_k7_fm_conv(gy, K, OH, OW, L.k7_fold ? 6 : 3, 0, workspace, nullptr, gx0, C, N, H, W, ACT_NONE, 0.f, L.k7_fold, st);
        }
        what = "conv2d_bwd_data (7x7, 16-bit pipe)";
        break;
    case DgradPlan::SPLIT16: {
        if (!prepacked) nemar_split16_pack(w, workspace, K, C, R, 1, g_split16_variant, st);
        const Split16Done done = nemar_split16_conv(gy, workspace, nullptr, gx0, N, H, W, C, K, R, R - 1 - pad, OH, OW, H, W,
                                                    refl ? SPLIT16_DGRAD_REFLECT : SPLIT16_ZERO, call.scratch, g_xcd_map, g_split16_variant, g_tl,
                                                    L.want_gy_planes ? call.gy_planes_out : nullptr, call.src_max, call.src_planes,
                                                    call.src_planes_kind, call.addend, call.out_max, st);
        call.gy_planes_written = done.dual_written;
        call.epilogue_fused = done.epilogue_fused;
        what = "conv2d_bwd_data (split-16)";
        break;
    }
    case DgradPlan::S16G:
    case DgradPlan::S16G_FOLD: {            // (fold: one destination, no skip — the gradient of the padded input into scratch, then the fold)
        const bool fold16 = L.sub == DgradPlan::S16G_FOLD;
        S16gProblem& q = L.q;
        q.src0 = gy; q.src1 = nullptr; q.bias = bias ? bias + mskip : nullptr;
        if (fold16) { q.dst0 = wsf + L.padded_off; q.dst1 = nullptr; q.M0 = q.M; }
        else if (mskip) { q.dst0 = gx1; q.dst1 = nullptr; q.M0 = q.M; }
        else { q.dst0 = gx0; q.dst1 = gx1; q.M0 = C0; }
        // output row m = input channel m + mskip, reduction channel = k:  w[k][c][r][s]
        if (!prepacked) nemar_s16g_pack(q, L.pl, w + (size_t)mskip * R * S, (long long)R * S, (long long)C * R * S, workspace, st);
        nemar_s16g_conv(q, L.pl, workspace, st);
        if (fold16) fold_padded(q.dst0, gx0, H, W, pad, total, call.addend, st);
        if (fold16 && call.addend) call.addend_done = true;
        what = fold16 ? "conv2d_bwd_data (16-bit pipe on the padded domain + fold)" : "conv2d_bwd_data (16-bit pipe, in-kernel split)";
        break;
    }
    case DgradPlan::EXACT: {
    // Reflect padding, ring form: the zero-padded data gradient on the unpadded domain, then the same implicit GEMM at the border-ring positions
    // into a compact scratch, which ring_gather_kernel adds to the texels it mirrors.  Fold form: the padded domain into scratch, then the fold.
    const bool ring = L.ring, fold = L.fold;
    bool folded = false;                  // fold_small: the slab sum folded the border already
    const int Hd = fold ? H + 2 * pad : H, Wd = fold ? W + 2 * pad : W;
    const int padd = fold ? 0 : pad;
    float* padded = fold ? wsf + L.padded_off : nullptr;
    int cls = 0;
    for (int ph = 0; ph < stride; ++ph)
        for (int pw = 0; pw < stride; ++pw, ++cls) {
            IgemmParams p;
            dgrad_taps(p.taps, R, S, padd, stride, ph, pw);
            const int OHc = (Hd - ph + stride - 1) / stride, OWc = (Wd - pw + stride - 1) / stride;
            if (OHc <= 0 || OWc <= 0) continue;
            const int Mc = C - mskip;
            p.src0 = gy; p.src1 = nullptr; p.C0 = K; p.C1 = 0; p.Hs = OH; p.Ws = OW;
            p.M = Mc; p.Mpad = igemm_mpad(Mc); p.Kred = p.taps.n * K;
            p.bias = bias ? bias + mskip : nullptr;
            if (fold) { p.dst0 = padded; p.dst1 = nullptr; p.M0 = Mc; }
            else if (mskip) { p.dst0 = gx1; p.dst1 = nullptr; p.M0 = Mc; }
            else { p.dst0 = gx0; p.dst1 = gx1; p.M0 = C0; }
            p.OH = OHc; p.OW = OWc; p.OHf = Hd; p.OWf = Wd; p.osy = stride; p.ooy = ph; p.osx = stride; p.oox = pw;
            p.N = N; p.P = N * OHc * OWc;
            p.sy = 1; p.sx = 1; p.border = BORDER_ZERO; p.act = act; p.slope = slope;
            p.pad = pad;
            p.ring_p = 0; p.ring_H = 0; p.ring_W = 0; p.ksplit = 1; p.part = nullptr; p.part_stride = 0;
            p.rf = 0; p.rf_row = nullptr; p.rf_col = nullptr; p.xcd = 0;
            p.fd_ohw = make_fastdiv(OHc * OWc); p.fd_ow = make_fastdiv(OWc); p.fd_cs = make_fastdiv(K);
            float* wp = wsf + L.pack_stride * (size_t)cls;
            p.wp = wp;
            p.zero = wp + packed_core_floats(Mc, K * (p.taps.n > 0 ? p.taps.n : 1));
            p.dbg = g_dbg; p.tl = nullptr;
            if (p.taps.n == 0) {
                // no tap reaches this class (e.g. k1 s2): gradient is bias-only / zero; run with one zero tap
                p.taps.n = 1; p.taps.dy[0] = -32000; p.taps.dx[0] = -32000; p.taps.wofs[0] = 0; p.Kred = K;
                p.taps.dyx[0] = (int)(((unsigned)-32000 << 16) | ((unsigned)-32000 & 0xffffu));
            }
            // A[(t*K + k)][c] = w[k][c + mskip][r][s]
            if (!prepacked) launch_pack(w + (size_t)mskip * R * S, wp, Mc, K, R * S, C * R * S, p.taps, st);
            bool ring_done = false;
            if (L.narrow) {
                // <= 4 input channels: the zero-padded data gradient is a <= 4-output-channel correlation of gy — the narrow VALU kernel's job
                float* w2 = wsf + L.w2_off;
                if (!prepacked) {
                    if (nemar_pack_recording()) {
                        FlipTArgs a{w, w2, K, C, R, S, nemar_stream_grid((long long)K * C * R * S, 256), 1};
                        nemar_pack_record_job(PACK_FAM_FLIPT, &a, a.gx, 1);
                    }
                    hipLaunchKernelGGL(flip_transpose_kernel, dim3(nemar_stream_grid((long long)K * C * R * S, 256)),
                                       dim3(256), 0, st, w, w2, K, C, R, S);
                }
                nemar_narrow_fwd(gy, w2, nullptr, gx0, N, K, OH, OW, C, R, R - 1 - pad, BORDER_ZERO, ACT_NONE, 0.f, nullptr, 0, st);
            } else {
                if (L.split) {      // each split stores its partial gradient to its own slab, summed in order
                    p.ksplit = L.ksplit;
                    p.part = wsf + L.slab_off;
                    p.part_stride = (long long)N * C * Hd * Wd;       // (fold_small: slabs of the padded domain)
                    if (gx1) { p.M0 = C; p.dst1 = nullptr; }      // two destinations: the slabs hold all C rows, the sum pass parts them
                }
                // on the wave-specialised 16-byte-load kernel the border folds INTO the main launch (reflect_aux_kernel); else the ring launch below
                bool vec = false;
                if (L.aux_rows && route_ws2(p, &vec) && vec) {
                    float* rows = wsf + L.aux_rows_off, * cols = wsf + L.aux_cols_off;
                    hipLaunchKernelGGL(reflect_aux_kernel, dim3(nemar_stream_grid(6ll * N * K * W + 8ll * N * K * H, 256)),
                                       dim3(256), 0, st, gy, rows, cols, N, K, H, W);
                    p.rf = 1; p.rf_row = rows; p.rf_col = cols;
                    ring_done = true;
                }
                launch_igemm(p, st);
                if (p.ksplit > 1 && fold) {                       // slabs of the padded domain -> sum + fold in one pass (one destination: the plan)
                    nemar_sum_partials_fold(p.part, p.part_stride, p.ksplit, gx0, (long long)N * C, H, W, pad, call.addend, st);
                    if (call.addend) call.addend_done = true;
                    folded = true;
                }
                else if (p.ksplit > 1 && gx1) nemar_sum_partials_two(p.part, p.part_stride, p.ksplit, gx0, gx1, N, C0, C1, H * W, st);
                else if (p.ksplit > 1) nemar_sum_partials(p.part, p.part_stride, p.ksplit, gx0, p.part_stride, false, st);
                p.rf = 0;
            }
            if (ring && !ring_done) {
                // same weights (stride 1: every tap, same order), taps re-based to padded coordinates
                dgrad_taps(p.taps, R, S, 0, 1, 0, 0);
                const int ring_len = L.ring_len;
                p.ring_p = pad; p.ring_H = H; p.ring_W = W;
                p.ksplit = L.ring_ksplit;
                p.part = L.ring_ksplit > 1 ? wsf + L.ring_slab_off : nullptr;
                p.part_stride = (long long)N * Mc * ring_len;
                p.OH = 1; p.OW = ring_len; p.P = N * ring_len;
                p.fd_ohw = make_fastdiv(ring_len); p.fd_ow = make_fastdiv(ring_len);
                float* ring_buf = wsf + L.ring_off;
                p.dst0 = ring_buf; p.dst1 = nullptr; p.M0 = Mc;
                launch_igemm(p, st);
                if (p.ksplit > 1) nemar_sum_partials(p.part, p.part_stride, p.ksplit, ring_buf, p.part_stride, false, st);
                RingBand band;
                band.nrows = band.ncols = 0;
                for (int t = 0; t < H; ++t)
                    if ((t >= 1 && t <= pad) || (t <= H - 2 && t >= H - 1 - pad)) band.rows[band.nrows++] = t;
                for (int t = 0; t < W; ++t)
                    if ((t >= 1 && t <= pad) || (t <= W - 2 && t >= W - 1 - pad)) band.cols[band.ncols++] = t;
                const long long planes = (long long)N * Mc;
                const long long work = planes * ((long long)band.nrows * W + (long long)H * band.ncols);
                if (work > 0)
                    hipLaunchKernelGGL(ring_gather_kernel, dim3(nemar_stream_grid(work, 256)), dim3(256), 0, st,
                                       (const float*)ring_buf, gx0 ? gx0 : gx1, H, W, pad, ring_len, band, planes);
            }
        }
    if (fold && !folded) {
        const float* const add = (gx0 && !gx1) ? call.addend : nullptr;
        fold_padded(padded, gx0 ? gx0 : gx1, H, W, pad, total, add, st);
        if (add) call.addend_done = true;
    }
    }
    }
    NEMAR_CHECK_LAUNCH(what);
    return NEMAR_OK;
}

// ---- weight gradient.  Its scratch: per-split slabs of the fixed-order reduction (max over the routes the shape could take) ----
NEMAR_API size_t nemar_conv2d_bwd_weight_workspace(int N, int C, int H, int W, int K, int OH, int OW, int R, int S, int stride, int pad) {
    if (N <= 0 || C <= 0 || K <= 0 || OH <= 0 || OW <= 0 || R <= 0 || S <= 0) return 0;
    return sizeof(float) * plan_wgrad({N, C, 0, H, W, K, R, S, stride, pad, BORDER_ZERO, OH, OW}, ConvFacts::canonical()).total;
}

// gw[K][C][R][S] += d loss / d w, and (gb != NULL) gb[K] += sum_pixels gy   (always accumulate: the caller zero-fills once per optimizer step)
// Honours call.scratch, .src_max (x0), .src2_max (gy), .x_planes, .src2_planes and .bias_partials (the wide route); sets .bias_rode
static int conv2d_bwd_weight(ConvCall& call, const float* x0, int C0, const float* x1, int C1, const float* gy, float* gw,
                             float* gb, int N, int H, int W, int K, int OH, int OW, int R, int S, int stride,
                             int pad, int pad_mode, void* workspace, size_t ws_bytes, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(x0 && gy && gw, "conv2d_bwd_weight: null pointer");
    NEMAR_REQUIRE(C0 > 0 && C1 >= 0 && (C1 == 0 || x1), "conv2d_bwd_weight: bad channel split");
    NEMAR_REQUIRE(N > 0 && H > 0 && W > 0 && K > 0 && OH > 0 && OW > 0 && R > 0 && S > 0, "conv2d_bwd_weight: bad shape");
    NEMAR_REQUIRE(pad_mode == BORDER_ZERO || (pad < H && pad < W), "conv2d_bwd_weight: reflect pad too large");
    NEMAR_REQUIRE((long long)N * OH * OW < (1ll << 31) && (long long)(C0 + C1) * H * W < (1ll << 31),
                  "conv2d_bwd_weight: problem too large for 32-bit tile indexing");
    ConvFacts f = facts_of(call, nullptr, ACT_NONE, 0.f);
    f.part = g_deterministic != 0;
    f.gy_aligned = (reinterpret_cast<uintptr_t>(gy) & 15) == 0;
    f.part_aligned = (reinterpret_cast<uintptr_t>(workspace) & 15) == 0;
    const WgradPlan P = plan_wgrad({N, C0, C1, H, W, K, R, S, stride, pad, pad_mode, OH, OW}, f);
    float* part = nullptr;
    if (g_deterministic) {
        const size_t need = sizeof(float) * P.total;
        if (!workspace || ws_bytes < need) {
            nemar_set_error("conv2d_bwd_weight: workspace %zu < %zu", workspace ? ws_bytes : (size_t)0, need);
            return NEMAR_EWORKSPACE;
        }
        part = (float*)workspace;
    }
    hipStream_t st = (hipStream_t)stream;
    const int J = (C0 + C1) * R * S;
    const char* what = "conv2d_bwd_weight";
    g_last_route = P.route;
    switch (P.sub) {
    case WgradPlan::K7:
        if (!nemar_k7_wgrad(x0, gy, gw, gb, N, C0, H, W, K, pad_mode, part, st))      // (head: K <= 4 planes of gy, its own small reduction)
            bias_grad_slabs(gy, gb, part + P.bias_off, N, K, OH * OW, st);
        what = "conv2d_bwd_weight (7x7, 16-bit pipe)";
        break;
    case WgradPlan::NARROW:
        nemar_narrow_wgrad(x0, gy, gw, N, C0, H, W, K, R, pad, pad_mode, part, st);
        if (gb) bias_grad_slabs(gy, gb, part ? part + P.bias_off : nullptr, N, K, OH * OW, st);
        what = "conv2d_bwd_weight (narrow)";
        break;
    case WgradPlan::S16G:
        nemar_s16g_wgrad(x0, C0, x1, C1, gy, gw, gb, N, H, W, K, OH, OW, R, stride, pad_mode, part, g_dbg, st);
        what = "conv2d_bwd_weight (16-bit pipe, in-kernel split)";
        break;
    case WgradPlan::SPLIT16:
        call.bias_rode = gb && call.bias_partials;               // the producer's per-plane sums: reduced inside the slab-sum launch
        nemar_split16_wgrad(x0, gy, gw, N, C0, H, W, K, R, pad_mode == BORDER_REFLECT ? 1 : 0, call.scratch, part, g_xcd_map,
                            R == 3 ? call.src2_planes : nullptr, (R == 3 && pad_mode == BORDER_REFLECT) ? call.x_planes : nullptr,
                            call.src_max, call.src2_max, call.bias_rode ? call.bias_partials : nullptr, gb, st);
        if (gb && !call.bias_rode) bias_grad_slabs(gy, gb, part + P.bias_off, N, K, OH * OW, st);
        what = "conv2d_bwd_weight (split-16)";
        break;
    case WgradPlan::WGRAD2:
        nemar_wgrad2_launch(x0, C0, x1, C1, gy, gw, gb, N, H, W, K, OH, OW, R, S, stride, pad, pad_mode, g_wgrad_blocks,
                            g_wgrad != 2, g_dbg, part, st);
        what = "conv2d_bwd_weight (wide)";
        break;
    case WgradPlan::WGRAD2_PADDED_GY: {
        float* gyp = part + P.gyp_off;
        const long long total = (long long)N * K * P.ohv * OW;
        hipLaunchKernelGGL(pad_planes_kernel, dim3(nemar_stream_grid(total, 256)), dim3(256), 0, st, gy, gyp, OH * OW, P.ohv * OW, total);
        nemar_wgrad2_launch(x0, C0, x1, C1, gyp, gw, gb, N, H, W, K, P.ohv, OW, R, S, stride, pad, pad_mode, g_wgrad_blocks,
                            g_wgrad != 2, g_dbg, part, st);
        what = "conv2d_bwd_weight (wide, padded gy)";
        break;
    }
    case WgradPlan::LEGACY: {
        WgradParams p;
        p.src0 = x0; p.src1 = x1; p.C0 = C0; p.C1 = C1; p.Hs = H; p.Ws = W;
        p.gy = gy; p.K = K; p.OH = OH; p.OW = OW;
        p.gw = gw; p.gb = gb; p.J = J;
        p.N = N; p.P = N * OH * OW; p.sy = stride; p.sx = stride; p.R = R; p.S = S; p.pad = pad; p.border = pad_mode;
        p.fd_ohw = make_fastdiv(OH * OW); p.fd_ow = make_fastdiv(OW);
        p.dbg = g_dbg;
        p.pix_per_split = P.pix_per_split;
        p.part = part;
        p.partb = part ? part + P.bias_off : nullptr;
        const bool wide = K > 32;
        dim3 grid(nemar_cdiv(K, wide ? 128 : 32), nemar_cdiv(J, wide ? 128 : 256), P.splits), block(256);
        if (wide) hipLaunchKernelGGL((wgrad_kernel<2, 2, 2, 2>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((wgrad_kernel<1, 4, 1, 2>), grid, block, 0, st, p);
        if (part) nemar_sum_partials_pair(part, (long long)K * J, P.splits, gw, (long long)K * J, gb ? p.partb : nullptr, K, P.splits, gb, K, true, st);
    }
    }
    NEMAR_CHECK_LAUNCH(what);
    return NEMAR_OK;
}

NEMAR_API int nemar_last_route(void) { return g_last_route; }
NEMAR_API int nemar_config_epoch(void) { return g_config_epoch; }      // product build: always 0 (no switch can change)

#ifdef NEMAR_AB
// Measurement switches (include/nemar_hip_ab.h): only libnemar_hip_ab.so has these entry points.
NEMAR_API int nemar_tune_ptr(void* p) { g_tl = (long long*)p; return NEMAR_OK; }

NEMAR_API int nemar_tune(int key, int value) {
    ++g_config_epoch;
    if (key == 0) { g_cfg128 = value; return NEMAR_OK; }
    if (key == 1) { g_lds_pad = value; return NEMAR_OK; }
    if (key == 2) { g_dbg = value; return NEMAR_OK; }
    if (key == 3) { g_narrow = value; return NEMAR_OK; }
    if (key == 4) { g_wgrad = value; return NEMAR_OK; }
    if (key == 6) { g_min_blocks = value > 0 ? value : 384; return NEMAR_OK; }
    if (key == 14) { g_deterministic = value != 0; return NEMAR_OK; }
    if (key == 8) { g_reflect_aux = value != 0; return NEMAR_OK; }
    if (key == 15) { g_xcd_map = value != 0; return NEMAR_OK; }
    if (key == 20) { g_split16 = value != 0; return NEMAR_OK; }
    if (key == 24) { g_s16g = value != 0; return NEMAR_OK; }
    if (key == 25) { g_s16g_min_mmac = value < 0 ? 0 : value; return NEMAR_OK; }
    if (key == 26) { g_s16g_wgrad_first = value != 0; return NEMAR_OK; }
    if (key == 27) { nemar_s16g_tune(0, value); return NEMAR_OK; }
    if (key == 29) { g_s16g_wgrad = value != 0; return NEMAR_OK; }
    if (key == 31) { nemar_norm_planes_debug(value); return NEMAR_OK; }
    if (key == 32) { g_split16_ring3 = value != 0; return NEMAR_OK; }
    if (key == 33) { g_k7 = value != 0; return NEMAR_OK; }
    if (key == 36) { g_split_act = value != 0; return NEMAR_OK; }
    if (key == 43) { g_fold_small = value != 0; return NEMAR_OK; }      // tiny stride-1 reflect data gradients: padded domain + sum-and-fold (1) / interior + ring (0)
    if (key == 37) { g_lds_claim = value; return NEMAR_OK; }      // kernel families whose workgroups claim the whole CU's LDS (common.h)
    if (key == 38) { g_wg_xreg = value != 0; return NEMAR_OK; }   // wide 3x3 weight gradient: X pieces through registers
    if (key == 39) { g_split16_ksplit_cap = value < 1 ? 1 : (value > 8 ? 8 : value); return NEMAR_OK; }      // most reduction runs per tile of the wide-layer kernel
    if (key == 45) { g_overlap_per_lane = value != 0; return NEMAR_OK; }  // nemar_label_overlap: every lane adds to the LDS histogram itself (1) / wave-aggregated adds (0, default)
    if (key == 46) { g_histogram_per_lane = value != 0; return NEMAR_OK; }  // nemar_joint_histogram: every lane adds to the LDS table itself (1, default) / wave-aggregated adds (0)
    if (key == 44) { g_register_vec4 = value != 0; return NEMAR_OK; }   // nemar_warp_resampled_fwd: 4 pixels per lane + 16-byte stores (1) / one pixel per lane (0, default)
    if (key == 47) { g_pointwise_rows = value != 0; return NEMAR_OK; }  // row-vector forms of pool backward / 2x resize / reflect fold (1, default) / one element per lane (0)
    if (key == 35) { g_dual_gy = value != 0; return NEMAR_OK; }
    if (key == 34) { nemar_split16_wgrad_tune(value); return NEMAR_OK; }      // wide weight gradient: 1 one gy copy (default), 0 KS shifted copies
    if (key == 30) { g_s16g_fold = value != 0; return NEMAR_OK; }
    if (key == 28) { nemar_s16g_tune(1, value); return NEMAR_OK; }
    if (key == 40) { nemar_s16g_tune(2, value); return NEMAR_OK; }
    if (key == 42) { nemar_s16g_tune(4, value); return NEMAR_OK; }      // class-fused stride-2 data gradients (conv_s16g.hip CF): 0 off, 1 on (default), 2 on + required
    if (key == 41) { nemar_s16g_tune(3, value); return NEMAR_OK; }      // ... while the grid keeps this many workgroups (256)      // most channel blocks per s16g workgroup (4; 1 = one workgroup per block)
    if (key == 23) { g_split16_min_mmac = value < 0 ? 0 : value; return NEMAR_OK; }
    if (key == 21) { g_split16_variant = value == 3 ? 3 : 4; return NEMAR_OK; }      // packed images made under the other setting are stale
    if (key == 16) { g_adir = value != 0; return NEMAR_OK; }
    if (key == 17) { g_mt8 = value; return NEMAR_OK; }
    if (key == 19) { g_narrow_fwd4 = value != 0; return NEMAR_OK; }
    if (key == 18) { g_ring = (value == 4 || value == 5) ? value : 3; return NEMAR_OK; }
    if (key == 12) { g_ksplit = value != 0; return NEMAR_OK; }
    if (key == 11) { g_nl4_scalar = value != 0; return NEMAR_OK; }
    if (key == 10) { g_deep64 = value != 0; return NEMAR_OK; }
    if (key == 7) { g_ws2_mt = (value == 1 || value == 2 || value == 4) ? value : 0; return NEMAR_OK; }
    if (key == 5) { g_wgrad_blocks = value > 0 ? value : 512; return NEMAR_OK; }
    nemar_set_error("nemar_tune: unknown key %d", key);
    return NEMAR_EINVAL;
}
#endif  // NEMAR_AB

// the data-gradient plan of a layer's usual call (ConvFacts::canonical), for the queries below
static DgradPlan usual_dgrad(int N, int C, int H, int W, int K, int R, int S, int stride, int pad, int pad_mode) {
    DgradPlan P{};
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || K <= 0 || R <= 0 || S <= 0 || stride < 1) return P;      // (nothing to plan)
    return plan_dgrad({N, C, 0, H, W, K, R, S, stride, pad, pad_mode}, ConvFacts::canonical());
}
static bool fusable(const DgradPlan& P) { return P.gy_planes_need != 0 && P.split16_ksplit == 1; }

// Scratch bytes nemar_conv2d_fwd / nemar_conv2d_bwd_data want for this layer (0: the layer never uses the arena)
NEMAR_API size_t nemar_conv2d_scratch(int N, int H, int W, int K, int C, int R, int S, int stride, int pad) {
    if (N <= 0 || H <= 0 || W <= 0 || K <= 0 || C <= 0) return 0;
    return plan_arena_bytes({N, C, 0, H, W, K, R, S, stride, pad, BORDER_ZERO});
}

// bytes of the gy planes the data-gradient call can leave behind for the weight-gradient call (0: they do not both run on the wide route)
NEMAR_API size_t nemar_conv2d_gy_planes_bytes(int N, int C, int H, int W, int K, int R, int S, int stride, int pad, int pad_mode) {
    return usual_dgrad(N, C, H, W, K, R, S, stride, pad, pad_mode).gy_planes_need;
}

// 1 when the data-gradient call honours addend / out_max_words and both gradient calls take planes: the wide 3x3 route, reduction unsplit
NEMAR_API int nemar_conv2d_bwd_data_fusable(int N, int C, int H, int W, int K, int R, int S, int stride, int pad, int pad_mode) {
    return fusable(usual_dgrad(N, C, H, W, K, R, S, stride, pad, pad_mode)) ? 1 : 0;
}

// 1 when the usual data-gradient call adds nemar_conv_extras.addend: the wide route's fused epilogue, or a stride-1 reflect layer whose data
// gradient ends with a fold pass.  Not a layer any operator's wide route may take, nor a 7x7 layer (open items).
NEMAR_API int nemar_conv2d_bwd_data_addend_ok(int N, int C, int H, int W, int K, int R, int S, int stride, int pad, int pad_mode) {
    const DgradPlan P = usual_dgrad(N, C, H, W, K, R, S, stride, pad, pad_mode);
    if (fusable(P)) return 1;
    if (pad_mode != BORDER_REFLECT || pad <= 0 || stride != 1 || pad >= H || pad >= W || R != S || R == 7) return 0;
    return (P.fold16 || P.fold) && plan_arena_bytes({N, C, 0, H, W, K, R, S, stride, pad, BORDER_ZERO}) == 0 ? 1 : 0;
}

// 1 when the last nemar_conv2d_bwd_data_ex call on this thread filled its gy_planes_out buffer (the route it took supports it): only then
// may the buffer be handed to nemar_conv2d_bwd_weight_ex as src2_planes
NEMAR_API int nemar_last_gy_planes(void) { return g_last_gy_planes; }

// ---- the C-ABI entry points of the three operators.  The side inputs of the wide-layer route (scratch arena, per-sample max words, producer-
// written planes) travel WITH the call (nemar_conv_extras): each _ex entry copies the members its operator documents into the ConvCall the
// operator runs with; the plain entries run with an empty one.
namespace {
// what every operator takes: the arena and the source's max words
ConvCall call_from(const nemar_conv_extras* ex) {
    ConvCall call;
    if (!ex) return call;
    if (ex->scratch && ex->scratch_bytes) { call.scratch = ex->scratch; call.scratch_bytes = ex->scratch_bytes; }
    if (ex->src_max_words && ex->src_max_count > 0) call.src_max = {(const unsigned*)ex->src_max_words, ex->src_max_count};
    return call;
}
}  // namespace

NEMAR_API int nemar_conv2d_fwd(const float* x0, int C0, const float* x1, int C1, const float* w, const float* bias,
                               float* y, int N, int H, int W, int K, int R, int S, int stride, int pad, int pad_mode,
                               int act, float slope, void* workspace, size_t ws_bytes, int prepacked, void* stream) {
    ConvCall call;
    return conv2d_fwd(call, x0, C0, x1, C1, w, bias, y, N, H, W, K, R, S, stride, pad, pad_mode, act, slope, workspace, ws_bytes, prepacked, stream);
}

NEMAR_API int nemar_conv2d_fwd_ex(const float* x0, int C0, const float* x1, int C1, const float* w, const float* bias, float* y, int N,
                                  int H, int W, int K, int R, int S, int stride, int pad, int pad_mode, int act, float slope,
                                  void* workspace, size_t ws_bytes, int prepacked, void* stream, const nemar_conv_extras* extras) {
    ConvCall call = call_from(extras);
    if (extras) { call.src_planes = extras->src_planes; call.src_planes_kind = SPLIT16_REFLECT; }      // (a forward producer's planes)
    return conv2d_fwd(call, x0, C0, x1, C1, w, bias, y, N, H, W, K, R, S, stride, pad, pad_mode, act, slope, workspace, ws_bytes, prepacked, stream);
}

NEMAR_API int nemar_conv2d_bwd_data(const float* gy, const float* w, const float* bias, int act, float slope,
                                    float* gx0, int C0, float* gx1, int C1, int N, int H, int W, int K, int OH, int OW,
                                    int R, int S, int stride, int pad, int pad_mode, void* workspace, size_t ws_bytes,
                                    int prepacked, void* stream) {
    ConvCall call;
    return conv2d_bwd_data(call, gy, w, bias, act, slope, gx0, C0, gx1, C1, N, H, W, K, OH, OW, R, S, stride, pad, pad_mode, workspace, ws_bytes,
                           prepacked, stream);
}

NEMAR_API int nemar_conv2d_bwd_data_ex(const float* gy, const float* w, const float* bias, int act, float slope, float* gx0, int C0,
                                       float* gx1, int C1, int N, int H, int W, int K, int OH, int OW, int R, int S, int stride, int pad,
                                       int pad_mode, void* workspace, size_t ws_bytes, int prepacked, void* stream,
                                       const nemar_conv_extras* extras) {
    ConvCall call = call_from(extras);
    if (extras) {
        // (src_planes: the data-gradient planes of gy nemar_instnorm_bwd_planes wrote, in the content of THIS layer's padding)
        call.src_planes = extras->src_planes;
        call.src_planes_kind = pad_mode == BORDER_REFLECT ? SPLIT16_DGRAD_REFLECT : SPLIT16_ZERO;
        call.gy_planes_out = extras->gy_planes_out; call.gy_planes_bytes = extras->gy_planes_bytes;
        call.addend = extras->addend; call.out_max = extras->out_max_words;
    }
    const int rc = conv2d_bwd_data(call, gy, w, bias, act, slope, gx0, C0, gx1, C1, N, H, W, K, OH, OW, R, S, stride, pad, pad_mode, workspace,
                                   ws_bytes, prepacked, stream);
    g_last_gy_planes = call.gy_planes_written ? 1 : 0;
    if (rc == NEMAR_OK && ((call.addend && !call.epilogue_fused && !call.addend_done) || (call.out_max && !call.epilogue_fused))) {
        nemar_set_error("conv2d_bwd_data_ex: this layer's route has no fused epilogue (addend / out_max_words): ask nemar_conv2d_bwd_data_fusable / "
                        "nemar_conv2d_bwd_data_addend_ok first");
        return NEMAR_EINVAL;
    }
    return rc;
}

NEMAR_API int nemar_conv2d_bwd_weight(const float* x0, int C0, const float* x1, int C1, const float* gy, float* gw,
                                      float* gb, int N, int H, int W, int K, int OH, int OW, int R, int S, int stride,
                                      int pad, int pad_mode, void* workspace, size_t ws_bytes, void* stream) {
    ConvCall call;
    return conv2d_bwd_weight(call, x0, C0, x1, C1, gy, gw, gb, N, H, W, K, OH, OW, R, S, stride, pad, pad_mode, workspace, ws_bytes, stream);
}

NEMAR_API int nemar_conv2d_bwd_weight_ex(const float* x0, int C0, const float* x1, int C1, const float* gy, float* gw, float* gb, int N,
                                         int H, int W, int K, int OH, int OW, int R, int S, int stride, int pad, int pad_mode,
                                         void* workspace, size_t ws_bytes, void* stream, const nemar_conv_extras* extras) {
    ConvCall call = call_from(extras);
    if (extras) {
        if (extras->src2_max_words && extras->src2_max_count > 0) call.src2_max = {(const unsigned*)extras->src2_max_words, extras->src2_max_count};
        // (src_planes: the weight gradient's X planes of x0 nemar_instnorm_fwd_planes wrote — pixel-major, not the channel-blocked kind)
        call.x_planes = extras->src_planes;
        call.src2_planes = extras->src2_planes;
        call.bias_partials = extras->bias_partials;
    }
    const int rc = conv2d_bwd_weight(call, x0, C0, x1, C1, gy, gw, gb, N, H, W, K, OH, OW, R, S, stride, pad, pad_mode, workspace, ws_bytes, stream);
    if (rc == NEMAR_OK && call.bias_partials && gb && !call.bias_rode) {
        nemar_set_error("conv2d_bwd_weight_ex: bias_partials are only taken on the wide route (nemar_conv2d_bwd_data_fusable); gb was reduced from gy");
        return NEMAR_EINVAL;
    }
    return rc;
}

// max |t| (finite elements) per sample of a tensor, for callers that feed the same tensor to several split-16 convolution calls
// (forward + weight gradient take x, data + weight gradient take gy): computed once, passed as nemar_conv_extras.src_max_words, it replaces
// the max pass inside each call.  nemar_absmax = one sample of n elements.
NEMAR_API int nemar_absmax(const float* t, long long n, void* out_word, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(t && out_word && n > 0, "absmax: null pointer");
    nemar_split16_absmax(t, 1, n, out_word, (hipStream_t)stream);
    NEMAR_CHECK_LAUNCH("absmax");
    return NEMAR_OK;
}

NEMAR_API int nemar_absmax_samples(const float* t, int samples, long long per_sample, void* out_words, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(t && out_words && samples > 0 && samples <= 65535 && per_sample > 0, "absmax_samples: bad arguments");
    nemar_split16_absmax(t, samples, per_sample, out_words, (hipStream_t)stream);
    NEMAR_CHECK_LAUNCH("absmax_samples");
    return NEMAR_OK;
}

// bench.py's roofline entry: time the main kernel (igemm_split16_kernel) of every forward / data-gradient call of the wide 3x3
// layers with HIP events recorded on the launch stream, between enable and read
NEMAR_API int nemar_kernel_timer(int enable) {
    nemar_split16_timer(enable);
    return NEMAR_OK;
}

NEMAR_API int nemar_kernel_timer_read(double* total_ms, double* total_flop, int* launches) {
    NEMAR_REQUIRE(total_ms && total_flop && launches, "kernel_timer_read: null pointer");
    *launches = nemar_split16_timer_read(total_ms, total_flop);
    return NEMAR_OK;
}

NEMAR_API size_t nemar_bias_grad_workspace(int N, int C, int HW) {
    if (N <= 0 || C <= 0 || HW <= 0) return 0;
    return sizeof(float) * (size_t)N * nemar_cdiv(HW, BIAS_CHUNK) * C;
}

// gb[C] += sum over N and the plane of g [N,C,HW]   (bias gradient; also ConvTranspose2d's)
NEMAR_API int nemar_bias_grad(const float* g, float* gb, int N, int C, int HW, void* workspace, size_t ws_bytes,
                              void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(g && gb && N > 0 && C > 0 && HW > 0, "bias_grad: bad arguments");
    if (g_deterministic && (!workspace || ws_bytes < nemar_bias_grad_workspace(N, C, HW))) {
        nemar_set_error("bias_grad: workspace %zu < %zu", workspace ? ws_bytes : (size_t)0, nemar_bias_grad_workspace(N, C, HW));
        return NEMAR_EWORKSPACE;
    }
    bias_grad_slabs(g, gb, g_deterministic ? (float*)workspace : nullptr, N, C, HW, (hipStream_t)stream);
    NEMAR_CHECK_LAUNCH("bias_grad");
    return NEMAR_OK;
}
