// MIND, the modality-independent neighbourhood descriptor (Heinrich et al. 2012), as a training loss (DESIGN.md "MIND"), forward and
// backward.  Not a call site of the reference, whose image terms compare two images of ONE modality; this one compares descriptors.
//   x [N,Cx,H,W], y [N,Cy,H,W]; each image enters through its channel mean g(q) = (1/C) sum_c img[n,c,q] (as in similarity.hip).
//   patch 3 or 5 (radius p), dil 1 or 2, the four offsets s = (0,-dil), (0,+dil), (-dil,0), (+dil,0) as (dy, dx), in that order
//   E_s(q) = (g(q) - g(clamp(q + s)))^2, D_s(u) = sum_{q in Omega(u)} E_s(q) / n(u)  (Omega: the in-image part of the patch, no padding)
//   V = (D_0 + D_1 + D_2 + D_3) / 4,  m_s = exp(-D_s / (V + eps)),  dm = (1/4) sum_s (m_s^x - m_s^y)^2,  loss = factor * mean dm
// without the division by max_s m_s (a kink wherever two D_s tie).  exp is expf, the library routine (about 1 ulp), not __expf.
//
// Tiling: BOTH kernels work on 32 x 16 tiles (MD_TW x MD_TH), one workgroup of 256 lanes per tile and sample, two pixels per lane.
//
// Staging (mind_stage): the channel means of a tile plus a halo go to LDS, the channels summed on the way in (the mean planes never
// exist in HBM), at CLAMPED coordinates: g(clamp(q + s)) is then the staged value at q + s.  The staged columns are whole quads (the
// halo rounded up to 4: 40 columns forward, 40 or 48 backward); a quad inside the row is one 16-byte load per channel where W % 4 == 0
// and the image's base is 16-byte aligned, four clamped scalar loads otherwise.
// Row sums (mind_row_sums): for every row that a descriptor of the region reads, the sums of E_s over the 2p + 1 columns, E_s formed
// on the fly from the staged means (0 for q outside the image), a lane per column: stride 1 across the lanes.  D_s is then 2p + 1
// additions down a column (mind_desc).  Every patch is summed directly, in a fixed order.
//
// Forward: halo p + dil.  A lane forms dm of two pixels, writes dm_map where asked; the tile's sum goes through the lanes' partials, the
// xor tree of each wave and the waves in ascending order into one record per workgroup; mind_finish_kernel merges the records in a
// fixed order.  No atomics: bitwise repeatable.  A dm passes through at most 2 (lane) + 6 (wave) + 3 (workgroup) additions in the tile
// kernel and ceil(records / 256) + 6 + 4 in the finish, which ends with sum / (N H W) in double, rounded once, and its float product
// with factor.
//
// Backward: ONE launch, a pure gather, no workspace.  The tile's pixels t hear from e_s on the tile + dil, e_s from b_s on the tile +
// dil + p, b_s from the descriptors there, those from E on + p more and E from g on + dil more: a halo of 2 (p + dil) <= 8, the
// staged means at most 32 x 48 per image.  Each lane forms the descriptors and b_s / n of up to four pixels u in registers (towards x
// and, with gy, towards y), the workgroup writes them over the dead row sums, box-sums them by a row and a column pass into e_s and
// applies
//   dL/dg(t) = sum_s [ 2 e_s(t) (g(t) - g(clamp(t + s))) - sum_{q in image : clamp(q + s) = t} 2 e_s(q) (g(q) - g(t)) ]
// where q = t - s in the interior and, for t on the border that the clamp maps onto, also the q up to dil - 1 further in (q = t itself
// adds nothing).  Every channel of gx gets gscale * factor / (4 N H W Cx) times that; gy likewise, in a second round over the same LDS.
// Static LDS: 48 KiB at patch 5, dil 2 (MindGeo has the sums), so two workgroups fit a CU.
#include "common.h"
#include <math.h>

namespace {

constexpr int MD_THREADS = 256;
constexpr int MD_TW = 32, MD_TH = 16;      // the tile of both kernels

template <int P, int DIL, bool BWD>
struct MindGeo {
    static constexpr int HALO = BWD ? 2 * (P + DIL) : P + DIL;      // of the staged means
    static constexpr int HP = (HALO + 3) & ~3;                      // ... in columns: whole quads
    static constexpr int GW = MD_TW + 2 * HP, GH = MD_TH + 2 * HALO;
    static constexpr int DR = BWD ? P + DIL : 0;                    // the descriptors' region: the tile + DR
    static constexpr int DW = MD_TW + 2 * DR, DH = MD_TH + 2 * DR;
    static constexpr int RH = DH + 2 * P;                           // rows of the row-sum planes
    static constexpr int G = GH * GW, RS = 8 * RH * DW;             // floats: one image's means; the row sums of both images
    // backward: e_s on the tile + dil; b_s / n, its row sums and e_s lie over the dead row sums
    static constexpr int EW = MD_TW + 2 * DIL, EH = MD_TH + 2 * DIL;
    static constexpr int BN = 4 * DH * DW, CROW = 4 * DH * EW, E = 4 * EH * EW;
    static constexpr int ITEMS = (DH * DW + MD_THREADS - 1) / MD_THREADS;      // descriptor pixels per lane
    static_assert(!BWD || (BN + CROW <= RS && E <= BN), "b / n, its row sums and e fit the row sums' place");
    static_assert((2 * G + RS + 16) * 4 <= 64 * 1024, "static LDS");
};

// |Omega| along one axis: the in-image pixels within p of i
__device__ __forceinline__ int mind_count(int i, int n, int p) { return min(i + p, n - 1) - max(i - p, 0) + 1; }

// g [GH x GW] = the channel mean of sample `img` [C,H,W] at clamp(gy0 + r), clamp(gx0 + c); gx0 is a multiple of 4
template <int GW, int GH>
__device__ __forceinline__ void mind_stage(float* g, const float* __restrict__ img, int C, int gx0, int gy0, int H, int W, bool vec, int tid) {
    constexpr int QW = GW / 4;
    const size_t plane = (size_t)H * W;
    const float fc = (float)C;
    for (int e = tid; e < GH * QW; e += MD_THREADS) {
        const int r = e / QW, qc = e - r * QW;
        const int h = min(max(gy0 + r, 0), H - 1), w = gx0 + 4 * qc;
        const float* row = img + (size_t)h * W;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        if (vec && w >= 0 && w + 3 < W) {
            for (int c = 0; c < C; ++c) {
                const float4 v = *reinterpret_cast<const float4*>(row + c * plane + w);
                a0 += v.x;
                a1 += v.y;
                a2 += v.z;
                a3 += v.w;
            }
        } else {
            const int w0 = min(max(w, 0), W - 1), w1 = min(max(w + 1, 0), W - 1), w2 = min(max(w + 2, 0), W - 1), w3 = min(max(w + 3, 0), W - 1);
            for (int c = 0; c < C; ++c) {
                const float* p = row + c * plane;
                a0 += p[w0];
                a1 += p[w1];
                a2 += p[w2];
                a3 += p[w3];
            }
        }
        float* o = g + r * GW + 4 * qc;
        o[0] = a0 / fc;
        o[1] = a1 / fc;
        o[2] = a2 / fc;
        o[3] = a3 / fc;
    }
}

// rs [4][RH x DW]: the sums over the 2p + 1 columns around (ry0 + r, dx0 + c) of E_s, for the means g staged from (gy0, gx0)
template <int P, int DIL, int GW, int DW, int RH>
__device__ __forceinline__ void mind_row_sums(const float* g, float* rs, int dx0, int ry0, int gx0, int gy0, int H, int W, int tid) {
    for (int e = tid; e < RH * DW; e += MD_THREADS) {
        const int r = e / DW, c = e - r * DW;
        const int h = ry0 + r, w = dx0 + c;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        if ((unsigned)h < (unsigned)H) {
            const float* q = g + (h - gy0) * GW + (w - P - gx0);
#pragma unroll
            for (int j = 0; j <= 2 * P; ++j) {
                const bool in = (unsigned)(w - P + j) < (unsigned)W;
                const float v = q[j];
                const float d0 = v - q[j - DIL], d1 = v - q[j + DIL], d2 = v - q[j - DIL * GW], d3 = v - q[j + DIL * GW];
                s0 += in ? d0 * d0 : 0.f;
                s1 += in ? d1 * d1 : 0.f;
                s2 += in ? d2 * d2 : 0.f;
                s3 += in ? d3 * d3 : 0.f;
            }
        }
        rs[e] = s0;
        rs[RH * DW + e] = s1;
        rs[2 * RH * DW + e] = s2;
        rs[3 * RH * DW + e] = s3;
    }
}

// D_s, m_s and V + eps of region pixel (r, c), from one image's four row-sum planes; n = |Omega|
template <int P, int DW, int RH>
__device__ __forceinline__ void mind_desc(const float* rs, int r, int c, float n, float eps, float (&D)[4], float (&m)[4], float& ve) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const float* q = rs + s * RH * DW + r * DW + c;
        float t = 0.f;
#pragma unroll
        for (int j = 0; j <= 2 * P; ++j) t += q[j * DW];
        D[s] = t / n;
    }
    ve = (((D[0] + D[1]) + D[2]) + D[3]) * 0.25f + eps;
#pragma unroll
    for (int s = 0; s < 4; ++s) m[s] = expf(-D[s] / ve);
}

template <int P, int DIL>
__global__ __launch_bounds__(MD_THREADS) void mind_fwd_kernel(const float* __restrict__ x, int Cx, const float* __restrict__ y, int Cy, float eps,
                                                              float* __restrict__ partial, float* __restrict__ dm_map, int tiles_x, int H,
                                                              int W, int vecx, int vecy) {
    using G = MindGeo<P, DIL, false>;
    __shared__ float gl[2 * G::G];
    __shared__ float rs[G::RS];
    __shared__ float red[16];
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * MD_TW, y0 = ty * MD_TH;
    const int gx0 = x0 - G::HP, gy0 = y0 - G::HALO;
    const size_t plane = (size_t)H * W, n = blockIdx.z;
    mind_stage<G::GW, G::GH>(gl, x + n * Cx * plane, Cx, gx0, gy0, H, W, vecx != 0, tid);
    mind_stage<G::GW, G::GH>(gl + G::G, y + n * Cy * plane, Cy, gx0, gy0, H, W, vecy != 0, tid);
    __syncthreads();
    mind_row_sums<P, DIL, G::GW, G::DW, G::RH>(gl, rs, x0, y0 - P, gx0, gy0, H, W, tid);
    mind_row_sums<P, DIL, G::GW, G::DW, G::RH>(gl + G::G, rs + 4 * G::RH * G::DW, x0, y0 - P, gx0, gy0, H, W, tid);
    __syncthreads();

    float sum = 0.f;
    constexpr int ROWS = MD_THREADS / MD_TW, RUNS = MD_TH / ROWS;      // a lane owns one pixel in each of RUNS rows
#pragma unroll
    for (int i = 0; i < RUNS; ++i) {
        const int r = tid / MD_TW + ROWS * i, c = tid % MD_TW;
        const int h = y0 + r, w = x0 + c;
        if (h >= H || w >= W) continue;
        const float cnt = (float)(mind_count(h, H, P) * mind_count(w, W, P));
        float Dx[4], mx[4], Dy[4], my[4], vex, vey;
        mind_desc<P, G::DW, G::RH>(rs, r, c, cnt, eps, Dx, mx, vex);
        mind_desc<P, G::DW, G::RH>(rs + 4 * G::RH * G::DW, r, c, cnt, eps, Dy, my, vey);
        float dm = 0.f;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float d = mx[s] - my[s];
            dm += d * d;
        }
        dm *= 0.25f;
        if (dm_map) dm_map[n * plane + (size_t)h * W + w] = dm;
        sum += dm;
    }
    // the workgroup's record, in thread 0: the xor tree of each wave, then the waves in ascending order
    sum = wave_sum(sum);
    const int lane = tid & 63, wid = tid >> 6;
    if (lane == 0) red[wid] = sum;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < MD_THREADS / 64; ++i) sum += red[i];
        partial[n * gridDim.x + blockIdx.x] = sum;
    }
}

// loss[0] (+)= factor * sum / M: thread t takes records t, t + 256, ... in ascending order, then the fixed workgroup tree; sum / M in
// double, rounded to float once, then the float product with factor
__global__ __launch_bounds__(256) void mind_finish_kernel(const float* __restrict__ partial, long long total, float factor, double M,
                                                          int accumulate, float* __restrict__ loss) {
    __shared__ float red[16];
    float acc = 0.f;
    for (long long i = threadIdx.x; i < total; i += 256) acc += partial[i];
    const float t = block_sum(acc, red);
    if (threadIdx.x == 0) loss[0] = (accumulate ? loss[0] : 0.f) + factor * (float)((double)t / M);
}

template <int P, int DIL, bool GY>
__global__ __launch_bounds__(MD_THREADS) void mind_bwd_kernel(const float* __restrict__ x, int Cx, const float* __restrict__ y, int Cy, float eps,
                                                              const float* __restrict__ gscale, float scale_x, float scale_y,
                                                              float* __restrict__ gx, float* __restrict__ gy, int accumulate, int tiles_x,
                                                              int H, int W, int vecx, int vecy) {
    using G = MindGeo<P, DIL, true>;
    constexpr int DW = G::DW, DH = G::DH, RH = G::RH, GW = G::GW, EW = G::EW, EH = G::EH;
    __shared__ float gl[2 * G::G];
    __shared__ float work[G::RS];
    float* bn = work;                 // b_s / n on the descriptors' region
    float* crow = work + G::BN;       // its sums over 2p + 1 columns
    float* es = work;                 // e_s (over bn, once crow is made)
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * MD_TW, y0 = ty * MD_TH;
    const int gx0 = x0 - G::HP, gy0 = y0 - G::HALO;
    const size_t plane = (size_t)H * W, n = blockIdx.z;
    mind_stage<GW, G::GH>(gl, x + n * Cx * plane, Cx, gx0, gy0, H, W, vecx != 0, tid);
    mind_stage<GW, G::GH>(gl + G::G, y + n * Cy * plane, Cy, gx0, gy0, H, W, vecy != 0, tid);
    __syncthreads();
    mind_row_sums<P, DIL, GW, DW, RH>(gl, work, x0 - G::DR, y0 - G::DR - P, gx0, gy0, H, W, tid);
    mind_row_sums<P, DIL, GW, DW, RH>(gl + G::G, work + 4 * RH * DW, x0 - G::DR, y0 - G::DR - P, gx0, gy0, H, W, tid);
    __syncthreads();

    // b_s / n of up to ITEMS pixels u, in registers (0 outside the image: the box sums run over the in-image u only); a_s without the
    // constant factor / (4 N H W), which the last line applies
    constexpr int NIMG = GY ? 2 : 1;
    float b[NIMG][G::ITEMS][4];
#pragma unroll
    for (int i = 0; i < G::ITEMS; ++i) {
        const int e = tid + MD_THREADS * i;
#pragma unroll
        for (int k = 0; k < NIMG; ++k)
#pragma unroll
            for (int s = 0; s < 4; ++s) b[k][i][s] = 0.f;
        if (e >= DH * DW) continue;
        const int r = e / DW, c = e - r * DW;
        const int h = y0 - G::DR + r, w = x0 - G::DR + c;
        if ((unsigned)h >= (unsigned)H || (unsigned)w >= (unsigned)W) continue;
        const float cnt = (float)(mind_count(h, H, P) * mind_count(w, W, P));
        float Dx[4], mx[4], Dy[4], my[4], vex, vey;
        mind_desc<P, DW, RH>(work, r, c, cnt, eps, Dx, mx, vex);
        mind_desc<P, DW, RH>(work + 4 * RH * DW, r, c, cnt, eps, Dy, my, vey);
        float am_x[4], am_y[4], tx_ = 0.f, ty_ = 0.f;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float a = 2.f * (mx[s] - my[s]);
            am_x[s] = a * mx[s];
            am_y[s] = -(a * my[s]);
            tx_ += am_x[s] * Dx[s];
            ty_ += am_y[s] * Dy[s];
        }
        const float cx_ = tx_ / (4.f * (vex * vex)), cy_ = ty_ / (4.f * (vey * vey));
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            b[0][i][s] = (cx_ - am_x[s] / vex) / cnt;
            if (GY) b[NIMG - 1][i][s] = (cy_ - am_y[s] / vey) / cnt;
        }
    }
    const float gs = gscale[0];
    constexpr int ROWS = MD_THREADS / MD_TW, RUNS = MD_TH / ROWS;
#pragma unroll
    for (int k = 0; k < NIMG; ++k) {
        __syncthreads();      // every row sum has been read (k = 1: every e_s of the first round)
#pragma unroll
        for (int i = 0; i < G::ITEMS; ++i) {
            const int e = tid + MD_THREADS * i;
            if (e >= DH * DW) continue;
#pragma unroll
            for (int s = 0; s < 4; ++s) bn[s * DH * DW + e] = b[k][i][s];
        }
        __syncthreads();
        // the box, horizontally: for every row of the descriptors' region, the columns of the tile + dil
        for (int e = tid; e < DH * EW; e += MD_THREADS) {
            const int r = e / EW, c = e - r * EW;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float* q = bn + s * DH * DW + r * DW + c;
                float t = 0.f;
#pragma unroll
                for (int j = 0; j <= 2 * P; ++j) t += q[j];
                crow[s * DH * EW + e] = t;
            }
        }
        __syncthreads();
        // ... vertically: e_s on the tile + dil
        for (int e = tid; e < EH * EW; e += MD_THREADS) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float* q = crow + s * DH * EW + e;
                float t = 0.f;
#pragma unroll
                for (int j = 0; j <= 2 * P; ++j) t += q[j * EW];
                es[s * EH * EW + e] = t;
            }
        }
        __syncthreads();
        // the gradient towards the mean, and every channel's share of it
        const float* g = gl + k * G::G;
        float* out = k == 0 ? gx : gy;
        const int C = k == 0 ? Cx : Cy;
        const float scale = gs * (k == 0 ? scale_x : scale_y);
#pragma unroll
        for (int i = 0; i < RUNS; ++i) {
            const int r = tid / MD_TW + ROWS * i, c = tid % MD_TW;
            const int h = y0 + r, w = x0 + c;
            if (h >= H || w >= W) continue;
            const int gi = (r + G::HALO) * GW + c + G::HP, ei = (r + DIL) * EW + c + DIL;
            const float gt = g[gi];
            float acc = 0.f;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int sy = s == 2 ? -1 : s == 3 ? 1 : 0, sx = s == 0 ? -1 : s == 1 ? 1 : 0;
                const float* ep = es + s * EH * EW;
                const bool edge = s == 0 ? w == 0 : s == 1 ? w == W - 1 : s == 2 ? h == 0 : h == H - 1;
                acc += 2.f * ep[ei] * (gt - g[gi + DIL * (sy * GW + sx)]);
#pragma unroll
                for (int d = 1; d <= DIL; ++d) {      // the q with clamp(q + s) = t: t - s, and on the border the nearer ones too
                    const int qh = h - sy * d, qw = w - sx * d;
                    const bool on = (unsigned)qh < (unsigned)H && (unsigned)qw < (unsigned)W && (d == DIL || edge);
                    const float v = 2.f * ep[ei - d * (sy * EW + sx)] * (g[gi - d * (sy * GW + sx)] - gt);
                    acc -= on ? v : 0.f;
                }
            }
            const float val = scale * acc;
            float* o = out + n * C * plane + (size_t)h * W + w;
            for (int ch = 0; ch < C; ++ch) {
                if (accumulate) o[ch * plane] += val; else o[ch * plane] = val;
            }
        }
    }
}

bool mind_cfg_ok(int patch, int dil) { return (patch == 3 || patch == 5) && (dil == 1 || dil == 2); }

bool mind_shape_ok(int N, int H, int W) { return N > 0 && H > 0 && W > 0 && N <= 65535 && (long long)H * W < (1ll << 31); }

long long mind_tiles(int H, int W) { return (long long)nemar_cdiv(W, MD_TW) * nemar_cdiv(H, MD_TH); }

// the bytes of an [N,C,H,W] float tensor, saturated (C is any positive int)
size_t mind_bytes(int N, int C, int H, int W) {
    const unsigned __int128 b = (unsigned __int128)N * (unsigned)C * (unsigned)H * (unsigned)W * 4u;
    const size_t cap = (size_t)1 << 62;
    return b > cap ? cap : (size_t)b;
}

// do [a, a + na) and [b, b + nb) share a byte?
bool mind_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
    return p <= q ? q - p < na : p - q < nb;
}

// 16-byte loads: the base aligned and every row a whole number of quads
int mind_vec(const float* p, int W) { return (((uintptr_t)p & 15) == 0 && (W & 3) == 0) ? 1 : 0; }

template <int P, int DIL>
void mind_launch_fwd(hipStream_t st, const float* x, int Cx, const float* y, int Cy, float eps, float* partial, float* dm_map, int N, int H,
                     int W) {
    const int tiles_x = nemar_cdiv(W, MD_TW);
    const dim3 grid((unsigned)mind_tiles(H, W), 1, N), block(MD_THREADS);
    hipLaunchKernelGGL((mind_fwd_kernel<P, DIL>), grid, block, 0, st, x, Cx, y, Cy, eps, partial, dm_map, tiles_x, H, W, mind_vec(x, W),
                       mind_vec(y, W));
}

template <int P, int DIL>
void mind_launch_bwd(hipStream_t st, const float* x, int Cx, const float* y, int Cy, float eps, const float* gscale, float sx, float sy,
                     float* gx, float* gy, int accumulate, int N, int H, int W) {
    const int tiles_x = nemar_cdiv(W, MD_TW);
    const dim3 grid((unsigned)mind_tiles(H, W), 1, N), block(MD_THREADS);
    if (gy)
        hipLaunchKernelGGL((mind_bwd_kernel<P, DIL, true>), grid, block, 0, st, x, Cx, y, Cy, eps, gscale, sx, sy, gx, gy, accumulate, tiles_x,
                           H, W, mind_vec(x, W), mind_vec(y, W));
    else
        hipLaunchKernelGGL((mind_bwd_kernel<P, DIL, false>), grid, block, 0, st, x, Cx, y, Cy, eps, gscale, sx, sy, gx, gy, accumulate, tiles_x,
                           H, W, mind_vec(x, W), mind_vec(y, W));
}

}  // namespace

NEMAR_API size_t nemar_mind_loss_workspace(int N, int H, int W, int patch, int dil) {
    if (!mind_shape_ok(N, H, W) || !mind_cfg_ok(patch, dil)) return 0;
    return sizeof(float) * (size_t)mind_tiles(H, W) * N;
}

NEMAR_API int nemar_mind_loss_fwd(const float* x, int Cx, const float* y, int Cy, int patch, int dil, float eps, float factor, float* loss,
                                  int accumulate, float* dm_map, void* workspace, size_t ws_bytes, int N, int H, int W, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(x && y && loss && workspace, "mind_loss_fwd: null pointer");
    NEMAR_REQUIRE(((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)loss) | ((uintptr_t)dm_map) | ((uintptr_t)workspace)) & 3) == 0,
                  "mind_loss_fwd: x, y, loss, dm_map and workspace must be 4-byte aligned");
    NEMAR_REQUIRE(mind_cfg_ok(patch, dil), "mind_loss_fwd: patch %d (3 or 5) or dil %d (1 or 2) is not supported", patch, dil);
    NEMAR_REQUIRE(eps > 0.f, "mind_loss_fwd: eps %g must be positive", (double)eps);
    NEMAR_REQUIRE(mind_shape_ok(N, H, W) && Cx > 0 && Cy > 0, "mind_loss_fwd: bad shape N=%d Cx=%d Cy=%d H=%d W=%d", N, Cx, Cy, H, W);
    const size_t bx = mind_bytes(N, Cx, H, W), by = mind_bytes(N, Cy, H, W), bm = mind_bytes(N, 1, H, W);
    NEMAR_REQUIRE(!dm_map || (!mind_overlap(dm_map, bm, x, bx) && !mind_overlap(dm_map, bm, y, by)),
                  "mind_loss_fwd: dm_map must not alias an input (neighbouring tiles read it)");
    NEMAR_REQUIRE(ws_bytes >= nemar_mind_loss_workspace(N, H, W, patch, dil), "mind_loss_fwd: workspace %zu < %zu", ws_bytes,
                  nemar_mind_loss_workspace(N, H, W, patch, dil));
    hipStream_t st = (hipStream_t)stream;
    float* partial = (float*)workspace;
    if (patch == 3 && dil == 1) mind_launch_fwd<1, 1>(st, x, Cx, y, Cy, eps, partial, dm_map, N, H, W);
    else if (patch == 3) mind_launch_fwd<1, 2>(st, x, Cx, y, Cy, eps, partial, dm_map, N, H, W);
    else if (dil == 1) mind_launch_fwd<2, 1>(st, x, Cx, y, Cy, eps, partial, dm_map, N, H, W);
    else mind_launch_fwd<2, 2>(st, x, Cx, y, Cy, eps, partial, dm_map, N, H, W);
    hipLaunchKernelGGL(mind_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)partial, mind_tiles(H, W) * N, factor, (double)N * H * W,
                       accumulate, loss);
    NEMAR_CHECK_LAUNCH("mind_loss_fwd");
    return NEMAR_OK;
}

NEMAR_API int nemar_mind_loss_bwd(const float* x, int Cx, const float* y, int Cy, int patch, int dil, float eps, const float* gscale,
                                  float factor, float* gx, float* gy, int accumulate, int N, int H, int W, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(x && y && gscale && gx, "mind_loss_bwd: null pointer");
    NEMAR_REQUIRE(((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)gscale) | ((uintptr_t)gx) | ((uintptr_t)gy)) & 3) == 0,
                  "mind_loss_bwd: x, y, gscale, gx and gy must be 4-byte aligned");
    NEMAR_REQUIRE(mind_cfg_ok(patch, dil), "mind_loss_bwd: patch %d (3 or 5) or dil %d (1 or 2) is not supported", patch, dil);
    NEMAR_REQUIRE(eps > 0.f, "mind_loss_bwd: eps %g must be positive", (double)eps);
    NEMAR_REQUIRE(mind_shape_ok(N, H, W) && Cx > 0 && Cy > 0, "mind_loss_bwd: bad shape N=%d Cx=%d Cy=%d H=%d W=%d", N, Cx, Cy, H, W);
    const size_t bx = mind_bytes(N, Cx, H, W), by = mind_bytes(N, Cy, H, W);
    NEMAR_REQUIRE(!mind_overlap(gx, bx, x, bx) && !mind_overlap(gx, bx, y, by), "mind_loss_bwd: gx must not alias an input (neighbouring tiles read it)");
    NEMAR_REQUIRE(!gy || (!mind_overlap(gy, by, x, bx) && !mind_overlap(gy, by, y, by) && !mind_overlap(gy, by, gx, bx)),
                  "mind_loss_bwd: gy must not alias an input or gx");
    hipStream_t st = (hipStream_t)stream;
    const double c = (double)factor / (4.0 * (double)N * H * W);
    const float sx = (float)(c / Cx), sy = (float)(c / Cy);
    if (patch == 3 && dil == 1) mind_launch_bwd<1, 1>(st, x, Cx, y, Cy, eps, gscale, sx, sy, gx, gy, accumulate, N, H, W);
    else if (patch == 3) mind_launch_bwd<1, 2>(st, x, Cx, y, Cy, eps, gscale, sx, sy, gx, gy, accumulate, N, H, W);
    else if (dil == 1) mind_launch_bwd<2, 1>(st, x, Cx, y, Cy, eps, gscale, sx, sy, gx, gy, accumulate, N, H, W);
    else mind_launch_bwd<2, 2>(st, x, Cx, y, Cy, eps, gscale, sx, sy, gx, gy, accumulate, N, H, W);
    NEMAR_CHECK_LAUNCH("mind_loss_bwd");
    return NEMAR_OK;
}
