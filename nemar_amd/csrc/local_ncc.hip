// A windowed normalised cross-correlation as a training loss (DESIGN.md "Local NCC"), forward and backward.  Not a call site of the
// reference, whose image terms are the global L1 (loss.hip); similarity.hip's NCC is global and has no gradient.
//   x, y [N,C,H,W]; Omega(p) = the in-image part of the win x win square centred at p, n(p) = |Omega(p)| (no zero padding);
//   mx = sum x / n, my = sum y / n, vx = max(0, sum x^2 / n - mx^2), vy likewise, cov = sum xy / n - mx my, D = vx vy + eps
//   cc(p) = cov^2 / D,   loss = factor * (1 - sum_p cc(p) / M),   M = N C H W
//   alpha = 2 cov / D, beta = -2 cov^2 vy / D^2, gamma = -(alpha my + beta mx), each / n(p)
//   gx(q) = -gscale * factor / M * ( y(q) Box(alpha)(q) + x(q) Box(beta)(q) + Box(gamma)(q) ),   gy: the roles of x and y swapped.
// Every statistic is invariant to a constant added to x or y, and so is y(q) Box(alpha) + Box(-alpha my): the kernels subtract the mean
// of the staged patch from both images before anything is squared (the cancellation in sum x^2 / n - mx^2 is then that of the local
// contrast, not of the grey level), and use the shifted values for x(q), y(q) as well.
//
// Statistics of a TW x TH region (lncc_row_sums, lncc_stat): the (TW + 2r) x (TH + 2r) patches of x and y go to LDS (0 outside the
// image), their in-image mean is taken (block_sum: a fixed tree) and subtracted in place; a horizontal pass writes the five row-sum
// planes (sum x, y, xx, yy, xy over the 2r + 1 columns) for every patch row, a lane per column: stride 1 across the lanes.  A pixel's
// window sums are then 2r + 1 additions down a column of each plane.  Every window is summed directly, in a fixed order: no running
// window, no drift.
//
// Forward: one workgroup per 64 x 16 tile and plane; TW x TH is the tile.  A lane owns one pixel in each of four rows (a wave = 64 pixels
// of a row), writes cc_map where asked, and the tile's sum goes through the lanes' partials, the xor tree of each wave and the waves in
// ascending order into one record per workgroup; lncc_finish_kernel reads the records in a fixed order.  No atomics: bitwise repeatable.
// A cc passes through at most 4 (lane) + 6 (wave) + 3 (workgroup) additions in the tile kernel and ceil(records / 256) + 6 + 3 in the
// finish, which ends with 1 - sum / M (in double, rounded once) and its float product with factor.
//
// Backward: ONE launch, a pure gather, no workspace — the fused form.  One workgroup per 32 x 16 tile and plane.  The pixels q of the
// tile hear from every p within r: the coefficients are needed on the tile plus r, their statistics read the images on the tile plus
// 2r.  TW x TH = (32 + 2r) x (16 + 2r): each lane re-forms the statistics and the three (with gy: five) coefficients of up to five
// pixels p in registers, the workgroup then writes them over the dead row sums (0 for p outside the image), box-filters them in LDS by
// a horizontal and a vertical pass and writes gx (and gy).  The tile is 32 wide because the row sums of a 64-wide one exceed 64 KiB of
// static LDS from win 9 on (DESIGN.md has the budget per win).
#include "common.h"

namespace {

constexpr int LN_THREADS = 256;
constexpr int LN_FW = 64, LN_FH = 16;      // the forward tile
constexpr int LN_BW = 32, LN_BH = 16;      // the backward tile
constexpr int LN_MIN_WIN = 3, LN_MAX_WIN = 11;

// |Omega| along one axis: the in-image pixels within r of i
__device__ __forceinline__ int lncc_count(int i, int n, int r) { return min(i + r, n - 1) - max(i - r, 0) + 1; }

// The row sums of the TW x TH region whose first pixel is (oy, ox) (it may start outside the image; its patch meets the image):
// px, py [(TH + 2r) x (TW + 2r)] the shifted patches, rs [5][(TH + 2r) x TW] the row-sum planes; red: 16 floats.  Ends with a barrier.
template <int TW, int TH, int R>
__device__ __forceinline__ void lncc_row_sums(float* px, float* py, float* rs, float* red, const float* __restrict__ xP,
                                              const float* __restrict__ yP, int ox, int oy, int H, int W, int tid) {
    constexpr int PW = TW + 2 * R, PH = TH + 2 * R;
    float sx = 0.f, sy = 0.f;
    for (int e = tid; e < PH * PW; e += LN_THREADS) {
        const int r = e / PW, c = e - r * PW;
        const int h = oy - R + r, w = ox - R + c;
        float a = 0.f, b = 0.f;
        if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) {
            const size_t o = (size_t)h * W + w;
            a = xP[o];
            b = yP[o];
        }
        px[e] = a;
        py[e] = b;
        sx += a;
        sy += b;
    }
    const int nh = min(oy - R + PH, H) - max(oy - R, 0), nw = min(ox - R + PW, W) - max(ox - R, 0);
    const float inv = 1.f / (float)(nh * nw);
    const float cx = block_sum(sx, red) * inv;      // (its barriers also order the stores above before the loads below)
    const float cy = block_sum(sy, red) * inv;
    for (int e = tid; e < PH * PW; e += LN_THREADS) {      // the elements this thread wrote
        const int r = e / PW, c = e - r * PW;
        const int h = oy - R + r, w = ox - R + c;
        if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) {
            px[e] -= cx;
            py[e] -= cy;
        }
    }
    __syncthreads();
    for (int e = tid; e < PH * TW; e += LN_THREADS) {
        const int r = e / TW, c = e - r * TW;
        const float* a = px + r * PW + c;
        const float* b = py + r * PW + c;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
#pragma unroll
        for (int j = 0; j <= 2 * R; ++j) {
            const float u = a[j], v = b[j];
            s0 += u;
            s1 += v;
            s2 += u * u;
            s3 += v * v;
            s4 += u * v;
        }
        rs[e] = s0;
        rs[PH * TW + e] = s1;
        rs[2 * PH * TW + e] = s2;
        rs[3 * PH * TW + e] = s3;
        rs[4 * PH * TW + e] = s4;
    }
    __syncthreads();
}

struct LnccStat {
    float mx, my, vx, vy, cov, n;      // (the means are those of the shifted images)
};
// the statistics of region pixel (r, c) = image pixel (h, w), inside the image
template <int TW, int TH, int R>
__device__ __forceinline__ LnccStat lncc_stat(const float* rs, int r, int c, int h, int w, int H, int W) {
    constexpr int PLANE = (TH + 2 * R) * TW;
    const float* q = rs + r * TW + c;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
#pragma unroll
    for (int j = 0; j <= 2 * R; ++j) {
        s0 += q[j * TW];
        s1 += q[PLANE + j * TW];
        s2 += q[2 * PLANE + j * TW];
        s3 += q[3 * PLANE + j * TW];
        s4 += q[4 * PLANE + j * TW];
    }
    LnccStat s;
    s.n = (float)(lncc_count(h, H, R) * lncc_count(w, W, R));
    s.mx = s0 / s.n;
    s.my = s1 / s.n;
    s.vx = fmaxf(0.f, s2 / s.n - s.mx * s.mx);
    s.vy = fmaxf(0.f, s3 / s.n - s.my * s.my);
    s.cov = s4 / s.n - s.mx * s.my;
    return s;
}

template <int R>
__global__ __launch_bounds__(LN_THREADS) void lncc_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, float eps,
                                                              float* __restrict__ partial, float* __restrict__ cc_map, int tiles_x, int H, int W) {
    constexpr int PW = LN_FW + 2 * R, PH = LN_FH + 2 * R;
    __shared__ float px[PH * PW];
    __shared__ float py[PH * PW];
    __shared__ float rs[5 * PH * LN_FW];
    __shared__ float red[16];
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * LN_FW, y0 = ty * LN_FH;
    const size_t base = (size_t)blockIdx.z * H * W;
    lncc_row_sums<LN_FW, LN_FH, R>(px, py, rs, red, x + base, y + base, x0, y0, H, W, tid);

    float sum = 0.f;
    constexpr int ROWS = LN_THREADS / LN_FW, RUNS = LN_FH / ROWS;      // a lane owns one pixel in each of RUNS rows: a wave = 64 pixels of a row
#pragma unroll
    for (int i = 0; i < RUNS; ++i) {
        const int r = tid / LN_FW + ROWS * i, c = tid % LN_FW;
        const int h = y0 + r, w = x0 + c;
        if (h >= H || w >= W) continue;
        const LnccStat s = lncc_stat<LN_FW, LN_FH, R>(rs, r, c, h, w, H, W);
        const float cc = s.cov * s.cov / (s.vx * s.vy + eps);
        if (cc_map) cc_map[base + (size_t)h * W + w] = cc;
        sum += cc;
    }
    // the workgroup's record, in thread 0: the xor tree of each wave, then the waves in ascending order
    sum = wave_sum(sum);
    __syncthreads();      // (red was block_sum's)
    const int lane = tid & 63, wid = tid >> 6;
    if (lane == 0) red[wid] = sum;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < LN_THREADS / 64; ++i) sum += red[i];
        partial[(size_t)blockIdx.z * gridDim.x + blockIdx.x] = sum;
    }
}

// loss[0] (+)= factor * (1 - sum / M): thread t takes records t, t + 256, ... in ascending order, then the fixed workgroup tree; 1 - sum / M
// in double, rounded to float once, then the float product with factor — factor * (the loss at factor 1), bit for bit
__global__ __launch_bounds__(256) void lncc_finish_kernel(const float* __restrict__ partial, long long total, float factor, double M,
                                                          int accumulate, float* __restrict__ loss) {
    __shared__ float red[16];
    float acc = 0.f;
    for (long long i = threadIdx.x; i < total; i += 256) acc += partial[i];
    const float t = block_sum(acc, red);
    if (threadIdx.x == 0) loss[0] = (accumulate ? loss[0] : 0.f) + factor * (float)(1.0 - (double)t / M);
}

// the LDS of the backward kernel, in floats: [ patches | row sums ] while the statistics are formed, then [ coefficient row sums ...
// coefficients ] (the coefficients at the end, over dead row sums; their row sums from the start, over the dead patches)
template <int R, bool GY>
struct LnccBwd {
    static constexpr int TW = LN_BW + 2 * R, TH = LN_BH + 2 * R;      // the coefficients' region
    static constexpr int PW = TW + 2 * R, PH = TH + 2 * R;
    static constexpr int NCOEF = GY ? 5 : 3;                          // alpha, beta_x, gamma_x (, beta_y, gamma_y), each / n
    static constexpr int PATCH = PH * PW, ROWSUMS = 5 * PH * TW, COEF = NCOEF * TH * TW, COEF_ROWS = NCOEF * TH * LN_BW;
    static constexpr int TOTAL = (2 * PATCH + ROWSUMS) > (COEF_ROWS + COEF) ? (2 * PATCH + ROWSUMS) : (COEF_ROWS + COEF);
    static constexpr int ITEMS = (TH * TW + LN_THREADS - 1) / LN_THREADS;      // coefficient pixels per lane
    static_assert(COEF <= ROWSUMS, "the coefficients overwrite row sums only");
    static_assert((TOTAL + 16) * 4 <= 64 * 1024, "static LDS");
};

template <int R, bool GY>
__global__ __launch_bounds__(LN_THREADS) void lncc_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, float eps,
                                                              const float* __restrict__ gscale, float scale, float* __restrict__ gx,
                                                              float* __restrict__ gy, int accumulate, int tiles_x, int H, int W) {
    using B = LnccBwd<R, GY>;
    constexpr int TW = B::TW, TH = B::TH, NCOEF = B::NCOEF;
    __shared__ float lds[B::TOTAL];
    __shared__ float red[16];
    float* px = lds;
    float* py = lds + B::PATCH;
    float* rs = lds + 2 * B::PATCH;
    float* coef = lds + (B::TOTAL - B::COEF);
    float* crow = lds;
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * LN_BW, y0 = ty * LN_BH;
    const size_t base = (size_t)blockIdx.z * H * W;
    lncc_row_sums<TW, TH, R>(px, py, rs, red, x + base, y + base, x0 - R, y0 - R, H, W, tid);

    // the tile's own pixels, shifted as the statistics are: a lane owns one pixel in each of two rows (a wave = two rows of 32)
    constexpr int ROWS = LN_THREADS / LN_BW, RUNS = LN_BH / ROWS;
    float xq[RUNS], yq[RUNS];
#pragma unroll
    for (int i = 0; i < RUNS; ++i) {
        const int r = tid / LN_BW + ROWS * i, c = tid % LN_BW;
        xq[i] = px[(r + 2 * R) * B::PW + c + 2 * R];
        yq[i] = py[(r + 2 * R) * B::PW + c + 2 * R];
    }
    // the coefficients of up to ITEMS pixels p, in registers (0 outside the image: Box sums the in-image p only)
    float k[B::ITEMS][NCOEF];
#pragma unroll
    for (int i = 0; i < B::ITEMS; ++i) {
        const int e = tid + LN_THREADS * i;
#pragma unroll
        for (int j = 0; j < NCOEF; ++j) k[i][j] = 0.f;
        if (e >= TH * TW) continue;
        const int r = e / TW, c = e - r * TW;
        const int h = y0 - R + r, w = x0 - R + c;
        if ((unsigned)h >= (unsigned)H || (unsigned)w >= (unsigned)W) continue;
        const LnccStat s = lncc_stat<TW, TH, R>(rs, r, c, h, w, H, W);
        const float D = s.vx * s.vy + eps;
        const float a = 2.f * s.cov / D;
        const float ac = a * s.cov;                        // 2 cov^2 / D
        const float bx = -(ac * s.vy) / D;
        k[i][0] = a / s.n;
        k[i][1] = bx / s.n;
        k[i][2] = -(a * s.my + bx * s.mx) / s.n;
        if (GY) {
            const float by = -(ac * s.vx) / D;
            k[i][3] = by / s.n;
            k[i][4] = -(a * s.mx + by * s.my) / s.n;
        }
    }
    __syncthreads();      // every row sum and patch value has been read
#pragma unroll
    for (int i = 0; i < B::ITEMS; ++i) {
        const int e = tid + LN_THREADS * i;
        if (e >= TH * TW) continue;
#pragma unroll
        for (int j = 0; j < NCOEF; ++j) coef[j * TH * TW + e] = k[i][j];
    }
    __syncthreads();
    // Box, horizontally: for every coefficient row, the tile's 32 columns
    for (int e = tid; e < TH * LN_BW; e += LN_THREADS) {
        const int r = e / LN_BW, c = e - r * LN_BW;
#pragma unroll
        for (int j = 0; j < NCOEF; ++j) {
            const float* q = coef + j * TH * TW + r * TW + c;
            float s = 0.f;
#pragma unroll
            for (int d = 0; d <= 2 * R; ++d) s += q[d];
            crow[j * TH * LN_BW + e] = s;
        }
    }
    __syncthreads();
    // Box, vertically, and the gradient
    const float s = -(gscale[0] * scale);
#pragma unroll
    for (int i = 0; i < RUNS; ++i) {
        const int r = tid / LN_BW + ROWS * i, c = tid % LN_BW;
        const int h = y0 + r, w = x0 + c;
        if (h >= H || w >= W) continue;
        float b[NCOEF];
#pragma unroll
        for (int j = 0; j < NCOEF; ++j) {
            const float* q = crow + j * TH * LN_BW + r * LN_BW + c;
            float t = 0.f;
#pragma unroll
            for (int d = 0; d <= 2 * R; ++d) t += q[d * LN_BW];
            b[j] = t;
        }
        const size_t o = base + (size_t)h * W + w;
        const float g0 = s * (yq[i] * b[0] + xq[i] * b[1] + b[2]);
        if (accumulate) gx[o] += g0; else gx[o] = g0;
        if (GY) {
            const float g1 = s * (xq[i] * b[0] + yq[i] * b[3] + b[4]);
            if (accumulate) gy[o] += g1; else gy[o] = g1;
        }
    }
}

bool lncc_win_ok(int win) { return win >= LN_MIN_WIN && win <= LN_MAX_WIN && (win & 1); }

bool lncc_shape_ok(int N, int C, int H, int W) {
    return N > 0 && C > 0 && H > 0 && W > 0 && (long long)N * C <= 65535 && (long long)H * W < (1ll << 31);
}

long long lncc_tiles(int H, int W, int tw, int th) { return (long long)nemar_cdiv(W, tw) * nemar_cdiv(H, th); }

// do [a, a + bytes) and [b, b + bytes) share a byte?
bool lncc_overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
    return p < q + bytes && q < p + bytes;
}

template <int R>
void lncc_launch_fwd(hipStream_t st, const float* x, const float* y, float eps, float* partial, float* cc_map, int planes, int H, int W) {
    const int tiles_x = nemar_cdiv(W, LN_FW);
    const dim3 grid((unsigned)lncc_tiles(H, W, LN_FW, LN_FH), 1, planes), block(LN_THREADS);
    hipLaunchKernelGGL(lncc_fwd_kernel<R>, grid, block, 0, st, x, y, eps, partial, cc_map, tiles_x, H, W);
}

template <int R>
void lncc_launch_bwd(hipStream_t st, const float* x, const float* y, float eps, const float* gscale, float scale, float* gx, float* gy,
                     int accumulate, int planes, int H, int W) {
    const int tiles_x = nemar_cdiv(W, LN_BW);
    const dim3 grid((unsigned)lncc_tiles(H, W, LN_BW, LN_BH), 1, planes), block(LN_THREADS);
    if (gy)
        hipLaunchKernelGGL((lncc_bwd_kernel<R, true>), grid, block, 0, st, x, y, eps, gscale, scale, gx, gy, accumulate, tiles_x, H, W);
    else
        hipLaunchKernelGGL((lncc_bwd_kernel<R, false>), grid, block, 0, st, x, y, eps, gscale, scale, gx, gy, accumulate, tiles_x, H, W);
}

}  // namespace

NEMAR_API size_t nemar_local_ncc_workspace(int N, int C, int H, int W, int win) {
    if (!lncc_shape_ok(N, C, H, W) || !lncc_win_ok(win)) return 0;
    return sizeof(float) * (size_t)lncc_tiles(H, W, LN_FW, LN_FH) * N * C;
}

NEMAR_API int nemar_local_ncc_fwd(const float* x, const float* y, int win, float eps, float factor, float* loss, int accumulate,
                                  float* cc_map, void* workspace, size_t ws_bytes, int N, int C, int H, int W, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(x && y && loss && workspace, "local_ncc_fwd: null pointer");
    NEMAR_REQUIRE(((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)loss) | ((uintptr_t)cc_map) | ((uintptr_t)workspace)) & 3) == 0,
                  "local_ncc_fwd: x, y, loss, cc_map and workspace must be 4-byte aligned");
    NEMAR_REQUIRE(lncc_win_ok(win), "local_ncc_fwd: win %d is not an odd size from %d to %d", win, LN_MIN_WIN, LN_MAX_WIN);
    NEMAR_REQUIRE(eps > 0.f, "local_ncc_fwd: eps %g must be positive", (double)eps);
    NEMAR_REQUIRE(lncc_shape_ok(N, C, H, W), "local_ncc_fwd: bad shape N=%d C=%d H=%d W=%d", N, C, H, W);
    const size_t bytes = sizeof(float) * (size_t)N * C * H * W;
    NEMAR_REQUIRE(!cc_map || (!lncc_overlap(cc_map, x, bytes) && !lncc_overlap(cc_map, y, bytes)),
                  "local_ncc_fwd: cc_map must not alias an input (neighbouring tiles read it)");
    NEMAR_REQUIRE(ws_bytes >= nemar_local_ncc_workspace(N, C, H, W, win), "local_ncc_fwd: workspace %zu < %zu", ws_bytes,
                  nemar_local_ncc_workspace(N, C, H, W, win));
    hipStream_t st = (hipStream_t)stream;
    float* partial = (float*)workspace;
    switch (win / 2) {
        case 1: lncc_launch_fwd<1>(st, x, y, eps, partial, cc_map, N * C, H, W); break;
        case 2: lncc_launch_fwd<2>(st, x, y, eps, partial, cc_map, N * C, H, W); break;
        case 3: lncc_launch_fwd<3>(st, x, y, eps, partial, cc_map, N * C, H, W); break;
        case 4: lncc_launch_fwd<4>(st, x, y, eps, partial, cc_map, N * C, H, W); break;
        default: lncc_launch_fwd<5>(st, x, y, eps, partial, cc_map, N * C, H, W); break;
    }
    hipLaunchKernelGGL(lncc_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)partial, lncc_tiles(H, W, LN_FW, LN_FH) * N * C, factor,
                       (double)N * C * H * W, accumulate, loss);
    NEMAR_CHECK_LAUNCH("local_ncc_fwd");
    return NEMAR_OK;
}

NEMAR_API int nemar_local_ncc_bwd(const float* x, const float* y, int win, float eps, const float* gscale, float factor, float* gx,
                                  float* gy, int accumulate, int N, int C, int H, int W, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(x && y && gscale && gx, "local_ncc_bwd: null pointer");
    NEMAR_REQUIRE(((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)gscale) | ((uintptr_t)gx) | ((uintptr_t)gy)) & 3) == 0,
                  "local_ncc_bwd: x, y, gscale, gx and gy must be 4-byte aligned");
    NEMAR_REQUIRE(lncc_win_ok(win), "local_ncc_bwd: win %d is not an odd size from %d to %d", win, LN_MIN_WIN, LN_MAX_WIN);
    NEMAR_REQUIRE(eps > 0.f, "local_ncc_bwd: eps %g must be positive", (double)eps);
    NEMAR_REQUIRE(lncc_shape_ok(N, C, H, W), "local_ncc_bwd: bad shape N=%d C=%d H=%d W=%d", N, C, H, W);
    const size_t bytes = sizeof(float) * (size_t)N * C * H * W;
    NEMAR_REQUIRE(!lncc_overlap(gx, x, bytes) && !lncc_overlap(gx, y, bytes), "local_ncc_bwd: gx must not alias an input (neighbouring tiles read it)");
    NEMAR_REQUIRE(!gy || (!lncc_overlap(gy, x, bytes) && !lncc_overlap(gy, y, bytes) && !lncc_overlap(gy, gx, bytes)),
                  "local_ncc_bwd: gy must not alias an input or gx");
    hipStream_t st = (hipStream_t)stream;
    const float scale = (float)((double)factor / ((double)N * C * H * W));
    switch (win / 2) {
        case 1: lncc_launch_bwd<1>(st, x, y, eps, gscale, scale, gx, gy, accumulate, N * C, H, W); break;
        case 2: lncc_launch_bwd<2>(st, x, y, eps, gscale, scale, gx, gy, accumulate, N * C, H, W); break;
        case 3: lncc_launch_bwd<3>(st, x, y, eps, gscale, scale, gx, gy, accumulate, N * C, H, W); break;
        case 4: lncc_launch_bwd<4>(st, x, y, eps, gscale, scale, gx, gy, accumulate, N * C, H, W); break;
        default: lncc_launch_bwd<5>(st, x, y, eps, gscale, scale, gx, gy, accumulate, N * C, H, W); break;
    }
    NEMAR_CHECK_LAUNCH("local_ncc_bwd");
    return NEMAR_OK;
}
