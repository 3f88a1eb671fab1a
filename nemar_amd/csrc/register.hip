// Registration at any resolution: the STN's prediction applied to an image of another size in ONE pass (DESIGN.md "Registration at
// native size").  Not a call site of the reference, which only ever warps at the network's own size; it composes two that are:
//   F.interpolate(offsets, (Ho, Wo), 'bilinear', align_corners=False)          reference models/stn/unet_stn.py:139-141,165-166
//   F.grid_sample(img, identity + offsets, <mode>, 'zeros', align_corners=False) reference models/stn/unet_stn.py:167-174
//   F.affine_grid(theta, size) + F.grid_sample                                   reference models/stn/affine_stn.py:122,128
// The sampling grid is in normalised coordinates, so a prediction made at hf x wf describes the same transformation at Ho x Wo.
// nemar_bilinear_fwd + nemar_grid_sample_fwd would write the resized 2-channel field to HBM and read it straight back:
// 4 * (2C + 4) B/px against 4 * 2C B/px here (40 against 24 at C = 3), where the coarse field is interpolated in registers.
//
// One workgroup per 64 x 16 output tile.  The coarse-field taps of a tile span at most (64 wf/Wo + 2) x (16 hf/Ho + 2) texels: with
// wf <= Wo and hf <= Ho they fit a 66 x 18 x 2 LDS patch (9.3 KiB), staged through registers with 4-byte loads — `pred` needs no
// 16-byte alignment on that route; a tile whose taps do not fit (a field being DOWN-sampled) reads them from global memory.  The
// sampling position is computed once per pixel and reused for every channel.  A lane owns ONE pixel in each of four rows of the tile, so
// that every gather and every store instruction of a wave covers whole cache lines.  The other shape — 4 consecutive pixels of one row
// per lane, 16-byte stores where Wo % 4 == 0 and `out` is 16-byte aligned — is in the measurement build only (nemar_tune(44, 1)):
// tools/microbench_register.py times the two side by side and profiles/register_fullres.txt holds the result, 16-byte stores take 27 % to
// 37 % longer, as in warp.hip's forward kernel (profiles/r4_gs_fwd_vec.txt).  No pointer needs more than 4-byte alignment.
//
// Arithmetic is shared, not restated: grid and position from warp_grid.h, the resize taps and their sum from resize_taps.h, the
// prediction's view, the tile's field patch and the texels a pixel reads from resampled_grid.h, the four-corner blend in the
// expression order of warp.hip's grid_sample_fwd_kernel.  With -ffp-contract=off the bilinear result equals the composed path's bit
// for bit (tests/register_cases.py).
#include "common.h"
#include "pred_grad.h"
#include "pred_launch.h"

namespace {

// VEC: pixels of one row a lane owns per run — 1 (the product: four runs, in four rows of the tile) or 4 (measurement build: one run)
template <int MODE, int SAMPLE, int VEC, bool RESAMPLE>
__global__ __launch_bounds__(RT_THREADS) void warp_resampled_kernel(const float* __restrict__ in, const float* __restrict__ pred,
                                                                    float* __restrict__ out, int C, int Hs, int Ws, int hf, int wf,
                                                                    int Ho, int Wo, float sh, float sw) {
    __shared__ float patch[RESAMPLE ? 2 * RT_PH * RT_PW : 1];
    const int n = blockIdx.z, tid = threadIdx.x;
    const int x0 = blockIdx.x * RT_W, y0 = blockIdx.y * RT_H;
    const auto pv = pred_view<MODE, RESAMPLE>(pred, n, hf, wf, Ho, Wo, sh, sw);
    const size_t splane = (size_t)Hs * Ws, oplane = pv.oplane;
    const float* inN = in + (size_t)n * C * splane;
    float* outN = out + (size_t)n * C * oplane;

    const FieldPatch fp = pv.stage(patch, x0, y0, tid);
    if (RESAMPLE) __syncthreads();

    constexpr int LPR = RT_W / VEC, ROWS = RT_THREADS / LPR, RUNS = RT_H / ROWS;      // lanes per tile row, rows per pass, passes
#pragma unroll
    for (int i = 0; i < RUNS; ++i) {
        const int h = y0 + tid / LPR + ROWS * i, w0 = x0 + (tid % LPR) * VEC;
        if (h >= Ho || w0 >= Wo) continue;                 // (VEC 4 only with Wo % 4 == 0: a run is inside the row or outside it)
        Taps t[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const int w = w0 + v;
            float gx, gy;
            pv.coord(patch, fp, h, w, gx, gy);
            t[v] = taps_at<SAMPLE>(gx, gy, Ws, Hs);
        }
        float* q = outN + (size_t)h * Wo + w0;
        for (int c = 0; c < C; ++c) {
            const float* p = inN + (size_t)c * splane;
            float r[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) r[v] = sample_at<SAMPLE>(p, t[v]);
            if constexpr (VEC == 4) {
                *reinterpret_cast<float4*>(q + (size_t)c * oplane) = make_float4(r[0], r[1], r[2], r[3]);
            } else {
                q[(size_t)c * oplane] = r[0];
            }
        }
    }
}

}  // namespace

// nemar_tune(44, 1) (measurement build): 4 consecutive pixels per lane and 16-byte stores where the output allows; 0 (default, and the
// product): one pixel per lane
NEMAR_SWITCH(int, g_register_vec4, 0);

namespace {

template <int MODE, int SAMPLE, bool RESAMPLE>
void launch(const float* in, const float* pred, float* out, int N, int C, int Hs, int Ws, int hf, int wf, int Ho, int Wo, float sh, float sw,
            hipStream_t st) {
    const dim3 grid(nemar_cdiv(Wo, RT_W), nemar_cdiv(Ho, RT_H), N), block(RT_THREADS);
    NEMAR_AB_ONLY(if (g_register_vec4 && (Wo & 3) == 0 && (((uintptr_t)out) & 15) == 0)
        hipLaunchKernelGGL((warp_resampled_kernel<MODE, SAMPLE, 4, RESAMPLE>), grid, block, 0, st, in, pred, out, C, Hs, Ws, hf, wf, Ho, Wo, sh, sw);
    else)
        hipLaunchKernelGGL((warp_resampled_kernel<MODE, SAMPLE, 1, RESAMPLE>), grid, block, 0, st, in, pred, out, C, Hs, Ws, hf, wf, Ho, Wo, sh, sw);
}

}  // namespace

NEMAR_API int nemar_warp_resampled_fwd(const float* in, const float* pred, int grid_mode, int sample_mode, float* out, int N, int C,
                                       int Hs, int Ws, int hf, int wf, int Ho, int Wo, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(in && pred && out, "warp_resampled_fwd: null pointer");
    NEMAR_REQUIRE(((((uintptr_t)in) | ((uintptr_t)pred) | ((uintptr_t)out)) & 3) == 0,
                  "warp_resampled_fwd: in, pred and out must be 4-byte aligned");
    NEMAR_REQUIRE(sample_mode == SAMPLE_BILINEAR || sample_mode == SAMPLE_NEAREST, "warp_resampled_fwd: unknown sample_mode %d", sample_mode);
    NEMAR_REQUIRE(N > 0 && C > 0 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0, "warp_resampled_fwd: bad shape N=%d C=%d source %dx%d output %dx%d", N,
                  C, Hs, Ws, Ho, Wo);
    NEMAR_REQUIRE((long long)Hs * Ws < (1ll << 31), "warp_resampled_fwd: source plane too large");
    NEMAR_REQUIRE_OK(pred_ok("warp_resampled_fwd", "", grid_mode, hf, wf) && tile_grid_ok("warp_resampled_fwd", N, Ho, Wo));
    hipStream_t st = (hipStream_t)stream;
    dispatch_pred(grid_mode, hf, wf, Ho, Wo, [&](auto mode, auto resample, int hf, int wf, float sh, float sw) {
        constexpr int MODE = decltype(mode)::value;
        constexpr bool RESAMPLE = decltype(resample)::value;
        if (sample_mode == SAMPLE_NEAREST) launch<MODE, SAMPLE_NEAREST, RESAMPLE>(in, pred, out, N, C, Hs, Ws, hf, wf, Ho, Wo, sh, sw, st);
        else launch<MODE, SAMPLE_BILINEAR, RESAMPLE>(in, pred, out, N, C, Hs, Ws, hf, wf, Ho, Wo, sh, sw, st);
    });
    NEMAR_CHECK_LAUNCH("warp_resampled_fwd");
    return NEMAR_OK;
}

// ---- backward: the gradient towards the prediction ------------------------------------------------------------------------------------------
// The adjoint of the kernel above with respect to `pred`, bilinear sampling (DESIGN.md "Refinement on the pair").  A pixel's gradient with
// respect to its own sampling coordinate is grid_sample_bwd_kernel's (warp.hip), restated in that order:
//   dvx = (Ws/2) sum_ch gout ((b - a) ey + (d - c) ty),   dvy = (Hs/2) sum_ch gout ((c - a) ex + (d - b) tx),   0 where gx or gy is not finite.
// What remains is the adjoint of how the coordinate came from the prediction, and it is a GATHER in a fixed order everywhere — no atomics:
//   UNET at the output's size   gpred = dv, written by the pixel's lane: one launch, no workspace.
//   UNET resampled              the adjoint of resize_blend.  The workgroup of a 64 x 16 tile stages dv in LDS and reduces it SEPARABLY into the
//                               field patch the tile taps (patch_span: PredView::stage's geometry): a row pass — for every tile row and patch
//                               column the sum over that row's pixels, ascending w, of Wx_j(w) dv — then a column pass, ascending h, of
//                               Wy_i(h) times the row sums: O(ratio) additions per texel and pixel row, not O(ratio^2).  The 2 ph pw sums are
//                               the tile's record in the workspace; a merge kernel, one thread per field texel, adds the records of the tiles
//                               whose patch holds the texel in ascending row-major tile order and writes or accumulates gpred.
//   AFFINE                      the workgroup's six sums of dvx (xb, yb, 1), dvy (xb, yb, 1) -> its record; epe_bwd_affine_merge_kernel
//                               (pred_grad.h) adds them in a fixed order.  Its gscale is a 1.0f the tile kernel leaves behind the records.
// LDS of the resampled kernel: patch 9504 + dv 8320 + row sums 8576 + tap tables and ranges 1312, 27 744 B as built: five workgroups per CU.
// The pitches (65, 67) are odd so that the row pass, whose lanes run over (channel, tile row) first, and the column pass, whose lanes run
// over the patch column first, both read and write without bank conflicts.
constexpr int RB_DP = RT_W + 1;       // pitch of a dv row
constexpr int RB_SP = RT_PW + 1;      // pitch of a row of row sums

namespace {

// d(out . gout) / d(gx, gy) of one output pixel at offset o of its plane
__device__ __forceinline__ void pixel_dv(const float* __restrict__ inN, const float* __restrict__ goN, size_t splane, size_t oplane, size_t o,
                                         float gx, float gy, int C, int Hs, int Ws, float& dvx, float& dvy) {
    const Taps t = taps_at<SAMPLE_BILINEAR>(gx, gy, Ws, Hs);
    const Sample s = locate(gx, gy, Ws, Hs);
    const float ex = 1.f - s.tx, ey = 1.f - s.ty;
    float gix = 0.f, giy = 0.f;
    for (int ch = 0; ch < C; ++ch) {
        const float g = goN[(size_t)ch * oplane + o];
        const float* p = inN + (size_t)ch * splane;
        const float ra = p[t.o00], rb = p[t.o01], rc = p[t.o10], rd = p[t.o11];
        const float a = (t.ok & 1u) ? ra : 0.f, b = (t.ok & 2u) ? rb : 0.f, cc = (t.ok & 4u) ? rc : 0.f, d = (t.ok & 8u) ? rd : 0.f;
        gix += g * ((b - a) * ey + (d - cc) * s.ty);
        giy += g * ((cc - a) * ex + (d - b) * s.tx);
    }
    const bool finite = fabsf(gx) <= 3.402823466e+38f && fabsf(gy) <= 3.402823466e+38f;      // (false for a NaN)
    dvx = finite ? gix * (0.5f * (float)Ws) : 0.f;
    dvy = finite ? giy * (0.5f * (float)Hs) : 0.f;
}

// the weight of output index `rel`'s tap pair (i0 relative to the patch, fraction l1, i1 = min(i0 + 1, last)) on patch index k: both
// weights where the two taps coincide at the border — the adjoint of resize_blend
__device__ __forceinline__ float tap_weight(int i0, float l1, int last, int k) {
    const int i1 = min(i0 + 1, last);
    return (i0 == k ? 1.f - l1 : 0.f) + (i1 == k ? l1 : 0.f);
}
// the output indices [lo, hi] of a tile axis (`count` valid ones, tap i0 in ti[], monotone) whose pair touches patch index k
__device__ __forceinline__ void tap_range(const int* ti, int count, int last, int k, int& lo, int& hi) {
    int a = 0, b = count - 1;                      // first index with i1 >= k (the last one has: k is inside the patch)
    while (a < b) {
        const int m = (a + b) >> 1;
        if (min(ti[m] + 1, last) >= k) b = m; else a = m + 1;
    }
    lo = a;
    a = 0; b = count - 1;                          // last index with i0 <= k (the first one has)
    while (a < b) {
        const int m = (a + b + 1) >> 1;
        if (ti[m] <= k) a = m; else b = m - 1;
    }
    hi = a;
}

// dst: gpred (UNET at the output's size), the tile records (UNET resampled: rec_ph x rec_pw x 2 floats a tile) or the six-word records (AFFINE)
template <int MODE, bool RESAMPLE>
__global__ __launch_bounds__(RT_THREADS) void warp_resampled_bwd_kernel(const float* __restrict__ in, const float* __restrict__ pred,
                                                                        const float* __restrict__ gout, float* __restrict__ dst,
                                                                        int accumulate, int C, int Hs, int Ws, int hf, int wf, int Ho, int Wo,
                                                                        float sh, float sw, int rec_ph, int rec_pw, float* __restrict__ one) {
    __shared__ float patch[RESAMPLE ? 2 * RT_PH * RT_PW : 1];
    __shared__ float dvs[RESAMPLE ? 2 * RT_H * RB_DP : 1];
    __shared__ float sums[RESAMPLE ? 2 * RT_H * RB_SP : 1];
    __shared__ int txi[RESAMPLE ? RT_W : 1], tyi[RESAMPLE ? RT_H : 1];
    __shared__ float txl[RESAMPLE ? RT_W : 1], tyl[RESAMPLE ? RT_H : 1];
    __shared__ int wlo[RESAMPLE ? RT_PW : 1], whi[RESAMPLE ? RT_PW : 1], hlo[RESAMPLE ? RT_PH : 1], hhi[RESAMPLE ? RT_PH : 1];
    __shared__ float red[MODE == GRID_AFFINE ? 16 : 1];
    const int n = blockIdx.z, tid = threadIdx.x;
    const int x0 = blockIdx.x * RT_W, y0 = blockIdx.y * RT_H;
    const auto pv = pred_view<MODE, RESAMPLE>(pred, n, hf, wf, Ho, Wo, sh, sw);
    const size_t splane = (size_t)Hs * Ws, oplane = pv.oplane;
    const float* inN = in + (size_t)n * C * splane;
    const float* goN = gout + (size_t)n * C * oplane;
    const int tw = min(RT_W, Wo - x0), th = min(RT_H, Ho - y0);      // the tile's valid columns and rows

    const FieldPatch fp = pv.stage(patch, x0, y0, tid);
    int pw = 0, ph = 0;
    if (RESAMPLE) {
        pw = patch_span(x0, RT_W, wf, Wo, sw).count;
        ph = patch_span(y0, RT_H, hf, Ho, sh).count;
        if (!fp.staged) return;                    // (a field being down-sampled: refused by the entry point; the same in every lane)
        if (tid < tw) {
            const Tap1D t = tap1d(x0 + tid, wf, sw);
            txi[tid] = t.i0 - fp.px0;
            txl[tid] = t.l1;
        } else if (tid >= RT_W && tid - RT_W < th) {
            const Tap1D t = tap1d(y0 + tid - RT_W, hf, sh);
            tyi[tid - RT_W] = t.i0 - fp.py0;
            tyl[tid - RT_W] = t.l1;
        }
        __syncthreads();
    }

    constexpr int ROWS = RT_THREADS / RT_W, RUNS = RT_H / ROWS;      // the forward's shape: one pixel in each of four rows per lane
    float acc[EPE_WORDS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < RUNS; ++i) {
        const int r = tid / RT_W + ROWS * i, lx = tid % RT_W;
        const int h = y0 + r, w = x0 + lx;
        float dvx = 0.f, dvy = 0.f;
        if (h < Ho && w < Wo) {
            float gx, gy;
            pv.coord(patch, fp, h, w, gx, gy);
            const size_t o = (size_t)h * Wo + w;
            pixel_dv(inN, goN, splane, oplane, o, gx, gy, C, Hs, Ws, dvx, dvy);
            if (MODE == GRID_UNET && !RESAMPLE) {
                float* q = dst + (size_t)n * 2 * oplane + o;
                if (accumulate) { q[0] += dvx; q[oplane] += dvy; } else { q[0] = dvx; q[oplane] = dvy; }
            }
            if (MODE == GRID_AFFINE) {
                const float xb = affine_base(w, Wo), yb = affine_base(h, Ho);
                acc[0] += dvx * xb; acc[1] += dvx * yb; acc[2] += dvx;
                acc[3] += dvy * xb; acc[4] += dvy * yb; acc[5] += dvy;
            }
        }
        if (RESAMPLE) {
            dvs[r * RB_DP + lx] = dvx;
            dvs[(RT_H + r) * RB_DP + lx] = dvy;
        }
    }

    if (MODE == GRID_AFFINE) {
        float* rec = dst + ((size_t)n * gridDim.y * gridDim.x + (size_t)blockIdx.y * gridDim.x + blockIdx.x) * EPE_WORDS;
#pragma unroll
        for (int c = 0; c < EPE_WORDS; ++c) {
            const float t = block_sum(acc[c], red);
            if (tid == 0) rec[c] = t;
        }
        if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) one[0] = 1.f;
    }

    if (RESAMPLE) {
        const int lastx = wf - 1 - fp.px0, lasty = hf - 1 - fp.py0;
        if (tid < pw) {
            int lo, hi;
            tap_range(txi, tw, lastx, tid, lo, hi);
            wlo[tid] = lo; whi[tid] = hi;
        } else if (tid >= 128 && tid - 128 < ph) {
            int lo, hi;
            tap_range(tyi, th, lasty, tid - 128, lo, hi);
            hlo[tid - 128] = lo; hhi[tid - 128] = hi;
        }
        __syncthreads();
        // row pass: lanes over (channel, tile row) first, then the patch column
        for (int e = tid; e < 2 * RT_H * pw; e += RT_THREADS) {
            const int cr = e & (2 * RT_H - 1), j = e / (2 * RT_H);
            const float* row = dvs + cr * RB_DP;
            float a = 0.f;
            for (int w = wlo[j]; w <= whi[j]; ++w) a += tap_weight(txi[w], txl[w], lastx, j) * row[w];
            sums[cr * RB_SP + j] = a;
        }
        __syncthreads();
        // column pass: lanes over the patch column first
        float* rec = dst + ((size_t)n * gridDim.y * gridDim.x + (size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 * rec_ph * rec_pw;
        for (int e = tid; e < 2 * ph * pw; e += RT_THREADS) {
            const int ci = e / pw, j = e - ci * pw;
            const int c = ci >= ph ? 1 : 0, i = ci - c * ph;
            const float* col = sums + c * RT_H * RB_SP + j;
            float a = 0.f;
            for (int r = hlo[i]; r <= hhi[i]; ++r) a += tap_weight(tyi[r], tyl[r], lasty, i) * col[r * RB_SP];
            // (record_extent bounds ph and pw: the index guard is memory safety, and a patch that did not fit is made loud)
            if (i < rec_ph && j < rec_pw) rec[(c * rec_ph + i) * rec_pw + j] = (ph <= rec_ph && pw <= rec_pw) ? a : NAN;
        }
    }
}

// the tiles [lo, hi] of one axis that can hold field index k in their patch: the output indices d whose source coordinate lies in
// (k - 1, k + 1), from the inverse of tap1d's map widened by two pixels (the test that follows is exact: patch_span)
__device__ __forceinline__ void tile_candidates(int k, float scale, int n_out, int tile, int& lo, int& hi) {
    const float top = (float)(n_out - 1);
    const float a = fminf(fmaxf(floorf(((float)k - 0.5f) / scale - 0.5f) - 2.f, 0.f), top);
    const float b = fminf(fmaxf(ceilf(((float)k + 1.5f) / scale - 0.5f) + 2.f, 0.f), top);
    lo = (int)a / tile;
    hi = (int)b / tile;
}

// gpred[n, c, i, j] (+)= the entries for texel (i, j) of the records of the tiles whose patch holds it, in ascending row-major tile order
__global__ __launch_bounds__(256) void warp_resampled_bwd_merge_kernel(const float* __restrict__ rec, float* __restrict__ gpred, int accumulate,
                                                                       int hf, int wf, int Ho, int Wo, float sh, float sw, int rec_ph, int rec_pw,
                                                                       int tiles_y, int tiles_x) {
    const int n = blockIdx.y, fplane = hf * wf;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 2 * fplane) return;
    const int c = e >= fplane ? 1 : 0, t = e - c * fplane;
    const int i = t / wf, j = t - i * wf;
    int ty0, ty1, tx0, tx1;
    tile_candidates(i, sh, Ho, RT_H, ty0, ty1);
    tile_candidates(j, sw, Wo, RT_W, tx0, tx1);
    const size_t slot = (size_t)2 * rec_ph * rec_pw;
    float acc = 0.f;
    for (int ty = ty0; ty <= ty1; ++ty) {
        const PatchSpan sy = patch_span(ty * RT_H, RT_H, hf, Ho, sh);
        const int ri = i - sy.first;
        if (ri < 0 || ri >= sy.count || ri >= rec_ph) continue;
        for (int tx = tx0; tx <= tx1; ++tx) {
            const PatchSpan sx = patch_span(tx * RT_W, RT_W, wf, Wo, sw);
            const int rj = j - sx.first;
            if (rj < 0 || rj >= sx.count || rj >= rec_pw) continue;
            acc += rec[(((size_t)n * tiles_y + ty) * tiles_x + tx) * slot + (size_t)(c * rec_ph + ri) * rec_pw + rj];
        }
    }
    float* q = gpred + (size_t)n * 2 * fplane + e;
    q[0] = accumulate ? q[0] + acc : acc;
}

// The most field texels one axis of a tile's patch spans (`tile` pixels, scale = n_in / n_out <= 1), an upper bound of patch_span's count:
//   the source coordinates s of the tile's first and last pixel differ by at most (tile - 1) scale, so their floors i0 differ by at most
//   floor((tile - 1) scale) + 1; the last pixel's i1 is at most one further, and the count includes both ends:
//   count <= floor(x) + 3 in exact arithmetic, x = (tile - 1) scale.  The device's s is fp32 ((d + 0.5) scale - 0.5, each rounding far
//   below one texel).  One end rounded across an integer only turns "the fractions did not carry" into "they did", which the + 1 above
//   already holds; BOTH ends rounded across integers, outwards, add one more — possible only where the fraction of x is just below 1.
//   The host's fp32 product below can floor one short of floor(x) only where that fraction is just above 0.  The two cannot coincide, so
//   floor(x) + 4 covers either.  Never more than the field or the LDS patch.  The kernels still guard every record index (memory
//   safety), and a tile whose patch did not fit writes NaN, not a short sum: an error here cannot pass for a gradient.
int record_extent(int n_in, int n_out, int tile) {
    const int e = (int)((float)(tile - 1) * ((float)n_in / (float)n_out)) + 4;
    const int cap = n_in < tile + 2 ? n_in : tile + 2;
    return e < cap ? e : cap;
}

bool field_resampled(int grid_mode, int hf, int wf, int Ho, int Wo) { return grid_mode == GRID_UNET && (hf != Ho || wf != Wo); }

}  // namespace

NEMAR_API size_t nemar_warp_resampled_bwd_workspace(int grid_mode, int N, int hf, int wf, int Ho, int Wo) {
    if (N <= 0 || Ho <= 0 || Wo <= 0) return 0;
    const size_t tiles = (size_t)nemar_cdiv(Wo, RT_W) * nemar_cdiv(Ho, RT_H) * N;
    if (grid_mode == GRID_AFFINE) return sizeof(float) * (tiles * EPE_WORDS + 1);
    if (hf <= 0 || wf <= 0 || hf > Ho || wf > Wo || !field_resampled(grid_mode, hf, wf, Ho, Wo)) return 0;
    return sizeof(float) * tiles * 2 * record_extent(hf, Ho, RT_H) * record_extent(wf, Wo, RT_W);
}

NEMAR_API int nemar_warp_resampled_bwd(const float* img, const float* pred, int grid_mode, const float* gout, float* gpred, int accumulate,
                                       int N, int C, int Hs, int Ws, int hf, int wf, int Ho, int Wo, void* ws, size_t ws_bytes, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(img && pred && gout && gpred, "warp_resampled_bwd: null pointer");
    NEMAR_REQUIRE(aligned4(img, pred, gout, gpred, ws), "warp_resampled_bwd: img, pred, gout, gpred and ws must be 4-byte aligned");
    NEMAR_REQUIRE(C > 0 && Hs > 0 && Ws > 0 && epe_shape_ok(N, Ho, Wo), "warp_resampled_bwd: bad shape N=%d C=%d source %dx%d output %dx%d", N, C,
                  Hs, Ws, Ho, Wo);
    NEMAR_REQUIRE((long long)Hs * Ws < (1ll << 31), "warp_resampled_bwd: source plane too large");
    // (the merge finds a texel's tiles from the fp32 inverse of tap1d's map, widened by two pixels.  Below 2^23 pixels a side the quotient,
    // the subtraction and tap1d's own two roundings are each at most a quarter of a pixel off in the output index: 1.25 px in all)
    NEMAR_REQUIRE(Ho < (1 << 23) && Wo < (1 << 23), "warp_resampled_bwd: output %d x %d (each side below 2^23)", Ho, Wo);
    NEMAR_REQUIRE_OK(pred_ok("warp_resampled_bwd", "", grid_mode, hf, wf) && tile_grid_ok("warp_resampled_bwd", N, Ho, Wo));
    NEMAR_REQUIRE(grid_mode != GRID_UNET || (hf <= Ho && wf <= Wo),
                  "warp_resampled_bwd: field %d x %d is being down-sampled to %d x %d (no backward: the forward's unstaged route has no adjoint here)",
                  hf, wf, Ho, Wo);
    NEMAR_REQUIRE(gpred != pred, "warp_resampled_bwd: gpred must not be the prediction");
    const size_t need = nemar_warp_resampled_bwd_workspace(grid_mode, N, hf, wf, Ho, Wo);
    NEMAR_REQUIRE(ws_bytes >= need && (ws || need == 0), "warp_resampled_bwd: workspace %zu < %zu", ws ? ws_bytes : (size_t)0, need);
    hipStream_t st = (hipStream_t)stream;
    const int tiles_x = nemar_cdiv(Wo, RT_W), tiles_y = nemar_cdiv(Ho, RT_H);
    const dim3 grid(tiles_x, tiles_y, N), block(RT_THREADS);
    float* rec = (float*)ws;
    dispatch_pred(grid_mode, hf, wf, Ho, Wo, [&](auto mode, auto resample, int hf, int wf, float sh, float sw) {
        constexpr int MODE = decltype(mode)::value;
        constexpr bool RESAMPLE = decltype(resample)::value;
        if constexpr (MODE == GRID_AFFINE) {
            float* one = rec + (size_t)tiles_x * tiles_y * N * EPE_WORDS;
            hipLaunchKernelGGL((warp_resampled_bwd_kernel<MODE, false>), grid, block, 0, st, img, pred, gout, rec, 0, C, Hs, Ws, hf, wf, Ho, Wo, sh,
                               sw, 0, 0, one);
            hipLaunchKernelGGL(epe_bwd_affine_merge_kernel, dim3(N), dim3(256), 0, st, (const float*)rec, tiles_x * tiles_y, (const float*)one, 1.f,
                               gpred, accumulate);
        } else if constexpr (RESAMPLE) {
            const int rec_ph = record_extent(hf, Ho, RT_H), rec_pw = record_extent(wf, Wo, RT_W);
            hipLaunchKernelGGL((warp_resampled_bwd_kernel<MODE, true>), grid, block, 0, st, img, pred, gout, rec, 0, C, Hs, Ws, hf, wf, Ho, Wo, sh,
                               sw, rec_ph, rec_pw, (float*)nullptr);
            hipLaunchKernelGGL(warp_resampled_bwd_merge_kernel, dim3(nemar_cdiv(2ll * hf * wf, 256), N), dim3(256), 0, st, (const float*)rec, gpred,
                               accumulate, hf, wf, Ho, Wo, sh, sw, rec_ph, rec_pw, tiles_y, tiles_x);
        } else {
            hipLaunchKernelGGL((warp_resampled_bwd_kernel<MODE, false>), grid, block, 0, st, img, pred, gout, gpred, accumulate, C, Hs, Ws, hf, wf,
                               Ho, Wo, sh, sw, 0, 0, (float*)nullptr);
        }
    });
    NEMAR_CHECK_LAUNCH("warp_resampled_bwd");
    return NEMAR_OK;
}
