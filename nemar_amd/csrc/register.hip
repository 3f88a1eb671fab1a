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
// four-corner blend in the expression order of warp.hip's grid_sample_fwd_kernel.  With -ffp-contract=off the bilinear result equals
// the composed path's bit for bit (tests/register_cases.py).
#include "common.h"
#include "resize_taps.h"
#include "warp_grid.h"

namespace {

constexpr int SAMPLE_BILINEAR = 0;  // F.grid_sample(mode='bilinear')
constexpr int SAMPLE_NEAREST = 1;   // F.grid_sample(mode='nearest'): round-half-to-even of the unnormalised position

constexpr int RT_W = 64, RT_H = 16, RT_THREADS = 256;
constexpr int RT_PW = RT_W + 2, RT_PH = RT_H + 2;      // the coarse patch of a tile when the field is not being down-sampled

// the pixel's two interpolated field values from `f` (channel 0 at f, channel 1 at f + cstep; rows `pitch` apart; the taps' indices
// relative to (oy, ox)) — called once with the LDS patch and once with the global field, so that each call keeps its address space
__device__ __forceinline__ RegSrc field_at(const float* f, int pitch, int cstep, int oy, int ox, const Tap1D& th, const Tap1D& tw) {
    const int r0 = (th.i0 - oy) * pitch, r1 = (th.i1 - oy) * pitch, c0 = tw.i0 - ox, c1 = tw.i1 - ox;
    const float* g = f + cstep;
    return RegSrc{resize_blend(f[r0 + c0], f[r0 + c1], f[r1 + c0], f[r1 + c1], tw, th),
                  resize_blend(g[r0 + c0], g[r0 + c1], g[r1 + c0], g[r1 + c1], tw, th)};
}

// where one output pixel reads the source: up to four texel offsets (clamped into the image, so that the loads are unconditional and the
// zeros of the padding are selected afterwards, as grid_sample_fwd_kernel does), their weights, bit k of `ok` = texel k is inside
struct Taps {
    int o00, o01, o10, o11;
    float wnw, wne, wsw, wse;
    unsigned ok;
};
template <int SAMPLE>
__device__ __forceinline__ Taps taps_at(float gx, float gy, int Ws, int Hs) {
    Taps t;
    if (SAMPLE == SAMPLE_NEAREST) {
        float ix, iy;
        sample_position(gx, gy, Ws, Hs, ix, iy);
        // round half to even (v_rndne_f32), clamped before the int conversion as locate() does
        const int xn = (int)fminf(fmaxf(rintf(ix), -2.f), (float)Ws + 1.f);
        const int yn = (int)fminf(fmaxf(rintf(iy), -2.f), (float)Hs + 1.f);
        t.ok = ((unsigned)xn < (unsigned)Ws && (unsigned)yn < (unsigned)Hs) ? 1u : 0u;
        t.o00 = t.o01 = t.o10 = t.o11 = min(max(yn, 0), Hs - 1) * Ws + min(max(xn, 0), Ws - 1);
        t.wnw = t.wne = t.wsw = t.wse = 0.f;
    } else {
        const Sample s = locate(gx, gy, Ws, Hs);
        const float ex = 1.f - s.tx, ey = 1.f - s.ty;
        t.wnw = ex * ey; t.wne = s.tx * ey; t.wsw = ex * s.ty; t.wse = s.tx * s.ty;
        const bool vx0 = (unsigned)s.x0 < (unsigned)Ws, vx1 = (unsigned)(s.x0 + 1) < (unsigned)Ws;
        const bool vy0 = (unsigned)s.y0 < (unsigned)Hs, vy1 = (unsigned)(s.y0 + 1) < (unsigned)Hs;
        t.ok = (vx0 && vy0 ? 1u : 0u) | (vx1 && vy0 ? 2u : 0u) | (vx0 && vy1 ? 4u : 0u) | (vx1 && vy1 ? 8u : 0u);
        const int xa = min(max(s.x0, 0), Ws - 1), xb = min(max(s.x0 + 1, 0), Ws - 1);
        const int ya = min(max(s.y0, 0), Hs - 1), yb = min(max(s.y0 + 1, 0), Hs - 1);
        t.o00 = ya * Ws + xa; t.o01 = ya * Ws + xb; t.o10 = yb * Ws + xa; t.o11 = yb * Ws + xb;
    }
    return t;
}
// the pixel's value in plane p — the four-corner blend in grid_sample_fwd_kernel's expression order
template <int SAMPLE>
__device__ __forceinline__ float sample_at(const float* __restrict__ p, const Taps& t) {
    if (SAMPLE == SAMPLE_NEAREST) {
        const float r = p[t.o00];
        return (t.ok & 1u) ? r : 0.f;
    }
    const float a = p[t.o00], b = p[t.o01], cc = p[t.o10], d = p[t.o11];
    return ((t.ok & 1u) ? a : 0.f) * t.wnw + ((t.ok & 2u) ? b : 0.f) * t.wne + ((t.ok & 4u) ? cc : 0.f) * t.wsw + ((t.ok & 8u) ? d : 0.f) * t.wse;
}

// VEC: pixels of one row a lane owns per run — 1 (the product: four runs, in four rows of the tile) or 4 (measurement build: one run)
template <int MODE, int SAMPLE, int VEC, bool RESAMPLE>
__global__ __launch_bounds__(RT_THREADS) void warp_resampled_kernel(const float* __restrict__ in, const float* __restrict__ pred,
                                                                    float* __restrict__ out, int C, int Hs, int Ws, int hf, int wf,
                                                                    int Ho, int Wo, float sh, float sw) {
    __shared__ float patch[RESAMPLE ? 2 * RT_PH * RT_PW : 1];
    const int n = blockIdx.z, tid = threadIdx.x;
    const int x0 = blockIdx.x * RT_W, y0 = blockIdx.y * RT_H;
    float th[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (MODE == GRID_AFFINE) {
        affine_theta(pred, n, th);
    }
    const size_t splane = (size_t)Hs * Ws, oplane = (size_t)Ho * Wo;
    const int fplane = RESAMPLE ? hf * wf : 0;
    const float* inN = in + (size_t)n * C * splane;
    float* outN = out + (size_t)n * C * oplane;
    const float* fN = MODE == GRID_UNET ? pred + (size_t)n * 2 * (RESAMPLE ? (size_t)fplane : oplane) : nullptr;

    // ---- the coarse-field texels this tile's pixels tap (tap1d is monotone in the pixel index: the first and the last pixel bound them) ----
    int px0 = 0, py0 = 0;
    bool staged = false;
    if (RESAMPLE) {
        const Tap1D ta = tap1d(x0, wf, sw), tb = tap1d(min(x0 + RT_W, Wo) - 1, wf, sw);
        const Tap1D tc = tap1d(y0, hf, sh), td = tap1d(min(y0 + RT_H, Ho) - 1, hf, sh);
        const int pw = tb.i1 - ta.i0 + 1, ph = td.i1 - tc.i0 + 1;
        px0 = ta.i0;
        py0 = tc.i0;
        staged = pw <= RT_PW && ph <= RT_PH;             // (the same in every lane of the workgroup)
        if (staged) {
            for (int e = tid; e < 2 * ph * RT_PW; e += RT_THREADS) {
                const int cr = e / RT_PW, rx = e - cr * RT_PW;      // cr: channel-major row of the patch
                const int c = cr >= ph ? 1 : 0, ry = cr - c * ph;
                if (rx < pw) patch[(c * RT_PH + ry) * RT_PW + rx] = fN[(size_t)c * fplane + (size_t)(py0 + ry) * wf + px0 + rx];
            }
        }
        __syncthreads();
    }

    constexpr int LPR = RT_W / VEC, ROWS = RT_THREADS / LPR, RUNS = RT_H / ROWS;      // lanes per tile row, rows per pass, passes
#pragma unroll
    for (int i = 0; i < RUNS; ++i) {
        const int h = y0 + tid / LPR + ROWS * i, w0 = x0 + (tid % LPR) * VEC;
        if (h >= Ho || w0 >= Wo) continue;                 // (VEC 4 only with Wo % 4 == 0: a run is inside the row or outside it)
        Taps t[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const int w = w0 + v;
            RegSrc src{0.f, 0.f};                          // the pixel's two grid_src values
            if (MODE == GRID_UNET) {
                if (RESAMPLE) {
                    const Tap1D ty = tap1d(h, hf, sh), tx = tap1d(w, wf, sw);
                    src = staged ? field_at(patch, RT_PW, RT_PH * RT_PW, py0, px0, ty, tx) : field_at(fN, wf, fplane, 0, 0, ty, tx);
                } else {
                    const size_t o = (size_t)h * Wo + w;
                    src = RegSrc{fN[o], fN[oplane + o]};
                }
            }
            float gx, gy;
            grid_coord<MODE>(src, h, w, Ho, Wo, th, gx, gy);
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
void launch_route(const float* in, const float* pred, float* out, int N, int C, int Hs, int Ws, int hf, int wf, int Ho, int Wo, hipStream_t st) {
    const dim3 grid(nemar_cdiv(Wo, RT_W), nemar_cdiv(Ho, RT_H), N), block(RT_THREADS);
    const float sh = (float)hf / (float)Ho, sw = (float)wf / (float)Wo;           // nemar_bilinear_fwd's scales
    NEMAR_AB_ONLY(if (g_register_vec4 && (Wo & 3) == 0 && (((uintptr_t)out) & 15) == 0)
        hipLaunchKernelGGL((warp_resampled_kernel<MODE, SAMPLE, 4, RESAMPLE>), grid, block, 0, st, in, pred, out, C, Hs, Ws, hf, wf, Ho, Wo, sh, sw);
    else)
        hipLaunchKernelGGL((warp_resampled_kernel<MODE, SAMPLE, 1, RESAMPLE>), grid, block, 0, st, in, pred, out, C, Hs, Ws, hf, wf, Ho, Wo, sh, sw);
}

template <int MODE, int SAMPLE>
void launch(const float* in, const float* pred, float* out, int N, int C, int Hs, int Ws, int hf, int wf, int Ho, int Wo, hipStream_t st) {
    if constexpr (MODE == GRID_UNET) {
        if (hf != Ho || wf != Wo) {
            launch_route<MODE, SAMPLE, true>(in, pred, out, N, C, Hs, Ws, hf, wf, Ho, Wo, st);
            return;
        }
    }
    launch_route<MODE, SAMPLE, false>(in, pred, out, N, C, Hs, Ws, hf, wf, Ho, Wo, st);
}

}  // namespace

NEMAR_API int nemar_warp_resampled_fwd(const float* in, const float* pred, int grid_mode, int sample_mode, float* out, int N, int C,
                                       int Hs, int Ws, int hf, int wf, int Ho, int Wo, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(in && pred && out, "warp_resampled_fwd: null pointer");
    NEMAR_REQUIRE(((((uintptr_t)in) | ((uintptr_t)pred) | ((uintptr_t)out)) & 3) == 0,
                  "warp_resampled_fwd: in, pred and out must be 4-byte aligned");
    NEMAR_REQUIRE(grid_mode == GRID_UNET || grid_mode == GRID_AFFINE,
                  "warp_resampled_fwd: grid_mode %d (NEMAR_GRID_UNET or NEMAR_GRID_AFFINE: an explicit grid has no other resolution)", grid_mode);
    NEMAR_REQUIRE(sample_mode == SAMPLE_BILINEAR || sample_mode == SAMPLE_NEAREST, "warp_resampled_fwd: unknown sample_mode %d", sample_mode);
    NEMAR_REQUIRE(N > 0 && C > 0 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0, "warp_resampled_fwd: bad shape N=%d C=%d source %dx%d output %dx%d", N,
                  C, Hs, Ws, Ho, Wo);
    NEMAR_REQUIRE(grid_mode != GRID_UNET || (hf >= 1 && wf >= 1), "warp_resampled_fwd: offset field %d x %d", hf, wf);
    NEMAR_REQUIRE((long long)Hs * Ws < (1ll << 31) && (long long)Ho * Wo < (1ll << 31) && N <= 65535 && nemar_cdiv(Ho, RT_H) <= 65535 &&
                      (grid_mode != GRID_UNET || (long long)hf * wf < (1ll << 30)),
                  "warp_resampled_fwd: plane too large");
    hipStream_t st = (hipStream_t)stream;
    if (grid_mode == GRID_UNET) {
        if (sample_mode == SAMPLE_NEAREST) launch<GRID_UNET, SAMPLE_NEAREST>(in, pred, out, N, C, Hs, Ws, hf, wf, Ho, Wo, st);
        else launch<GRID_UNET, SAMPLE_BILINEAR>(in, pred, out, N, C, Hs, Ws, hf, wf, Ho, Wo, st);
    } else {
        if (sample_mode == SAMPLE_NEAREST) launch<GRID_AFFINE, SAMPLE_NEAREST>(in, pred, out, N, C, Hs, Ws, 1, 1, Ho, Wo, st);
        else launch<GRID_AFFINE, SAMPLE_BILINEAR>(in, pred, out, N, C, Hs, Ws, 1, 1, Ho, Wo, st);
    }
    NEMAR_CHECK_LAUNCH("warp_resampled_fwd");
    return NEMAR_OK;
}
