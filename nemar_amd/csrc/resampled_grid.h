// Where nemar_warp_resampled_fwd samples, for every kernel that must sample THERE: register.hip (the warp itself), score.hip
// (nemar_label_overlap counts the labels that warp would write; nemar_map_points evaluates the grid between the pixels), compose.hip
// (nemar_compose_pred reads one prediction where another samples), regularity.hip (nemar_jacobian_stats differences the positions),
// similarity.hip (nemar_joint_histogram bins the values that warp would write) and, through jacobian_tile.h, fold.hip.  The 64 x 16
// output tile, a prediction as one sample of one launch sees it (PredView: the coarse-field patch a tile stages in LDS and the pixel's
// grid coordinate from it) and the texel(s) that coordinate reads — one statement of the arithmetic on top of warp_grid.h and
// resize_taps.h, so that the kernels cannot drift apart.  The host side of a launch over these tiles is in pred_launch.h.
#pragma once
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

// the CONTINUOUS extension of a prediction's grid at output size (Ho, Wo): the normalised coordinate at the position (px, py), in pixels,
// between or beyond the pixels — at an integer position inside the image, the pixel's own coordinate.  UNET: the align_corners=False resize
// of the sample's field fN [2,hf,wf] evaluated at the position (tap1d_at: the border texel outside the image) added to the linearly
// extended identity; AFFINE: theta applied to the base coordinate.  One statement for score.hip (nemar_map_points: annotated points) and
// compose.hip (nemar_compose_pred: where the second prediction's sampling position reads the first)
template <int MODE>
__device__ __forceinline__ void grid_at(const float* __restrict__ fN, int hf, int wf, float sh, float sw, const float* th, float px, float py,
                                        int Ho, int Wo, float& gx, float& gy) {
    if (MODE == GRID_UNET) {
        const Tap1D ty = tap1d_at(py, hf, sh), tx = tap1d_at(px, wf, sw);
        const RegSrc d = field_at(fN, wf, hf * wf, 0, 0, ty, tx);
        gx = linspace_at(px, Wo) + d.x();
        gy = linspace_at(py, Ho) + d.y();
    } else {
        const float xb = affine_base_at(px, Wo), yb = affine_base_at(py, Ho);
        gx = th[0] * xb + th[1] * yb + th[2];
        gy = th[3] * xb + th[4] * yb + th[5];
    }
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

// ---- the coarse-field texels a tile's pixels tap (tap1d is monotone in the pixel index: the first and the last pixel bound them) ----
struct FieldPatch {
    int px0, py0;      // the patch's first texel in the field
    bool staged;       // the taps fit the LDS patch (the same in every lane of the workgroup); otherwise they are read from global memory
};
// one axis of it: the texels [first, first + count) that the `tile` output pixels from d0 on (cut at n_out) tap in a field of n_in.
// The one statement of the patch geometry: PredView::stage fills it, register.hip's backward reduces into it and finds it again
struct PatchSpan { int first, count; };
__device__ __forceinline__ PatchSpan patch_span(int d0, int tile, int n_in, int n_out, float scale) {
    const Tap1D ta = tap1d(d0, n_in, scale), tb = tap1d(min(d0 + tile, n_out) - 1, n_in, scale);
    return PatchSpan{ta.i0, tb.i1 - ta.i0 + 1};
}

// One prediction as one sample of one launch reads it: everything that is fixed for the launch and the sample.  Built inside the kernel
// from its scalar arguments (pred_view) and indexed with constants only, so that theta and the sizes stay in scalar registers.
// RESAMPLE: the UNet field has another size (hf, wf) than the output (Ho, Wo) and is interpolated; otherwise it is read at the pixel.
template <int MODE, bool RESAMPLE>
struct PredView {
    float th[6];             // AFFINE: theta of the sample
    const float* fN;         // UNET: the sample's field [2,hf,wf] (RESAMPLE) or [2,Ho,Wo]
    int fplane;              // hf * wf when RESAMPLE
    size_t oplane;           // Ho * Wo
    int hf, wf, Ho, Wo;
    float sh, sw;            // nemar_bilinear_fwd's scales hf / Ho, wf / Wo

    // fills `patch` (2 * RT_PH * RT_PW floats of LDS) for the tile at (y0, x0); the caller's __syncthreads() follows.  Nothing to stage
    // without RESAMPLE
    __device__ __forceinline__ FieldPatch stage(float* patch, int x0, int y0, int tid) const {
        if (!RESAMPLE) return FieldPatch{0, 0, false};
        const PatchSpan sx = patch_span(x0, RT_W, wf, Wo, sw), sy = patch_span(y0, RT_H, hf, Ho, sh);
        const int pw = sx.count, ph = sy.count;
        const FieldPatch fp{sx.first, sy.first, pw <= RT_PW && ph <= RT_PH};
        if (fp.staged) {
            for (int e = tid; e < 2 * ph * RT_PW; e += RT_THREADS) {
                const int cr = e / RT_PW, rx = e - cr * RT_PW;      // cr: channel-major row of the patch
                const int c = cr >= ph ? 1 : 0, ry = cr - c * ph;
                if (rx < pw) patch[(c * RT_PH + ry) * RT_PW + rx] = fN[(size_t)c * fplane + (size_t)(fp.py0 + ry) * wf + fp.px0 + rx];
            }
        }
        return fp;
    }
    // the normalised grid coordinate of output pixel (h, w): the field value (UNET: interpolated from the patch or the global field when
    // RESAMPLE, read at the pixel otherwise) added to the identity, or theta applied (AFFINE)
    __device__ __forceinline__ void coord(const float* patch, const FieldPatch& fp, int h, int w, float& gx, float& gy) const {
        RegSrc src{0.f, 0.f};                          // the pixel's two grid_src values
        if (MODE == GRID_UNET) {
            if (RESAMPLE) {
                const Tap1D ty = tap1d(h, hf, sh), tx = tap1d(w, wf, sw);
                src = fp.staged ? field_at(patch, RT_PW, RT_PH * RT_PW, fp.py0, fp.px0, ty, tx) : field_at(fN, wf, fplane, 0, 0, ty, tx);
            } else {
                const size_t o = (size_t)h * Wo + w;
                src = RegSrc{fN[o], fN[oplane + o]};
            }
        }
        grid_coord<MODE>(src, h, w, Ho, Wo, th, gx, gy);
    }
    // the same coordinate where no staged patch covers the pixel: always the global field (jacobian_tile.h; regularity.hip's halo takes
    // this path per lane, through coord with the patch switched off)
    __device__ __forceinline__ void coord_unstaged(int h, int w, float& gx, float& gy) const {
        coord(nullptr, FieldPatch{0, 0, false}, h, w, gx, gy);
    }
};

// the view of sample n of `pred` (UNET: the field [N,2,hf,wf]; AFFINE: dtheta [N,6], hf = wf = 1)
template <int MODE, bool RESAMPLE>
__device__ __forceinline__ PredView<MODE, RESAMPLE> pred_view(const float* __restrict__ pred, int n, int hf, int wf, int Ho, int Wo, float sh,
                                                              float sw) {
    PredView<MODE, RESAMPLE> v{{0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, nullptr, RESAMPLE ? hf * wf : 0, (size_t)Ho * Wo, hf, wf, Ho, Wo, sh, sw};
    if (MODE == GRID_AFFINE) {
        affine_theta(pred, n, v.th);
    }
    if (MODE == GRID_UNET) v.fN = pred + (size_t)n * 2 * (RESAMPLE ? (size_t)v.fplane : v.oplane);
    return v;
}

}  // namespace
