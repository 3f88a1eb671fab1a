// The host side of a launch that applies a prediction to resampled_grid.h's 64 x 16 output tiles, for every entry point that makes one
// (register.hip, score.hip, compose.hip, regularity.hip, similarity.hip): what a prediction and an output plane must satisfy, which
// PredView<MODE, RESAMPLE> serves the call, and how many workgroups a tile-walking kernel gets.
#pragma once
#include <type_traits>

#include "resampled_grid.h"

namespace {

// ---- refusals: false with nemar_last_error() set to "<entry>: ...".  What only one entry point needs (aliasing, class and bin counts,
// ranges, workspace sizes) stays with it ----
// a prediction that has a resolution of its own (`what`: "" or which of two predictions): a known mode, a field the kernels can index
inline bool pred_ok(const char* entry, const char* what, int grid_mode, int hf, int wf) {
    if (grid_mode != GRID_UNET && grid_mode != GRID_AFFINE) {
        nemar_set_error("%s: %sgrid_mode %d (NEMAR_GRID_UNET or NEMAR_GRID_AFFINE: an explicit grid has no other resolution)", entry, what, grid_mode);
    } else if (grid_mode == GRID_UNET && (hf < 1 || wf < 1)) {
        nemar_set_error("%s: %soffset field %d x %d", entry, what, hf, wf);
    } else if (grid_mode == GRID_UNET && (long long)hf * wf >= (1ll << 30)) {
        nemar_set_error("%s: %soffset field %d x %d too large", entry, what, hf, wf);
    } else {
        return true;
    }
    return false;
}
// N planes of Ho x Wo pixels that one grid of tiles covers: pixel offsets fit an int, samples and tile rows fit a grid dimension
inline bool tile_grid_ok(const char* entry, int N, int Ho, int Wo) {
    if ((long long)Ho * Wo < (1ll << 31) && N <= 65535 && nemar_cdiv(Ho, RT_H) <= 65535) return true;
    nemar_set_error("%s: plane too large (N=%d output %dx%d)", entry, N, Ho, Wo);
    return false;
}
#define NEMAR_REQUIRE_OK(ok) do { if (!(ok)) return NEMAR_EINVAL; } while (0)

// ---- the route of a checked prediction at output size (Ho, Wo): calls f(mode, resample, hf, wf, sh, sw) once, `mode` and `resample`
// carrying PredView's template arguments as std::integral_constant values, (sh, sw) nemar_bilinear_fwd's scales of the field to the output.
// AFFINE has no field: hf = wf = 1 ----
template <class F>
void dispatch_pred(int grid_mode, int hf, int wf, int Ho, int Wo, F&& f) {
    if (grid_mode == GRID_AFFINE) hf = wf = 1;
    const float sh = (float)hf / (float)Ho, sw = (float)wf / (float)Wo;
    using Unet = std::integral_constant<int, GRID_UNET>;
    if (grid_mode == GRID_AFFINE) f(std::integral_constant<int, GRID_AFFINE>{}, std::false_type{}, hf, wf, sh, sw);
    else if (hf != Ho || wf != Wo) f(Unet{}, std::true_type{}, hf, wf, sh, sw);
    else f(Unet{}, std::false_type{}, hf, wf, sh, sw);
}

// ---- workgroups per sample of a kernel that walks a sample's tiles (tiles >= 1) with per-workgroup LDS state it clears and flushes:
// what the chip holds AT ONCE and no more — 256 CUs x the workgroups whose LDS fits a CU, shared among the N samples; a grid one
// workgroup per CU larger runs a second, nearly empty round and takes almost twice as long ----
inline int resident_groups(int N, int workgroups_per_cu, long long tiles) {
    const int share = 256 * workgroups_per_cu / N > 0 ? 256 * workgroups_per_cu / N : 1;
    return tiles < share ? (int)tiles : share;
}

}  // namespace
