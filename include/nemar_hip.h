/* nemar_hip.h — C ABI of libnemar_hip.so: the gfx950 (MI355X / CDNA4) operator library behind the NeMAR
 * training step, NEMARModel.optimize_parameters() (reference models/nemar_model.py:266-288).
 *
 * The reference has no FFI of its own: its operator boundary is the set of torch call sites listed in
 * SURVEY.md §2.2 (K1..K15).  Each entry point below replaces one of those call sites and cites it.
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch types.  Every pointer is DEVICE memory owned by the caller;
 *     tensors are contiguous NCHW float32.  The library never allocates, frees or synchronises.
 *   - every launch goes on `stream` (a hipStream_t passed as void*; NULL = the null stream), so the caller's
 *     stream ordering (torch's current stream under autograd) holds.  Re-entrant per stream: every input of an operator —
 *     including the side inputs of the wide-layer route (scratch arena, max words, planes: nemar_conv_extras) — travels with
 *     the call.  The only process-global state are the recorded weight-pack plans
 *     (the measurement switches of earlier versions live in a separate build of the library: nemar_hip_ab.h).
 *   - return value: 0 on success, negative on error (NEMAR_EINVAL bad shape/pointer/unsupported,
 *     NEMAR_ELAUNCH HIP launch error, NEMAR_EWORKSPACE workspace too small); nemar_last_error() returns the
 *     message of the calling thread's last failure.  Python glue raises on non-zero.
 *   - gradients are WRITTEN unless the matching `accumulate` flag is non-zero (then added in place).
 *   - scratch: ops that need it take (workspace, ws_bytes) and export nemar_<op>_workspace(...) -> bytes.
 */
#ifndef NEMAR_HIP_H
#define NEMAR_HIP_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NEMAR_OK 0
#define NEMAR_EINVAL (-1)
#define NEMAR_ELAUNCH (-2)
#define NEMAR_EWORKSPACE (-3)

/* library */
int nemar_version(void);              /* major*10000 + minor*100 + patch; 618 = this header (0.4.x exported nemar_tune*) */
const char* nemar_last_error(void);   /* thread-local message of the last failing call */

/* ---- K9/K10/K11: sampling-grid generation fused into bilinear grid_sample ------------------------------
 * F.grid_sample(img, grid, 'bilinear', 'zeros', align_corners=False)
 *     reference models/stn/unet_stn.py:173-174, models/stn/affine_stn.py:129-130
 * grid_mode selects how the (never materialised) grid is synthesised from grid_src:
 *   NEMAR_GRID_EXPLICIT  grid_src = grid [N,Ho,Wo,2] (x,y), normalised coordinates
 *   NEMAR_GRID_UNET      grid_src = offsets [N,2,Ho,Wo] planar; grid = linspace(-1,1) identity + offsets
 *                        (reference models/stn/unet_stn.py:121-129,167; channel 0 = x)
 *   NEMAR_GRID_AFFINE    grid_src = dtheta [N,6]; theta = dtheta + [1,0,0,0,1,0];
 *                        grid = F.affine_grid(theta, align_corners=False) (models/stn/affine_stn.py:122,128)
 * in [N,C,H,W] -> out [N,C,Ho,Wo]. */
#define NEMAR_GRID_EXPLICIT 0
#define NEMAR_GRID_UNET 1
#define NEMAR_GRID_AFFINE 2
int nemar_grid_sample_fwd(const float* in, const float* grid_src, int grid_mode, float* out,
                          int N, int C, int H, int W, int Ho, int Wo, void* stream);
/* gin [N,C,H,W] may be NULL (source is data, e.g. real_A).  ggrid has the layout of grid_src
 * (EXPLICIT [N,Ho,Wo,2]; UNET [N,2,Ho,Wo]; AFFINE [N,6]).
 * With a workspace (and same-size input/output, C <= 4: the training path) grad_input is computed WITHOUT floating-point
 * atomics and is bitwise reproducible: a gather per 64x16 destination tile for pixels that sample within 3 texels of their
 * own position, 64-bit fixed-point atomics (40 bits below max |gout|) for the others; the affine grid gradient is summed
 * in a fixed order.  Workspace contract: nemar_grid_sample_bwd_workspace() bytes, of which the leading
 * nemar_grid_sample_bwd_zeroed_bytes() must be ZERO on entry of the first call and are left zero by every call (the
 * fixed-point accumulator); the rest is scratch.  workspace == NULL: fp32-atomic scatter (any shape; not reproducible).
 * Range of the fixed-point path.  A contribution w * gout is rounded to a multiple of 2^(e - 40), 2^(e-1) <= m < 2^e, m the largest
 * |gout| of the tiles that have such pixels (at most the call's): an error of at most 2^-40 * max |gout| each.  That holds for
 * 2^-81 <= m and up to the largest finite float; e is clamped at -80, so below that (m = 0 included) the step is 2^-120 whatever m
 * is.  Scaling gout by a power of two scales gin and ggrid by it bit for bit while m stays in that range and nothing leaves the
 * normal floats.  Headroom: the accumulator holds (contributions to one texel) * 2^40 and must stay below 2^63, i.e. fewer than 2^23
 * output pixels may land on one texel.
 * Non-finite data.  Whatever gout and grid_src hold, the call returns NEMAR_OK, the zeroed bytes come back zero and the next call on
 * the workspace is what it would be on a fresh one.  A NaN or Inf in gout reaches d loss / d grid of its own pixel (NaN or +-Inf) and
 * the at most four texels of its channel that the pixel samples: NaN or +-Inf from the gather, and from the fixed-point path NaN, +-Inf
 * or a finite value without meaning (the conversion of a NaN or Inf to the accumulator's integer is not specified).  Everything else
 * keeps the bound above — with one exception: an INFINITE gout in a tile that has fixed-point pixels becomes m, and every finite
 * fixed-point contribution of that call then rounds to zero (finite, but the far part of grad_input is lost).  A NaN never becomes m.
 * A non-finite grid_src value sends its pixel outside the plane: no contribution to grad_input, NaN or 0 in its own ggrid elements
 * (nemar_grid_sample_fwd writes NaN for that pixel where torch writes 0). */
size_t nemar_grid_sample_bwd_workspace(int N, int C, int H, int W);
size_t nemar_grid_sample_bwd_zeroed_bytes(int N, int C, int H, int W);
int nemar_grid_sample_bwd(const float* in, const float* grid_src, int grid_mode, const float* gout,
                          float* gin, int accum_gin, float* ggrid, int accum_ggrid,
                          int N, int C, int H, int W, int Ho, int Wo, void* workspace, size_t ws_bytes, void* stream);

/* ---- K12: deformation smoothness / bilateral regulariser -------------------------------------------------
 * smoothness_loss(deformation, img, alpha)   reference models/stn/stn_losses.py:4-30,
 * called from UnetSTN._calculate_regularization_term, models/stn/unet_stn.py:179-201.
 * d [N,2,H,W]; img [N,Ci,H,W] or NULL (alpha<=0 or NULL => unweighted).
 * fwd: loss[0] = (accumulate ? loss[0] : 0) + factor * smoothness(d, img, alpha)
 * bwd: gd (+)= gscale[0] * factor * d smoothness / d d     (gscale: device scalar, the upstream gradient) */
size_t nemar_smoothness_workspace(int N, int H, int W);
int nemar_smoothness_fwd(const float* d, const float* img, int Ci, float alpha, float factor,
                         float* loss, int accumulate, void* workspace, size_t ws_bytes,
                         int N, int H, int W, void* stream);
int nemar_smoothness_bwd(const float* d, const float* img, int Ci, float alpha, const float* gscale,
                         float factor, float* gd, int accumulate, int N, int H, int W, void* stream);

/* Fold penalty (csrc/fold.hip; not in the reference, whose only regulariser is the smoothness term above): a hinge on the Jacobian
 * determinant nemar_jacobian_stats measures, as a differentiable loss on a UNet offset field.  d [N,2,H,W], channel 0 = x, taken at the
 * size the warp reads it (NEMAR_GRID_UNET).  For pixel (h,w):
 *   g   = (linspace(-1,1,W)[w] + d[n,0,h,w], linspace(-1,1,H)[h] + d[n,1,h,w])        the warp's normalised coordinate (the same bits)
 *   p   = ((g.x + 1) * W - 1) / 2, ((g.y + 1) * H - 1) / 2                             the position it samples, in pixels
 *   a   = p(h,w+1) - p(h,w),  b = p(h+1,w) - p(h,w),  det = a.x * b.y - b.x * a.y      the bits nemar_jacobian_stats computes with
 *                                                                                      NEMAR_GRID_UNET at hf = Ho = H, wf = Wo = W
 *   interior = h < H-1 and w < W-1;  M = N (H-1) (W-1).
 * fwd: loss[0] = (accumulate ? loss[0] : 0) + factor / M * sum over the interior pixels of max(0, margin - det);
 *      active [N] uint32: active[n] = #(interior pixels of sample n with det <= margin) — with margin = 0, nemar_jacobian_stats' fold count.
 *      M = 0 (H == 1 or W == 1): the sum is 0 and active = 0, both WRITTEN.  Per-workgroup records (one per 64 x 16 tile) go to the
 *      workspace and are merged in a fixed order: no atomics, bitwise repeatable.
 * bwd: gd [N,2,H,W] (+)= gscale[0] * d loss / d d (gscale: device scalar, the upstream gradient).  The hinge has slope -1 where
 *      det < margin and 0 elsewhere, equality included (torch's relu).  With s(h,w) = -gscale[0] * factor / M on such interior pixels, 0 elsewhere:
 *        gd[n,0,h,w] = (W/2) * [ s(h,w) * (a.y - b.y)(h,w) + s(h,w-1) * b.y(h,w-1) + s(h-1,w) * (-a.y)(h-1,w) ]
 *        gd[n,1,h,w] = (H/2) * [ s(h,w) * (b.x - a.x)(h,w) + s(h,w-1) * (-b.x)(h,w-1) + s(h-1,w) * a.x(h-1,w) ]
 *      — the texel as p(h,w) of its own pixel, as p(h,w+1) of the left one, as p(h+1,w) of the upper one; a term whose pixel does not
 *      exist or is not interior is absent; the three are added in this order.  M = 0: all zeros, written.  A gather: no atomics, no workspace.
 * NEMAR_EINVAL, nothing launched: a required pointer NULL (d, loss, active, workspace; d, gscale, gd) or not 4-byte aligned (all the
 * alignment asked for); a non-positive N, H or W; N > 65535; H*W >= 2^31; H > 16 * 65535; gd equal to d;
 * ws_bytes < nemar_fold_penalty_workspace(). */
size_t nemar_fold_penalty_workspace(int N, int H, int W);
int nemar_fold_penalty_fwd(const float* d, float margin, float factor, float* loss, int accumulate, unsigned* active, void* workspace,
                           size_t ws_bytes, int N, int H, int W, void* stream);
int nemar_fold_penalty_bwd(const float* d, float margin, const float* gscale, float factor, float* gd, int accumulate, int N, int H,
                           int W, void* stream);

/* EPE loss (csrc/epe.hip; not in the reference, which has no ground-truth field): the residual nemar_registration_error measures, as a
 * differentiable loss on the prediction the warp reads.  pred: NEMAR_GRID_UNET offsets [N,2,H,W] or NEMAR_GRID_AFFINE dtheta [N,6];
 * g [N,2,H,W] the ground-truth field IN PIXELS, channel 0 = x.  For output pixel x = (w, h) of sample n:
 *   S    = (ix, iy), the position the warp samples (the bits of nemar_grid_sample_fwd and nemar_registration_error)
 *   g(S)   read bilinearly with the position clamped into the image, as nemar_registration_error reads it:
 *          cx = min(max(ix, 0), W-1), xa = floor(cx), xb = min(xa + 1, W-1), tx = cx - xa; likewise in y
 *   r    = (ix - w + g_x(S), iy - h + g_y(S)),   rho = sqrt(r.x^2 + r.y^2 + eps^2)     (Charbonnier; eps = 0: the meter's |r|, whose
 *                                                                                        gradient at r = 0 is NaN)
 * fwd: loss[0] = (accumulate ? loss[0] : 0) + factor / (N H W) * sum of rho over ALL pixels — not the meter's valid-only mean: a sample
 *      that left the image is not excused; the clamped read extends g by its border value and the residual grows with the distance.
 *      One float per workgroup goes to the workspace, merged in a fixed order: no atomics, bitwise repeatable.
 * bwd: with u = r / rho and the slope of the cell floor() chose, dg/dix = (1-ty) (g01 - g00) + ty (g11 - g10) — exactly 0 where ix < 0 or
 *      ix > W-1 (the clamp), and 0 where xa == xb — likewise in y:
 *        Dx = u.x (1 + dx g_x) + u.y dx g_y,   Dy = u.x dy g_x + u.y (1 + dy g_y),   k = gscale[0] * factor / (N H W)
 *      (gscale: device scalar, the upstream gradient).
 *      UNET:   gpred[n,0,h,w] (+)= k (W/2) Dx,  gpred[n,1,h,w] (+)= k (H/2) Dy — one gather launch that does not touch the workspace.
 *      AFFINE: gpred[n,0..5] (+)= k * sum over (h,w) of [(W/2) Dx (xb, yb, 1), (H/2) Dy (xb, yb, 1)], xb = (2w+1)/W - 1, yb = (2h+1)/H - 1
 *              (affine_grid's base coordinates); one 6-vector per workgroup goes to the workspace, merged in a fixed order.
 *      No atomics in either: bitwise repeatable.
 * NEMAR_EINVAL, nothing launched, outputs untouched: a pointer NULL or not 4-byte aligned (all the alignment asked for; both calls want
 * the workspace, whichever mode); a grid_mode other than the two; a non-positive N, H or W; N > 65535; H*W >= 2^31;
 * ws_bytes < nemar_epe_loss_workspace(); gpred equal to pred; eps < 0 or not finite.
 * Non-finite data: NEMAR_OK, and NaN or Inf in exactly what hears from it — the loss; for UNET the two gradient elements of a pixel whose
 * offsets or whose four read texels of g hold it; for AFFINE the six of a sample.  No address depends on it. */
size_t nemar_epe_loss_workspace(int N, int H, int W);
int nemar_epe_loss_fwd(const float* pred, int grid_mode, const float* g, float eps, float factor, float* loss, int accumulate,
                       void* workspace, size_t ws_bytes, int N, int H, int W, void* stream);
int nemar_epe_loss_bwd(const float* pred, int grid_mode, const float* g, float eps, const float* gscale, float factor, float* gpred,
                       int accumulate, void* workspace, size_t ws_bytes, int N, int H, int W, void* stream);

/* Soft-Dice loss (csrc/dice.hip; not in the reference, which has no labels): the Dice nemar_label_overlap reports, as a differentiable loss
 * on the prediction the warp reads.  pred: NEMAR_GRID_UNET offsets [N,2,H,W] or NEMAR_GRID_AFFINE dtheta [N,6]; labels_moving and
 * labels_fixed [N,H,W]: float class ids by nemar_label_overlap's rule (k iff the value == (float)k for an integer 0 <= k < K, anything
 * else — negative, >= K, fractional, NaN, Inf — is no class).  For output pixel x of sample n:
 *   S      = (ix, iy), the position the warp samples (the bits of nemar_grid_sample_fwd), x0 = floor(ix), tx = ix - x0, likewise in y;
 *   p_k(x) = the sum of the bilinear weights (1-tx)(1-ty), tx(1-ty), (1-tx)ty, tx ty of those of the four corners (y0,x0), (y0,x0+1),
 *            (y0+1,x0), (y0+1,x0+1) that lie INSIDE the image (zeros padding, as the image warp) and whose class in labels_moving is k;
 *   f_k(x) = [class of labels_fixed[x] == k];
 *   per sample and class  I = sum_x p_k f_k,  M = sum_x p_k,  F = sum_x f_k;
 *   dice = (2 I + eps) / (M + F + eps), eps > 0 in pixels;
 *   loss = factor / (N Kc) * sum_n sum_{k >= k0} (1 - dice), k0 = 0 or 1 (1 leaves the background class 0 out), Kc = K - k0.
 * A class absent from both maps has dice 1 and gradient 0; the denominator does not depend on the data.
 * A pixel whose ix or iy is NOT FINITE contributes nothing to I and M and gets gradient exactly 0 (its f_k still counts) — unlike
 * nemar_epe_loss_*, which is NaN where it hears from one: the sums are integers and cannot carry a NaN.  No address depends on the data
 * beyond the clamped corner reads.
 * nemar_dice_sums: sums [N,K,3] uint64 = I and M in fixed point with 30 fractional bits (every corner weight rounded once to nearest,
 *      then added as an integer: H W < 2^31 pixels of total weight <= 1 plus four half-unit roundings stay below 2^63), F a plain pixel
 *      count.  Integer atomics: independent of the order of arrival, bitwise repeatable, the same bits for aligned and unaligned tensors.
 * nemar_dice_loss_fwd: the sums, then one finalising workgroup that converts them in double, adds the terms in a fixed order,
 *      loss[0] = (accumulate ? loss[0] : 0) + loss, and writes coef [N,K,2] float for the backward: with D = M + F + eps, c = factor / (N Kc),
 *      a = -2 c / D, b = c (2 I + eps) / D^2 (both 0 for k < k0), so that dL/dp_k(x) = a f_k(x) + b.
 * nemar_dice_loss_bwd: a gather that reads coef and does not repeat the sums.  Per pixel q_c = a[k_c] [k_c == kf] + b[k_c] for the four
 *      corners (0 outside the image or of no class), dL/dix = (1-ty)(q01 - q00) + ty (q11 - q10), dL/diy = (1-tx)(q10 - q00) + tx (q11 - q01):
 *      the slope of the cell floor() chose.  gscale: device scalar, the upstream gradient.
 *      UNET:   gpred[n,0,h,w] (+)= gscale[0] (W/2) dL/dix,  gpred[n,1,h,w] (+)= gscale[0] (H/2) dL/diy — one launch, no workspace use.
 *      AFFINE: gpred[n,0..5] (+)= gscale[0] * sum over (h,w) of [(W/2) dL/dix (xb, yb, 1), (H/2) dL/diy (xb, yb, 1)], (xb, yb) affine_grid's
 *              base coordinates; one 6-vector per workgroup goes to the workspace, merged in a fixed order.  No float atomics anywhere.
 * NEMAR_EINVAL, nothing launched, outputs untouched: a pointer NULL or not 4-byte aligned (sums: 8-byte); a grid_mode other than the two;
 * K outside 1 .. 1024; k0 not 0 or 1, or k0 >= K; eps not finite or <= 0; a non-positive N, H or W; N > 65535; H*W >= 2^31;
 * ws_bytes < nemar_dice_loss_workspace(); gpred equal to pred. */
size_t nemar_dice_loss_workspace(int N, int H, int W);
int nemar_dice_sums(const float* pred, int grid_mode, const float* labels_moving, const float* labels_fixed, unsigned long long* sums,
                    int N, int K, int H, int W, void* stream);
int nemar_dice_loss_fwd(const float* pred, int grid_mode, const float* labels_moving, const float* labels_fixed, int K, int k0, float eps,
                        float factor, float* loss, int accumulate, unsigned long long* sums, float* coef, int N, int H, int W, void* stream);
int nemar_dice_loss_bwd(const float* pred, int grid_mode, const float* labels_moving, const float* labels_fixed, const float* coef, int K,
                        const float* gscale, float* gpred, int accumulate, void* workspace, size_t ws_bytes, int N, int H, int W,
                        void* stream);

/* Local NCC (csrc/local_ncc.hip; not a call site of the reference, whose image terms are global L1 losses): a windowed normalised
 * cross-correlation as a differentiable loss.  x, y [N,C,H,W], planar.  win: odd window size, 3 <= win <= 11, radius r = win / 2.  For
 * pixel p of plane (n,c) the window Omega(p) is the in-image part of the win x win square centred at p and n(p) = |Omega(p)| its pixel
 * count: there is no zero padding, so every statistic below is invariant to a constant added to x or to y.
 *   mx = sum_Omega x / n,  my = sum_Omega y / n
 *   vx = max(0, sum_Omega x^2 / n - mx^2),  vy likewise,  cov = sum_Omega x y / n - mx my
 *   cc(p) = cov^2 / (vx vy + eps)
 * fwd: loss[0] = (accumulate ? loss[0] : 0) + factor * (1 - (1/M) sum_p cc(p)),  M = N C H W;  cc_map [N,C,H,W] = cc, or NULL.
 *      One record per workgroup (a 64 x 16 tile of one plane) goes to the workspace, the records are merged in a fixed order: no atomics,
 *      bitwise repeatable.  Every window is summed directly (no running window).
 * bwd: with D = vx vy + eps and, at every pixel p,
 *        alpha = 2 cov / D,  beta = -2 cov^2 vy / D^2,  gamma = -(alpha my + beta mx),  each divided by n(p)
 *      (the clamp at 0 is taken as the identity it is mathematically: it only keeps D >= eps)
 *        gx(q) (+)= -gscale[0] * factor / M * ( y(q) Box(alpha)(q) + x(q) Box(beta)(q) + Box(gamma)(q) )
 *      Box sums over the in-image pixels within radius r of q; gscale: device scalar, the upstream gradient.  gy [N,C,H,W] or NULL: the
 *      same with the roles of x and y swapped.  One launch, a gather: no atomics, no workspace, bitwise repeatable.
 * The kernels subtract a constant per tile from x and y before anything is squared (the mean of the staged patch), which the definition's
 * shift invariance allows; results therefore differ in the last bits from an evaluation of the formulas on the raw values.
 * NEMAR_EINVAL, nothing launched: win even or outside 3..11; eps <= 0 (or NaN); a required pointer NULL (x, y, loss, workspace; x, y,
 * gscale, gx) or any pointer not 4-byte aligned (all the alignment asked for); a non-positive N, C, H or W; N*C > 65535; H*W >= 2^31;
 * cc_map, gx or gy overlapping x or y, gy overlapping gx; ws_bytes < nemar_local_ncc_workspace() (which is 0 for arguments the calls
 * refuse).  Non-finite input: NEMAR_OK, NaN or Inf in the outputs that hear from it, no access outside the buffers (no index depends on
 * the data). */
size_t nemar_local_ncc_workspace(int N, int C, int H, int W, int win);
int nemar_local_ncc_fwd(const float* x, const float* y, int win, float eps, float factor, float* loss, int accumulate, float* cc_map,
                        void* workspace, size_t ws_bytes, int N, int C, int H, int W, void* stream);
int nemar_local_ncc_bwd(const float* x, const float* y, int win, float eps, const float* gscale, float factor, float* gx, float* gy,
                        int accumulate, int N, int C, int H, int W, void* stream);

/* MIND (csrc/mind.hip; not a call site of the reference, whose image terms compare two images of one modality): the modality-independent
 * neighbourhood descriptor (Heinrich et al. 2012) as a differentiable loss between two modalities.  x [N,Cx,H,W], y [N,Cy,H,W], planar;
 * Cx and Cy may differ.  Each image enters through its channel mean, as in nemar_joint_histogram: g(q) = (1/C) sum_c img[n,c,q].
 * patch: 3 or 5, radius p = patch / 2.  dil: 1 or 2.  eps > 0.  The four search offsets s = (0,-dil), (0,+dil), (-dil,0), (+dil,0) as
 * (dy, dx), in that order.
 *   E_s(q) = ( g(q) - g(clamp(q + s)) )^2           q in the image; clamp = each coordinate to [0,H-1] / [0,W-1]
 *   D_s(u) = (1 / n(u)) sum_{q in Omega(u)} E_s(q)   Omega(u) = the in-image part of the patch x patch square at u, n(u) = |Omega(u)|
 *                                                    (no zero padding)
 *   V(u)   = (1/4) sum_s D_s(u)
 *   m_s(u) = exp( -D_s(u) / (V(u) + eps) )
 *   dm(u)  = (1/4) sum_s ( m_s^x(u) - m_s^y(u) )^2
 *   loss   = factor * (1 / (N H W)) sum_{n,u} dm(u)
 * This is MIND without the division by max_s m_s (equivalently without the - min_s D_s): that step has a kink wherever two D_s tie, and
 * the descriptors stay bounded without it (sum_s D_s / V = 4).  Every quantity is invariant to a constant added to x or to y, and the
 * map is symmetric in x and y.  exp is the library's expf, not the hardware approximation.
 * fwd: loss[0] = (accumulate ? loss[0] : 0) + loss;  dm_map [N,1,H,W] = dm, or NULL.  One record per workgroup (a 32 x 16 tile of one
 *      sample) goes to the workspace, the records are merged in a fixed order: no atomics, bitwise repeatable.
 * bwd: with c = factor / (4 N H W),
 *        a_s(u) = 2 c (m_s^x - m_s^y)
 *        b_s(u) = -a_s m_s / (V + eps) + (1 / (4 (V + eps)^2)) sum_r a_r m_r D_r
 *        e_s(q) = sum_{u : q in Omega(u)} b_s(u) / n(u)
 *        dL/dg(t) = sum_s [ 2 e_s(t) (g(t) - g(clamp(t + s))) - sum_{q : clamp(q + s) = t} 2 e_s(q) (g(q) - g(t)) ]
 *        gx[n,c,t] (+)= gscale[0] * dL/dg(t) / Cx, the same value for every channel
 *      (m, V, D those of x; the inner sum has one term in the interior, q = t - s, and up to dil + 1 on the border rows or columns that
 *      the clamp maps onto).  gscale: device scalar, the upstream gradient.  gy [N,Cy,H,W] or NULL: the same with the roles of x and y
 *      swapped.  One launch on 32 x 16 tiles with a halo of 2 (p + dil), a gather: no atomics, no workspace, bitwise repeatable.
 * NEMAR_EINVAL, nothing launched: patch not 3 or 5; dil not 1 or 2; eps <= 0 (or NaN); a required pointer NULL (x, y, loss, workspace;
 * x, y, gscale, gx) or any pointer not 4-byte aligned (all the alignment asked for; rows are read with 16-byte loads where the base is
 * 16-byte aligned and W % 4 == 0); a non-positive N, Cx, Cy, H or W; N > 65535; H*W >= 2^31; dm_map, gx or gy overlapping x or y, gy
 * overlapping gx; ws_bytes < nemar_mind_loss_workspace() (which is 0 for arguments the calls refuse).  Non-finite input: NEMAR_OK, NaN
 * or Inf in the outputs that hear from it (within p + dil of it forward, 2 (p + dil) backward), no access outside the buffers (no index
 * depends on the data). */
size_t nemar_mind_loss_workspace(int N, int H, int W, int patch, int dil);
int nemar_mind_loss_fwd(const float* x, int Cx, const float* y, int Cy, int patch, int dil, float eps, float factor, float* loss,
                        int accumulate, float* dm_map, void* workspace, size_t ws_bytes, int N, int H, int W, void* stream);
int nemar_mind_loss_bwd(const float* x, int Cx, const float* y, int Cy, int patch, int dil, float eps, const float* gscale, float factor,
                        float* gx, float* gy, int accumulate, int N, int H, int W, void* stream);

/* Scaling and squaring (csrc/integrate.hip; not in the reference, whose UNet STN warps with the network's output as it is): the network's
 * output as a stationary velocity field v, the warp reads exp(v).  One squaring step on a displacement field u [N,2,H,W], planar, in the
 * units of NEMAR_GRID_UNET offsets.  Channel 0 times W/2 and channel 1 times H/2 are pixels.  s is a scale:
 *   a      = s * u                                   (one fp32 product; s == 1 leaves the bits alone)
 *   p(h,w) = ( clamp(w + a0(h,w) * W/2, 0, W-1),  clamp(h + a1(h,w) * H/2, 0, H-1) )
 *   out(h,w) = a(h,w) + bilinear(a, p(h,w))          both channels, align_corners=True texel centres (true identity: a zero field
 *                                                    samples its own texel), border texel outside the image
 * The zoom of linspace(-1,1) under align_corners=False (what NEMAR_GRID_UNET adds to the offsets) stays where it is, in the final warp
 * only: the integration itself uses a true identity, K squarings would otherwise apply that zoom 2^K times.  bilinear: x0 = floor(p.x),
 * x1 = min(x0 + 1, W-1), t = p.x - x0 (the same in y), a00 (1-tx)(1-ty) + a01 tx (1-ty) + a10 (1-tx) ty + a11 tx ty.  Positions are
 * clamped in float before the integer conversion (NaN -> 0): no input value indexes outside the plane.
 * Gradient with respect to u given gout: three parts, each times s.
 *   The direct term is gout(x).
 *   The image path is w_k(x') * gout(x') scattered into the four corners of every p(x').
 *   The position path at the texel itself is sum_ch gout_ch(x) * d bilinear_ch / d p_c * (W/2 or H/2) * s.  It is zero along an axis
 *   whose raw position was clamped (raw < 0 or raw > size-1).
 * bwd: gu = (accumulate ? gu : 0) + s * ((direct + position) + image), the bracket rounded to fp32 before it is added.  The image path
 * goes through 64-bit fixed-point integer atomics into the zeroed leading bytes of the workspace — each w * gout rounded to a multiple of
 * 2^(e - FIX), 2^(e-1) <= max |gout| of the call < 2^e (found on the device; e clamped at -80), FIX = min(40, 62 - ceil(log2(H W))): no
 * overflow even if every pixel of a plane lands on one texel — no fp32 atomics: bitwise repeatable, whatever the field.  No host sync.
 * Workspace: nemar_svf_step_bwd_workspace() bytes, 8-byte aligned, whose first nemar_svf_step_bwd_zeroed_bytes() are zero on entry and
 * left zero on return (the contract of nemar_grid_sample_bwd_workspace); the rest is scratch.  Non-finite u or gout: NEMAR_OK, nothing
 * outside the buffers is touched, the zeroed bytes come back zero; the values have no meaning.
 * Chain: integrate(v, K, sign) is u_0 = v, then K steps.  The first step carries s = sign / 2^K and the others s = 1.  K = 0 is the
 * identity (sign * v).  sign = -1 gives exp(-v), the inverse of exp(v) in this true-identity convention (it does not undo the warp's
 * zoom).
 * NEMAR_EINVAL, nothing launched: a required pointer NULL or misaligned; a non-positive N, H or W; N > 65535; H*W >= 2^31;
 * H > 16 * 65535; out == u; gu == u; gu == gout; ws_bytes < nemar_svf_step_bwd_workspace(). */
int nemar_svf_step_fwd(const float* u, float scale, float* out, int N, int H, int W, void* stream);
size_t nemar_svf_step_bwd_workspace(int N, int H, int W);
size_t nemar_svf_step_bwd_zeroed_bytes(int N, int H, int W);
int nemar_svf_step_bwd(const float* u, float scale, const float* gout, float* gu, int accumulate, void* workspace, size_t ws_bytes,
                       int N, int H, int W, void* stream);

/* ---- K1/K2/K4/K8: convolution family on fp32 MFMA (exact fp32) ---------------------------------------------
 * nn.Conv2d / nn.ConvTranspose2d with the ReflectionPad2d and torch.cat feeding them folded in —
 *     reference models/networks.py:349-377 (ResnetGenerator), :418-439 (ResnetBlock), :576-597
 *     (NLayerDiscriminator); models/stn/layers.py:85 (Conv); models/stn/unet_stn.py:80,97 (cat);
 *     models/stn/affine_stn.py:69-72 (nn.Linear == 1x1 conv on a 1x1 image).
 * x = channel concat of x0 [N,C0,H,W] and x1 [N,C1,H,W] (x1 NULL/C1=0 for a single source), never materialised.
 * w [K,C0+C1,R,S] (torch layout), bias [K] or NULL.  pad_mode: NEMAR_PAD_ZERO | NEMAR_PAD_REFLECT
 * (reflect == nn.ReflectionPad2d(pad) followed by an unpadded conv).  act is applied in the epilogue:
 * NEMAR_ACT_NONE | RELU | LRELU(slope) | TANH.  y [N,K,OH,OW], OH = (H + 2 pad - R) / stride + 1.
 * workspace: packed weights, then the slabs of a split reduction (tiny, deep layers; summed in a fixed order, so the forward
 * pass stays bitwise reproducible) — nemar_conv2d_fwd_workspace bytes.  prepacked != 0: the workspace already holds this
 * weight tensor's packed image from an earlier call with the same (w values, shape, stride, pad): the pack launch is
 * skipped (the caller caches one workspace per weight tensor and invalidates it when the optimizer steps). */
#define NEMAR_PAD_ZERO 0
#define NEMAR_PAD_REFLECT 1
#define NEMAR_ACT_NONE 0
#define NEMAR_ACT_RELU 1
#define NEMAR_ACT_LRELU 2
#define NEMAR_ACT_TANH 3
size_t nemar_conv2d_fwd_workspace(int N, int H, int W, int K, int C, int R, int S, int stride, int pad);
int nemar_conv2d_fwd(const float* x0, int C0, const float* x1, int C1, const float* w, const float* bias,
                     float* y, int N, int H, int W, int K, int R, int S, int stride, int pad, int pad_mode,
                     int act, float slope, void* workspace, size_t ws_bytes, int prepacked, void* stream);
/* Data gradient: gy [N,K,OH,OW] -> gx0 [N,C0,H,W] | gx1 [N,C1,H,W] (gx0 NULL: its channels are skipped, e.g. the
 * real_A half of the discriminator input).  With bias/act it is ALSO the forward of
 * nn.ConvTranspose2d(K -> C, k, stride, pad, output_padding) whose weight is w [K,C,R,S]
 * (reference models/networks.py:369-372): pass gy := input, (H,W) := the transposed conv's output size. */
size_t nemar_conv2d_bwd_data_workspace(int N, int C, int H, int W, int K, int R, int S, int stride, int pad,
                                       int pad_mode);
int nemar_conv2d_bwd_data(const float* gy, const float* w, const float* bias, int act, float slope,
                          float* gx0, int C0, float* gx1, int C1, int N, int H, int W, int K, int OH, int OW,
                          int R, int S, int stride, int pad, int pad_mode, void* workspace, size_t ws_bytes,
                          int prepacked, void* stream);
/* Weight gradient, ACCUMULATED into gw [K,C0+C1,R,S] and, when gb != NULL, the bias gradient ACCUMULATED into
 * gb [K] in the same pass (the caller zero-fills once per optimizer step; the translation net receives two passes
 * per step) — autograd's conv backward + AccumulateGrad under loss.backward(), reference models/nemar_model.py:223,260.
 * The pixel reduction is split across workgroups; every split stores its partial result to its own slab of `workspace`
 * and a second launch adds the slabs in split order.  Split data gradients (few-tile deep layers) do the same, so the
 * whole backward pass of the conv family is BITWISE REPRODUCIBLE run to run, like the forward pass (and like the
 * reference's CPU path). */
size_t nemar_conv2d_bwd_weight_workspace(int N, int C, int H, int W, int K, int OH, int OW, int R, int S, int stride,
                                         int pad);
int nemar_conv2d_bwd_weight(const float* x0, int C0, const float* x1, int C1, const float* gy, float* gw, float* gb,
                            int N, int H, int W, int K, int OH, int OW, int R, int S, int stride, int pad,
                            int pad_mode, void* workspace, size_t ws_bytes, void* stream);
/* The same three entry points with the SIDE INPUTS of the wide-layer fp16 x 3 route (below) passed with the call — the only way to
 * hand them over (rounds 2-3 also had process-wide registrations: nemar_set_scratch / nemar_absmax_hint / nemar_planes_hint; they are
 * gone).  Any member may be NULL / 0 = "not given"; extras == NULL is the plain entry point.  Same kernels, bit-identical results.
 *   scratch / scratch_bytes     transient arena of the wide-layer fp16 x 3 route for THIS call (nemar_conv2d_scratch bytes)
 *   src_max_words / _count      per-sample max |source| words (source = x0 for fwd / bwd_weight, gy for bwd_data); count = N or 1
 *   src2_max_words / _count     bwd_weight only: the same for gy
 *   src_planes                  the source's operand planes written by its producer, scaled by src_max_words (count = N).  fwd: the
 *                               channel-blocked planes of x0 (nemar_instnorm_fwd_planes `planes`); bwd_data: the data-gradient planes of
 *                               gy (nemar_instnorm_bwd_planes `dgrad_planes`, written for THIS layer's pad_mode); bwd_weight: the
 *                               pixel-major X planes of x0 (nemar_instnorm_fwd_planes `wgrad_planes`).  With planes the fp32 tensor of
 *                               that operand is not read: its pointer only has to be non-NULL and distinct
 *   gy_planes_out / _bytes      bwd_data only: a buffer of nemar_conv2d_gy_planes_bytes(...) bytes.  When given together with
 *                               src_max_words (count = N) on a layer of the wide route, the pass that splits gy for the data gradient
 *                               ALSO writes the operand planes the weight gradient of the same layer needs (gy is read once) ...
 *   src2_planes                 ... and bwd_weight takes them here (with the SAME words as src2_max_words) instead of splitting gy again.
 *                               The buffer must stay untouched between the two calls.  (nemar_instnorm_bwd_planes `wgrad_planes`
 *                               are the same planes from the producer of gy.)
 *   addend                      bwd_data only: a tensor of gx0's shape ADDED to the data gradient in the kernel's epilogue (the
 *                               ResnetBlock skip gradient, reference models/networks.py:443-446: out = x + conv_block(x))
 *   out_max_words               bwd_data only: a NEMAR_MAX_WORDS(N) buffer; the epilogue publishes the per-sample max |gx0| (words 0..N-1)
 *                               Both only where nemar_conv2d_bwd_data_fusable(...) says 1 (the addend alone: where
 *                               nemar_conv2d_bwd_data_addend_ok(...) says 1) — elsewhere the call fails with NEMAR_EINVAL.
 * A packed-weight workspace (prepacked = 1) must be reused under the same route conditions it was written under (arena present or
 * not, nemar_config_epoch unchanged). */
typedef struct nemar_conv_extras {
    void* scratch;
    size_t scratch_bytes;
    const void* src_max_words;
    int src_max_count;
    const void* src2_max_words;
    int src2_max_count;
    const void* src_planes;
    void* gy_planes_out;
    size_t gy_planes_bytes;
    const void* src2_planes;
    const float* addend;
    void* out_max_words;
    const float* bias_partials;   /* (ABI 602) bwd_weight only, with gb != NULL on a layer of the wide route: per-plane sums of gy [N, K]
                                   * (nemar_instnorm_bwd_planes `bias_partials`); gb += their sum over the batch, in batch order, inside the
                                   * launch that sums the weight gradient's slabs — instead of a nemar_bias_from_partials call of its own */
} nemar_conv_extras;
/* 1: the layer's bwd_data_ex honours addend / out_max_words and takes src_planes, and its bwd_weight_ex takes both operands as planes */
int nemar_conv2d_bwd_data_fusable(int N, int C, int H, int W, int K, int R, int S, int stride, int pad, int pad_mode);
/* (ABI 602) 1: the layer's bwd_data_ex (one destination, no bias, no activation) adds extras.addend to gx0 — the wide route's epilogue, or
 * the fold pass that ends the data gradient of a small stride-1 reflect layer (out_max_words is NOT honoured there: only where _fusable says 1) */
int nemar_conv2d_bwd_data_addend_ok(int N, int C, int H, int W, int K, int R, int S, int stride, int pad, int pad_mode);
/* bytes of the pixel-major X planes nemar_instnorm_fwd_planes can write for the weight gradient of a KS x KS / pad-1 reflect layer (0: none) */
size_t nemar_conv2d_x_planes_bytes(int N, int C, int H, int W, int KS);
/* bytes of the gy planes a bwd_data call can leave behind for the bwd_weight call of the same layer (0: this layer does not take them) */
size_t nemar_conv2d_gy_planes_bytes(int N, int C, int H, int W, int K, int R, int S, int stride, int pad, int pad_mode);
/* 1 when the last nemar_conv2d_bwd_data_ex call on this thread filled its gy_planes_out buffer (check before passing it on as src2_planes) */
int nemar_last_gy_planes(void);
int nemar_conv2d_fwd_ex(const float* x0, int C0, const float* x1, int C1, const float* w, const float* bias, float* y, int N,
                        int H, int W, int K, int R, int S, int stride, int pad, int pad_mode, int act, float slope,
                        void* workspace, size_t ws_bytes, int prepacked, void* stream, const nemar_conv_extras* extras);
int nemar_conv2d_bwd_data_ex(const float* gy, const float* w, const float* bias, int act, float slope, float* gx0, int C0,
                             float* gx1, int C1, int N, int H, int W, int K, int OH, int OW, int R, int S, int stride, int pad,
                             int pad_mode, void* workspace, size_t ws_bytes, int prepacked, void* stream,
                             const nemar_conv_extras* extras);
int nemar_conv2d_bwd_weight_ex(const float* x0, int C0, const float* x1, int C1, const float* gy, float* gw, float* gb, int N,
                               int H, int W, int K, int OH, int OW, int R, int S, int stride, int pad, int pad_mode,
                               void* workspace, size_t ws_bytes, void* stream, const nemar_conv_extras* extras);
/* Weight-pack plans.  Every convolution family reads its weights from a packed operand image in the `workspace` of the call
 * (prepacked = 0: the call rebuilds it first — a max reduction and a pack launch per weight and direction, ~240 launches of 4-6 us per
 * training step).  A plan batches them: while nemar_pack_plan_record(plan) is in effect on the calling thread, the pack launches the
 * convolution entry points issue are ALSO recorded as jobs of `plan` (record(-1) stops); nemar_pack_plan_commit copies the recorded
 * job arguments into a caller-owned device buffer of nemar_pack_plan_bytes(plan) bytes (once per change: nemar_pack_plan_dirty);
 * nemar_pack_plan_run re-runs every job — the same images, bit for bit — in at most five launches (one multi-job kernel per family,
 * job arguments read from that buffer), after which the owners of those workspaces may call with prepacked = 1.  The caller keeps the
 * weights, the workspaces and the device buffer alive and unmoved while the plan is in use, and uses one plan per group of weights
 * that change together (an optimizer).  nemar_pack_plan_jobs -> pack jobs recorded; nemar_pack_plan_reset forgets the plan. */
int nemar_pack_plan_record(int plan);
int nemar_pack_plan_jobs(int plan);
size_t nemar_pack_plan_bytes(int plan);
int nemar_pack_plan_dirty(int plan);
int nemar_pack_plan_commit(int plan, void* device_buffer, size_t bytes, void* stream);
int nemar_pack_plan_run(int plan, void* stream);
int nemar_pack_plan_reset(int plan);
/* Which kernel family served the calling thread's last nemar_conv2d_* call: 0 exact-fp32 implicit GEMM, 1 narrow (<= 4 channel)
 * VALU kernels, 2 split-16 kernels of the wide residual-block layers, 3 general 16-bit-pipe kernels (tests / tools). */
int nemar_last_route(void);
/* The route a shape takes — and with it the FORMAT of the packed weight image a `prepacked` call finds in its workspace — is a
 * function of the shape and of the library's measurement switches.  This library has none: always 0.  In the measurement build
 * (nemar_hip_ab.h) it is a counter bumped by every nemar_tune call, and a caller that caches packed workspaces keys them with it. */
int nemar_config_epoch(void);
/* Per calling thread, 1 / 0, returns the previous setting (0.6.1).  While on, the two producers of per-sample maxima on the residual blocks'
 * path — nemar_instnorm_fwd_planes (max_words) and nemar_conv2d_bwd_data_ex (nemar_conv_extras.out_max_words) — do NOT launch the reduction
 * of their per-workgroup partial words; word n of the buffer holds a marker (0xFFFF0000 | partials) instead.  Such a buffer may ONLY be
 * passed on as nemar_instnorm_fwd_planes residual_max_words or nemar_instnorm_bwd_planes gy_max_words, which reduce a sample's partials
 * themselves; every other consumer of max words needs finalized words (the default).  One launch less per producer call: 4 us on one
 * stream, 12 us beside a second stream, 25 times per training step on the chain the rest of the step waits for. */
int nemar_set_max_words_lazy(int on);
/* (ABI 602) The reduction a lazy producer skipped, on demand: every sample whose result word still holds the marker gets the maximum of its partial
 * words; finalized words are left alone.  nemar_instnorm_fwd_max / _bwd_max honour the lazy setting too (ABI 602): a binding that publishes maxima
 * "in case the consumer is a wide-route convolution" pays the reduction only for the tensors such a consumer actually reads. */
int nemar_max_words_finalize(void* max_words, int samples, void* stream);
/* Transient scratch arena for nemar_conv2d_fwd / nemar_conv2d_bwd_data / nemar_conv2d_bwd_weight.  The wide stride-1 / pad-1
 * layers (the 3x3 ResnetBlock convolutions, reference models/networks.py:418-439, and the discriminator's 256->512 4x4 layer,
 * :576-597; >= 128 channels, >= 2 G multiply-adds) run on the 16-bit matrix pipe at fp32 accuracy: each fp32 operand is split into
 * two power-of-two-scaled fp16 terms and three partial products are accumulated in fp32 (csrc/conv_split16*.hip; measured error
 * against float64 below that of the exact-fp32 MFMA kernels).  The split copies of the source tensors live in this
 * arena for the duration of the call.  nemar_conv2d_scratch -> bytes the layer wants (0: never uses it); the caller passes a device
 * buffer of at least that size as nemar_conv_extras.scratch (one stream at a time per buffer).  A layer called without an arena, or
 * with one that is too small, runs on the exact-fp32 MFMA kernels instead — same results within fp32 rounding. */
size_t nemar_conv2d_scratch(int N, int H, int W, int K, int C, int R, int S, int stride, int pad);
/* The fp16 form of those kernels scales every SAMPLE of a source tensor by its own power of two, derived from the largest finite
 * magnitude of the sample (so samples of very different magnitude in one batch — the batched real / fake passes — do not share a
 * scale).  Error bound of the fp16 x 3 form, per product v w: |error| <= 3 * 2^-22 |v w| as long as |v| >= 2^-14 max_sample|v|
 * (both fp16 terms normal); below that the absolute error of v is 2^-37 max_sample|v|.  Non-finite elements do not take part in the
 * maximum and propagate as Inf / NaN; an all-zero sample has scale 1.  (The general kernels of tune key 24 go further: their scale
 * is per workgroup tile and 16-channel chunk, or per channel row in the weight gradient — csrc/conv_s16g*.hip.)
 * A caller that feeds one tensor to several calls (x: forward and weight gradient; gy: data and weight gradient) computes the words
 * once with nemar_absmax_samples (out_words: `samples` 4-byte words that are ZERO on entry — the kernel takes an atomic max of the bit
 * patterns into them; nemar_absmax = one sample) and passes them as nemar_conv_extras.src_max_words / src2_max_words (count = the
 * tensor's batch size, or 1 = one word for the whole tensor).  Without them every call runs its own max pass. */
int nemar_absmax(const float* t, long long n, void* out_word, void* stream);
int nemar_absmax_samples(const float* t, int samples, long long per_sample, void* out_words, void* stream);
/* Measurement hook for bench.py's roofline entry: while enabled, HIP events are recorded on the launch stream around the main
 * kernel (igemm_split16_kernel) of every forward / data-gradient call of those layers; read -> summed duration, summed algorithmic
 * (fp32-equivalent) flop 2 N OH OW K C R S of the timed launches, and their count (synchronises on the recorded events, resets). */
int nemar_kernel_timer(int enable);
int nemar_kernel_timer_read(double* total_ms, double* total_flop, int* launches);
/* gb[C] += sum over batch and plane of g [N,C,HW] (bias gradient; two fixed-order stages through `workspace`). */
size_t nemar_bias_grad_workspace(int N, int C, int HW);
int nemar_bias_grad(const float* g, float* gb, int N, int C, int HW, void* workspace, size_t ws_bytes, void* stream);

/* ---- K3 (+K5): InstanceNorm2d(affine=False, track_running_stats=False) with fused activation / residual -------
 * nn.InstanceNorm2d — reference models/networks.py:24 (used :351,358,373,426,439,584,592), models/stn/layers.py:16;
 * the ReLU/LeakyReLU(0.2) after it, and the ResnetBlock skip `x + conv_block(x)` (models/networks.py:445).
 * x,y,residual: [planes = N*C, HW]; stats [planes,2] = (mean, rstd) saved for the backward.
 * fwd: y = (residual ? residual : 0) + act((x - mean) * rstd), biased variance, eps inside the sqrt.
 * bwd: gx = rstd * (g - mean(g) - xhat * mean(g * xhat)), g = gy * act'(xhat).  act: NONE | RELU | LRELU. */
int nemar_instnorm_fwd(const float* x, const float* residual, float* y, float* stats, int planes, int HW,
                       float eps, int act, float slope, void* stream);
int nemar_instnorm_bwd(const float* x, const float* stats, const float* gy, float* gx, int planes, int HW,
                       int act, float slope, void* stream);
/* The same, and max |output| (finite elements) of every SAMPLE into max_words[sample]: what nemar_absmax_samples would compute in a
 * pass of its own — the producer has the values in registers.  The words are what nemar_conv_extras.src_max_words takes (the
 * fp16 x 3 convolutions consume them).  max_words is a buffer of NEMAR_MAX_WORDS(samples) 4-byte words, no initialisation needed: the first
 * `samples` words are the result, the rest is scratch for the per-workgroup partials a second tiny launch reduces (no atomics —
 * thousands of workgroups' device-scope atomicMax on a handful of words cost more than the pass they replaced).
 * planes_per_sample <= NEMAR_MAX_PARTIALS. */
#define NEMAR_MAX_PARTIALS 2048
#define NEMAR_MAX_WORDS(samples) ((size_t)(samples) * (1 + NEMAR_MAX_PARTIALS))
int nemar_instnorm_fwd_max(const float* x, const float* residual, float* y, float* stats, int planes, int HW,
                           float eps, int act, float slope, void* max_words, int planes_per_sample, void* stream);
int nemar_instnorm_bwd_max(const float* x, const float* stats, const float* gy, float* gx, int planes, int HW,
                           int act, float slope, void* max_words, int planes_per_sample, void* stream);

/* InstanceNorm (+ activation, + Dropout(p) drawn exactly as nemar_dropout draws it over the [N,C,H,W] tensor, + residual) that ALSO
 * writes its output as the fp16 x 3 planes a following 3x3 / pad-1 REFLECT convolution of the wide-layer route consumes
 * (reference: the conv -> InstanceNorm -> ReLU -> [Dropout] -> ReflectionPad2d(1) -> conv chain of ResnetBlock,
 * models/networks.py:418-446) — the consumer then skips its max and split passes (nemar_conv_extras.src_planes + .src_max_words).
 *   y          fp32 output or NULL (planes only: nothing else reads it)
 *   planes     2 * N * (C/8) * (H+4) * (W+4) 16-byte words (hi plane, lo plane), layout of conv_split16.hip
 *   scale_words[N]  out: the a-priori BOUND each sample was scaled by, sqrt(HW) [/ (1-p)] [+ max |residual| of the sample] —
 *              InstanceNorm's output cannot exceed it, so the scale is known before the first element exists; pass these words as
 *              src_max_words of the consuming convolution (its epilogue unscales with them).  A bound 2^k above the actual
 *              maximum costs nothing for k <= 8: elements above 2^(k-14) x max keep the split's 22 bits, smaller ones are off by
 *              <= 2^(k-36) x max (norm_planes.hip).
 *   residual_max_words[N]  required with a residual: its per-sample maxima (a producer's max words)
 *   max_words  NEMAR_MAX_WORDS(N) buffer or NULL: the ACTUAL per-sample maxima of the output (the next layer's residual bound)
 *   wgrad_planes  NULL, or nemar_conv2d_x_planes_bytes(N, C, H, W, 3) bytes: ALSO the pixel-major X planes the WEIGHT gradient of that
 *              convolution reads (same scale; pass as src_planes + src_max_words of its nemar_conv2d_bwd_weight_ex): the layer then
 *              runs neither of its split passes over this tensor
 * Limits: C % 8 == 0, W % 4 == 0, H * W <= 4096, N <= 256. */
int nemar_instnorm_fwd_planes(const float* x, const float* residual, const void* residual_max_words, float* y, float* stats,
                              int N, int C, int H, int W, float eps, int act, float slope, float dropout_p,
                              unsigned long long seed, unsigned offset, void* planes, void* scale_words, void* max_words,
                              void* wgrad_planes, void* stream);
/* The backward of that producer for a 3x3 / pad-1 convolution of the wide route IN FRONT of it (reference: autograd through
 * conv -> InstanceNorm -> ReLU -> [Dropout] of ResnetBlock, models/networks.py:418-446): gx = InstanceNorm backward of gy through
 * [dropout ->] act -> InstanceNorm (nemar_instnorm_bwd's formula; the dropout mask of (p, seed, offset) regenerated), written as the
 * OPERAND PLANES of the convolution's two gradient calls instead of (gx != NULL: besides) the fp32 tensor:
 *   dgrad_planes   2 * N * (C/8) * (H+4) * (W+4) 16-byte words: gy planes of nemar_conv2d_bwd_data_ex (extras.src_planes) for a layer
 *                  with this pad_mode (0 zero, 1 reflect: the folded border rows of the reflect data gradient)
 *   wgrad_planes   nemar_conv2d_gy_planes_bytes(...) bytes: gy planes of nemar_conv2d_bwd_weight_ex (extras.src2_planes)
 *   scale_words[N] out: the a-priori bound the planes are scaled by, rstd_max(sample) * (2 + sqrt(HW)) [/ (1-p)] * max|gy|(sample);
 *                  pass as src_max_words / src2_max_words of the two calls
 *   gy_max_words[N]  per-sample max |gy| (a producer's words, nemar_conv_extras.out_max_words, or nemar_absmax_samples)
 *   bias_partials  NULL or [N, C]: the sum of gx over each plane (the convolution's bias gradient = their sum over the batch:
 *                  nemar_bias_from_partials)
 * Either planes pointer may be NULL.  Limits as nemar_instnorm_fwd_planes; wgrad_planes: C % 64 == 0, W % 8 == 0. */
int nemar_instnorm_bwd_planes(const float* x, const float* stats, const float* gy, const void* gy_max_words, int N, int C,
                              int H, int W, int act, float slope, float dropout_p, unsigned long long seed, unsigned offset,
                              int pad_mode, float* gx, void* dgrad_planes, void* wgrad_planes, void* scale_words,
                              float* bias_partials, void* stream);
/* gb[C] += sum over the batch of bias_partials [N, C], in batch order (bitwise reproducible) */
int nemar_bias_from_partials(const float* bias_partials, int N, int C, float* gb, void* stream);
/* ---- BatchNorm2d(C, affine=True, track_running_stats=True) (ABI 603) ---------------------------------------------------------
 * nn.BatchNorm2d — reference models/networks.py:22 (`--norm batch`), the norm_layer of ResnetGenerator :351,358,373, ResnetBlock
 * :426,439, UnetSkipConnectionBlock :517,519, NLayerDiscriminator :584,592 and PixelDiscriminator :626 — with the ReLU / LeakyReLU,
 * Dropout and residual add that follow it fused in.  x, y, residual, gy, gx: [N, C, HW] fp32.  The N samples form `segments` equal
 * segments: statistics, running-stat updates and gradient sums are per (segment, channel), the updates applied in segment order (what
 * `segments` separate calls of the layer compute).  Every reduction has a fixed order: no floating-point atomics, bitwise reproducible.
 *   train: mean, var = biased statistics of the segment, eps inside the sqrt;  y = [residual +] dropout(act(x * scale + shift)),
 *          scale = weight * rstd, shift = bias - mean * scale;  saved[2, segments, C] = (mean | rstd);  running_mean / running_var
 *          (nullable together) <- (1 - momentum) running + momentum (mean | var * M / (M - 1)) per segment in order, M = N / segments * HW
 *          (> 1 required);  num_batches_tracked (nullable, int64) += segments.
 *   eval:  the same apply with the running statistics (untouched); saved (nullable) [2, C] receives (running_mean | rstd) for the backward.
 *   Dropout(p) (p = 0: none) is drawn exactly as nemar_dropout draws it over the [N, C, HW] tensor with (seed, offset) (+ the
 *   nemar_set_dropout_base word).  max_words (nullable): NEMAR_MAX_WORDS(N) buffer, per-sample max |y| as nemar_instnorm_fwd_max.
 *   bwd:   z = x * scale + shift recomputed, g = gy [* mask / (1 - p)] * act'(z), xhat = (x - mean) * rstd;
 *          grad_weight[c] += sum g xhat, grad_bias[c] += sum g (nullable; summed over segments in order and ACCUMULATED);
 *          gx (nullable) = scale * (g - sum g / M - xhat * sum(g xhat) / M) per segment (training), = scale * g (training == 0, with the
 *          saved statistics of the eval forward).
 * workspace: nemar_batchnorm_workspace(N, C, HW, segments) bytes. */
size_t nemar_batchnorm_workspace(int N, int C, int HW, int segments);
int nemar_batchnorm_fwd_train(const float* x, const float* residual, float* y, const float* weight, const float* bias,
                              float* running_mean, float* running_var, long long* num_batches_tracked, float* saved,
                              int N, int C, int HW, int segments, float eps, float momentum, int act, float slope,
                              float dropout_p, unsigned long long seed, unsigned offset, void* max_words,
                              void* workspace, size_t workspace_bytes, void* stream);
int nemar_batchnorm_fwd_eval(const float* x, const float* residual, float* y, const float* weight, const float* bias,
                             const float* running_mean, const float* running_var, float* saved, int N, int C, int HW, float eps,
                             int act, float slope, float dropout_p, unsigned long long seed, unsigned offset, void* max_words,
                             void* stream);
int nemar_batchnorm_bwd(const float* x, const float* gy, float* gx, const float* weight, const float* bias, const float* saved,
                        float* grad_weight, float* grad_bias, int N, int C, int HW, int segments, int training, int act,
                        float slope, float dropout_p, unsigned long long seed, unsigned offset, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- K5/K6/K7: pointwise, pooling, resize, dropout -----------------------------------------------------------------
 * act_bwd: gx = gy * f'(.) expressed with the activation OUTPUT y (f fused into a conv epilogue):
 *     nn.LeakyReLU / nn.ReLU / nn.Tanh — reference models/networks.py:377,576 ; models/stn/layers.py:61-64. */
int nemar_act_bwd(const float* gy, const float* y, float* gx, long long n, int act, float slope, void* stream);
/* y = act(x) as a stand-alone pass (nn.ReLU / nn.LeakyReLU / nn.Tanh where no producer epilogue can carry it: the U-Net
 * generator's skip path, reference models/networks.py:516-553).  Backward = nemar_act_bwd on the output. */
int nemar_act_fwd(const float* x, float* y, long long n, int act, float slope, void* stream);
/* (ABI 602) dst = [piece 0 | piece 1 | ... | piece k-1] (k <= 8 contiguous pieces of counts[i] floats; `pieces` / `counts` are HOST arrays,
 * read during the call; a NULL piece contributes zeros).  The concatenation along the batch of the model's batched passes
 * (torch.cat of reference models/nemar_model.py:181,220 evaluated once for several images) and, with the incoming gradients as pieces, the
 * backward of slicing such a batch — instead of autograd's cat / zero-fill / copy / add kernels. */
int nemar_concat_pieces(const float* const* pieces, const long long* counts, int k, float* dst, void* stream);
/* (ABI 602) out = a + b (out may alias a or b): the sum of the gradients of a tensor with two consumers (a ResnetBlock's input, a U-Net skip:
 * reference models/networks.py:443-446, models/stn/unet_stn.py:80-97), which autograd would add with an ATen kernel. */
int nemar_add2(const float* a, const float* b, float* out, long long n, void* stream);
/* nn.MaxPool2d(2) — reference models/stn/layers.py:174.  x [planes,H,W] -> y [planes,H/2,W/2].
 * bwd: gx = (addend ? addend : 0) + unpool(gy); the argmax (first maximum, row-major) is recomputed from x. */
int nemar_maxpool2_fwd(const float* x, float* y, int planes, int H, int W, void* stream);
int nemar_maxpool2_bwd(const float* x, const float* gy, const float* addend, float* gx, int planes, int H, int W,
                       void* stream);
/* F.interpolate(x, (Ho,Wo), mode='bilinear', align_corners=False) — reference models/stn/unet_stn.py:96,188-195,
 * models/nemar_model.py:187-188,204-205,226-227,240-241,254-255.  bwd WRITES gx [planes,H,W]. */
int nemar_bilinear_fwd(const float* x, float* y, int planes, int H, int W, int Ho, int Wo, void* stream);
int nemar_bilinear_bwd(const float* gy, float* gx, int planes, int H, int W, int Ho, int Wo, void* stream);
/* nn.Dropout(p) in training mode — reference models/networks.py:427-428.  y = x * mask / (1-p), mask drawn from
 * Philox4x32-10(seed, offset); the backward is the same call on the upstream gradient (mask regenerated). */
int nemar_dropout(const float* x, float* y, long long n, float p, unsigned long long seed, unsigned offset,
                  void* stream);
/* ... with the per-sample maxima of the output (max_words[i]; a NEMAR_MAX_WORDS(samples) buffer as above) for `samples` samples of
 * `per_sample` elements (a multiple of 4); the masks are those of nemar_dropout over all samples * per_sample elements. */
int nemar_dropout_max(const float* x, float* y, int samples, long long per_sample, float p, unsigned long long seed,
                      unsigned offset, void* max_words, void* stream);

/* Replaying a step as a captured hipGraph: launch arguments are frozen at capture time, so what changes from step to step must live in
 * device memory.  nemar_set_dropout_base registers a device word that every dropout-type launch (nemar_dropout, nemar_dropout_max,
 * nemar_instnorm_fwd_planes) adds to its `offset` at run time (NULL = none, the default); the caller rewrites the word before each replay.
 * nemar_adam_step_dev is nemar_adam_step with hyper[0] = lr / (1 - beta1^step) and hyper[1] = sqrt(1 - beta2^step) read from device memory
 * (computed by the caller in double, rounded to float — exactly what nemar_adam_step passes to its kernel). */
int nemar_set_dropout_base(const void* device_word);
/* dst[0..n) = the n <= 8 four-byte words at host_words, stream-ordered: the values travel as KERNEL ARGUMENTS (read from host memory
 * during the call), so the host buffer may be reused at once — unlike an asynchronous copy from pageable memory, whose source may be
 * read later.  How the step's device-resident parameters (dropout base word, Adam's two scalars) are rewritten before a graph replay. */
int nemar_store_words(void* dst, const void* host_words, int n, void* stream);
int nemar_adam_step_dev(float* p, const float* g, float* m, float* v, long long n, const float* hyper, double beta1,
                        double beta2, double eps, void* stream);

/* Input pipeline, on the GPU: random crop + horizontal flip + ToTensor/Normalize(0.5, 0.5) of a pool of images resident in
 * HBM — reference data/base_dataset.py:63-78 (get_params: ONE crop position / flip per A-B pair) and :81-112
 * (get_transform; Normalize :111).  pool [M,C,H,W] with values in [0, 1/scale]; params [B,4] int32 device array
 * (pool index, y0, x0, flip), 16-byte aligned; y [B,C,Hc,Wc] = (pool[...] * scale - 0.5) / 0.5. */
int nemar_crop_flip_normalize(const float* pool, const int* params, float* y, int M, int B, int C, int H, int W,
                              int Hc, int Wc, float scale, void* stream);

/* Known-misalignment training pairs and the registration-error meter (not in the reference, whose data sets come misaligned: here the
 * pipeline deforms modality A by a seeded smooth transformation and carries its ground truth with the batch).
 * Conventions: pixel coordinates q = (x, y), integer values at pixel centres, origin at the top-left pixel of the output crop
 * [Hc,Wc]; a ground-truth field g is [B,2,Hc,Wc] IN PIXELS, channel 0 = x (the UNet STN's order); the deformed image is
 * A'(q) = A_crop(q + g(q)).  Tensors of any alignment and odd widths are served (one pixel per lane instead of 16-byte accesses).
 *
 * nemar_deform_field: g from params [B, 6 + 2*gh*gw] (device): a11 a12 tx a21 a22 ty, an affine map about the crop centre
 * c = ((Wc-1)/2, (Hc-1)/2) whose displacement is (M - I)(q - c) + t, then a control lattice [2,gh,gw] of displacements in pixels
 * interpolated over the crop by a uniform cubic B-spline (gh, gw >= 4: its gh-3 x gw-3 segments span the crop; gh = gw = 0: no
 * lattice) and added to the affine displacement. */
int nemar_deform_field(const float* params, float* g, int B, int Hc, int Wc, int gh, int gw, void* stream);
/* nemar_crop_flip_normalize (same pool, params [B,4], scale) with every output pixel q read bilinearly from the cropped-and-flipped
 * image at q + g(q), the position clamped to the crop window (border padding).  g == 0 gives nemar_crop_flip_normalize's output bit
 * for bit. */
int nemar_crop_flip_deform_normalize(const float* pool, const int* params, const float* g, float* y, int M, int B, int C,
                                     int H, int W, int Hc, int Wc, float scale, void* stream);
/* The label twin of nemar_crop_flip_deform_normalize: pool [M,1,H,W] float class ids, the same params (crop window, flip) and the same
 * positions q + g(q) clamped to the crop window, read by NEAREST sampling — round half to even, the rounding of
 * nemar_warp_resampled_fwd(NEMAR_SAMPLE_NEAREST) — and copied: no blending, no normalisation.  y [B,1,Hc,Wc].  g == NULL is the plain
 * crop / flip copy, and so is g == 0. */
int nemar_crop_flip_deform_labels(const float* pool, const int* params, const float* g, float* y, int M, int B, int H, int W, int Hc,
                                  int Wc, void* stream);
/* The meter.  pred is the STN's prediction as nemar_grid_sample_fwd takes it: NEMAR_GRID_UNET offsets [N,2,H,W] or NEMAR_GRID_AFFINE
 * dtheta [N,6].  S(x) = the pixel position that kernel samples for output pixel x; the registered image is A'(S(x)) =
 * A(S(x) + g(S(x))), so the residual is r(x) = S(x) + g(S(x)) - x, g read bilinearly at S(x); |.| is the Euclidean length.
 * out [N,6] per sample, SUMS (the caller divides): valid_count (S(x) inside [0,W-1] x [0,H-1]), sum |r| over valid pixels,
 * max |r| over valid pixels, sum |g(x)| over all pixels (the error before registration), fold_count (determinant of the forward-
 * difference Jacobian of x -> S(x) <= 0), interior_count (pixels that have both forward neighbours).  Per-workgroup partials merged in
 * a fixed order: bitwise repeatable.  A workspace smaller than nemar_registration_error_workspace() bytes is NEMAR_EINVAL. */
size_t nemar_registration_error_workspace(int N, int H, int W);
int nemar_registration_error(const float* pred, int grid_mode, const float* g, float* out, void* workspace, size_t ws_bytes,
                             int N, int H, int W, void* stream);

/* Registration at any resolution (not a call site of the reference, which warps at the network's own size only): the STN's prediction
 * applied to an image of another size in one pass.  It fuses the reference's upsampling of a coarse deformation to the output size
 * with the warp itself — F.interpolate(offsets, (Ho,Wo), 'bilinear', align_corners=False) then F.grid_sample(in, identity + offsets),
 * reference models/stn/unet_stn.py:139-141,165-174 — and F.affine_grid(theta, (Ho,Wo)) + F.grid_sample, models/stn/affine_stn.py:122,128:
 * the sampling grid is in normalised coordinates, so the same prediction describes the transformation at every size.
 *   NEMAR_GRID_UNET    pred = offsets [N,2,hf,wf]; grid(h,w) = linspace(-1,1,Wo)[w] + R(pred)[0,h,w], linspace(-1,1,Ho)[h] + R(pred)[1,h,w],
 *                      R = the bilinear resize to (Ho,Wo) whenever (hf,wf) != (Ho,Wo), evaluated in registers (never written), and the
 *                      identity when the sizes are equal.  (The "only if BOTH dims differ" rule of the reference is the caller's.)
 *   NEMAR_GRID_AFFINE  pred = dtheta [N,6]; the grid is affine_grid(dtheta + I, align_corners=False) at (Ho,Wo); hf, wf are ignored.
 *   NEMAR_GRID_EXPLICIT is NEMAR_EINVAL (a materialised grid has one resolution).
 * sample_mode: NEMAR_SAMPLE_BILINEAR = F.grid_sample(..., 'bilinear', 'zeros', align_corners=False), bit for bit what
 * nemar_bilinear_fwd + nemar_grid_sample_fwd give; NEMAR_SAMPLE_NEAREST = F.grid_sample(..., 'nearest', 'zeros', align_corners=False):
 * the unnormalised position rounded half-to-even, zero where that texel is outside the source — for label maps, whose class ids must
 * not be blended.  in [N,C,Hs,Ws] -> out [N,C,Ho,Wo]; the source size is free.
 * Alignment: in, pred and out need 4-byte alignment only (anything else is NEMAR_EINVAL): the kernel handles one pixel per lane, so odd
 * widths and views off the 16-byte grid take the same route as everything else.  (A 16-byte-store route exists in the measurement build,
 * nemar_hip_ab.h key 44; profiles/register_fullres.txt has the two side by side.) */
#define NEMAR_SAMPLE_BILINEAR 0
#define NEMAR_SAMPLE_NEAREST 1
int nemar_warp_resampled_fwd(const float* in, const float* pred, int grid_mode, int sample_mode, float* out,
                             int N, int C, int Hs, int Ws, int hf, int wf, int Ho, int Wo, void* stream);

/* The gradient of that pass towards the prediction (csrc/register.hip: the adjoint of nemar_warp_resampled_fwd with respect to `pred`,
 * NEMAR_SAMPLE_BILINEAR only; not in the reference, which never warps at another size) — what refining a registration on its own pair
 * at the pair's native size needs.  img [N,C,Hs,Ws] and pred are the forward's operands, gout [N,C,Ho,Wo] the gradient of its output.
 * For sample n and output pixel (h,w), with (gx,gy) the coordinate the forward computes, a, b, c, d the four texels of channel ch it
 * blends (0 outside the image) and tx, ty the fractions of the position, ex = 1 - tx, ey = 1 - ty:
 *   dvx(n,h,w) = (Ws/2) sum_ch gout[n,ch,h,w] ((b - a) ey + (d - c) ty),   dvy(n,h,w) = (Hs/2) sum_ch gout[n,ch,h,w] ((c - a) ex + (d - b) tx)
 * in the expression order of nemar_grid_sample_bwd's grid gradient, and exactly 0 where gx or gy is not finite.
 *   NEMAR_GRID_UNET, (hf,wf) != (Ho,Wo)   gpred[n,0,j,i] = sum_{h,w} Wy_j(h) Wx_i(w) dvx(n,h,w), plane 1 with dvy: Wx_i(w) the weight the
 *                                         resize gives field column i at output column w (both taps where they coincide at the border),
 *                                         the exact adjoint of the forward's interpolation;
 *   NEMAR_GRID_UNET, equal sizes          gpred = dv: bit for bit nemar_grid_sample_bwd's grid gradient at a source of the output's size;
 *   NEMAR_GRID_AFFINE                     gpred[n,0..2] = sum dvx (xb, yb, 1), gpred[n,3..5] = sum dvy (xb, yb, 1), (xb, yb) affine_grid's base
 *                                         coordinates at (Ho,Wo); hf, wf are ignored.
 * accumulate = 1 adds to gpred (several images warped by one prediction share one gradient); 0 writes every element of gpred [N,2,hf,wf]
 * or [N,6]: no zero-fill is expected.  Every sum is a gather in a fixed order — per-tile records in the workspace, merged by one thread
 * per element: no atomics, bitwise repeatable, no host synchronisation.  No gradient towards img.  Pointers need 4-byte alignment only.
 * NEMAR_EINVAL, with nothing launched and gpred untouched: a null pointer (ws may be NULL where the query is 0: UNET at equal sizes); a
 * non-positive size; grid_mode other than UNET or AFFINE; N > 65535; Ho or Wo of 2^23 or more; ws_bytes below nemar_warp_resampled_bwd_workspace(); gpred equal
 * to pred; a UNet field being DOWN-sampled (hf > Ho or wf > Wo): the forward serves it by an unstaged global-memory route that has no
 * counterpart here — refinement, which optimises a prediction at the network's size against a larger pair, never needs it. */
size_t nemar_warp_resampled_bwd_workspace(int grid_mode, int N, int hf, int wf, int Ho, int Wo);
int nemar_warp_resampled_bwd(const float* img, const float* pred, int grid_mode, const float* gout, float* gpred, int accumulate,
                             int N, int C, int Hs, int Ws, int hf, int wf, int Ho, int Wo, void* ws, size_t ws_bytes, void* stream);

/* Scoring a registration of real data (csrc/score.hip; not in the reference, which has no evaluation code): segmentation overlap and
 * annotated-point distances, both read off the transformation exactly as nemar_warp_resampled_fwd applies it.  pred, grid_mode, hf and
 * wf are what that entry point takes (NEMAR_GRID_UNET offsets [N,2,hf,wf], resized in registers; NEMAR_GRID_AFFINE dtheta [N,6], hf and
 * wf ignored; NEMAR_GRID_EXPLICIT is NEMAR_EINVAL).
 *
 * nemar_label_overlap: the nearest-sampled warp of a label map and its per-class counts against the fixed map, in one pass.
 * labels_moving [N,Hs,Ws] (modality A's map, any size), labels_fixed [N,Ho,Wo].  For output pixel x, m(x) is the value
 * nemar_warp_resampled_fwd(..., NEMAR_SAMPLE_NEAREST) would write there (position rounded half-to-even, 0 where the texel is outside the
 * source) — the same code computes it; the warped map is never written to memory — and f(x) = labels_fixed(x).
 * A value v belongs to class k iff v == (float)k for an integer 0 <= k < K; any other value (negative, >= K, fractional, NaN, Inf)
 * belongs to no class on that side and is not counted.  Zero padding is the value 0: pixels warped from outside the source count as
 * class 0 (the background id by the usual convention; score foreground classes only if that matters).
 * counts [N,K,3] uint32 is OVERWRITTEN (cleared on `stream` by the entry point; no workspace): per sample and class
 *   [0] inter = #{x : m(x) == k and f(x) == k}    [1] moving = #{x : m(x) == k}    [2] fixed = #{x : f(x) == k}
 * Dice_k = 2 inter / (moving + fixed) is the caller's arithmetic.  The score BEFORE registration is the same call with an identity
 * prediction (NEMAR_GRID_AFFINE, dtheta = 0), which also brings maps of different sizes together.
 * The counts are integers, added with integer atomics: the result does not depend on the order of the additions and is bitwise
 * repeatable — no fixed-order merge is needed (nemar_registration_error's float sums need one).
 * NEMAR_EINVAL, nothing launched: K outside 1 .. 1024, Ho*Wo or Hs*Ws >= 2^31, a non-positive size, N > 65535, hf or wf < 1 with
 * NEMAR_GRID_UNET, a null pointer or one that is not 4-byte aligned (odd widths and views off the 16-byte grid take the normal route). */
int nemar_label_overlap(const float* labels_moving, const float* labels_fixed, const float* pred, int grid_mode, unsigned* counts,
                        int N, int K, int Hs, int Ws, int hf, int wf, int Ho, int Wo, void* stream);
/* nemar_map_points: the transformation at annotated points.  pts [N,P,2] = (x, y) in pixels of the fixed image at size (Ho,Wo), fractional
 * values and points beyond the border allowed; out [N,P,2] = S(p), the position in pixels of the (Hs,Ws) source that the warp samples for
 * p: the continuous extension of nemar_warp_resampled_fwd's grid, ((g + 1) * size_s - 1) / 2 of
 *   NEMAR_GRID_UNET    g = -1 + 2p/(size-1) (linspace(-1,1,size) at integer p) + the align_corners=False bilinear resize of pred evaluated
 *                      at p: source coordinate (p + 0.5) * hf/Ho - 0.5 clamped to [0, hf-1], the taps of nemar_bilinear_fwd; with
 *                      (hf,wf) == (Ho,Wo) that is the bilinear interpolation of pred itself;
 *   NEMAR_GRID_AFFINE  g = theta applied to the base coordinate (2p + 1)/size - 1 (affine_grid, align_corners=False).
 * A NaN coordinate (a missing annotation) gives a NaN pair.  One lane per point, plain fp32. */
int nemar_map_points(const float* pts, const float* pred, int grid_mode, float* out, int N, int P, int Hs, int Ws, int hf, int wf,
                     int Ho, int Wo, void* stream);

/* Composing two predictions (csrc/compose.hip; not in the reference, which applies one): ONE prediction that samples where two would in
 * sequence, so that a second look at an already-registered pair (a "recursive cascade"), or a registration carried over from an earlier
 * run, interpolates the image once — and so that nemar_warp_resampled_fwd, nemar_label_overlap and nemar_map_points, which read one
 * transformation, can apply and score the pair.
 * `first` (P1: first_mode, field size h1 x w1) is applied to the image first, A1(x) = A(S1(x)); `second` (P2: second_mode, h2 x w2) to
 * the result, A2(x) = A1(S2(x)) = A(S1(S2(x))).  Operands as nemar_warp_resampled_fwd takes them: NEMAR_GRID_UNET offsets [N,2,h,w] or
 * NEMAR_GRID_AFFINE dtheta [N,6] (h, w ignored); NEMAR_GRID_EXPLICIT is NEMAR_EINVAL.  At the composition size (H,W), for output pixel (h,w):
 *   (gx2, gy2) = the normalised coordinate nemar_warp_resampled_fwd computes for P2 at output size (H,W) (a UNet field resized in registers
 *                whenever (h2,w2) != (H,W));
 *   p          = ((gx2 + 1) * W - 1) / 2, ((gy2 + 1) * H - 1) / 2: the pixel position in the intermediate image, which has the same size;
 *   (gx1, gy1) = the continuous extension of P1's grid at p for output size (H,W), exactly what nemar_map_points evaluates before it
 *                unnormalises (beyond the border: the border texel of a UNet field, the linearly extended identity);
 *   out_field[n,0,h,w] = gx1 - linspace(-1,1,W)[w],  out_field[n,1,h,w] = gy1 - linspace(-1,1,H)[h].
 * The composite is always a NEMAR_GRID_UNET offset field [N,2,H,W], whatever the two modes were.  A zero UNet prediction is the
 * reference's slight zoom (linspace under align_corners=False), not the identity, and composition keeps that faithfully: compose(P1, 0) != P1.
 * (The identity is NEMAR_GRID_AFFINE with dtheta = 0.)
 * Optional fused warp, img [N,C,H,W] and out_img [N,C,H,W] both given or both NULL: out_img is bit for bit what
 * nemar_warp_resampled_fwd(img, out_field, NEMAR_GRID_UNET, NEMAR_SAMPLE_BILINEAR, out_img, N, C, H, W, H, W, H, W) writes — the moving
 * image of the next cascade pass, produced while the position is in registers; out_field is the same bits with and without it.
 * Plain fp32, no atomics, no workspace: bitwise repeatable.
 * NEMAR_EINVAL, nothing launched: NEMAR_GRID_EXPLICIT (or no mode at all) on either side; first, second or out_field NULL; exactly one
 * of img / out_img; any given pointer not 4-byte aligned (that is all the alignment asked for); C < 1 with img; a non-positive N, H or W;
 * h or w < 1 on a NEMAR_GRID_UNET side; N > 65535; H*W >= 2^31 (a field plane >= 2^30); out_field equal to first or second, or out_img
 * equal to an operand, img or out_field (the kernel gathers from them). */
int nemar_compose_pred(const float* first, int first_mode, int h1, int w1, const float* second, int second_mode, int h2, int w2,
                       float* out_field, const float* img, float* out_img, int C, int N, int H, int W, void* stream);

/* The gradient of nemar_compose_pred's out_field towards its two operands (csrc/compose.hip): what training a cascade with shared weights
 * needs.  Training size only: a NEMAR_GRID_UNET operand is AT the composition size, (h,w) == (H,W) — a resampled one is NEMAR_EINVAL (the
 * forward keeps accepting it); h and w of a NEMAR_GRID_AFFINE operand are ignored.  With out_c(x) = grid_at<M1>(first, p(x))_c - linspace_c(x),
 * p(x) = ((g2 + 1) * size - 1) / 2 of second's coordinate g2 at x, and gout [N,2,H,W]:
 *   gfirst, first UNET [N,2,H,W]   sum over x of w_k(p(x)) * gout_c(x) at the four texels the forward's bilinear taps read (source
 *                                  coordinate (p + 0.5) - 0.5 clamped to [0, size-1]; weights l0x l0y, l1x l0y, l0x l1y, l1x l1y).  p is
 *                                  anywhere, so this is a scatter: 64-bit fixed-point integer atomics into the zeroed leading bytes of the
 *                                  workspace, each w * gout rounded to a multiple of 2^(e - FIX), 2^(e-1) <= max |gout| of the call < 2^e
 *                                  (found on the device; e clamped at -80), FIX = min(40, 62 - ceil(log2(H W))) — the rule of
 *                                  nemar_svf_step_bwd — then gfirst = (accumulate_first ? gfirst : 0) + sum, the sum rounded to fp32 first;
 *   gfirst, first AFFINE [N,6]     sum over x of gout_x * (xb, yb, 1), gout_y * (xb, yb, 1), xb = (2 p.x + 1)/W - 1, yb = (2 p.y + 1)/H - 1:
 *                                  one record per 64 x 16 tile, merged in a fixed order;
 *   gp_a(x)                        sum_c gout_c(x) * d grid_at_c / d p_a.  First UNET: the identity's slope 2/(size-1) (0 for size 1) on
 *                                  the diagonal plus the bilinear slope of first's 2 x 2 cell, which is zero along an axis whose source
 *                                  coordinate was clamped (< 0 or > size-1).  First AFFINE: theta's 2 x 2 part times 2/W, 2/H;
 *   gsecond, second UNET [N,2,H,W] (gp_x * W/2, gp_y * H/2) at the pixel itself: (accumulate_second ? gsecond : 0) + that, no atomics;
 *   gsecond, second AFFINE [N,6]   sum over x of gp_x W/2 * (xb, yb, 1), gp_y H/2 * (xb, yb, 1) at the PIXEL's base coordinates
 *                                  xb = (2w + 1)/W - 1, yb = (2h + 1)/H - 1: tile records and the same merge.
 * A pixel whose position p is not finite contributes exactly 0 to both gradients.  Positions are clamped in float before the integer
 * conversion: no input value indexes outside a plane.  gfirst or gsecond may be NULL (not both): that gradient is not computed, and the
 * bits of the other do not depend on it.  Bitwise repeatable, no fp32 atomics, no host sync (capturable into a graph).
 * Workspace: nemar_compose_pred_bwd_workspace() bytes, 8-byte aligned, whose first nemar_compose_pred_bwd_zeroed_bytes() (the accumulator
 * of a UNET first; 0 for an AFFINE first) are zero on entry and left zero on return; the rest is scratch.
 * NEMAR_EINVAL, nothing launched: first, second, gout or workspace NULL; gfirst and gsecond both NULL; a given pointer not 4-byte aligned
 * (workspace: 8-byte); a non-positive N, H or W; N > 65535; H*W >= 2^31 (a UNET operand: >= 2^30); H > 16 * 65535; a mode that is not
 * NEMAR_GRID_UNET or NEMAR_GRID_AFFINE; a UNET operand with (h,w) != (H,W); gfirst or gsecond equal to first, second, gout or each other;
 * ws_bytes < nemar_compose_pred_bwd_workspace(). */
size_t nemar_compose_pred_bwd_workspace(int first_mode, int second_mode, int N, int H, int W);
size_t nemar_compose_pred_bwd_zeroed_bytes(int first_mode, int second_mode, int N, int H, int W);
int nemar_compose_pred_bwd(const float* first, int first_mode, int h1, int w1, const float* second, int second_mode, int h2, int w2,
                           const float* gout, float* gfirst, int accumulate_first, float* gsecond, int accumulate_second, void* workspace,
                           size_t ws_bytes, int N, int H, int W, void* stream);

/* Regularity of a registration (csrc/regularity.hip; not in the reference, which has no evaluation code): the Jacobian determinant of
 * the transformation a prediction describes, as a map and as fold / log-Jacobian statistics, at the size the images are registered at,
 * in one pass over the output.  pred, grid_mode, hf and wf are what nemar_warp_resampled_fwd takes (NEMAR_GRID_UNET offsets
 * [N,2,hf,wf], resized in registers; NEMAR_GRID_AFFINE dtheta [N,6], hf and wf ignored; NEMAR_GRID_EXPLICIT is NEMAR_EINVAL).
 * For output pixel (h,w) of size (Ho,Wo):
 *   (gx, gy) = the normalised coordinate nemar_warp_resampled_fwd, nemar_label_overlap and nemar_compose_pred compute for it (the same bits);
 *   p(h,w)   = ((gx + 1) * Wo - 1) / 2, ((gy + 1) * Ho - 1) / 2: the position in pixels of an image of the OUTPUT's own size (the p of
 *              nemar_compose_pred), so that the determinant does not depend on the source image's size and a pure resize has determinant 1;
 *   interior = h < Ho-1 and w < Wo-1: the pixel has both forward neighbours (nemar_registration_error's rule);
 *   det      = a.x * b.y - b.x * a.y with a = p(h,w+1) - p(h,w), b = p(h+1,w) - p(h,w), at interior pixels (nemar_registration_error's
 *              forward-difference expression); a FOLD is det <= 0.
 * det_out [N,Ho,Wo] or NULL: det at interior pixels, a quiet NaN in the last row and the last column; 4-byte alignment is all it needs.
 * counts [N,2] uint32 = (interior, folds), exact.  stats [N,5] = (min det, max det, sum det, sum log det, sum (log det)^2): min, max
 * and sum det over the interior pixels; the two log sums over the interior pixels with det > 0, of which there are interior - folds
 * (SDlogJ = sqrt(sum2 / k - (sum1 / k)^2) is the caller's arithmetic, in double).  Without an interior pixel (Ho == 1 or Wo == 1):
 * counts = (0, 0), min = +inf, max = -inf, sums 0.  Every statistic is a function of exactly the det values the map holds, and counts and
 * stats are the same bits with and without det_out.  A zero UNet prediction is the reference's slight zoom (linspace under
 * align_corners=False): det = Wo Ho / ((Wo-1)(Ho-1)); NEMAR_GRID_AFFINE gives theta's 2 x 2 determinant at every pixel.
 * Per-workgroup partials (one per 64 x 16 output tile) go to the workspace and are merged in a fixed order: no atomics, bitwise
 * repeatable.
 * NEMAR_EINVAL, nothing launched: pred, counts, stats or workspace NULL; any given pointer not 4-byte aligned; a grid_mode other than
 * NEMAR_GRID_UNET / NEMAR_GRID_AFFINE; a non-positive N, Ho or Wo; hf or wf < 1 with NEMAR_GRID_UNET; N > 65535; Ho*Wo >= 2^31 (a field
 * plane >= 2^30, Ho > 16 * 65535); det_out equal to pred; ws_bytes < nemar_jacobian_stats_workspace(). */
size_t nemar_jacobian_stats_workspace(int N, int Ho, int Wo);
int nemar_jacobian_stats(const float* pred, int grid_mode, float* det_out, unsigned* counts, float* stats, void* workspace,
                         size_t ws_bytes, int N, int hf, int wf, int Ho, int Wo, void* stream);

/* Intensity agreement of a registration (csrc/similarity.hip; not in the reference, which has no evaluation code): a score that needs
 * no annotation — the joint histogram of the registered moving image and the fixed image (mutual information, across modalities) and
 * the moments behind NCC / MSE / MAE (within one modality), in one pass over the output.  pred, grid_mode, hf and wf are what
 * nemar_warp_resampled_fwd takes (NEMAR_GRID_UNET offsets [N,2,hf,wf], resized in registers; NEMAR_GRID_AFFINE dtheta [N,6], hf and wf
 * ignored; NEMAR_GRID_EXPLICIT is NEMAR_EINVAL).  moving [N,Cm,Hs,Ws] (any size), fixed [N,Cf,Ho,Wo].  For output pixel x:
 *   a(x) = (sum over the Cm channels, ascending, of the value nemar_warp_resampled_fwd(..., NEMAR_SAMPLE_BILINEAR) would write there —
 *          the same code computes it; the warped image is never written to memory) * (1.f / Cm);
 *   b(x) = (sum over the Cf channels, ascending, of fixed(x)) * (1.f / Cf).
 * x COUNTS iff the nearest texel of its sampling position lies inside the source (the pixels where nemar_label_overlap's warped map is
 * not padding: an identity prediction at equal sizes counts every pixel) and neither a(x) nor b(x) is NaN.
 *   bin(v) = clamp((int)floorf((v - lo) * (bins / (hi - lo))), 0, bins - 1) per side: values outside [lo, hi] go to the end bins.
 * counts [N,bins,bins] uint32 is OVERWRITTEN (cleared on `stream` by the entry point): counts[n][bin(a)][bin(b)] over the counted pixels.
 * Its sum is the number of counted pixels, its row and column sums the marginals.  Integers added with integer atomics: order
 * independent, bitwise repeatable.
 * moments [N,6] or NULL: sum a, sum b, sum a^2, sum b^2, sum ab, sum |a - b| over the counted pixels (NCC, MSE, MAE are the caller's
 * arithmetic, in double).  Per-workgroup records go to the workspace and are merged in a fixed order: no atomics, bitwise repeatable.
 * With moments == NULL no workspace is needed (workspace and ws_bytes are ignored) and counts holds the same bits.
 * NEMAR_EINVAL, nothing launched: moving, fixed, pred or counts NULL; moments without a workspace; any pointer in use not 4-byte
 * aligned (that is all the alignment asked for); a grid_mode other than NEMAR_GRID_UNET / NEMAR_GRID_AFFINE; bins outside 2 .. 64; Cm or
 * Cf outside 1 .. 64; hi <= lo on either side (or a range without a finite bin width); a non-positive size; hf or wf < 1 with
 * NEMAR_GRID_UNET; N > 65535; Ho*Wo or Hs*Ws >= 2^31 (a field plane >= 2^30); with moments, ws_bytes < nemar_joint_histogram_workspace(). */
size_t nemar_joint_histogram_workspace(int N, int Ho, int Wo);
int nemar_joint_histogram(const float* moving, const float* fixed, const float* pred, int grid_mode, unsigned* counts, float* moments,
                          void* workspace, size_t ws_bytes, int N, int Cm, int Cf, int bins, float lo_m, float hi_m, float lo_f,
                          float hi_f, int Hs, int Ws, int hf, int wf, int Ho, int Wo, void* stream);

/* Boundary agreement of a registration (csrc/surface.hip; not in the reference, which has no evaluation code): the distances between the
 * class boundaries of the warped moving label map and of the fixed label map, from which the Hausdorff distance, its 95th percentile
 * (HD95) and the average symmetric surface distance (ASSD) follow.  Everything happens on the fixed image's plane Ho x Wo at pixel
 * spacing 1.  labels_moving, labels_fixed, pred, grid_mode, hf and wf are what nemar_label_overlap takes.
 *   m(x) = the class (nemar_label_overlap's rule: k iff the value == (float)k for an integer 0 <= k < K, else no class) of the value
 *          nemar_warp_resampled_fwd(..., NEMAR_SAMPLE_NEAREST) would write at x — the same code computes it; zero padding is class 0;
 *   f(x) = the class of labels_fixed(x).
 * A BOUNDARY pixel of class k in a map is a pixel of class k with at least one 4-neighbour that is not of class k; a neighbour outside
 * the plane is not of class k (S ^ binary_erosion(S), 4-connected, border_value = 0: MedPy's convention), so a class that fills the
 * plane has the plane's border as its boundary.  A pixel of no class is never a boundary pixel.
 * Direction 0 (moving -> fixed): for every boundary pixel p of class k in m, d2(p) = min over the boundary pixels q of class k in f of
 * |p - q|^2, a non-negative integer.  Direction 1 swaps the maps.  The pair (sample, class) is DEFINED when the class has boundary
 * pixels in both maps; otherwise it has no distances.
 * With B = max_dist * max_dist:
 *   counts [N,K,2,3] uint32 (OVERWRITTEN) per sample, class and direction: [0] boundary pixels (counted whether or not the pair is
 *          defined), [1] far = those with d2 >= B, [2] the largest d2; far and the largest d2 are 0 where the pair is not defined;
 *   hist   [N,K,2,B] uint32 (OVERWRITTEN): hist[n,k,dir,b] = boundary pixels with d2 == b; all zero where the pair is not defined;
 *   dist2  [N,2,Ho,Wo] int32 or NULL: plane 0 holds d2 at every boundary pixel of m, plane 1 at every boundary pixel of f; -1 where the
 *          pixel is no boundary pixel, -2 at a boundary pixel whose pair is not defined.  counts and hist are the same bits without it.
 * counts and hist are cleared on `stream` by the entry point.  Everything after the warp's coordinate is integer arithmetic, added with
 * integer atomics (atomicAdd, atomicMax): exact, independent of the order of arrival, bitwise repeatable; no host synchronisation.
 * The workspace holds the two class maps twice (with and without the boundary flag, 16 bits per pixel) and, for one chunk of classes
 * at a time, two 16-bit planes of vertical distances per class and sample: the entry point takes min(K, max(1, 128 MiB / (4 N Ho Wo)))
 * classes per chunk, so nemar_surface_distance_workspace = 8 N Ho Wo + that many * 4 N Ho Wo bytes (0 for a shape the call refuses).
 * A class without boundary pixels on either side costs no sweep of the plane: the kernels read the counts on the device.
 * NEMAR_EINVAL, nothing written: labels_moving, labels_fixed, pred, counts, hist or workspace NULL; any given pointer not 4-byte
 * aligned; K outside 1 .. 1024; max_dist outside 1 .. 128; Ho or Wo above 32768 (so that d2 < 2^31); a non-positive size; N > 65535;
 * Hs*Ws >= 2^31; a grid_mode other than NEMAR_GRID_UNET / NEMAR_GRID_AFFINE; hf or wf < 1 with NEMAR_GRID_UNET (a field plane >= 2^30);
 * workspace_bytes < nemar_surface_distance_workspace(). */
size_t nemar_surface_distance_workspace(int N, int K, int Ho, int Wo);
int nemar_surface_distance(const float* labels_moving, const float* labels_fixed, const float* pred, int grid_mode, unsigned* counts,
                           unsigned* hist, int* dist2, void* workspace, size_t workspace_bytes, int N, int K, int max_dist, int Hs, int Ws,
                           int hf, int wf, int Ho, int Wo, void* stream);

/* ---- K13: losses (already multiplied by their lambda `weight`; optionally accumulated into a device scalar) ------
 * l1:  torch.nn.L1Loss — reference models/nemar_model.py:68,179,195; b == NULL gives mean|a|
 *      (affine STN regulariser, reference models/stn/affine_stn.py:136-138).
 * gan: GANLoss.__call__ against a constant target — reference models/networks.py:263-281.
 *      mode NEMAR_GAN_VANILLA (BCEWithLogits) | NEMAR_GAN_LSGAN (MSE) | NEMAR_GAN_WGANGP (+-mean).
 * fwd: loss[0] = (accumulate ? loss[0] : 0) + weight * L ;  bwd: grad = gscale[0] * weight * dL/dx. */
#define NEMAR_GAN_VANILLA 0
#define NEMAR_GAN_LSGAN 1
#define NEMAR_GAN_WGANGP 2
size_t nemar_loss_workspace(void);
int nemar_l1_loss_fwd(const float* a, const float* b, long long n, float weight, float* loss, int accumulate,
                      void* workspace, size_t ws_bytes, void* stream);
int nemar_l1_loss_bwd(const float* a, const float* b, long long n, const float* gscale, float weight, float* ga,
                      int accumulate, void* stream);
int nemar_gan_loss_fwd(const float* x, long long n, int mode, int target_is_real, float weight, float* loss,
                       int accumulate, void* workspace, size_t ws_bytes, void* stream);
int nemar_gan_loss_bwd(const float* x, long long n, int mode, int target_is_real, const float* gscale,
                       float weight, float* gx, void* stream);

/* ---- K15: fused Adam over a flat parameter buffer --------------------------------------------------------------------
 * torch.optim.Adam(lr, betas=(beta1, beta2), eps).step() — reference models/nemar_model.py:128-137 (construction),
 * :274,282-283 (step).  p,g,m,v: length n; step is 1-based.  Hyper-parameters are doubles, as in torch. */
int nemar_adam_step(float* p, const float* g, float* m, float* v, long long n, double lr, double beta1,
                    double beta2, double eps, int step, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NEMAR_HIP_H */
