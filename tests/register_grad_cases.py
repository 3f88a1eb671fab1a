"""Backend-agnostic test bodies of nemar_warp_resampled_bwd (csrc/register.hip: the gradient of the fused resample + warp towards the
prediction), driven through tests/backends.py (EmuBackend: host-emulated kernels, CPU tier; HipBackend: the gfx950 library, `-m gpu`).

Inputs are register_cases.draw's (smooth field, amp 0.15).  gout is seeded normal noise, set to ZERO at every output pixel whose float64
sampling position lies within KINK_BAND px of an integer in x or y: the warp's derivative jumps there and an fp32 evaluation may sit in
the neighbouring cell.  Truth and kernel get the same zeroed gout, so nothing is left out of a comparison; the float64 reference alone
must mark <= 1 % of a case's pixels.

The float64 truth is torch on the CPU with autograd: F.interpolate + torch.linspace / F.affine_grid + F.grid_sample (register_cases.ref_warp
made differentiable).  The rules:
  float64   per element of gpred: |kernel - truth| <= MARGIN x yardstick + CHAIN x 2^-24 x S.  yardstick = the max-abs error of the same
            torch code in float32 (both are fp32 evaluations of one formula: the error is position error times the image's second
            difference); S = the float64 sum of the absolute contributions to the element (|dv| of every pixel times its weight);
            CHAIN = the fp32 additions and multiplications a contribution passes through in the kernel as built:
              every route     C (the channel sum of a pixel) + 1 (the W/2 scale)
              UNET equal      + 1 (accumulate)
              UNET resampled  + 2 (weight x dv, weight x row sum) + 1 (the sum of a coinciding tap pair)
                              + row pass: the pixels of a tile row that tap one field column, <= min(64, floor(2 Wo / wf) + 1)
                              + column pass: likewise <= min(16, floor(2 Ho / hf) + 1)
                              + merge: the tiles whose patch holds the texel, <= (span_y / 16 + 2)(span_x / 64 + 2), + 1 (accumulate)
              AFFINE          + 1 (x base coordinate) + 4 (the lane's pixels) + 6 (wave tree) + 4 (waves)
                              + merge: ceil(tiles / 256) + 6 + 4 + 1 (accumulate)
  bitwise   UNET at equal sizes with the source at the output's size: nemar_grid_sample_bwd's grid gradient on the same backend, bit for
            bit (the expression is restated in that order, -ffp-contract=off).
  adjoint   <gout, (fwd(pred + e d) - fwd(pred - e d)) / 2e> in float64 arithmetic on the fused FORWARD's outputs against <gpred, d>, d one
            texel (or one dtheta entry): no reference.  The bound is the same with the yardstick replaced by the difference's own error
            (case_adjoint works it out).
  repeat    two calls give the same bits; accumulate = 1 onto a pre-fill equals pre-fill + result within one rounding; accumulate = 0
            overwrites poison everywhere; every pointer 4 bytes off the 16-byte grid gives the aligned call's bits."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from register_cases import BILINEAR, DOWN, EQUAL, GRID_AFFINE, GRID_EXPLICIT, GRID_UNET, MARGIN, _shape, draw

KINK_BAND = 1e-3           # px
KINK_SHARE = 0.01
EPS24 = 2.0 ** -24
# fp32 roundings on the way to a pixel's normalised coordinate (case_adjoint): UNET the linspace fma, the three of the resize blend, the
# sum; AFFINE (2 w + 1) / n, - 1, two products, two sums
COORD_ROUNDINGS = {GRID_UNET: 5, GRID_AFFINE: 6}

#           (hf, wf),  (Ho, Wo),   (Hs, Ws) or None = the output size,  C
RESAMPLED = [((32, 48), (131, 203), None, 3), ((16, 24), (67, 45), None, 5), ((32, 48), (131, 203), (90, 120), 3),
             ((9, 7), (131, 203), None, 2), ((1, 1), (33, 70), None, 1), ((64, 64), (65, 65), None, 1), ((5, 64), (17, 64), (30, 50), 3)]
TILE_EDGES = [((8, 12), hw, None, 2) for hw in ((15, 70), (16, 64), (17, 65), (33, 129))]
SIZES = RESAMPLED + [EQUAL] + TILE_EDGES
MODES = [GRID_UNET, GRID_AFFINE]
mode_id = lambda m: "unet" if m == GRID_UNET else "affine"


# ---- torch on the CPU, differentiable: the float64 truth and (dtype float32) the yardstick ------------------------------------------------
def _grid(p, mode, Ho, Wo):
    dtype = p.dtype
    if mode == GRID_UNET:
        f = p if tuple(p.shape[2:]) == (Ho, Wo) else F.interpolate(p, size=(Ho, Wo), mode='bilinear', align_corners=False)
        x, y = torch.linspace(-1, 1, Wo, dtype=dtype), torch.linspace(-1, 1, Ho, dtype=dtype)
        return torch.stack([x[None, None, :] + f[:, 0], y[None, :, None] + f[:, 1]], dim=-1)
    theta = p + torch.tensor([1, 0, 0, 0, 1, 0], dtype=dtype)[None]
    return F.affine_grid(theta.view(-1, 2, 3), (p.shape[0], 1, Ho, Wo), align_corners=False)


def ref_grad(img, pred, mode, Ho, Wo, gout, dtype=torch.float64):
    """(d <gout, warp(img, pred)> / d pred, d / d grid [N,Ho,Wo,2]) as float64 numpy"""
    p = torch.tensor(np.asarray(pred), dtype=dtype, requires_grad=True)
    grid = _grid(p, mode, Ho, Wo)
    grid.retain_grad()
    out = F.grid_sample(torch.as_tensor(np.asarray(img), dtype=dtype), grid, mode='bilinear', padding_mode='zeros', align_corners=False)
    (out * torch.as_tensor(np.asarray(gout), dtype=dtype)).sum().backward()
    return p.grad.numpy().astype(np.float64), grid.grad.numpy().astype(np.float64)


def abs_sum(pred, mode, Ho, Wo, ggrid):
    """S: |d / d grid| of every pixel pushed through the (linear) map from the prediction to the grid with the weights' magnitudes"""
    a = torch.as_tensor(np.abs(ggrid))
    if mode == GRID_UNET:
        p = torch.zeros(np.asarray(pred).shape, dtype=torch.float64, requires_grad=True)
        (_grid(p, mode, Ho, Wo) * a).sum().backward()          # the resize's weights are non-negative
        return p.grad.numpy()
    xb = (2 * torch.arange(Wo, dtype=torch.float64) + 1) / Wo - 1
    yb = (2 * torch.arange(Ho, dtype=torch.float64) + 1) / Ho - 1
    base = torch.stack([xb.abs()[None, :].expand(Ho, Wo), yb.abs()[:, None].expand(Ho, Wo), torch.ones(Ho, Wo, dtype=torch.float64)])
    return torch.einsum('nhwk,chw->nkc', a, base).reshape(-1, 6).numpy()


def kink_mask(pred, mode, Ho, Wo, Hs, Ws):
    """[N,Ho,Wo] True where the float64 sampling position is within KINK_BAND px of an integer in x or y"""
    g = _grid(torch.as_tensor(np.asarray(pred), dtype=torch.float64), mode, Ho, Wo).numpy()
    ix, iy = ((g[..., 0] + 1) * Ws - 1) / 2, ((g[..., 1] + 1) * Hs - 1) / 2
    near = lambda v: np.abs(v - np.rint(v)) < KINK_BAND
    return near(ix) | near(iy)


def chain(mode, size):
    (hf, wf), (Ho, Wo), _, C = size
    tiles = math.ceil(Ho / 16) * math.ceil(Wo / 64)
    if mode == GRID_AFFINE:
        return C + 1 + 1 + 4 + 6 + 4 + math.ceil(tiles / 256) + 6 + 4 + 1
    if (hf, wf) == (Ho, Wo):
        return C + 1 + 1
    span_x, span_y = 2 * Wo // wf + 1, 2 * Ho // hf + 1
    return C + 1 + 3 + min(64, span_x) + min(16, span_y) + (span_y // 16 + 2) * (span_x // 64 + 2) + 1


def draw_case(seed, mode, size, N=2):
    """(shape, img, pred, gout) — gout zeroed on the kinks, the share of zeroed pixels asserted"""
    shape = _shape(size, N)
    N, C, Hs, Ws, hf, wf, Ho, Wo = shape
    img, pred = draw(seed, mode, N, C, hf, wf, Hs, Ws)
    gout = np.random.default_rng(seed + 100).standard_normal((N, C, Ho, Wo)).astype(np.float32)
    kink = kink_mask(pred, mode, Ho, Wo, Hs, Ws)
    assert kink.mean() <= KINK_SHARE, (size, mode, kink.mean())
    gout[np.broadcast_to(kink[:, None], gout.shape)] = 0.0
    return shape, img, pred, gout


# ---- drivers ------------------------------------------------------------------------------------------------------------------------------
def pred_shape(mode, shape):
    N, C, Hs, Ws, hf, wf, Ho, Wo = shape
    return (N, 2, hf, wf) if mode == GRID_UNET else (N, 6)


def workspace(be, mode, shape):
    """exactly the queried bytes"""
    N, C, Hs, Ws, hf, wf, Ho, Wo = shape
    nbytes = be.lib.warp_resampled_bwd_workspace(mode, N, hf, wf, Ho, Wo)
    return be.bytes_buf(nbytes), nbytes


def run_bwd(be, d_img, d_pred, d_gout, mode, shape, d_gpred=None, accumulate=0, ws=None):
    N, C, Hs, Ws, hf, wf, Ho, Wo = shape
    d_gpred = be.full(pred_shape(mode, shape), np.nan) if d_gpred is None else d_gpred
    d_ws, nbytes = workspace(be, mode, shape) if ws is None else ws
    be.lib.warp_resampled_bwd(be.ptr(d_img), be.ptr(d_pred), mode, be.ptr(d_gout), be.ptr(d_gpred), accumulate, N, C, Hs, Ws, hf, wf, Ho, Wo,
                              be.ptr(d_ws), nbytes, be.stream)
    return d_gpred


def run_fwd(be, d_img, d_pred, mode, shape):
    N, C, Hs, Ws, hf, wf, Ho, Wo = shape
    d_out = be.full((N, C, Ho, Wo), np.nan)
    be.lib.warp_resampled_fwd(be.ptr(d_img), be.ptr(d_pred), mode, BILINEAR, be.ptr(d_out), N, C, Hs, Ws, hf, wf, Ho, Wo, be.stream)
    return d_out


def _what(mode, size):
    (hf, wf), (Ho, Wo), src, C = size
    return "%s field %s -> %s source %s C %d" % (mode_id(mode), (hf, wf), (Ho, Wo), src or (Ho, Wo), C)


# ---- 1. against float64 ----------------------------------------------------------------------------------------------------------------------
def case_float64(be, mode, size, seed=1):
    shape, img, pred, gout = draw_case(seed, mode, size)
    N, C, Hs, Ws, hf, wf, Ho, Wo = shape
    got = be.np(run_bwd(be, be.dev(img), be.dev(pred), be.dev(gout), mode, shape))
    want, ggrid = ref_grad(img, pred, mode, Ho, Wo, gout)
    yard = np.abs(ref_grad(img, pred, mode, Ho, Wo, gout, torch.float32)[0] - want).max()
    S = abs_sum(pred, mode, Ho, Wo, ggrid).reshape(want.shape)
    err = np.abs(got.reshape(want.shape) - want)
    bound = MARGIN * yard + chain(mode, size) * EPS24 * S
    print("register grad %-58s kernel %.3e  torch-fp32 %.3e  ratio %.2f  worst err/bound %.3f  max |g| %.3e"
          % (_what(mode, size), err.max(), yard, err.max() / yard if yard else float('inf'), (err / bound).max(), np.abs(want).max()))
    assert np.all(np.isfinite(got)), _what(mode, size)
    assert np.all(err <= bound), (_what(mode, size), float(err.max()), float(yard), float((err / bound).max()))
    return err.max(), yard


# ---- 2. equal sizes: nemar_grid_sample_bwd's grid gradient, bit for bit ---------------------------------------------------------------------
def case_equal_bitwise(be, size=EQUAL, seed=2):
    shape, img, pred, gout = draw_case(seed, GRID_UNET, size)
    N, C, Hs, Ws, hf, wf, Ho, Wo = shape
    assert (hf, wf) == (Ho, Wo) == (Hs, Ws)
    d_img, d_pred, d_gout = be.dev(img), be.dev(pred), be.dev(gout)
    got = be.raw(run_bwd(be, d_img, d_pred, d_gout, GRID_UNET, shape))
    d_gg = be.full((N, 2, Ho, Wo), np.nan)
    be.lib.grid_sample_bwd(be.ptr(d_img), be.ptr(d_pred), GRID_UNET, be.ptr(d_gout), None, 0, be.ptr(d_gg), 0, N, C, Hs, Ws, Ho, Wo, None, 0,
                           be.stream)
    assert np.array_equal(got, be.raw(d_gg)), "gpred != nemar_grid_sample_bwd's grid gradient at equal sizes"


# ---- 3. adjoint identity on the fused forward ------------------------------------------------------------------------------------------------
def case_adjoint(be, mode, size, seed=3, step=2.0 ** -8):
    """<gout, (fwd(pred + e d) - fwd(pred - e d)) / 2e> against <gpred, d>, d a unit perturbation of one element of pred (e = 2^-8
    normalised units: 0.4 px at a 203-wide source — large, to keep the forward's rounding small against the difference).

    One element of pred moves a pixel's sampling position along ONE axis, and the forward is linear in that inside a cell.  gout is
    therefore also zeroed wherever a displaced evaluation changes cell or comes within KINK_BAND of doing so (float64 reference positions
    at pred +- e d): on what remains the central difference has NO truncation error, and what it carries is the forward's own fp32
    rounding, amplified by 1 / 2e.  That rounding, modelled per pixel whose two outputs differ at all:
      position   each evaluation's sampling position along the moved axis is off by at most _position_error (half a float32 spacing
                 per rounding, at the pixel's own values), which moves the pixel's term by that times |sum_ch gout x slope|, the slope
                 being the float64 slope of the cell the pixel samples (_slopes): the local texel differences, not the image's range;
      other axis its coordinate has the SAME bits in both evaluations, so its error enters only through how much the slope along it
                 differs between the two: _position_error x |sum_ch gout (slope_hi - slope_lo)|, once;
      blend      per channel and evaluation FWD_ULPS x 2^-24 x |gout out| (four weighted products, three sums, the weights' products).
    The terms of different pixels (and the blend's of different channels) are roundings of unrelated values: taken as independent,
    zero-mean and bounded by the above, Hoeffding's inequality bounds their sum by SIGMAS x sqrt(sum of squares) except with probability
    2 exp(-SIGMAS^2 / 2) = 3e-8 at SIGMAS = 6 — the usual probabilistic rounding model, here on fixed seeds.  That, over 2e, takes the
    yardstick's place in the float64 rule, without MARGIN.  The test also asserts that the bound is small against the gradient it
    checks: a bound that a zero gradient would pass checks nothing."""
    FWD_ULPS, SIGMAS = 8, 6.0
    shape, img, pred, gout = draw_case(seed, mode, size)
    N, C, Hs, Ws, hf, wf, Ho, Wo = shape
    d_img = be.dev(img)
    flat = pred.reshape(N, -1)
    S_all = abs_sum(pred, mode, Ho, Wo, ref_grad(img, pred, mode, Ho, Wo, gout)[1]).reshape(N, -1)
    if mode == GRID_UNET:
        cells = sorted({(0, 0), (hf - 1, wf - 1), (0, wf // 2), (hf // 2, wf // 2)})
        picks = []
        for k, (i, j) in enumerate(cells):       # (sample, element): planes and samples alternate; an element nothing reaches (its pixels
            tries = [(n, p * hf * wf + i * wf + j) for p in (k % 2, 1 - k % 2) for n in (k % 2, 1 - k % 2)]      # sample outside the
            live = [t for t in tries if S_all[t] > 0]                                                            # source) is no check
            assert live, (_what(mode, size), (i, j), "no sample or plane of this texel receives a gradient")
            picks.append(live[0])
    else:
        picks = [(0, 0), (1, 1), (0, 2), (1, 5)]
    base_cell = None
    for n, e in picks:
        delta = np.zeros_like(flat)
        delta[n, e] = 1.0
        lo, hi = (flat - step * delta).reshape(pred.shape), (flat + step * delta).reshape(pred.shape)
        cell = lambda p: _cells(p, mode, Ho, Wo, Hs, Ws)
        base_cell = cell(pred) if base_cell is None else base_cell
        moved = np.any(cell(lo) != base_cell, axis=-1) | np.any(cell(hi) != base_cell, axis=-1)
        moved |= kink_mask(lo, mode, Ho, Wo, Hs, Ws) | kink_mask(hi, mode, Ho, Wo, Hs, Ws)
        g = gout.copy()
        g[np.broadcast_to(moved[:, None], g.shape)] = 0.0
        out_hi = be.np(run_fwd(be, d_img, be.dev(hi), mode, shape))
        out_lo = be.np(run_fwd(be, d_img, be.dev(lo), mode, shape))
        fd = float((g.astype(np.float64) * (out_hi - out_lo)).sum() / (2 * step))
        gpred = be.np(run_bwd(be, d_img, be.dev(pred), be.dev(g), mode, shape)).reshape(N, -1)
        _, ggrid = ref_grad(img, pred, mode, Ho, Wo, g)
        S = abs_sum(pred, mode, Ho, Wo, ggrid).reshape(N, -1)[n, e]
        assert S > 0, (_what(mode, size), n, e, "the masks left this element nothing to check")
        differs = (out_hi != out_lo).any(axis=1)     # [N,Ho,Wo] (a pixel the element does not reach gives the same bits twice: no error)
        ax = 0 if (e < hf * wf if mode == GRID_UNET else e < 3) else 1               # the axis this element moves the position along
        g64 = g.astype(np.float64)
        var = 0.0
        slopes = {}
        for name, p, out in (("hi", hi, out_hi), ("lo", lo, out_lo)):
            slopes[name] = _slopes(img, p, mode, Ho, Wo)                             # [N,C,Ho,Wo,2] d out / d (ix, iy), float64
            pos = _position_error(p, mode, Ho, Wo, Hs, Ws)[..., ax] * np.abs((g64 * slopes[name][..., ax]).sum(axis=1))
            var += float((pos[differs] ** 2).sum()) + float(((FWD_ULPS * EPS24 * g64 * out) ** 2).sum(axis=1)[differs].sum())
        cross = _position_error(pred, mode, Ho, Wo, Hs, Ws)[..., 1 - ax] * np.abs((g64 * (slopes["hi"][..., 1 - ax] - slopes["lo"][..., 1 - ax])).sum(axis=1))
        var += float((cross[differs] ** 2).sum())
        fd_err = SIGMAS * np.sqrt(var) / (2 * step)
        bound = fd_err + chain(mode, size) * EPS24 * S
        diff = abs(fd - gpred[n, e])
        print("register adjoint %-52s element (%d, %d)  fd %+.6e  gpred %+.6e  diff %.2e  bound %.2e (%.1f %% of |gpred|)  moved %.4f"
              % (_what(mode, size), n, e, fd, gpred[n, e], diff, bound, 100 * bound / abs(gpred[n, e]), moved.mean()))
        assert diff <= bound, (_what(mode, size), n, e, fd, float(gpred[n, e]), bound)
        assert bound <= 0.05 * abs(gpred[n, e]), (_what(mode, size), n, e, "the bound could not tell this gradient from a wrong one", bound)


def _slopes(img, pred, mode, Ho, Wo):
    """[N,C,Ho,Wo,2]: d out[n,c,h,w] / d (ix, iy), the slopes of the cell each pixel samples, float64"""
    im = torch.as_tensor(np.asarray(img), dtype=torch.float64)
    Hs, Ws = im.shape[2:]
    per_channel = []
    for c in range(im.shape[1]):
        grid = _grid(torch.as_tensor(np.asarray(pred), dtype=torch.float64), mode, Ho, Wo).requires_grad_(True)
        F.grid_sample(im[:, c:c + 1], grid, mode='bilinear', padding_mode='zeros', align_corners=False).sum().backward()
        per_channel.append(grid.grad.numpy() / np.array([Ws / 2.0, Hs / 2.0]))
    return np.stack(per_channel, axis=1)


def _position_error(pred, mode, Ho, Wo, Hs, Ws):
    """[N,Ho,Wo,2]: the most the fp32 sampling position (ix, iy) of each pixel can be off, in px — half a float32 spacing per rounding of
    the kernel's expression ((g + 1) size - 1) / 2, at the values the float64 reference has there.  g itself: COORD_ROUNDINGS at the size
    of its largest intermediate (|g| + 0.5 covers the identity or base term and the offset or theta products next to it)."""
    g = _grid(torch.as_tensor(np.asarray(pred), dtype=torch.float64), mode, Ho, Wo).numpy()
    size = np.array([float(Ws), float(Hs)])
    half = lambda v: 0.5 * np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)
    e_g = COORD_ROUNDINGS[mode] * half(np.abs(g) + 0.5)
    return 0.5 * ((e_g + half(g + 1)) * size + half((g + 1) * size) + half((g + 1) * size - 1))


def _cells(pred, mode, Ho, Wo, Hs, Ws):
    g = _grid(torch.as_tensor(np.asarray(pred), dtype=torch.float64), mode, Ho, Wo).numpy()
    return np.stack([np.floor(((g[..., 0] + 1) * Ws - 1) / 2), np.floor(((g[..., 1] + 1) * Hs - 1) / 2)], axis=-1)


# ---- 4. repeatable, accumulate, overwrite, alignment -----------------------------------------------------------------------------------------
def _off_by_4_bytes(be, a):
    """`a` in a buffer that starts 4 bytes past a 16-byte boundary"""
    d_buf = be.dev(np.concatenate([[0.0], np.asarray(a, dtype=np.float32).ravel()]))
    return be.sub(d_buf, 1, d_buf.shape[0])


def case_repeat_accumulate(be, mode, size, seed=4):
    shape, img, pred, gout = draw_case(seed, mode, size)
    d_img, d_pred, d_gout = be.dev(img), be.dev(pred), be.dev(gout)
    first = run_bwd(be, d_img, d_pred, d_gout, mode, shape)              # onto NaN poison: accumulate = 0 overwrites every element
    a = be.raw(first)
    assert np.all(np.isfinite(be.np(first)))
    assert np.array_equal(a, be.raw(run_bwd(be, d_img, d_pred, d_gout, mode, shape))), "not repeatable: " + _what(mode, size)
    fill = np.random.default_rng(seed).standard_normal(pred_shape(mode, shape)).astype(np.float32)
    got = be.np(run_bwd(be, d_img, d_pred, d_gout, mode, shape, d_gpred=be.dev(fill), accumulate=1))
    want = fill.astype(np.float64) + be.np(first)
    assert np.all(np.abs(got - want) <= EPS24 * np.abs(want) * (1 + 1e-9)), "accumulate: " + _what(mode, size)


def case_unaligned(be, mode, size, seed=5):
    """every pointer one float past a 16-byte boundary: the aligned call's bits"""
    shape, img, pred, gout = draw_case(seed, mode, size)
    N, C, Hs, Ws, hf, wf, Ho, Wo = shape
    aligned = be.raw(run_bwd(be, be.dev(img), be.dev(pred), be.dev(gout), mode, shape))
    d_ws, nbytes = workspace(be, mode, shape)
    d_wbuf = be.bytes_buf(nbytes + 4)
    d_gpred = _off_by_4_bytes(be, np.full(int(np.prod(pred_shape(mode, shape))), np.nan))
    run_bwd(be, _off_by_4_bytes(be, img), _off_by_4_bytes(be, pred), _off_by_4_bytes(be, gout), mode, shape, d_gpred=d_gpred,
            ws=(be.sub(d_wbuf, 4, nbytes + 4), nbytes))
    assert np.array_equal(be.raw(d_gpred), aligned), "unaligned != aligned: " + _what(mode, size)


# ---- 5. non-finite predictions ---------------------------------------------------------------------------------------------------------------
def case_non_finite(be, mode, size, seed=6):
    """one NaN texel in a field, one Inf in a dtheta: the pixels it reaches contribute exactly 0 — gpred finite, guards intact"""
    shape, img, pred, gout = draw_case(seed, mode, size)
    pred = pred.copy()
    if mode == GRID_UNET:
        pred[0, 1, pred.shape[2] // 2, pred.shape[3] // 3] = np.nan
    else:
        pred[1, 4] = np.inf
    got = be.np(run_bwd(be, be.dev(img), be.dev(pred), be.dev(gout), mode, shape))
    assert np.all(np.isfinite(got)), _what(mode, size)
    if mode == GRID_AFFINE:
        assert np.all(got[1] == 0.0)          # every pixel of that sample has a non-finite coordinate
        assert np.any(got[0] != 0.0)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------
def case_refusals(be):
    """NEMAR_EINVAL (-1), a message, nothing launched: gpred keeps its fill"""
    from nemar_amd._lib import NemarHipError
    einval = r"failed \(-1\): warp_resampled_bwd: \S"
    N, C, Hs, Ws, hf, wf, Ho, Wo = 2, 3, 12, 16, 6, 8, 24, 40
    d_img, d_pred, d_th, d_gout = be.zeros(N, C, Hs, Ws), be.zeros(N, 2, hf, wf), be.zeros(N, 6), be.zeros(N, C, Ho, Wo)
    d_gpred = be.full((N, 2, hf, wf), 7.0)
    nbytes = max(be.lib.warp_resampled_bwd_workspace(GRID_UNET, N, hf, wf, Ho, Wo), be.lib.warp_resampled_bwd_workspace(GRID_AFFINE, N, hf, wf, Ho, Wo))
    assert be.lib.warp_resampled_bwd_workspace(GRID_UNET, N, hf, wf, Ho, Wo) > 0
    d_ws = be.bytes_buf(nbytes)
    img, pred, th, gout, gpred, ws = (be.ptr(d) for d in (d_img, d_pred, d_th, d_gout, d_gpred, d_ws))
    good = [img, pred, GRID_UNET, gout, gpred, 0, N, C, Hs, Ws, hf, wf, Ho, Wo, ws, nbytes]
    names = ("img", "pred", "mode", "gout", "gpred", "acc", "N", "C", "Hs", "Ws", "hf", "wf", "Ho", "Wo", "ws", "wsb")

    def refused(**change):
        args = [change.get(k, v) for k, v in zip(names, good)]
        with pytest.raises(NemarHipError, match=einval):
            be.lib.warp_resampled_bwd(*args, be.stream)

    for k in ("img", "pred", "gout", "gpred", "ws"):             # null pointers
        refused(**{k: None})
    for k in ("N", "C", "Hs", "Ws", "Ho", "Wo", "hf", "wf"):     # non-positive sizes
        refused(**{k: 0})
        refused(**{k: -3})
    for m in (GRID_EXPLICIT, 3, -1):
        refused(mode=m)
    refused(wsb=be.lib.warp_resampled_bwd_workspace(GRID_UNET, N, hf, wf, Ho, Wo) - 1)       # a workspace smaller than the query
    refused(mode=GRID_AFFINE, pred=th, wsb=be.lib.warp_resampled_bwd_workspace(GRID_AFFINE, N, hf, wf, Ho, Wo) - 1)
    refused(N=65536)                                             # beyond the launch's limit
    refused(mode=GRID_AFFINE, pred=th, Ho=1, Wo=1 << 23)         # a side the merge's tile search is not exact for
    refused(gpred=pred)
    (dhf, dwf), (dHo, dWo), (dHs, dWs), dC = DOWN                # a field being down-sampled: no backward
    refused(hf=dhf, wf=dwf, Ho=dHo, Wo=dWo, Hs=dHs, Ws=dWs, C=dC)
    refused(hf=Ho + 1)
    refused(wf=Wo + 1)
    be.sync()
    assert np.all(be.np(d_gpred) == 7.0)
    # and the good call goes through: a zero source has a zero gradient
    be.lib.warp_resampled_bwd(*good, be.stream)
    assert np.all(be.np(d_gpred) == 0.0)
