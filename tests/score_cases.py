"""Backend-agnostic test bodies of nemar_label_overlap and nemar_map_points (csrc/score.hip: a registration scored by segmentation
overlap and by annotated-point distances), driven through tests/backends.py (EmuBackend: host-emulated kernels, CPU tier; HipBackend:
the gfx950 library, `-m gpu` tier).  Every buffer is guard-banded there; `counts` is an int32 buffer read back bit for bit.

The grid has ONE truth, tests/register_cases.py (draw, smooth_field, ref_grid, ref_warp, tie_mask); what is new is written out here in
float64: the class rule and the counting (count_np), and the continuous extension of the grid at a point (ref_points).
The rules (why each bound is what it is):
  exact     counts == numpy counting over nemar_warp_resampled_fwd(NEAREST, C = 1) of the same backend, integer for integer, no pixel
            excluded: the fused kernel states the same arithmetic (resampled_grid.h), and integer addition has no order.
  float64   against ref_warp(NEAREST) in float64: a pixel can change class only where the float64 sampling position lies within
            TIE_BAND px of a rounding tie, and one pixel moves any one count by at most one: per sample, every |count difference| <= the
            number of that sample's pixels in tie_mask; the float64 reference alone must put <= TIE_SHARE of a case's pixels there.
            The predictions are register_cases.case_nearest's own (same draw, same seed), whose tests meet that cap.
  points    against float64: the yardstick of a case is the max-abs error of numpy's OWN float32 evaluation of the same formula; the
            kernel's must be <= MARGIN x that (register_cases.MARGIN: two fp32 evaluations of one formula in different rounding orders)."""
import ctypes

import numpy as np
import pytest
import torch

from backends import both_poisons
from register_cases import (ALL_SIZES, GRID_AFFINE, GRID_EXPLICIT, GRID_UNET, MARGIN, NEAREST, TIE_SHARE, UPSAMPLING, EQUAL, DOWN, draw,
                            ref_grid, ref_warp, run_fused, smooth_field, tie_mask)

GARBAGE = 0x5a5a5a5a
#          (hf, wf), (Ho, Wo), (Hs, Ws) or None, C of register_cases' draw (the label map is channel 0)
THIN = [((8, 12), (1, 77), (9, 13), 2), ((8, 12), (50, 1), (9, 13), 2)]
ONE_TEXEL_FIELD = ((1, 1), (20, 36), None, 1)
LEAVES_SOURCE = ((16, 24), (67, 45), (30, 41), 3)          # with amp = 1.5: the field leaves the source, class 0 grows
CONTENT_SIZE = UPSAMPLING[0]                               # 131 x 203: odd sizes, three tile columns, nine tile rows
KINDS = ("random", "blocky", "single")
JUNK = (-1.0, None, None, 2.5, np.nan, np.inf)             # None: K and K + 7, filled in per case


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _shape(size, N):
    (hf, wf), (Ho, Wo), src, C = size
    Hs, Ws = src or (Ho, Wo)
    return (N, C, Hs, Ws, hf, wf, Ho, Wo)


def label_map(kind, seed, N, H, W, K, junk=False):
    """[N,H,W] float32 ids in [0, K): per-pixel random (no two neighbouring lanes agree by design), blocky (random ids on an 8 x 8-pixel
    lattice: piecewise constant, the wave-aggregated path), single (one class only: every lane on one counter); ids 0 and K-1 are present
    in the first two kinds.  junk: 5 % of the pixels hold values that belong to no class"""
    rng = np.random.default_rng(seed)
    if kind == "random":
        a = rng.integers(0, K, (N, H, W))
    elif kind == "blocky":
        a = rng.integers(0, K, (N, (H + 7) // 8, (W + 7) // 8)).repeat(8, 1).repeat(8, 2)[:, :H, :W]
    else:
        a = np.full((N, H, W), (K - 1) // 2)
    a = np.ascontiguousarray(a).astype(np.float32)
    if kind != "single":
        a[:, 0, 0], a[:, -1, -1] = 0, K - 1
    if junk:
        bad = np.array([K if v is None and i == 1 else K + 7 if v is None else v for i, v in enumerate(JUNK)], dtype=np.float32)
        hit = rng.random((N, H, W)) < 0.05
        a[hit] = bad[rng.integers(0, len(bad), int(hit.sum()))]
    return a


# ---- the float64 truth that is new here ---------------------------------------------------------------------------------------------------
def class_np(v, K):
    """class of every value: k iff v == k for an integer 0 <= k < K, else -1 (negative, >= K, fractional, NaN, Inf)"""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        ok = (v >= 0) & (v < K) & (v == np.floor(v))
    return np.where(ok, np.where(ok, v, 0).astype(np.int64), -1)


def count_np(m, f, K):
    """[N,K,3] int64: per sample and class #{m == k and f == k}, #{m == k}, #{f == k} over maps m, f [N,Ho,Wo]"""
    km, kf = class_np(m, K), class_np(f, K)
    N = km.shape[0]
    out = np.zeros((N, K, 3), dtype=np.int64)
    for n in range(N):
        a, b = km[n].ravel(), kf[n].ravel()
        out[n, :, 0] = np.bincount(a[(a == b) & (a >= 0)], minlength=K)
        out[n, :, 1] = np.bincount(a[a >= 0], minlength=K)
        out[n, :, 2] = np.bincount(b[b >= 0], minlength=K)
    return out


def _resize_at(f, p, n_out, dtype):
    """taps of the align_corners=False resize of an axis of n_in = f texels at continuous output coordinates p: i0, i1, l0, l1"""
    n_in = f
    s = (p + dtype(0.5)) * (dtype(n_in) / dtype(n_out)) - dtype(0.5)
    s = np.clip(s, dtype(0), dtype(n_in - 1))
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = s - i0.astype(dtype)
    return i0, i1, dtype(1) - l1, l1


def ref_points(pts, pred, mode, Hs, Ws, Ho, Wo, dtype=np.float64):
    """S(p) [N,P,2] of include/nemar_hip.h nemar_map_points, written out: dtype float64 is the truth, float32 the yardstick"""
    p = np.asarray(pts).astype(dtype)
    pred = np.asarray(pred).astype(dtype)
    x, y = p[..., 0], p[..., 1]
    one, two = dtype(1), dtype(2)
    if mode == GRID_UNET:
        N, _, hf, wf = pred.shape
        y0, y1, ly0, ly1 = _resize_at(hf, y, Ho, dtype)
        x0, x1, lx0, lx1 = _resize_at(wf, x, Wo, dtype)
        n = np.arange(N)[:, None]
        d = []
        for c in (0, 1):
            f = pred[:, c]
            top = f[n, y0, x0] * lx0 + f[n, y0, x1] * lx1
            bot = f[n, y1, x0] * lx0 + f[n, y1, x1] * lx1
            d.append(top * ly0 + bot * ly1)
        ident = lambda q, size: (-one + two * q / dtype(size - 1)) if size > 1 else np.full_like(q, -one)
        gx, gy = ident(x, Wo) + d[0], ident(y, Ho) + d[1]
    else:
        th = pred + np.array([1, 0, 0, 0, 1, 0], dtype=dtype)[None]
        xb, yb = (two * x + one) / dtype(Wo) - one, (two * y + one) / dtype(Ho) - one
        t = lambda i: th[:, i][:, None]
        gx, gy = t(0) * xb + t(1) * yb + t(2), t(3) * xb + t(4) * yb + t(5)
    return np.stack([((gx + one) * dtype(Ws) - one) / two, ((gy + one) * dtype(Hs) - one) / two], axis=-1).astype(np.float64)


# ---- drivers ----------------------------------------------------------------------------------------------------------------------------------
def counts_of(be, d_counts, N, K):
    return be.raw(d_counts).view(np.uint32).reshape(N, K, 3).astype(np.int64)


def run_overlap(be, d_lm, d_lf, d_pred, mode, K, shape, d_counts=None):
    """-> the counts handle, pre-filled with garbage unless the caller brings its own"""
    N, _, Hs, Ws, hf, wf, Ho, Wo = shape
    d_counts = be.dev_i32(np.full((N, K, 3), GARBAGE, dtype=np.int32)) if d_counts is None else d_counts
    be.lib.label_overlap(be.ptr(d_lm), be.ptr(d_lf), be.ptr(d_pred), mode, be.ptr(d_counts), N, K, Hs, Ws, hf, wf, Ho, Wo, be.stream)
    return d_counts


def run_points(be, d_pts, d_pred, mode, shape, P, d_out=None):
    N, _, Hs, Ws, hf, wf, Ho, Wo = shape
    d_out = be.full((N, P, 2), 7.0) if d_out is None else d_out
    be.lib.map_points(be.ptr(d_pts), be.ptr(d_pred), mode, be.ptr(d_out), N, P, Hs, Ws, hf, wf, Ho, Wo, be.stream)
    return d_out


def library_warp(be, d_lm, d_pred, mode, shape):
    """the label map as nemar_warp_resampled_fwd(NEAREST, C = 1) of the same backend writes it: [N,Ho,Wo]"""
    N, _, Hs, Ws, hf, wf, Ho, Wo = shape
    return be.np(run_fused(be, d_lm, d_pred, mode, NEAREST, (N, 1, Hs, Ws, hf, wf, Ho, Wo)))[:, 0]


def _inputs(size, mode, N, seed, amp, K=8, moving="random", fixed="blocky", junk=False):
    """the prediction of register_cases.draw (same seed, same C: the same numbers as that file's cases) and two label maps"""
    shape = _shape(size, N)
    N, C, Hs, Ws, hf, wf, Ho, Wo = shape
    img, pred = draw(seed, mode, N, C, hf, wf, Hs, Ws, amp, labels=True)
    lm = img[:, 0] if (K == 8 and moving == "random" and not junk) else label_map(moving, seed + 100, N, Hs, Ws, K, junk)
    lf = label_map(fixed, seed + 200, N, Ho, Wo, K, junk)
    return shape, np.ascontiguousarray(lm), lf, pred


# ---- 1. exact against the library's own warp ---------------------------------------------------------------------------------------------------
def check_exact(be, shape, lm, lf, pred, mode, K, what):
    N, _, Hs, Ws, hf, wf, Ho, Wo = shape
    d_lm, d_pred = be.dev(lm[:, None]), be.dev(pred)
    got = counts_of(be, run_overlap(be, d_lm, be.dev(lf), d_pred, mode, K, shape), N, K)
    m = library_warp(be, d_lm, d_pred, mode, shape)
    want = count_np(m, lf, K)
    assert np.array_equal(got, want), (what, int(np.abs(got - want).max()))
    ignored = (class_np(m, K) < 0).reshape(N, -1).sum(1)
    assert np.array_equal(got[:, :, 1].sum(1) + ignored, np.full(N, Ho * Wo)), what       # every pixel is in one class or in none
    return got, m


def case_exact(be, size, mode=GRID_UNET, N=2, seed=0, amp=0.15):
    shape, lm, lf, pred = _inputs(size, mode, N, seed, amp)
    got, m = check_exact(be, shape, lm, lf, pred, mode, 8, "exact %s mode %d amp %g" % (size, mode, amp))
    assert got[:, :, 0].sum() > 0, "no pixel agrees: the case would show nothing about `inter`"
    if amp >= 1.0:             # the field really leaves the source: zero padding lands in class 0
        Hs, Ws = shape[2:4]
        g = ref_grid(pred, mode, shape[6], shape[7], torch.float64).numpy()
        ix, iy = ((g[..., 0] + 1) * Ws - 1) / 2, ((g[..., 1] + 1) * Hs - 1) / 2
        outside = (ix < -0.6) | (ix > Ws - 0.4) | (iy < -0.6) | (iy > Hs - 0.4)        # (0.1 px clear of the rounding tie at the border)
        assert outside.mean() > 0.05, "the field does not leave the source: the case would show nothing"
        assert np.all(got[:, 0, 1] >= outside.reshape(N, -1).sum(1))


# ---- 2. against float64 ------------------------------------------------------------------------------------------------------------------------
def case_float64(be, size, mode=GRID_UNET, N=2, seed=2, amp=0.15):
    shape, lm, lf, pred = _inputs(size, mode, N, seed, amp)
    N, _, Hs, Ws, hf, wf, Ho, Wo = shape
    tie = tie_mask(pred, mode, Ho, Wo, Hs, Ws)
    what = "mode %d field %s -> %s source %s" % (mode, (hf, wf), (Ho, Wo), (Hs, Ws))
    got = counts_of(be, run_overlap(be, be.dev(lm[:, None]), be.dev(lf), be.dev(pred), mode, 8, shape), N, 8)
    want = count_np(ref_warp(lm[:, None], pred, mode, Ho, Wo, NEAREST)[:, 0], lf, 8)
    diff, allowed = np.abs(got - want).reshape(N, -1).max(1), tie.reshape(N, -1).sum(1)
    print("overlap float64   %-46s excluded %.4f  count difference %s of %s allowed" % (what, tie.mean(), diff.tolist(), allowed.tolist()))
    assert tie.mean() <= TIE_SHARE, (what, tie.mean())
    assert np.all(diff <= allowed), (what, diff, allowed)
    assert np.array_equal(got[:, :, 2], want[:, :, 2]), what            # the fixed map's histogram has no rounding in it


# ---- 3. label content ----------------------------------------------------------------------------------------------------------------------------
@both_poisons
def case_content(be, kind, K, mode=GRID_UNET, size=CONTENT_SIZE, N=2, seed=7, junk=False):
    """moving and fixed of the same kind (different seeds); junk: values of no class on either side, ignored exactly as specified"""
    shape, lm, lf, pred = _inputs(size, mode, N, seed, 0.15, K=K, moving=kind, fixed=kind, junk=junk)
    got, m = check_exact(be, shape, lm, lf, pred, mode, K, "content %s K %d junk %s mode %d" % (kind, K, junk, mode))
    if kind != "single" and not junk:
        assert np.all(got[:, 0, 2] > 0) and np.all(got[:, K - 1, 2] > 0)          # ids 0 and K - 1 are there
    if kind == "single" and not junk:
        k = (K - 1) // 2
        assert got[:, :, 2].sum() == got[:, k, 2].sum() == N * shape[6] * shape[7]
    if junk:
        assert np.all((class_np(lf, K) < 0).reshape(N, -1).sum(1) > 0) and np.all(got[:, :, 2].sum(1) < shape[6] * shape[7])


# ---- 4. identity -----------------------------------------------------------------------------------------------------------------------------------
def case_identity(be, hw=(67, 45), K=5, N=2, seed=8):
    """dtheta = 0, equal sizes, the same map on both sides: inter == moving == fixed == the plain histogram"""
    H, W = hw
    lab = label_map("blocky", seed, N, H, W, K)
    d_lab = be.dev(lab)
    got = counts_of(be, run_overlap(be, d_lab, d_lab, be.zeros(N, 6), GRID_AFFINE, K, (N, 1, H, W, 0, 0, H, W)), N, K)
    hist = np.stack([np.bincount(lab[n].astype(np.int64).ravel(), minlength=K) for n in range(N)])
    for c in range(3):
        assert np.array_equal(got[:, :, c], hist), c


# ---- 5. repeatable and unaligned -------------------------------------------------------------------------------------------------------------
def _off_by_4_bytes(be, a, dev):
    """`a` in a buffer that starts 4 bytes past a 16-byte boundary (a view of a guarded block one element longer)"""
    a = np.asarray(a)
    d_buf = dev(np.concatenate([np.zeros(1, dtype=a.dtype), a.ravel()]))
    return be.sub(d_buf, 1, d_buf.shape[0])


@both_poisons
def case_repeatable_unaligned(be, size, mode=GRID_UNET, N=1, seed=3):
    shape, lm, lf, pred = _inputs(size, mode, N, seed, 0.15)
    N, _, Hs, Ws, hf, wf, Ho, Wo = shape
    d_lm, d_lf, d_pred = be.dev(lm), be.dev(lf), be.dev(pred)
    a = be.raw(run_overlap(be, d_lm, d_lf, d_pred, mode, 8, shape))
    b = be.raw(run_overlap(be, d_lm, d_lf, d_pred, mode, 8, shape, d_counts=be.dev_i32(np.full((N, 8, 3), -1, dtype=np.int32))))     # other garbage
    assert np.array_equal(a, b), "two calls, different bits"
    d_counts = _off_by_4_bytes(be, np.full(N * 8 * 3, GARBAGE, dtype=np.int32), be.dev_i32)
    run_overlap(be, _off_by_4_bytes(be, lm, be.dev), _off_by_4_bytes(be, lf, be.dev), _off_by_4_bytes(be, pred, be.dev), mode, 8, shape, d_counts=d_counts)
    assert np.array_equal(be.raw(d_counts), a), "views 4 bytes off the 16-byte grid: different counts"
    assert np.array_equal(a.view(np.uint32).reshape(N, 8, 3)[:, :, 2].astype(np.int64), count_np(lf, lf, 8)[:, :, 2])


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------
def case_refusals(be):
    """NEMAR_EINVAL (-1), a message, and nothing launched: `counts` and `out` keep their fill"""
    from nemar_amd._lib import NemarHipError
    N, K, P, Hs, Ws, hf, wf, Ho, Wo = 2, 4, 5, 12, 16, 6, 8, 10, 14
    d_lm, d_lf, d_pred, d_th = be.zeros(N, Hs, Ws), be.zeros(N, Ho, Wo), be.zeros(N, 2, hf, wf), be.zeros(N, 6)
    d_counts = be.dev_i32(np.full((N, 1025, 3), GARBAGE, dtype=np.int32))       # (room for the K = 1025 call, should it ever launch)
    d_pts, d_out = be.zeros(N, P, 2), be.full((N, P, 2), 7.0)
    off2 = lambda p: ctypes.c_void_p(p.value + 2)

    def refuser(fn, what, names, good):
        def refused(**change):
            args = [change.get(k, v) for k, v in zip(names, good)]
            with pytest.raises(NemarHipError, match=r"failed \(-1\): %s: \S" % what):
                fn(*args, be.stream)
        return refused

    names = ("lm", "lf", "pred", "mode", "counts", "N", "K", "Hs", "Ws", "hf", "wf", "Ho", "Wo")
    good = [be.ptr(d_lm), be.ptr(d_lf), be.ptr(d_pred), GRID_UNET, be.ptr(d_counts), N, K, Hs, Ws, hf, wf, Ho, Wo]
    refused = refuser(be.lib.label_overlap, "label_overlap", names, good)
    for k in ("lm", "lf", "pred", "counts"):
        refused(**{k: None})                                      # null pointers
        refused(**{k: off2(good[names.index(k)])})                # not even 4-byte aligned
    for k in ("N", "Hs", "Ws", "Ho", "Wo"):                       # non-positive sizes
        refused(**{k: 0})
        refused(**{k: -3})
    for k in (0, -1, 1025):
        refused(K=k)
    for m in (GRID_EXPLICIT, 3, -1):                              # an explicit grid has one resolution; 3 and -1 are no modes at all
        refused(mode=m)
    for k in ("hf", "wf"):                                        # UNET without a field
        refused(**{k: 0})
        refused(**{k: -1})
    refused(Ho=1 << 16, Wo=1 << 15)                               # Ho * Wo = 2^31

    names = ("pts", "pred", "mode", "out", "N", "P", "Hs", "Ws", "hf", "wf", "Ho", "Wo")
    good = [be.ptr(d_pts), be.ptr(d_pred), GRID_UNET, be.ptr(d_out), N, P, Hs, Ws, hf, wf, Ho, Wo]
    refused = refuser(be.lib.map_points, "map_points", names, good)
    for k in ("pts", "pred", "out"):
        refused(**{k: None})
        refused(**{k: off2(good[names.index(k)])})
    for k in ("N", "P", "Hs", "Ws", "Ho", "Wo"):
        refused(**{k: 0})
        refused(**{k: -3})
    for m in (GRID_EXPLICIT, 3, -1):
        refused(mode=m)
    for k in ("hf", "wf"):
        refused(**{k: 0})
    be.sync()
    assert np.all(be.raw(d_counts).view(np.uint32) == GARBAGE) and np.all(be.np(d_out) == 7.0)
    # AFFINE ignores hf, wf; K = 1024 is served
    be.lib.label_overlap(be.ptr(d_lm), be.ptr(d_lf), be.ptr(d_th), GRID_AFFINE, be.ptr(d_counts), N, 1024, Hs, Ws, 0, 0, Ho, Wo, be.stream)
    got = be.raw(d_counts).view(np.uint32)[:N * 1024 * 3].reshape(N, 1024, 3)
    assert np.all(got[:, 0] == Ho * Wo) and np.all(got[:, 1:] == 0)           # two maps of zeros: everything in class 0
    be.lib.map_points(be.ptr(d_pts), be.ptr(d_th), GRID_AFFINE, be.ptr(d_out), N, P, Hs, Ws, 0, 0, Ho, Wo, be.stream)
    assert np.all(np.isfinite(be.np(d_out)))


# ---- 7. points: agreement with the grid -----------------------------------------------------------------------------------------------------
def check_points(got, pts, pred, mode, shape, what, want=None):
    N, _, Hs, Ws, hf, wf, Ho, Wo = shape
    want = ref_points(pts, pred, mode, Hs, Ws, Ho, Wo) if want is None else want
    yard = np.abs(ref_points(pts, pred, mode, Hs, Ws, Ho, Wo, np.float32) - want).max()
    err = np.abs(got - want).max()
    print("map_points %-52s kernel %.3e  numpy-fp32 %.3e  ratio %.2f" % (what, err, yard, err / yard if yard else float('inf')))
    assert np.all(np.isfinite(got)), what
    assert err <= MARGIN * yard, (what, err, yard)


def case_points(be, size, mode=GRID_UNET, N=2, seed=9, P=1500):
    shape = _shape(size, N)
    N, C, Hs, Ws, hf, wf, Ho, Wo = shape
    _, pred = draw(seed, mode, N, C, hf, wf, Hs, Ws)
    d_pred = be.dev(pred)
    rng = np.random.default_rng(seed)
    what = "mode %d field %s -> %s source %s " % (mode, (hf, wf), (Ho, Wo), (Hs, Ws))
    # integer points (the four corners among them): the grid of the warp itself, register_cases.ref_grid unnormalised in float64
    iy, ix = rng.integers(0, Ho, (N, P)), rng.integers(0, Wo, (N, P))
    iy[:, :4], ix[:, :4] = [0, 0, Ho - 1, Ho - 1], [0, Wo - 1, 0, Wo - 1]
    pts = np.stack([ix, iy], -1).astype(np.float32)
    g = ref_grid(pred, mode, Ho, Wo, torch.float64).numpy()[np.arange(N)[:, None], iy, ix]
    want = np.stack([((g[..., 0] + 1) * Ws - 1) / 2, ((g[..., 1] + 1) * Hs - 1) / 2], -1)
    assert np.abs(want - ref_points(pts, pred, mode, Hs, Ws, Ho, Wo)).max() < 1e-9          # the formula written out here IS that grid
    check_points(be.np(run_points(be, be.dev(pts), d_pred, mode, shape, P)), pts, pred, mode, shape, what + "integer", want=want)
    # fractional points inside the image; then points on and beyond the border (the clamped taps)
    frac = (rng.random((N, P, 2)) * [Wo, Ho] - 0.5).astype(np.float32)
    check_points(be.np(run_points(be, be.dev(frac), d_pred, mode, shape, P)), frac, pred, mode, shape, what + "fractional")
    far = ((rng.random((N, P, 2)) * 1.6 - 0.3) * [Wo, Ho]).astype(np.float32)
    far[:, :6] = [[-0.5, -0.5], [Wo - 0.5, Ho - 0.5], [0, Ho - 1], [Wo - 1, 0], [-3.25, Ho + 2.5], [Wo + 4.75, -1.5]]
    check_points(be.np(run_points(be, be.dev(far), d_pred, mode, shape, P)), far, pred, mode, shape, what + "border and beyond")


# ---- 8. points: edges ----------------------------------------------------------------------------------------------------------------------------
def case_points_edges(be, mode=GRID_UNET, size=UPSAMPLING[4], N=2, seed=10):
    """NaN rows (a missing annotation: either coordinate) come back as NaN pairs and disturb nobody; P = 1 and P = 130 (more than two waves)"""
    shape = _shape(size, N)
    N, C, Hs, Ws, hf, wf, Ho, Wo = shape
    _, pred = draw(seed, mode, N, C, hf, wf, Hs, Ws)
    d_pred = be.dev(pred)
    rng = np.random.default_rng(seed)
    for P in (1, 130):
        pts = (rng.random((N, P, 2)) * [Wo, Ho] - 0.5).astype(np.float32)
        clean = be.np(run_points(be, be.dev(pts), d_pred, mode, shape, P))
        check_points(clean, pts, pred, mode, shape, "edges mode %d P %d" % (mode, P))
        holes = pts.copy()
        rows = [0] if P == 1 else [0, 63, 64, 65, 129]
        for j, r in enumerate(rows):
            holes[0, r, j % 2] = np.nan                     # x of one row, y of the next
        holes[N - 1, rows[-1]] = np.nan                     # both
        got = be.np(run_points(be, be.dev(holes), d_pred, mode, shape, P))
        missing = np.isnan(holes).any(-1)
        assert np.all(np.isnan(got[missing])), "a missing annotation must give a NaN pair"
        assert np.array_equal(got[~missing], clean[~missing]), "a NaN row disturbed its neighbours"
