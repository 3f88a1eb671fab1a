"""Backend-agnostic test bodies of nemar_compose_pred (csrc/compose.hip: ONE prediction that samples where two would in sequence, with
an optional fused warp), driven through tests/backends.py (EmuBackend: host-emulated kernels, CPU tier; HipBackend: the gfx950 library,
`-m gpu` tier).  Every buffer is guard-banded there.

The truth is written out here in float64 (ref_compose) on top of what the project already has: register_cases.ref_grid (the grid the
second prediction gives every output pixel), score_cases._resize_at (the taps of a coarse field at a continuous coordinate) and the
`ident` extension of the linspace identity, as score_cases.ref_points does.  The same function with dtype float32 is the yardstick.
The rules (why each bound is what it is):
  float64     offsets converted to pixels (x W/2, x H/2): the kernel's max-abs error <= MARGIN x the yardstick's on the same case
              (register_cases.MARGIN: two fp32 evaluations of one formula in different rounding orders); where the yardstick is 0, exact.
  fused warp  out_img == nemar_warp_resampled_fwd(img, out_field, UNET, BILINEAR) of the same backend bit for bit (one statement of the
              arithmetic, resampled_grid.h, no contraction); out_field is the same bits with and without img.
  sequential  independent of ref_compose: bilinear sampling of a coordinate ramp is exact where all four taps are inside the image, so
              grid_sample(grid_sample(ramps, P1), P2) IS S1(S2(x)) there.  The yardstick is that two-warp procedure in torch-CPU fp32
              against float64; only pixels whose taps are inside (in float64, INSIDE_BAND px clear of the border) are compared, and the
              float64 reference alone must keep >= SEQ_SHARE of them.
  closed form AffineSTN.compose (theta1 o theta2) densified by the kernel (composed with the identity dtheta = 0) against ref_compose of
              the two operands, by the float64 rule."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from backends import both_poisons
from register_cases import BILINEAR, GRID_AFFINE, GRID_EXPLICIT, GRID_UNET, MARGIN, draw, ref_grid, run_fused, smooth_field
from score_cases import _resize_at

U, A = GRID_UNET, GRID_AFFINE
MODE_PAIRS = [(U, U), (U, A), (A, U), (A, A)]
#        (h1, w1),  (h2, w2),  (H, W)
RAGGED = ((32, 48), (16, 24), (35, 131))        # three ragged tile columns and rows, both fields coarser than the output
EQUAL = ((40, 56), (40, 56), (40, 56))          # no resampling
DOWN = ((64, 64), (64, 64), (24, 40))           # down-sampling: the un-staged global path
ONE_TEXEL = ((1, 1), (8, 12), (20, 36))         # a one-texel field
THIN = [((8, 12), (8, 12), (1, 77)), ((8, 12), (8, 12), (50, 1))]      # thin outputs: linspace of one element is -1
SIZES = [RAGGED, EQUAL, DOWN, ONE_TEXEL] + THIN
SEQ_HW = (67, 131)
SEQ_SHARE = 0.60
SEQ_AMP = 0.05
INSIDE_BAND = 1e-3         # px


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def draw_pair(seed, m1, m2, N, size, amp=0.15):
    """two predictions of register_cases.draw (different seeds)"""
    (h1, w1), (h2, w2), (H, W) = size
    _, first = draw(seed, m1, N, 1, h1, w1, 1, 1, amp)
    _, second = draw(seed + 50, m2, N, 1, h2, w2, 1, 1, amp)
    return first, second


# ---- the float64 truth, and (dtype float32) the yardstick -------------------------------------------------------------------------------
def _np_grid_at(x, y, pred, mode, Ho, Wo, dtype):
    """the continuous extension of a prediction's grid at pixel positions x, y [N,P] for output size (Ho, Wo): normalised (gx, gy) —
    what include/nemar_hip.h nemar_map_points evaluates before it unnormalises (score_cases.ref_points, without its last line)"""
    pred = np.asarray(pred).astype(dtype)
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
        return ident(x, Wo) + d[0], ident(y, Ho) + d[1]
    th = pred + np.array([1, 0, 0, 0, 1, 0], dtype=dtype)[None]
    xb, yb = (two * x + one) / dtype(Wo) - one, (two * y + one) / dtype(Ho) - one
    t = lambda i: th[:, i][:, None]
    return t(0) * xb + t(1) * yb + t(2), t(3) * xb + t(4) * yb + t(5)


def ref_compose(first, m1, second, m2, H, W, dtype=np.float64):
    """out_field [N,2,H,W] of include/nemar_hip.h nemar_compose_pred, written out: dtype float64 is the truth, float32 the yardstick"""
    tdtype = torch.float64 if dtype is np.float64 else torch.float32
    g2 = ref_grid(second, m2, H, W, tdtype).numpy()                       # [N,H,W,2]: where P2 sends every output pixel
    N = g2.shape[0]
    one, two = dtype(1), dtype(2)
    px = (((g2[..., 0] + one) * dtype(W) - one) / two).reshape(N, -1)      # the position in the intermediate image, which has the same size
    py = (((g2[..., 1] + one) * dtype(H) - one) / two).reshape(N, -1)
    gx1, gy1 = _np_grid_at(px, py, first, m1, H, W, dtype)
    lx, ly = torch.linspace(-1, 1, W, dtype=tdtype).numpy(), torch.linspace(-1, 1, H, dtype=tdtype).numpy()
    out = np.stack([gx1.reshape(N, H, W) - lx[None, None, :], gy1.reshape(N, H, W) - ly[None, :, None]], 1)
    assert out.dtype == dtype
    return out.astype(np.float64)


def in_pixels(field, H, W):
    return np.asarray(field, dtype=np.float64) * np.array([W / 2.0, H / 2.0])[None, :, None, None]


# ---- drivers ----------------------------------------------------------------------------------------------------------------------------------
def run_compose(be, d_first, m1, d_second, m2, size, N, d_img=None, C=0, d_field=None, d_out=None):
    """-> (field handle, warped handle or None); outputs pre-filled with NaN unless the caller brings its own"""
    (h1, w1), (h2, w2), (H, W) = size
    d_field = be.full((N, 2, H, W), np.nan) if d_field is None else d_field
    if d_img is not None and d_out is None:
        d_out = be.full((N, C, H, W), np.nan)
    be.lib.compose_pred(be.ptr(d_first), m1, h1, w1, be.ptr(d_second), m2, h2, w2, be.ptr(d_field), be.ptr(d_img), be.ptr(d_out), C, N, H, W,
                        be.stream)
    return d_field, d_out


def check_field(got, first, m1, second, m2, H, W, what):
    """the float64 rule; -> (kernel error, yardstick error) in pixels"""
    want = ref_compose(first, m1, second, m2, H, W)
    yard = np.abs(in_pixels(ref_compose(first, m1, second, m2, H, W, np.float32) - want, H, W)).max()
    assert np.all(np.isfinite(got)), what
    err = np.abs(in_pixels(got - want, H, W)).max()
    print("compose float64 %-64s kernel %.3e  numpy-fp32 %.3e  ratio %.2f" % (what, err, yard, err / yard if yard else (0.0 if err == 0 else float('inf'))))
    assert err <= MARGIN * yard, (what, err, yard)
    return err, yard


def _what(m1, m2, size, amp):
    return "%s%s %s,%s -> %s amp %g" % ("UA"[m1 == A], "UA"[m2 == A], *size, amp)


# ---- 1. against float64 ------------------------------------------------------------------------------------------------------------------------
def case_float64(be, size, m1, m2, N=2, seed=1, amp=0.15):
    first, second = draw_pair(seed, m1, m2, N, size, amp)
    H, W = size[2]
    d_field, _ = run_compose(be, be.dev(first), m1, be.dev(second), m2, size, N)
    got = be.np(d_field)
    if amp >= 1.0:         # p really leaves the image: the border texel and the linearly extended identity are exercised
        g2 = ref_grid(second, m2, H, W, torch.float64).numpy()
        ix, iy = ((g2[..., 0] + 1) * W - 1) / 2, ((g2[..., 1] + 1) * H - 1) / 2
        assert ((ix < -0.5) | (ix > W - 0.5) | (iy < -0.5) | (iy > H - 0.5)).mean() > 0.05, "p does not leave the image: the case would show nothing"
    return check_field(got, first, m1, second, m2, H, W, _what(m1, m2, size, amp))


# ---- 2. the fused warp is the library's warp ----------------------------------------------------------------------------------------------
def case_fused_warp(be, size, m1, m2, C, N=2, seed=2, amp=0.15):
    first, second = draw_pair(seed, m1, m2, N, size, amp)
    H, W = size[2]
    img = np.random.default_rng(seed).random((N, C, H, W)).astype(np.float32)
    d_first, d_second, d_img = be.dev(first), be.dev(second), be.dev(img)
    d_plain, none = run_compose(be, d_first, m1, d_second, m2, size, N)
    d_field, d_out = run_compose(be, d_first, m1, d_second, m2, size, N, d_img, C)
    assert none is None
    assert np.array_equal(be.raw(d_field), be.raw(d_plain)), "out_field differs with and without img: " + _what(m1, m2, size, amp)
    d_want = run_fused(be, d_img, d_field, GRID_UNET, BILINEAR, (N, C, H, W, H, W, H, W))
    assert np.all(np.isfinite(be.np(d_out)))
    assert np.array_equal(be.raw(d_out), be.raw(d_want)), "fused warp != warp_resampled_fwd of the composite: " + _what(m1, m2, size, amp)


# ---- 3. composition means what sequential warping means ---------------------------------------------------------------------------------------
def _two_warps(ramps, first, m1, second, m2, H, W, dtype):
    g1, g2 = ref_grid(first, m1, H, W, dtype), ref_grid(second, m2, H, W, dtype)
    gs = lambda im, g: F.grid_sample(im, g, mode='bilinear', padding_mode='zeros', align_corners=False)
    return gs(gs(torch.as_tensor(ramps, dtype=dtype), g1), g2).numpy().astype(np.float64)


def _inside(g, H, W):
    """[N,H,W] True where the float64 sampling position of grid g has its four taps inside the image, INSIDE_BAND px clear of the border"""
    ix, iy = ((g[..., 0] + 1) * W - 1) / 2, ((g[..., 1] + 1) * H - 1) / 2
    return (ix >= INSIDE_BAND) & (ix <= W - 1 - INSIDE_BAND) & (iy >= INSIDE_BAND) & (iy <= H - 1 - INSIDE_BAND), ix, iy


def sequential_mask(first, m1, second, m2, H, W):
    """pixels where, in float64, S2(x)'s four taps are inside the image and S1 at each of those taps is inside"""
    in1, _, _ = _inside(ref_grid(first, m1, H, W, torch.float64).numpy(), H, W)
    in2, ix, iy = _inside(ref_grid(second, m2, H, W, torch.float64).numpy(), H, W)
    x0, y0 = np.clip(np.floor(ix).astype(np.int64), 0, W - 2), np.clip(np.floor(iy).astype(np.int64), 0, H - 2)
    n = np.arange(in1.shape[0])[:, None, None]
    return in2 & in1[n, y0, x0] & in1[n, y0, x0 + 1] & in1[n, y0 + 1, x0] & in1[n, y0 + 1, x0 + 1]


def case_sequential(be, m1, m2, hw=SEQ_HW, N=2, seed=4, amp=SEQ_AMP):
    H, W = hw
    size = (hw, hw, hw)
    first, second = draw_pair(seed, m1, m2, N, size, amp)
    ramps = np.broadcast_to(np.stack([np.broadcast_to(np.arange(W, dtype=np.float64)[None, :], (H, W)),
                                      np.broadcast_to(np.arange(H, dtype=np.float64)[:, None], (H, W))])[None], (N, 2, H, W)).copy()
    want = _two_warps(ramps, first, m1, second, m2, H, W, torch.float64)
    keep = sequential_mask(first, m1, second, m2, H, W)
    what = "sequential " + _what(m1, m2, size, amp)
    assert keep.mean() >= SEQ_SHARE, (what, keep.mean())
    keep = np.broadcast_to(keep[:, None], want.shape)
    yard = np.abs(_two_warps(ramps, first, m1, second, m2, H, W, torch.float32) - want)[keep].max()
    d_field, _ = run_compose(be, be.dev(first), m1, be.dev(second), m2, size, N)
    g = be.np(d_field)                                                     # the kernel's fp32 offsets; the rest in float64
    gx = np.linspace(-1, 1, W)[None, None, :] + g[:, 0]
    gy = np.linspace(-1, 1, H)[None, :, None] + g[:, 1]
    got = np.stack([((gx + 1) * W - 1) / 2, ((gy + 1) * H - 1) / 2], 1)
    err = np.abs(got - want)[keep].max()
    print("compose %-68s kept %.3f  kernel %.3e  torch-fp32 two warps %.3e  ratio %.2f" % (what, keep.mean(), err, yard, err / yard if yard else float('inf')))
    assert err <= MARGIN * yard, (what, err, yard)


# ---- 4. the affine closed form ----------------------------------------------------------------------------------------------------------------
def case_affine_closed_form(be, size, N=2, seed=5, amp=0.15):
    from nemar_amd.models.stn.affine_stn import AffineSTN
    first, second = draw_pair(seed, A, A, N, size, amp)
    H, W = size[2]
    both = AffineSTN.compose(None, torch.from_numpy(first), torch.from_numpy(second)).numpy()
    assert both.shape == (N, 6) and both.dtype == np.float32
    d_field, _ = run_compose(be, be.dev(both), A, be.zeros(N, 6), A, size, N)
    check_field(be.np(d_field), first, A, second, A, H, W, "closed form " + _what(A, A, size, amp))


# ---- 5. repeatable, overwritten, unaligned, refusals ----------------------------------------------------------------------------------------
def _off_by_4_bytes(be, a):
    """`a` in a buffer that starts 4 bytes past a 16-byte boundary (a view of a guarded block one element longer)"""
    d_buf = be.dev(np.concatenate([[0.0], np.asarray(a, dtype=np.float32).ravel()]))
    return be.sub(d_buf, 1, d_buf.shape[0])


@both_poisons
def case_repeatable_unaligned(be, size, m1, m2, N=2, C=3, seed=3):
    first, second = draw_pair(seed, m1, m2, N, size)
    H, W = size[2]
    img = np.random.default_rng(seed).random((N, C, H, W)).astype(np.float32)
    d_first, d_second, d_img = be.dev(first), be.dev(second), be.dev(img)
    d_f, d_o = run_compose(be, d_first, m1, d_second, m2, size, N, d_img, C)
    a_f, a_o = be.raw(d_f), be.raw(d_o)
    d_f, d_o = run_compose(be, d_first, m1, d_second, m2, size, N, d_img, C, d_field=be.full((N, 2, H, W), 7.0), d_out=be.full((N, C, H, W), -3.0))
    assert np.array_equal(be.raw(d_f), a_f) and np.array_equal(be.raw(d_o), a_o), "two calls (other garbage in the outputs), different bits"
    assert np.all(np.isfinite(be.np(d_f))) and np.all(np.isfinite(be.np(d_o))), "an output element was not written"
    d_f, d_o = _off_by_4_bytes(be, np.full(N * 2 * H * W, np.nan)), _off_by_4_bytes(be, np.full(N * C * H * W, np.nan))
    run_compose(be, _off_by_4_bytes(be, first), m1, _off_by_4_bytes(be, second), m2, size, N, _off_by_4_bytes(be, img), C, d_field=d_f, d_out=d_o)
    assert np.array_equal(be.raw(d_f), a_f) and np.array_equal(be.raw(d_o), a_o), "views 4 bytes off the 16-byte grid: different bits"


def case_refusals(be):
    """NEMAR_EINVAL (-1), a message, and nothing launched: the outputs keep their fill"""
    from nemar_amd._lib import NemarHipError
    N, C, h1, w1, h2, w2, H, W = 2, 3, 6, 8, 5, 7, 12, 16
    d_first, d_second, d_th = be.zeros(N, 2, h1, w1), be.zeros(N, 2, h2, w2), be.zeros(N, 6)
    d_img, d_field, d_out = be.zeros(N, C, H, W), be.full((N, 2, H, W), 7.0), be.full((N, C, H, W), 7.0)
    off2 = lambda p: ctypes.c_void_p(p.value + 2)
    names = ("first", "m1", "h1", "w1", "second", "m2", "h2", "w2", "field", "img", "out", "C", "N", "H", "W")
    good = [be.ptr(d_first), U, h1, w1, be.ptr(d_second), U, h2, w2, be.ptr(d_field), be.ptr(d_img), be.ptr(d_out), C, N, H, W]

    def refused(**change):
        args = [change.get(k, v) for k, v in zip(names, good)]
        with pytest.raises(NemarHipError, match=r"failed \(-1\): compose_pred: \S"):
            be.lib.compose_pred(*args, be.stream)

    for m in (GRID_EXPLICIT, 3, -1):                              # an explicit grid has one resolution; 3 and -1 are no modes at all
        refused(m1=m)
        refused(m2=m)
    for k in ("first", "second", "field"):                        # required pointers: null, not even 4-byte aligned
        refused(**{k: None})
        refused(**{k: off2(good[names.index(k)])})
    for k in ("img", "out"):
        refused(**{k: None})                                      # exactly one of img / out_img
        refused(**{k: off2(good[names.index(k)])})
    for c in (0, -2):                                             # C < 1 with img
        refused(C=c)
    for k in ("N", "H", "W"):                                     # non-positive sizes
        refused(**{k: 0})
        refused(**{k: -3})
    for k in ("h1", "w1", "h2", "w2"):                            # a UNet side without a field
        refused(**{k: 0})
        refused(**{k: -1})
    refused(N=65536)
    refused(H=1 << 16, W=1 << 15)                                 # H * W = 2^31
    refused(field=good[0])                                        # out_field is an operand: the kernel gathers from them
    refused(field=good[4])
    be.sync()
    assert np.all(be.np(d_field) == 7.0) and np.all(be.np(d_out) == 7.0)
    # h, w of an affine side are ignored; C is ignored without img
    be.lib.compose_pred(be.ptr(d_th), A, 0, -1, be.ptr(d_th), A, 0, 0, be.ptr(d_field), None, None, 0, N, H, W, be.stream)
    assert np.all(np.abs(be.np(d_field)) < 0.2) and np.all(be.np(d_out) == 7.0)        # identity o identity, minus the linspace zoom: 1/H, 1/W at most
