"""Backend-agnostic test bodies of nemar_compose_pred_bwd (csrc/compose.hip: the gradient of the composed prediction towards its two
operands), driven through tests/backends.py (EmuBackend: host-emulated kernels, CPU tier; HipBackend: the gfx950 library, `-m gpu`).
Every buffer is guard-banded there.

Inputs are compose_cases.draw_pair's (N = 2, amp 0.15), UNet operands AT the composition size.  gout is seeded normal noise, set to ZERO
at every output pixel whose float64 position p lies within KINK_BAND px of an integer in x or y: the slope towards `second` jumps where p
crosses an integer (the cell changes; the clamp edges 0 and size - 1 are integers too) and an fp32 evaluation may sit on the other side.
Truth and kernel get the same zeroed gout; the float64 reference alone must mark <= KINK_SHARE of a case's pixels (draw_case asserts).
The THIN sizes sit on the clamp by construction (one texel along an axis: p is -0.5 + half the offset there).  Where a thin case cannot
meet the cap — with these seeds the (1, 77) size under an AFFINE second, (UNET, AFFINE) and (AFFINE, AFFINE): p along the one-texel
axis is half of theta's own coordinate there and runs THROUGH 0, 2.6 % of the pixels within the band — gout is left unmasked and gfirst
alone is checked (gfirst is continuous in p: a weight is 0 where its texel changes); draw_case says which.

The float64 truth is compose_cases.ref_compose restated in torch with autograd (t_compose); the same code in float32 is the yardstick.
  float64   per element |kernel - truth| <= MARGIN x yardstick + CHAIN x 2^-24 x S + Q.  yardstick = the max-abs error of the float32
            torch code over the tensor; S = the float64 sum of the absolute contributions to the element; CHAIN = the fp32 operations a
            contribution passes through in the kernel as built (the error of p itself is the yardstick's part):
              gfirst UNET      5: 1 - l1, the weight product, x gout, int64 -> float, accumulate                    (+ Q, below)
              gfirst AFFINE    4 (the base coordinate (2p + 1)/n - 1 of p) + 1 (x gout) + 4 (the lane's pixels) + 6 (wave tree) + 4 (waves)
                               + merge: ceil(tiles / 256) + 6 + 4, + 1 (x k) + 1 (accumulate)
              gsecond UNET     first UNET 9: 1 - l1, texel difference, x l, the sum of the two rows, + the identity's slope, x gout,
                               the sum over the channels, x W/2, accumulate;  first AFFINE 7: dtheta + 1, x gout, the sum, 2 / W, x it,
                               x W/2, accumulate
              gsecond AFFINE   the same without accumulate, + 3 (the pixel's base coordinate) + 1 (x it) + 4 + 6 + 4 + merge as above + 2
            Q, gfirst UNET only: (the float64 reference's count of contributions to the texel) x 2^(e - fix - 1), the kernel's rule:
            2^(e-1) <= max |gout| < 2^e, fix = min(40, 62 - ceil(log2(H W))) — each contribution is rounded to a multiple of 2^(e - fix).
            gfirst alone, gsecond alone and both: the bits of one do not depend on the other.
  adjoint   the forward is exactly linear in `first`: <gout, fwd(first + s d) - fwd(first)> / s in float64 on the kernel's own FORWARD
            outputs against <gfirst, d>, d one texel or one dtheta entry.  The bound is the forward's fp32 rounding (case_adjoint).
  anchor    second = a zero UNET field: the float64 rule, and two calls give the same bits.
  repeat    two calls, the same bits; accumulate = 1 onto a pre-fill equals pre-fill + result within one rounding; accumulate = 0
            overwrites poison everywhere; every pointer 4 bytes off the 16-byte grid (the workspace 8) gives the aligned call's bits.
  the zeroed part of the workspace is all-zero after every call (run_bwd checks it)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from compose_cases import A, MODE_PAIRS, U, draw_pair
from register_cases import GRID_EXPLICIT, MARGIN, ref_grid
from score_cases import _resize_at

KINK_BAND = 1e-3           # px
KINK_SHARE = 0.01
EPS24 = 2.0 ** -24
HWS = [(40, 56), (35, 131)]
TILE_EDGES = [(15, 70), (16, 64), (17, 65), (33, 129)]
THIN = [(1, 77), (50, 1)]
ALL_HW = HWS + TILE_EDGES + THIN
WANTS = [("first",), ("second",), ("first", "second")]
pair_id = lambda p: "UA"[p[0] == A] + "UA"[p[1] == A]


def _size(hw):
    return (hw, hw, hw)


# ---- torch on the CPU, differentiable: the float64 truth and (dtype float32) the yardstick -----------------------------------------------
def _t_grid(p, mode, H, W):
    dtype = p.dtype
    if mode == U:
        x, y = torch.linspace(-1, 1, W, dtype=dtype), torch.linspace(-1, 1, H, dtype=dtype)
        return x[None, None, :] + p[:, 0], y[None, :, None] + p[:, 1]
    th = p + torch.tensor([1, 0, 0, 0, 1, 0], dtype=dtype)[None]
    xb = ((2 * torch.arange(W, dtype=dtype) + 1) / W - 1)[None, None, :]
    yb = ((2 * torch.arange(H, dtype=dtype) + 1) / H - 1)[None, :, None]
    t = lambda i: th[:, i][:, None, None]
    return t(0) * xb + t(1) * yb + t(2), t(3) * xb + t(4) * yb + t(5)


def _t_taps(p, n):
    """the align_corners=False taps of an axis of n texels resized to n, at position p: i0, i1, l0, l1 (tap1d_at)"""
    s = ((p + 0.5) * 1.0 - 0.5).clamp(0, n - 1)
    i0 = s.detach().floor().long().clamp(max=n - 1)
    i1 = (i0 + 1).clamp(max=n - 1)
    l1 = s - i0.to(s.dtype)
    return i0, i1, 1 - l1, l1


def t_compose(first, m1, second, m2, H, W):
    """(out_field [N,2,H,W], px, py [N,H,W]) of include/nemar_hip.h nemar_compose_pred, UNet operands at (H, W)"""
    dtype = first.dtype
    gx2, gy2 = _t_grid(second, m2, H, W)
    px, py = ((gx2 + 1) * W - 1) / 2, ((gy2 + 1) * H - 1) / 2
    px, py = px.expand(first.shape[0], H, W), py.expand(first.shape[0], H, W)
    if m1 == U:
        x0, x1, lx0, lx1 = _t_taps(px, W)
        y0, y1, ly0, ly1 = _t_taps(py, H)
        n = torch.arange(first.shape[0])[:, None, None]
        d = []
        for c in (0, 1):
            f = first[:, c]
            d.append((f[n, y0, x0] * lx0 + f[n, y0, x1] * lx1) * ly0 + (f[n, y1, x0] * lx0 + f[n, y1, x1] * lx1) * ly1)
        ident = lambda q, size: (-1 + 2 * q / (size - 1)) if size > 1 else torch.full_like(q, -1)
        gx1, gy1 = ident(px, W) + d[0], ident(py, H) + d[1]
    else:
        th = first + torch.tensor([1, 0, 0, 0, 1, 0], dtype=dtype)[None]
        xb, yb = (2 * px + 1) / W - 1, (2 * py + 1) / H - 1
        t = lambda i: th[:, i][:, None, None]
        gx1, gy1 = t(0) * xb + t(1) * yb + t(2), t(3) * xb + t(4) * yb + t(5)
    lx, ly = torch.linspace(-1, 1, W, dtype=dtype), torch.linspace(-1, 1, H, dtype=dtype)
    return torch.stack([gx1 - lx[None, None, :], gy1 - ly[None, :, None]], 1), px, py


def ref_grad(first, m1, second, m2, H, W, gout, dtype=torch.float64):
    """(d <gout, out> / d first, d / d second, d / d px, d / d py) as float64 numpy"""
    f = torch.tensor(np.asarray(first), dtype=dtype, requires_grad=True)
    s = torch.tensor(np.asarray(second), dtype=dtype, requires_grad=True)
    out, px, py = t_compose(f, m1, s, m2, H, W)
    px.retain_grad()
    py.retain_grad()
    (out * torch.as_tensor(np.asarray(gout), dtype=dtype)).sum().backward()
    return tuple(t.grad.numpy().astype(np.float64) for t in (f, s, px, py))


def positions(second, m2, H, W):
    """float64 px, py [N,H,W]"""
    g2 = ref_grid(second, m2, H, W, torch.float64).numpy()
    return ((g2[..., 0] + 1) * W - 1) / 2, ((g2[..., 1] + 1) * H - 1) / 2


def kink_mask(second, m2, H, W):
    px, py = positions(second, m2, H, W)
    near = lambda v: np.abs(v - np.rint(v)) < KINK_BAND
    return near(px) | near(py)


def _bases(H, W):
    xb = np.abs((2 * np.arange(W, dtype=np.float64) + 1) / W - 1)
    yb = np.abs((2 * np.arange(H, dtype=np.float64) + 1) / H - 1)
    return np.stack([np.broadcast_to(xb[None, :], (H, W)), np.broadcast_to(yb[:, None], (H, W)), np.ones((H, W))])


def abs_sums(first, m1, second, m2, H, W, gout):
    """(S towards first, S towards second, the count of contributions to every texel of a UNET first or None), float64"""
    N = np.asarray(second).shape[0]
    g = np.abs(np.asarray(gout, dtype=np.float64))
    px, py = positions(second, m2, H, W)
    fin = np.isfinite(px) & np.isfinite(py)
    pxs, pys = np.where(fin, px, 0.0).reshape(N, -1), np.where(fin, py, 0.0).reshape(N, -1)
    count = None
    if m1 == U:
        x0, x1, lx0, lx1 = _resize_at(W, pxs, W, np.float64)
        y0, y1, ly0, ly1 = _resize_at(H, pys, H, np.float64)
        S1, count = np.zeros((N, 2, H * W)), np.zeros((N, H * W))
        n = np.broadcast_to(np.arange(N)[:, None], pxs.shape)
        for yy, ly in ((y0, ly0), (y1, ly1)):
            for xx, lx in ((x0, lx0), (x1, lx1)):
                w = lx * ly * fin.reshape(N, -1)
                for c in (0, 1):
                    np.add.at(S1[:, c], (n, yy * W + xx), w * g[:, c].reshape(N, -1))
                np.add.at(count, (n, yy * W + xx), (w > 0).astype(np.float64))
        S1, count = S1.reshape(N, 2, H, W), count.reshape(N, 1, H, W)
    else:
        base = np.stack([np.abs((2 * pxs + 1) / W - 1), np.abs((2 * pys + 1) / H - 1), np.ones_like(pxs)], 1)      # [N,3,P]
        S1 = np.einsum('ncp,nkp->nck', g.reshape(N, 2, -1) * fin.reshape(N, 1, -1), base).reshape(N, 6)
    # towards second: |gout_c| |d out_c / d p_a| per pixel, the identity's slope and the bilinear slope apart; then d p / d coord
    J = np.zeros((2, 2, N, H, W))
    for c in (0, 1):
        e = np.zeros((N, 2, H, W))
        e[:, c] = 1.0
        _, _, J[c, 0], J[c, 1] = ref_grad(first, m1, second, m2, H, W, e)
    slope = (2.0 / (W - 1) if W > 1 else 0.0, 2.0 / (H - 1) if H > 1 else 0.0) if m1 == U else (0.0, 0.0)
    Sp = []
    for a, half in ((0, W / 2.0), (1, H / 2.0)):
        own, other = a, 1 - a
        Sp.append((g[:, own] * (slope[a] + np.abs(J[own, a] - slope[a])) + g[:, other] * np.abs(J[other, a])) * half * fin)
    Sp = np.stack(Sp, 1)                                                            # [N,2,H,W]
    S2 = Sp if m2 == U else np.einsum('nahw,khw->nak', Sp, _bases(H, W)).reshape(N, 6)
    return S1, S2, count


def fixed_point_step(gout, H, W):
    """2^(e - fix - 1): half the fixed-point unit of the call (csrc/fixed_scatter.h)"""
    m = float(np.abs(np.asarray(gout, dtype=np.float32)).max())
    e = max(math.frexp(m)[1], -80) if m > 0 else -80
    fix = min(40, 62 - math.ceil(math.log2(H * W))) if H * W > 1 else 40
    return 2.0 ** (e - fix - 1)


def chains(m1, m2, H, W):
    """(CHAIN towards first, CHAIN towards second): the module docstring's counts"""
    merge = math.ceil(math.ceil(H / 16) * math.ceil(W / 64) / 256) + 6 + 4
    c1 = 5 if m1 == U else 4 + 1 + 4 + 6 + 4 + merge + 2
    c2 = 9 if m1 == U else 7
    if m2 == A:
        c2 = c2 - 1 + 3 + 1 + 4 + 6 + 4 + merge + 2
    return c1, c2


def draw_case(seed, m1, m2, hw, N=2, amp=0.15, second=None):
    """(first, second, gout, gsecond_checked): gout zeroed on the kinks and the share of zeroed pixels asserted — except at a THIN size that
    cannot meet the cap, where gout stays as drawn and gsecond is not to be compared (gsecond_checked False)"""
    H, W = hw
    first, drawn = draw_pair(seed, m1, m2, N, _size(hw), amp)
    second = drawn if second is None else second
    gout = np.random.default_rng(seed + 100).standard_normal((N, 2, H, W)).astype(np.float32)
    kink = kink_mask(second, m2, H, W)
    if hw in THIN and kink.mean() > KINK_SHARE:
        return first, second, gout, False
    assert kink.mean() <= KINK_SHARE, (hw, pair_id((m1, m2)), kink.mean())
    gout[np.broadcast_to(kink[:, None], gout.shape)] = 0.0
    return first, second, gout, True


# ---- drivers ------------------------------------------------------------------------------------------------------------------------------
def pred_shape(mode, N, H, W):
    return (N, 2, H, W) if mode == U else (N, 6)


def workspace(be, m1, m2, N, H, W):
    """exactly the queried bytes, zero"""
    nbytes = be.lib.compose_pred_bwd_workspace(m1, m2, N, H, W)
    assert nbytes >= be.lib.compose_pred_bwd_zeroed_bytes(m1, m2, N, H, W) and nbytes % 8 == 0
    return be.bytes_buf(nbytes), nbytes


def run_bwd(be, d_first, m1, d_second, m2, d_gout, N, H, W, want=("first", "second"), d_gfirst=None, d_gsecond=None, acc1=0, acc2=0, ws=None):
    """-> (gfirst handle or None, gsecond handle or None); outputs pre-filled with NaN unless the caller brings its own; the zeroed part
    of the workspace is checked to come back all-zero"""
    if "first" in want and d_gfirst is None:
        d_gfirst = be.full(pred_shape(m1, N, H, W), np.nan)
    if "second" in want and d_gsecond is None:
        d_gsecond = be.full(pred_shape(m2, N, H, W), np.nan)
    d_ws, nbytes = workspace(be, m1, m2, N, H, W) if ws is None else ws
    be.lib.compose_pred_bwd(be.ptr(d_first), m1, H, W, be.ptr(d_second), m2, H, W, be.ptr(d_gout), be.ptr(d_gfirst) if "first" in want else None,
                            acc1, be.ptr(d_gsecond) if "second" in want else None, acc2, be.ptr(d_ws), nbytes, N, H, W, be.stream)
    zeroed = be.lib.compose_pred_bwd_zeroed_bytes(m1, m2, N, H, W)
    assert zeroed == (16 * N * H * W if m1 == U else 0)
    assert not be.raw(d_ws)[:zeroed].any(), "the zeroed part of the workspace did not come back all-zero"
    return (d_gfirst if "first" in want else None), (d_gsecond if "second" in want else None)


def run_fwd(be, d_first, m1, d_second, m2, N, H, W):
    d_field = be.full((N, 2, H, W), np.nan)
    be.lib.compose_pred(be.ptr(d_first), m1, H, W, be.ptr(d_second), m2, H, W, be.ptr(d_field), None, None, 0, N, H, W, be.stream)
    return d_field


def _what(m1, m2, hw, amp=0.15):
    return "%s %s amp %g" % (pair_id((m1, m2)), hw, amp)


# ---- 1. against float64 ----------------------------------------------------------------------------------------------------------------------
def check_float64(be, first, m1, second, m2, gout, hw, checked, what):
    """all three forms of the call against the float64 rule; the bits of one output do not depend on the other's being asked for"""
    H, W = hw
    N = first.shape[0]
    d_first, d_second, d_gout = be.dev(first), be.dev(second), be.dev(gout)
    w1, w2, _, _ = ref_grad(first, m1, second, m2, H, W, gout)
    y1, y2, _, _ = ref_grad(first, m1, second, m2, H, W, gout, torch.float32)
    S1, S2, count = abs_sums(first, m1, second, m2, H, W, gout)
    c1, c2 = chains(m1, m2, H, W)
    Q = count.repeat(2, axis=1) * fixed_point_step(gout, H, W) if m1 == U else 0.0
    bound1 = MARGIN * np.abs(y1 - w1).max() + c1 * EPS24 * S1.reshape(w1.shape) + Q
    bound2 = MARGIN * np.abs(y2 - w2).max() + c2 * EPS24 * S2.reshape(w2.shape)
    bits = {}
    for want in WANTS:
        g1, g2 = run_bwd(be, d_first, m1, d_second, m2, d_gout, N, H, W, want)
        for name, h, truth, bound, on in (("first", g1, w1, bound1, True), ("second", g2, w2, bound2, checked)):
            if h is None:
                continue
            assert bits.setdefault(name, be.raw(h)).tobytes() == be.raw(h).tobytes(), "g%s depends on the other output: %s" % (name, what)
            got = be.np(h).reshape(truth.shape)
            assert np.all(np.isfinite(got)), (what, name)
            if not on:
                continue
            err = np.abs(got - truth)
            print("compose grad %-28s g%-6s kernel %.3e  worst err/bound %.3f  max |g| %.3e" % (what, name, err.max(), (err / bound).max(), np.abs(truth).max()))
            assert np.abs(truth).max() > 0, (what, name, "a zero gradient checks nothing")
            assert np.all(err <= bound), (what, name, float(err.max()), float((err / bound).max()))


def case_float64(be, m1, m2, hw, seed=1, amp=0.15):
    first, second, gout, checked = draw_case(seed, m1, m2, hw, amp=amp)
    if amp >= 1.0:         # p really leaves the image: the border texel, the clamp's zero slope and the extended identity are exercised
        px, py = positions(second, m2, *hw)
        assert ((px < -0.5) | (px > hw[1] - 0.5) | (py < -0.5) | (py > hw[0] - 0.5)).mean() > 0.05, "p does not leave the image: the case would show nothing"
    check_float64(be, first, m1, second, m2, gout, hw, checked, _what(m1, m2, hw, amp))


# ---- 2. adjoint towards first, on the kernel's own forward ---------------------------------------------------------------------------------
def case_adjoint(be, m1, m2, hw, seed=3, step=2.0 ** -3):
    """<gout, fwd(first + step d) - fwd(first)> / step against <gfirst, d> = gfirst[element], d one texel (the corners that receive
    anything, the centre; at the (50, 1) size texel (25, 0), which every p reaches only through the border clamp in x: p.x is
    -0.5 + half an offset there, always < 0) or one dtheta entry.  The forward is exactly linear in `first`, and `second` — so every p,
    every weight, linspace_at(p) and the subtracted linspace — has the same bits in both evaluations: the difference carries the
    forward's own fp32 rounding only.  Per output value and evaluation that is at most 2^-24 x (5 |D| + |g1| + |out|): the three
    roundings of the blend (or theta's two products and two sums, |base| <= 1.25) at the size D of the field's (theta's) term, the sum with the
    identity at |g1| = |out + linspace|, the subtraction at |out|.  Summed in absolute value over the pixels whose two outputs differ at
    all, times |gout|, over step: a worst-case bound, no statistics.  It must stay <= 5 % of |gfirst| to tell a gradient from a wrong one."""
    H, W = hw
    first, second, gout, _ = draw_case(seed, m1, m2, hw)
    N = first.shape[0]
    d_second, d_gout = be.dev(second), be.dev(gout)
    gfirst = be.np(run_bwd(be, be.dev(first), m1, d_second, m2, d_gout, N, H, W, ("first",))[0]).reshape(N, -1)
    S1, _, count = abs_sums(first, m1, second, m2, H, W, gout)
    S1 = S1.reshape(N, -1)
    Q = (count.repeat(2, axis=1).reshape(N, -1) * fixed_point_step(gout, H, W)) if m1 == U else np.zeros_like(S1)
    if m1 == U:
        cells = [(H // 2, W // 2)] if hw in THIN else [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)]
        picks = []
        for k, (i, j) in enumerate(cells):
            tries = [(n, c * H * W + i * W + j) for c in (k % 2, 1 - k % 2) for n in (k % 2, 1 - k % 2)]
            live = [t for t in tries if S1[t] > 0]
            picks += live[:1]
        assert len(picks) >= min(3, len(cells)), (_what(m1, m2, hw), "too few of the corner texels receive a gradient")
    else:
        picks = [(0, 0), (1, 1), (0, 2), (1, 3), (0, 4), (1, 5)]
    base = be.np(run_fwd(be, be.dev(first), m1, d_second, m2, N, H, W))
    lin = np.stack([np.broadcast_to(np.linspace(-1, 1, W)[None, :] if W > 1 else -np.ones((1, W)), (H, W)),
                    np.broadcast_to(np.linspace(-1, 1, H)[:, None] if H > 1 else -np.ones((H, 1)), (H, W))])[None]
    c1, _ = chains(m1, m2, H, W)
    g64 = gout.astype(np.float64)
    for n, e in picks:
        moved = first.copy().reshape(N, -1)
        moved[n, e] += step
        moved = moved.reshape(first.shape)
        out = be.np(run_fwd(be, be.dev(moved), m1, d_second, m2, N, H, W))
        fd = float((g64 * (out - base)).sum() / step)
        D = float(np.abs(moved).max()) + (1.0 if m1 == A else 0.0)         # theta = dtheta + identity
        differs = out != base
        rounding = sum(EPS24 * (5 * D + np.abs(o + lin) + np.abs(o)) for o in (out, base))
        fd_err = float((np.abs(g64) * rounding)[differs].sum() / step)
        bound = fd_err + c1 * EPS24 * S1[n, e] + Q[n, e]
        diff = abs(fd - gfirst[n, e])
        print("compose adjoint %-24s element (%d, %d)  fd %+.6e  gfirst %+.6e  diff %.2e  bound %.2e (%.2f %% of |gfirst|)"
              % (_what(m1, m2, hw), n, e, fd, gfirst[n, e], diff, bound, 100 * bound / abs(gfirst[n, e])))
        assert diff <= bound, (_what(m1, m2, hw), n, e, fd, float(gfirst[n, e]), bound)
        assert bound <= 0.05 * abs(gfirst[n, e]), (_what(m1, m2, hw), n, e, "the bound could not tell this gradient from a wrong one", bound)


# ---- 3. the anchor: a zero second field --------------------------------------------------------------------------------------------------
def case_anchor(be, hw=(40, 56), seed=2):
    """second = zeros UNET (the reference's slight zoom: p = w W / (W - 1) - 0.5), first UNET: the float64 rule, and the same bits twice"""
    N = 2
    zero = np.zeros((N, 2) + hw, dtype=np.float32)
    first, second, gout, checked = draw_case(seed, U, U, hw, second=zero)
    assert checked
    check_float64(be, first, U, second, U, gout, hw, True, "anchor " + _what(U, U, hw))
    d = [be.dev(a) for a in (first, second, gout)]
    a = [be.raw(h) for h in run_bwd(be, d[0], U, d[1], U, d[2], N, *hw)]
    b = [be.raw(h) for h in run_bwd(be, d[0], U, d[1], U, d[2], N, *hw)]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "two calls, different bits"


# ---- 4. repeatable, accumulate, overwrite, alignment -----------------------------------------------------------------------------------------
def _off_by_4_bytes(be, a):
    """`a` in a buffer that starts 4 bytes past a 16-byte boundary"""
    d_buf = be.dev(np.concatenate([[0.0], np.asarray(a, dtype=np.float32).ravel()]))
    return be.sub(d_buf, 1, d_buf.shape[0])


def case_repeat_accumulate(be, m1, m2, hw, seed=4):
    first, second, gout, _ = draw_case(seed, m1, m2, hw)
    N, (H, W) = first.shape[0], hw
    d = [be.dev(a) for a in (first, second, gout)]
    once = run_bwd(be, d[0], m1, d[1], m2, d[2], N, H, W)                 # onto NaN poison: accumulate = 0 overwrites every element
    a = [be.raw(h) for h in once]
    assert all(np.all(np.isfinite(be.np(h))) for h in once)
    again = run_bwd(be, d[0], m1, d[1], m2, d[2], N, H, W, d_gfirst=be.full(pred_shape(m1, N, H, W), 7.0), d_gsecond=be.full(pred_shape(m2, N, H, W), -3.0))
    assert all(np.array_equal(x, be.raw(h)) for x, h in zip(a, again)), "not repeatable: " + _what(m1, m2, hw)
    rng = np.random.default_rng(seed)
    fills = [rng.standard_normal(pred_shape(m, N, H, W)).astype(np.float32) for m in (m1, m2)]
    got = run_bwd(be, d[0], m1, d[1], m2, d[2], N, H, W, d_gfirst=be.dev(fills[0]), d_gsecond=be.dev(fills[1]), acc1=1, acc2=1)
    for fill, h, o in zip(fills, got, once):
        want = fill.astype(np.float64) + be.np(o)
        assert np.all(np.abs(be.np(h) - want) <= EPS24 * np.abs(want) * (1 + 1e-9)), "accumulate: " + _what(m1, m2, hw)
    # one flag each: accumulate towards first only leaves gsecond overwritten
    mixed = run_bwd(be, d[0], m1, d[1], m2, d[2], N, H, W, d_gfirst=be.dev(fills[0]), d_gsecond=be.dev(fills[1]), acc1=1, acc2=0)
    assert np.array_equal(be.raw(mixed[0]), be.raw(got[0])) and np.array_equal(be.raw(mixed[1]), a[1]), "the two accumulate flags: " + _what(m1, m2, hw)


def case_unaligned(be, m1, m2, hw, seed=5):
    """every pointer one float past a 16-byte boundary (the workspace 8 bytes past one): the aligned call's bits"""
    first, second, gout, _ = draw_case(seed, m1, m2, hw)
    N, (H, W) = first.shape[0], hw
    aligned = [be.raw(h) for h in run_bwd(be, be.dev(first), m1, be.dev(second), m2, be.dev(gout), N, H, W)]
    nbytes = be.lib.compose_pred_bwd_workspace(m1, m2, N, H, W)
    d_wbuf = be.bytes_buf(nbytes + 8)
    outs = [_off_by_4_bytes(be, np.full(int(np.prod(pred_shape(m, N, H, W))), np.nan)) for m in (m1, m2)]
    run_bwd(be, _off_by_4_bytes(be, first), m1, _off_by_4_bytes(be, second), m2, _off_by_4_bytes(be, gout), N, H, W, d_gfirst=outs[0],
            d_gsecond=outs[1], ws=(be.sub(d_wbuf, 8, nbytes + 8), nbytes))
    assert np.array_equal(be.raw(outs[0]), aligned[0]) and np.array_equal(be.raw(outs[1]), aligned[1]), "unaligned != aligned: " + _what(m1, m2, hw)


# ---- 5. non-finite positions -------------------------------------------------------------------------------------------------------------------
def case_non_finite(be, m1, m2, hw, seed=6):
    """one NaN texel in a UNET second, one Inf in an AFFINE second's dtheta: the pixels whose position is not finite contribute exactly 0 —
    both gradients finite; then sample 1 non-finite everywhere: its gradients are exactly 0, sample 0's are not"""
    first, second, gout, _ = draw_case(seed, m1, m2, hw)
    N, (H, W) = first.shape[0], hw
    second = second.copy()
    if m2 == U:
        second[0, 1, H // 2, W // 3] = np.nan
    else:
        second[1, 4] = np.inf
    d_first, d_gout = be.dev(first), be.dev(gout)
    g1, g2 = (be.np(h) for h in run_bwd(be, d_first, m1, be.dev(second), m2, d_gout, N, H, W))
    assert np.all(np.isfinite(g1)) and np.all(np.isfinite(g2)), _what(m1, m2, hw)
    if m2 == U:
        assert g2[0, 0, H // 2, W // 3] == 0.0 and g2[0, 1, H // 2, W // 3] == 0.0
        second[1] = np.nan
        second[1, 0, ::2] = np.inf
    g1, g2 = (be.np(h) for h in run_bwd(be, d_first, m1, be.dev(second), m2, d_gout, N, H, W))
    assert np.all(np.isfinite(g1)) and np.all(np.isfinite(g2)), _what(m1, m2, hw)
    assert np.all(g1[1] == 0.0) and np.all(g2[1] == 0.0), "a sample whose positions are all non-finite has a gradient: " + _what(m1, m2, hw)
    assert np.any(g1[0] != 0.0) and np.any(g2[0] != 0.0)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------
def case_refusals(be):
    """NEMAR_EINVAL (-1), a message, nothing launched: the outputs keep their fill; then the good call goes through"""
    from nemar_amd._lib import NemarHipError
    einval = r"failed \(-1\): compose_pred_bwd: \S"
    N, H, W = 2, 12, 16
    d_first, d_second, d_th, d_gout = be.zeros(N, 2, H, W), be.zeros(N, 2, H, W), be.zeros(N, 6), be.zeros(N, 2, H, W)
    d_g1, d_g2, d_gth = be.full((N, 2, H, W), 7.0), be.full((N, 2, H, W), 7.0), be.full((N, 6), 7.0)
    query = be.lib.compose_pred_bwd_workspace
    nbytes = max(query(m1, m2, N, H, W) for m1, m2 in MODE_PAIRS)
    d_ws, d_ws_affine = be.bytes_buf(nbytes), be.bytes_buf(nbytes)      # (the layout depends on the modes: one workspace per mode pair)
    first, second, th, gout, g1, g2, gth, ws = (be.ptr(d) for d in (d_first, d_second, d_th, d_gout, d_g1, d_g2, d_gth, d_ws))
    names = ("first", "m1", "h1", "w1", "second", "m2", "h2", "w2", "gout", "g1", "acc1", "g2", "acc2", "ws", "wsb", "N", "H", "W")
    good = [first, U, H, W, second, U, H, W, gout, g1, 0, g2, 0, ws, nbytes, N, H, W]
    off = lambda p, k: ctypes.c_void_p(p.value + k)

    def refused(**change):
        args = [change.get(k, v) for k, v in zip(names, good)]
        with pytest.raises(NemarHipError, match=einval):
            be.lib.compose_pred_bwd(*args, be.stream)

    for k in ("first", "second", "gout", "ws"):                  # null pointers
        refused(**{k: None})
    refused(g1=None, g2=None)                                    # nothing asked for
    for k in ("first", "second", "gout", "g1", "g2"):            # not even 4-byte aligned
        refused(**{k: off(good[names.index(k)], 2)})
    refused(ws=off(ws, 4))                                       # the accumulator is 64-bit
    for k, v in (("g1", first), ("g1", second), ("g1", gout), ("g2", first), ("g2", second), ("g2", gout), ("g2", g1)):      # aliased
        refused(**{k: v})
    for k in ("N", "H", "W"):                                    # non-positive sizes (a UNET operand is then not at the composition size either)
        refused(**{k: 0})
        refused(**{k: -3})
        refused(**{k: 0, "first": th, "m1": A, "second": th, "m2": A, "g1": gth, "g2": None})
    refused(N=65536)                                             # beyond the launch's limits
    refused(first=th, m1=A, second=th, m2=A, g1=gth, g2=None, H=1 << 16, W=1 << 15)      # H * W = 2^31
    refused(wsb=query(U, U, N, H, W) - 1)                         # a workspace smaller than the query
    refused(first=th, m1=A, g1=gth, wsb=query(A, U, N, H, W) - 1)
    refused(second=th, m2=A, g2=gth, wsb=query(U, A, N, H, W) - 1)
    for m in (GRID_EXPLICIT, 3, -1):                             # an unknown mode
        refused(m1=m)
        refused(m2=m)
    for k, v in (("h1", H // 2), ("w1", W // 2), ("h2", H + 1), ("w2", 2 * W), ("h1", 0), ("w2", -1)):      # a resampled (or empty) UNET operand
        refused(**{k: v})
    be.sync()
    assert all(np.all(be.np(d) == 7.0) for d in (d_g1, d_g2, d_gth))
    # the forward still takes the resampled operand; h, w of an affine side are ignored by both
    be.lib.compose_pred(first, U, H // 2, W // 2, second, U, H, W, g1, None, None, 0, N, H, W, be.stream)
    be.lib.compose_pred_bwd(th, A, 0, -1, second, U, H, W, gout, gth, 0, g2, 0, be.ptr(d_ws_affine), nbytes, N, H, W, be.stream)
    assert np.all(be.np(d_gth) == 0.0) and np.all(be.np(d_g2) == 0.0)        # a zero gout has a zero gradient
    be.lib.compose_pred_bwd(*good, be.stream)
    assert np.all(be.np(d_g1) == 0.0) and np.all(be.np(d_g2) == 0.0)
