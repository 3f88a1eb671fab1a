"""Backend-agnostic test bodies of nemar_local_ncc_fwd / _bwd (csrc/local_ncc.hip: the windowed normalised cross-correlation as a loss
with its gradient), driven through tests/backends.py (EmuBackend: host-emulated kernels, CPU tier; HipBackend: the gfx950 library,
`-m gpu` tier).  Every buffer is guard-banded and poisoned there, the workspace included (exactly the queried bytes).

The truth is the definition of include/nemar_hip.h in float64 torch on the CPU, the gradient by autograd (ref_lncc).  The yardstick is
the same code in float32, evaluated two ways — the box sums as one win x win convolution, and as a row pass then a column pass — and its
error is the LARGER of the two errors against float64: the two differ by up to 8 x from each other where a window of x is flat (the
variance cancels to rounding noise and 2 cov / D amplifies it by 1 / eps), so either one alone would be an arbitrary choice of rounding
order.  The rules (MARGIN = 4, from register_cases), over ALL pixels, none left out:
  cc_map    max-abs error against float64 <= MARGIN x the yardstick's.
  gx, gy    max-abs error against float64 <= MARGIN x the yardstick's (each against its own yardstick).
  loss      |loss - loss64| <= MARGIN x max(|loss32 - loss64|, factor x mean|cc32 - cc64|) + factor x CHAIN x 2^-24 x mean|cc64|
            (the yardstick's figures again the larger of the two formulations').
            CHAIN = 29: in the tile kernel a cc passes through at most 4 additions in its lane (one pixel in each of four rows), 6 in
            the wave's xor tree and 3 across the four waves: 13; in the finish kernel ceil(records / 256) = 1 addition per thread
            (records = N x C x tiles <= 60 at every size here), 6 + 3 in the workgroup tree: 10; then 1 - sum / M in double, rounded to
            float32 once, and its float32 product with factor: two roundings of 2^-24 |loss| each, which is (1 - m) / m <= 3 units of
            2^-24 x factor x m for a mean cc m >= 0.25 (what the textures here give, asserted where the loss is compared): 6."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from register_cases import MARGIN

CHAIN = 29
MIN_MEAN_CC = 0.25
EPS = 1e-5

#         (H, W)
SIZES = [(35, 131), (40, 56), (67, 131)]       # tile edges inside both axes of both tilings (64 x 16 forward, 32 x 16 backward)
WINS = [3, 9, 11]
EDGES = [(h, 40) for h in (15, 16, 17, 33)] + [(20, w) for w in (63, 64, 65, 129)]      # a window and the backward's 2r halo straddle tile edges
SMALL = (3, 5)                                 # smaller than the window at win 9: every window truncated
THIN = [(1, 77), (50, 1)]                      # one-dimensional windows
FLAT_AT = (slice(10, 24), slice(30, 50))       # the 14 x 20 patch of x that the flat variant overwrites with 0.3


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------
def _texture(rng, N, C, H, W):
    """per plane: six random sinusoid products (periods 8 .. 100 pixels) scaled to +-0.7, plus +-0.1 uniform noise"""
    hh, ww = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
    out = np.empty((N, C, H, W))
    for n in range(N):
        for c in range(C):
            t = np.zeros((H, W))
            for _ in range(6):
                fy, fx = rng.uniform(0.01, 0.125, 2)
                py, px = rng.uniform(0, 2 * np.pi, 2)
                t += rng.uniform(0.5, 1.0) * np.sin(2 * np.pi * fy * hh + py) * np.sin(2 * np.pi * fx * ww + px)
            out[n, c] = 0.7 * t / max(np.abs(t).max(), 1e-12) + rng.uniform(-0.1, 0.1, (H, W))
    return out


@functools.lru_cache(maxsize=None)
def _images(size, seed, flat, N, C):
    H, W = size
    rng = np.random.default_rng(1000 * seed + 7 * H + W)
    x = _texture(rng, N, C, H, W)
    y = 0.6 * x + 0.4 * _texture(rng, N, C, H, W)
    if flat:
        x[(slice(None), slice(None)) + FLAT_AT] = 0.3
    x, y = x.astype(np.float32), y.astype(np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def images(size, seed=1, flat=False, N=2, C=2):
    """-> (x, y) float32 [N,C,H,W]: y = 0.6 x + 0.4 (an independent texture); flat: a 14 x 20 patch of x is 0.3.  Copies of one
    cached pair: the same bits for every caller, whatever a caller does to its own"""
    x, y = _images(tuple(size), seed, flat, N, C)
    return x.copy(), y.copy()


# ---- the float64 truth, and (dtype float32) the yardstick ---------------------------------------------------------------------------------------
def ref_lncc(x, y, win, eps=EPS, factor=1.0, gscale=1.0, dtype=torch.float64, separable=False):
    """-> (cc [N,C,H,W], loss, gx, gy) as float64 numpy / a Python float, evaluated in `dtype`: include/nemar_hip.h's definition, the box
    sums as zero-padded convolutions with ones (the padding adds nothing; n counts the in-image pixels), the gradient by autograd"""
    N, C, H, W = x.shape
    r = win // 2
    X = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
    Y = torch.tensor(np.asarray(y), dtype=dtype, requires_grad=True)

    def box(t):
        t = t.reshape(N * C, 1, H, W)
        if separable:
            t = F.conv2d(F.conv2d(t, torch.ones(1, 1, 1, win, dtype=dtype), padding=(0, r)), torch.ones(1, 1, win, 1, dtype=dtype), padding=(r, 0))
        else:
            t = F.conv2d(t, torch.ones(1, 1, win, win, dtype=dtype), padding=r)
        return t.reshape(N, C, H, W)

    n = box(torch.ones(N, C, H, W, dtype=dtype))
    mx, my = box(X) / n, box(Y) / n
    vx = torch.clamp(box(X * X) / n - mx * mx, min=0)
    vy = torch.clamp(box(Y * Y) / n - my * my, min=0)
    cov = box(X * Y) / n - mx * my
    cc = cov * cov / (vx * vy + eps)
    loss = factor * (1 - cc.sum() / (N * C * H * W))
    assert loss.dtype == dtype
    (loss * gscale).backward()
    f = lambda t: t.detach().numpy().astype(np.float64)
    return f(cc), float(loss.detach()), f(X.grad), f(Y.grad)


class Ref:
    """the truth and the yardstick's errors of one input: computed once (reference), shared by the cases that need it"""

    def __init__(self, x, y, win, factor, gscale):
        self.cc, self.loss, self.gx, self.gy = ref_lncc(x, y, win, EPS, factor, gscale)
        both = [ref_lncc(x, y, win, EPS, factor, gscale, torch.float32, sep) for sep in (False, True)]
        worst = lambda f: max(f(*b) for b in both)
        self.yard_cc = worst(lambda cc, loss, gx, gy: np.abs(cc - self.cc).max())
        self.yard_gx = worst(lambda cc, loss, gx, gy: np.abs(gx - self.gx).max())
        self.yard_gy = worst(lambda cc, loss, gx, gy: np.abs(gy - self.gy).max())
        self.yard_loss = worst(lambda cc, loss, gx, gy: max(abs(loss - self.loss), factor * np.abs(cc - self.cc).mean()))
        self.loss_bound = MARGIN * self.yard_loss + factor * CHAIN * 2.0 ** -24 * np.abs(self.cc).mean()
        for a in (self.cc, self.gx, self.gy):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def reference(size, win, seed=1, flat=False, N=2, C=2, factor=1.0, gscale=1.0, swap=False, shift=0.0):
    x, y = images(size, seed, flat, N, C)
    if shift:
        x = x + np.float32(shift)
    return Ref(y, x, win, factor, gscale) if swap else Ref(x, y, win, factor, gscale)


# ---- drivers ----------------------------------------------------------------------------------------------------------------------------------
def _fill_value(be):
    """what outputs hold before a call: the float the poison in force reads as (a NaN, or 1e38)"""
    return np.array([be.poison], dtype=np.uint32).view(np.float32)[0]


def run_fwd(be, d_x, d_y, shape, win, eps=EPS, factor=1.0, accumulate=0, d_loss=None, want_map=True):
    """-> (loss float32, cc_map [N,C,H,W] float32 or None) on the host, bit for bit; outputs pre-filled; the workspace at exactly the
    queried bytes"""
    N, C, H, W = shape
    d_loss = be.full((1,), _fill_value(be)) if d_loss is None else d_loss
    d_map = be.full(shape, _fill_value(be)) if want_map else None
    wsb = int(be.lib.local_ncc_workspace(N, C, H, W, win))
    ws = be.bytes_buf(wsb)
    be.lib.local_ncc_fwd(be.ptr(d_x), be.ptr(d_y), win, eps, factor, be.ptr(d_loss), accumulate, be.ptr(d_map), be.ptr(ws), wsb, N, C, H, W, be.stream)
    return be.raw(d_loss).view(np.float32)[0], (be.raw(d_map).view(np.float32).reshape(shape) if want_map else None)


def run_bwd(be, d_x, d_y, shape, win, eps=EPS, factor=1.0, gscale=1.0, accumulate=0, d_gx=None, d_gy=None, want_gy=True):
    """-> (gx, gy or None) [N,C,H,W] float32 on the host, bit for bit; pre-filled"""
    N, C, H, W = shape
    d_gx = be.full(shape, _fill_value(be)) if d_gx is None else d_gx
    d_gy = (be.full(shape, _fill_value(be)) if d_gy is None else d_gy) if want_gy else None
    d_gs = be.dev(np.array([gscale]))
    be.lib.local_ncc_bwd(be.ptr(d_x), be.ptr(d_y), win, eps, be.ptr(d_gs), factor, be.ptr(d_gx), be.ptr(d_gy), accumulate, N, C, H, W, be.stream)
    return be.raw(d_gx).view(np.float32).reshape(shape), (be.raw(d_gy).view(np.float32).reshape(shape) if want_gy else None)


def _ratio(err, yard):
    return err / yard if yard else (0.0 if err == 0 else float('inf'))


def _check(what, ref, loss, cc, gx, gy, need_mean_cc=True):
    """the three rules of the docstring, every figure printed before it is asserted"""
    assert np.isfinite(loss) and np.all(np.isfinite(cc)) and np.all(np.isfinite(gx)) and (gy is None or np.all(np.isfinite(gy))), what
    e_cc = np.abs(cc.astype(np.float64) - ref.cc).max()
    print("lncc cc       %-46s kernel %.3e  torch-fp32 %.3e  ratio %.2f  (mean cc %.4f)" % (what, e_cc, ref.yard_cc, _ratio(e_cc, ref.yard_cc), ref.cc.mean()))
    e_gx = np.abs(gx.astype(np.float64) - ref.gx).max()
    print("lncc gx       %-46s kernel %.3e  torch-fp32 %.3e  ratio %.2f  (max |gx| %.3e)" % (what, e_gx, ref.yard_gx, _ratio(e_gx, ref.yard_gx), np.abs(ref.gx).max()))
    e_gy = None
    if gy is not None:
        e_gy = np.abs(gy.astype(np.float64) - ref.gy).max()
        print("lncc gy       %-46s kernel %.3e  torch-fp32 %.3e  ratio %.2f" % (what, e_gy, ref.yard_gy, _ratio(e_gy, ref.yard_gy)))
    e_l = abs(float(loss) - ref.loss)
    print("lncc loss     %-46s kernel %.9g  float64 %.9g  error %.3e  torch-fp32 %.3e  bound %.3e" % (what, loss, ref.loss, e_l, ref.yard_loss, ref.loss_bound))
    assert e_cc <= MARGIN * ref.yard_cc, (what, e_cc, ref.yard_cc)
    assert e_gx <= MARGIN * ref.yard_gx, (what, e_gx, ref.yard_gx)
    if gy is not None:
        assert e_gy <= MARGIN * ref.yard_gy, (what, e_gy, ref.yard_gy)
    if need_mean_cc:
        assert ref.cc.mean() >= MIN_MEAN_CC, "the mean cc of this input is below what CHAIN's last term assumes (%s)" % what
    assert e_l <= ref.loss_bound, (what, loss, ref.loss, e_l, ref.loss_bound)


# ---- against float64 ------------------------------------------------------------------------------------------------------------------------
def case_against_float64(be, size, win, seed=1, flat=False, N=2, C=2, factor=1.0, gscale=1.0):
    H, W = size
    shape = (N, C, H, W)
    x, y = images(size, seed, flat, N, C)
    ref = reference(size, win, seed, flat, N, C, factor, gscale)
    what = "%s win %d seed %d%s N %d C %d" % (size, win, seed, " flat" if flat else "", N, C)
    d_x, d_y = be.dev(x), be.dev(y)
    loss, cc = run_fwd(be, d_x, d_y, shape, win, EPS, factor)
    gx, gy = run_bwd(be, d_x, d_y, shape, win, EPS, factor, gscale)
    assert np.abs(ref.gx).max() > 0 and np.abs(ref.gy).max() > 0
    if flat:
        inner = ref.cc[(slice(None), slice(None)) + (slice(FLAT_AT[0].start + win // 2, FLAT_AT[0].stop - win // 2), slice(FLAT_AT[1].start + win // 2, FLAT_AT[1].stop - win // 2))]
        assert inner.size and np.abs(inner).max() < 1e-12, "the flat patch holds no window of zero variance: the case would show nothing"
    # (a plane smaller than the window, or one-dimensional, has few pixels per window: its mean cc is what it is)
    _check(what, ref, loss, cc, gx, gy, need_mean_cc=min(H, W) >= win)


# ---- symmetry, shift invariance ----------------------------------------------------------------------------------------------------------
def case_symmetry(be, size, win, seed=2):
    """local_ncc(x, y) and local_ncc(y, x): the same loss within the loss bound, and each one's gy is the other's gx against float64"""
    H, W = size
    shape = (2, 2, H, W)
    x, y = images(size, seed)
    ref, fer = reference(size, win, seed), reference(size, win, seed, swap=True)
    d_x, d_y = be.dev(x), be.dev(y)
    loss_xy, cc_xy = run_fwd(be, d_x, d_y, shape, win)
    loss_yx, cc_yx = run_fwd(be, d_y, d_x, shape, win)
    gx_xy, gy_xy = run_bwd(be, d_x, d_y, shape, win)
    gx_yx, gy_yx = run_bwd(be, d_y, d_x, shape, win)
    print("lncc symmetry %s win %d: loss(x,y) %.9g  loss(y,x) %.9g  bound %.3e" % (size, win, loss_xy, loss_yx, ref.loss_bound))
    assert abs(float(loss_xy) - float(loss_yx)) <= ref.loss_bound
    _check("%s win %d (x, y)" % (size, win), ref, loss_xy, cc_xy, gx_xy, gy_xy)
    _check("%s win %d (y, x)" % (size, win), fer, loss_yx, cc_yx, gx_yx, gy_yx)
    # across: d / d(second argument) of the (y, x) call is d / dx of the truth of (x, y), and the other way round
    for name, got, want, yard in (("gy(y,x) vs gx64(x,y)", gy_yx, ref.gx, ref.yard_gx), ("gx(y,x) vs gy64(x,y)", gx_yx, ref.gy, ref.yard_gy)):
        e = np.abs(got.astype(np.float64) - want).max()
        print("lncc symmetry %s win %d: %s  kernel %.3e  torch-fp32 %.3e  ratio %.2f" % (size, win, name, e, yard, _ratio(e, yard)))
        assert e <= MARGIN * yard, (name, e, yard)


def case_shift_invariance(be, size, win, seed=3, shift=0.5):
    """adding 0.5 to x moves cc by no more than the cc bound (the bound of the unshifted input: what is added is not part of its error)"""
    H, W = size
    shape = (2, 2, H, W)
    x, y = images(size, seed)
    ref = reference(size, win, seed)
    d_y = be.dev(y)
    _, cc0 = run_fwd(be, be.dev(x), d_y, shape, win)
    _, cc1 = run_fwd(be, be.dev(x + np.float32(shift)), d_y, shape, win)
    moved = np.abs(cc1.astype(np.float64) - cc0.astype(np.float64)).max()
    print("lncc shift    %s win %d: cc moved by %.3e  bound %.3e" % (size, win, moved, MARGIN * ref.yard_cc))
    assert moved <= MARGIN * ref.yard_cc, (moved, ref.yard_cc)


# ---- repeatable, accumulated, optional outputs ------------------------------------------------------------------------------------------
def case_repeatable_accumulate_optional(be, size, win, seed=4):
    H, W = size
    shape = (2, 2, H, W)
    x, y = images(size, seed)
    d_x, d_y = be.dev(x), be.dev(y)
    bits = lambda a: np.asarray(a).view(np.uint32)
    fill = _fill_value(be)
    loss, cc = run_fwd(be, d_x, d_y, shape, win, EPS, 0.5)
    gx, gy = run_bwd(be, d_x, d_y, shape, win, EPS, 0.5, 3.0)
    # (the outputs were pre-filled with the poison in force: an element that was not written would show as a NaN)
    assert np.isfinite(loss) and all(np.all(np.isfinite(a)) for a in (cc, gx, gy)), "an output element was not written"
    assert 0 < loss <= 0.5 and np.abs(gx).max() > 0 and np.abs(gy).max() > 0
    loss2, cc2 = run_fwd(be, d_x, d_y, shape, win, EPS, 0.5)
    gx2, gy2 = run_bwd(be, d_x, d_y, shape, win, EPS, 0.5, 3.0)
    assert bits(loss) == bits(loss2) and np.array_equal(bits(cc), bits(cc2)) and np.array_equal(bits(gx), bits(gx2)) \
        and np.array_equal(bits(gy), bits(gy2)), "two calls, different bits"
    # without the optional outputs: no other output bit changes
    loss3, none = run_fwd(be, d_x, d_y, shape, win, EPS, 0.5, want_map=False)
    gx3, none2 = run_bwd(be, d_x, d_y, shape, win, EPS, 0.5, 3.0, want_gy=False)
    assert none is None and none2 is None
    assert bits(loss) == bits(loss3), "cc_map = NULL changes the loss"
    assert np.array_equal(bits(gx), bits(gx3)), "gy = NULL changes gx"
    # the accumulate flags add to what was there (one float32 addition)
    loss4, _ = run_fwd(be, d_x, d_y, shape, win, EPS, 0.5, accumulate=1, d_loss=be.full((1,), 2.5))
    assert bits(loss4) == bits(np.float32(2.5) + loss)
    rng = np.random.default_rng(seed)
    before_x, before_y = (rng.standard_normal(shape).astype(np.float32) * np.float32(1e-3) for _ in range(2))
    gx4, gy4 = run_bwd(be, d_x, d_y, shape, win, EPS, 0.5, 3.0, accumulate=1, d_gx=be.dev(before_x), d_gy=be.dev(before_y))
    assert np.array_equal(bits(gx4), bits(before_x + gx)) and np.array_equal(bits(gy4), bits(before_y + gy)), \
        "accumulate: the gradient buffers are not what was there plus the gradient"
    assert fill != 2.5


# ---- non-finite input -------------------------------------------------------------------------------------------------------------------
def case_nonfinite(be, size=(35, 131), win=9):
    """NaN and Inf in the inputs: NEMAR_OK, intact guards (checked after every call), and the pixels that do not hear from them as before"""
    H, W = size
    shape = (2, 2, H, W)
    x, y = images(size, 5)
    d_y = be.dev(y)
    _, cc0 = run_fwd(be, be.dev(x), d_y, shape, win)
    gx0, gy0 = run_bwd(be, be.dev(x), d_y, shape, win)
    for bad in (np.nan, np.inf, -np.inf):
        xb = x.copy()
        xb[0, 1, 17, 70] = bad
        xb[1, 0, 0, 0] = bad
        xb[1, 0, H - 1, W - 1] = bad
        d_xb = be.dev(xb)
        loss, cc = run_fwd(be, d_xb, d_y, shape, win)
        gx, gy = run_bwd(be, d_xb, d_y, shape, win)
        assert not np.isfinite(loss)
        assert not np.isfinite(cc[0, 1, 17, 70]) and not np.isfinite(gx[0, 1, 17, 70])
        # the planes without a bad value are the bits they were
        for got, want in ((cc, cc0), (gx, gx0), (gy, gy0)):
            assert np.array_equal(got[0, 0].view(np.uint32), want[0, 0].view(np.uint32))
            assert np.array_equal(got[1, 1].view(np.uint32), want[1, 1].view(np.uint32))
    ally = be.dev(np.full(shape, np.nan))
    run_fwd(be, ally, ally, shape, win)
    run_bwd(be, ally, ally, shape, win)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def case_refusals(be):
    """NEMAR_EINVAL (-1), a message, and nothing launched: the outputs keep their fill"""
    from nemar_amd._lib import NemarHipError
    N, C, H, W, win = 2, 2, 12, 16, 9
    shape = (N, C, H, W)
    x, y = images((H, W), 6)
    d_x, d_y, d_gs = be.dev(x), be.dev(y), be.dev(np.array([1.0]))
    d_loss, d_map, d_gx, d_gy = be.full((1,), 7.0), be.full(shape, 7.0), be.full(shape, 7.0), be.full(shape, 7.0)
    wsq = be.lib.local_ncc_workspace
    wsb = int(wsq(N, C, H, W, win))
    assert wsb > 0 and int(wsq(N, C, H, 0, win)) == 0 and int(wsq(0, C, H, W, win)) == 0 and int(wsq(N, C, H, W, 4)) == 0 and int(wsq(N, C, H, W, 13)) == 0
    ws = be.bytes_buf(wsb + 4)
    off2 = lambda p: ctypes.c_void_p(p.value + 2)
    f_names = ("x", "y", "win", "eps", "factor", "loss", "acc", "cc_map", "ws", "wsb", "N", "C", "H", "W")
    f_good = [be.ptr(d_x), be.ptr(d_y), win, EPS, 1.0, be.ptr(d_loss), 0, be.ptr(d_map), be.ptr(ws), wsb, N, C, H, W]
    b_names = ("x", "y", "win", "eps", "gscale", "factor", "gx", "gy", "acc", "N", "C", "H", "W")
    b_good = [be.ptr(d_x), be.ptr(d_y), win, EPS, be.ptr(d_gs), 1.0, be.ptr(d_gx), be.ptr(d_gy), 0, N, C, H, W]

    def refused(which, **change):
        names, good, fn = (f_names, f_good, be.lib.local_ncc_fwd) if which == "fwd" else (b_names, b_good, be.lib.local_ncc_bwd)
        args = [change.get(k, v) for k, v in zip(names, good)]
        with pytest.raises(NemarHipError, match=r"failed \(-1\): local_ncc_%s: \S" % which):
            fn(*args, be.stream)

    for which, names, good, required, optional in (("fwd", f_names, f_good, ("x", "y", "loss", "ws"), ("cc_map",)),
                                                   ("bwd", b_names, b_good, ("x", "y", "gscale", "gx"), ("gy",))):
        for k in required:                                        # required pointers: null, not even 4-byte aligned
            refused(which, **{k: None})
            refused(which, **{k: off2(good[names.index(k)])})
        for k in optional:                                        # optional pointers: misaligned
            refused(which, **{k: off2(good[names.index(k)])})
        for w in (0, 1, 2, 4, 10, 13, -9):                        # win: odd, 3 .. 11
            refused(which, win=w)
        for e in (0.0, -1e-5, float('nan')):                      # eps
            refused(which, eps=e)
        for k in ("N", "C", "H", "W"):                            # non-positive sizes
            refused(which, **{k: 0})
            refused(which, **{k: -3})
        refused(which, N=65536, C=1)
        refused(which, N=256, C=256)                              # N * C = 65536
        refused(which, H=1 << 16, W=1 << 15)                      # H * W = 2^31
    refused("fwd", wsb=wsb - 1)                                   # a short workspace
    refused("fwd", wsb=0)
    refused("fwd", cc_map=f_good[0])                              # the map over an input
    refused("fwd", cc_map=f_good[1])
    for out in ("gx", "gy"):                                      # a gradient over an input
        refused("bwd", **{out: b_good[0]})
        refused("bwd", **{out: b_good[1]})
    refused("bwd", gy=b_good[6])                                  # gy over gx
    be.sync()
    assert all(np.all(be.np(d) == 7.0) for d in (d_loss, d_map, d_gx, d_gy))
    # and the good arguments are good
    be.lib.local_ncc_fwd(*f_good, be.stream)
    be.lib.local_ncc_bwd(*b_good, be.stream)
    assert all(np.all(np.isfinite(be.np(d))) and not np.any(be.np(d) == 7.0) for d in (d_loss, d_map, d_gx, d_gy))
