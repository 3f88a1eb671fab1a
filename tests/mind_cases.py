"""Backend-agnostic test bodies of nemar_mind_loss_fwd / _bwd (csrc/mind.hip: the MIND descriptor distance of two modalities as a loss
with its gradient), driven through tests/backends.py (EmuBackend: host-emulated kernels, CPU tier; HipBackend: the gfx950 library,
`-m gpu` tier).  Every buffer is guard-banded and poisoned there, the workspace included (exactly the queried bytes).

The truth is the definition of include/nemar_hip.h in float64 torch on the CPU, the gradient by autograd (ref_mind).  The yardstick is
the same code in float32, evaluated two ways — the box sums as one patch x patch convolution, and as a row pass then a column pass — and
its error is the LARGER of the two errors against float64, as in local_ncc_cases.py.  The rules (MARGIN = 4, from register_cases), over
ALL pixels, none left out:
  dm_map    max-abs error against float64 <= MARGIN x the yardstick's.
  gx, gy    max-abs error against float64 <= MARGIN x the yardstick's (each against its own yardstick).
  loss      |loss - loss64| <= MARGIN x max(|loss32 - loss64|, factor x mean|dm32 - dm64|) + factor x CHAIN x 2^-24 x mean dm64
            (the yardstick's figures again the larger of the two formulations').
            CHAIN = 24: every dm is >= 0, so every partial sum is at most the total and one float32 addition adds at most 2^-24 of the
            total.  In the tile kernel a dm passes through at most 2 additions in its lane (one pixel in each of two rows), 6 in the
            wave's xor tree and 3 across the four waves: 11; in the finish kernel ceil(records / 256) = 1 addition per thread (records
            = N x tiles <= 2 x 25 at every size here), 6 in the wave's tree and 4 across the waves (block_sum starts from 0): 11; then
            sum / (N H W) in double, rounded to float32 once, and its float32 product with factor: 2.
Worst kernel / yardstick ratios measured on the MI355X (tools/profiles/mind_loss.txt has the lines): dm 1.00, gx 1.47, gy 1.53, loss 0.09 of
its bound, the symmetry comparison 0.93, the channel sum 1.00."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from local_ncc_cases import _texture
from register_cases import MARGIN

CHAIN = 24
EPS = 1e-5
TILE_W, TILE_H = 32, 16                        # of both kernels (csrc/mind.hip)

#         (H, W)
SIZES = [(35, 131), (40, 56), (67, 131)]       # tile edges inside both axes
CONFIGS = [(3, 1), (3, 2), (5, 1), (5, 2)]     # (patch, dil)
EDGES = [(h, 40) for h in (TILE_H - 1, TILE_H, TILE_H + 1, 2 * TILE_H + 1)] + [(40, w) for w in (TILE_W - 1, TILE_W, TILE_W + 1, 2 * TILE_W + 1)]
SMALL = [(3, 5), (2, 2)]                       # smaller than a 5-patch with dil 2: every patch truncated, every offset clamps
THIN = [(1, 77), (50, 1)]                      # one axis shorter than dil
FLAT_AT = (slice(10, 24), slice(30, 50))       # the 14 x 20 patch of x that the flat variant overwrites with 0.3
OFFSETS = lambda dil: ((0, -dil), (0, dil), (-dil, 0), (dil, 0))


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _images(size, seed, flat, N, Cx):
    H, W = size
    rng = np.random.default_rng(1000 * seed + 7 * H + W)
    x = _texture(rng, N, Cx, H, W)
    y = -0.8 * np.tanh(2.0 * (0.6 * x.mean(axis=1, keepdims=True) + 0.4 * _texture(rng, N, 1, H, W)))
    if flat:
        x[(slice(None), slice(None)) + FLAT_AT] = 0.3
    x, y = x.astype(np.float32), y.astype(np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def images(size, seed=1, flat=False, N=2, Cx=3):
    """-> (x [N,Cx,H,W], y [N,1,H,W]) float32: x a texture per channel, y = -0.8 tanh(2 (0.6 mean_c x + 0.4 (an independent texture))),
    another "modality"; flat: a 14 x 20 patch of x is 0.3 in every channel.  Copies of one cached pair"""
    x, y = _images(tuple(size), seed, flat, N, Cx)
    return x.copy(), y.copy()


# ---- the float64 truth, and (dtype float32) the yardstick ---------------------------------------------------------------------------------------
def ref_mind(x, y, patch, dil, eps=EPS, factor=1.0, gscale=1.0, dtype=torch.float64, separable=False):
    """-> (dm [N,1,H,W], loss, gx, gy, Vx [N,1,H,W]) as float64 numpy / a Python float, evaluated in `dtype`: include/nemar_hip.h's
    definition, the box sums as zero-padded convolutions with ones (the padding adds nothing; n counts the in-image pixels), the
    gradient by autograd"""
    N, _, H, W = x.shape
    p = patch // 2
    X = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
    Y = torch.tensor(np.asarray(y), dtype=dtype, requires_grad=True)

    def box(t):
        if separable:
            return F.conv2d(F.conv2d(t, torch.ones(1, 1, 1, patch, dtype=dtype), padding=(0, p)), torch.ones(1, 1, patch, 1, dtype=dtype), padding=(p, 0))
        return F.conv2d(t, torch.ones(1, 1, patch, patch, dtype=dtype), padding=p)

    n = box(torch.ones(N, 1, H, W, dtype=dtype))
    hh, ww = torch.arange(H), torch.arange(W)

    def descriptor(img):
        g = img.mean(dim=1, keepdim=True)
        D = []
        for dy, dx in OFFSETS(dil):
            moved = g[:, :, (hh + dy).clamp(0, H - 1)][:, :, :, (ww + dx).clamp(0, W - 1)]
            D.append(box((g - moved) ** 2) / n)
        V = (D[0] + D[1] + D[2] + D[3]) / 4
        return [torch.exp(-d / (V + eps)) for d in D], V

    mx, Vx = descriptor(X)
    my, _ = descriptor(Y)
    dm = sum((a - b) ** 2 for a, b in zip(mx, my)) / 4
    loss = factor * (dm.sum() / (N * H * W))
    assert loss.dtype == dtype
    (loss * gscale).backward()
    f = lambda t: t.detach().numpy().astype(np.float64)
    return f(dm), float(loss.detach()), f(X.grad), f(Y.grad), f(Vx)


class Ref:
    """the truth and the yardstick's errors of one input: computed once (reference), shared by the cases that need it"""

    def __init__(self, x, y, patch, dil, factor, gscale):
        self.dm, self.loss, self.gx, self.gy, self.Vx = ref_mind(x, y, patch, dil, EPS, factor, gscale)
        both = [ref_mind(x, y, patch, dil, EPS, factor, gscale, torch.float32, sep) for sep in (False, True)]
        worst = lambda f: max(f(*b) for b in both)
        self.yard_dm = worst(lambda dm, loss, gx, gy, V: np.abs(dm - self.dm).max())
        self.yard_gx = worst(lambda dm, loss, gx, gy, V: np.abs(gx - self.gx).max())
        self.yard_gy = worst(lambda dm, loss, gx, gy, V: np.abs(gy - self.gy).max())
        self.yard_loss = worst(lambda dm, loss, gx, gy, V: max(abs(loss - self.loss), factor * np.abs(dm - self.dm).mean()))
        self.loss_bound = MARGIN * self.yard_loss + factor * CHAIN * 2.0 ** -24 * np.abs(self.dm).mean()
        for a in (self.dm, self.gx, self.gy, self.Vx):
            a.setflags(write=False)


def _shifted(x, y, shift):
    return (x + np.float32(shift[0]), y + np.float32(shift[1])) if shift else (x, y)


@functools.lru_cache(maxsize=None)
def reference(size, patch, dil, seed=1, flat=False, N=2, Cx=3, factor=1.0, gscale=1.0, swap=False, shift=None, plane3=False):
    x, y = _shifted(*images(size, seed, flat, N, Cx), shift)
    if plane3:
        x = np.repeat(x[:, :1], 3, axis=1)
    return Ref(y, x, patch, dil, factor, gscale) if swap else Ref(x, y, patch, dil, factor, gscale)


# ---- drivers ----------------------------------------------------------------------------------------------------------------------------------
def _fill_value(be):
    """what outputs hold before a call: the float the poison in force reads as (a NaN, or 1e38)"""
    return np.array([be.poison], dtype=np.uint32).view(np.float32)[0]


def _dev(be, a, off=0):
    """a on the device; off = 1: its first element one float past the 16-byte boundary every buffer starts on (the scalar path)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if not off:
        return be.dev(a)
    flat = be.dev(np.concatenate([np.zeros(off, np.float32), a.reshape(-1)]))
    return be.sub(flat, off, off + a.size)


def _out(be, shape, off=0, value=None):
    v = _fill_value(be) if value is None else value
    n = int(np.prod(shape))
    if not off:
        return be.full(shape, v)
    return be.sub(be.full((n + off,), v), off, off + n)


def run_fwd(be, d_x, d_y, shape, patch, dil, eps=EPS, factor=1.0, accumulate=0, d_loss=None, want_map=True, off=0):
    """shape = (N, Cx, Cy, H, W) -> (loss float32, dm_map [N,1,H,W] float32 or None) on the host, bit for bit; outputs pre-filled; the
    workspace at exactly the queried bytes"""
    N, Cx, Cy, H, W = shape
    d_loss = be.full((1,), _fill_value(be)) if d_loss is None else d_loss
    d_map = _out(be, (N, 1, H, W), off) if want_map else None
    wsb = int(be.lib.mind_loss_workspace(N, H, W, patch, dil))
    ws = be.bytes_buf(wsb)
    be.lib.mind_loss_fwd(be.ptr(d_x), Cx, be.ptr(d_y), Cy, patch, dil, eps, factor, be.ptr(d_loss), accumulate, be.ptr(d_map), be.ptr(ws), wsb,
                         N, H, W, be.stream)
    return be.raw(d_loss).view(np.float32)[0], (be.raw(d_map).view(np.float32).reshape(N, 1, H, W) if want_map else None)


def run_bwd(be, d_x, d_y, shape, patch, dil, eps=EPS, factor=1.0, gscale=1.0, accumulate=0, d_gx=None, d_gy=None, want_gy=True, off=0):
    """-> (gx [N,Cx,H,W], gy [N,Cy,H,W] or None) float32 on the host, bit for bit; pre-filled"""
    N, Cx, Cy, H, W = shape
    d_gx = _out(be, (N, Cx, H, W), off) if d_gx is None else d_gx
    d_gy = (_out(be, (N, Cy, H, W), off) if d_gy is None else d_gy) if want_gy else None
    d_gs = be.dev(np.array([gscale]))
    be.lib.mind_loss_bwd(be.ptr(d_x), Cx, be.ptr(d_y), Cy, patch, dil, eps, be.ptr(d_gs), factor, be.ptr(d_gx), be.ptr(d_gy), accumulate, N, H, W,
                         be.stream)
    return be.raw(d_gx).view(np.float32).reshape(N, Cx, H, W), (be.raw(d_gy).view(np.float32).reshape(N, Cy, H, W) if want_gy else None)


def _ratio(err, yard):
    return err / yard if yard else (0.0 if err == 0 else float('inf'))


def _check(what, ref, loss, dm, gx, gy):
    """the rules of the docstring, every figure printed before it is asserted"""
    assert np.isfinite(loss) and np.all(np.isfinite(dm)) and np.all(np.isfinite(gx)) and (gy is None or np.all(np.isfinite(gy))), what
    e_dm = np.abs(dm.astype(np.float64) - ref.dm).max()
    print("mind dm       %-46s kernel %.3e  torch-fp32 %.3e  ratio %.2f  (max dm %.4f)" % (what, e_dm, ref.yard_dm, _ratio(e_dm, ref.yard_dm), ref.dm.max()))
    e_gx = np.abs(gx.astype(np.float64) - ref.gx).max()
    print("mind gx       %-46s kernel %.3e  torch-fp32 %.3e  ratio %.2f  (max |gx| %.3e)" % (what, e_gx, ref.yard_gx, _ratio(e_gx, ref.yard_gx), np.abs(ref.gx).max()))
    e_gy = None
    if gy is not None:
        e_gy = np.abs(gy.astype(np.float64) - ref.gy).max()
        print("mind gy       %-46s kernel %.3e  torch-fp32 %.3e  ratio %.2f  (max |gy| %.3e)" % (what, e_gy, ref.yard_gy, _ratio(e_gy, ref.yard_gy), np.abs(ref.gy).max()))
    e_l = abs(float(loss) - ref.loss)
    print("mind loss     %-46s kernel %.9g  float64 %.9g  error %.3e  torch-fp32 %.3e  bound %.3e  ratio %.2f"
          % (what, loss, ref.loss, e_l, ref.yard_loss, ref.loss_bound, _ratio(e_l, ref.loss_bound)))
    assert e_dm <= MARGIN * ref.yard_dm, (what, e_dm, ref.yard_dm)
    assert e_gx <= MARGIN * ref.yard_gx, (what, e_gx, ref.yard_gx)
    if gy is not None:
        assert e_gy <= MARGIN * ref.yard_gy, (what, e_gy, ref.yard_gy)
    assert e_l <= ref.loss_bound, (what, loss, ref.loss, e_l, ref.loss_bound)


# ---- against float64 ------------------------------------------------------------------------------------------------------------------------
def case_against_float64(be, size, patch, dil, seed=1, flat=False, N=2, Cx=3, factor=1.0, gscale=1.0, off=0):
    """off = 1: every image and output buffer starts one float past a 16-byte boundary (the scalar path of the row loads)"""
    H, W = size
    shape = (N, Cx, 1, H, W)
    x, y = images(size, seed, flat, N, Cx)
    ref = reference(size, patch, dil, seed, flat, N, Cx, factor, gscale)
    what = "%s patch %d dil %d seed %d%s%s" % (size, patch, dil, seed, " flat" if flat else "", " off 1" if off else "")
    d_x, d_y = _dev(be, x, off), _dev(be, y, off)
    loss, dm = run_fwd(be, d_x, d_y, shape, patch, dil, EPS, factor, off=off)
    gx, gy = run_bwd(be, d_x, d_y, shape, patch, dil, EPS, factor, gscale, off=off)
    if min(H, W) > 2:
        assert np.abs(ref.gx).max() > 0 and np.abs(ref.gy).max() > 0
    if flat:
        p = patch // 2 + dil
        inner = ref.Vx[(slice(None), slice(None)) + (slice(FLAT_AT[0].start + p, FLAT_AT[0].stop - p), slice(FLAT_AT[1].start + p, FLAT_AT[1].stop - p))]
        assert inner.size and np.abs(inner).max() == 0, "the flat patch holds no descriptor with D = V = 0: the case would show nothing"
    _check(what, ref, loss, dm, gx, gy)
    for c in range(1, Cx):                                   # one value for every channel
        assert np.array_equal(gx[:, c].view(np.uint32), gx[:, 0].view(np.uint32)), "gx differs between channels"


# ---- symmetry, shift invariance ----------------------------------------------------------------------------------------------------------
def case_symmetry(be, size, patch, dil, seed=2):
    """mind(x, y) and mind(y, x): the same map and loss within the rules, and each one's gy is the other's gx against float64"""
    H, W = size
    x, y = images(size, seed)
    ref, fer = reference(size, patch, dil, seed), reference(size, patch, dil, seed, swap=True)
    d_x, d_y = be.dev(x), be.dev(y)
    xy, yx = (2, 3, 1, H, W), (2, 1, 3, H, W)
    loss_xy, dm_xy = run_fwd(be, d_x, d_y, xy, patch, dil)
    loss_yx, dm_yx = run_fwd(be, d_y, d_x, yx, patch, dil)
    gx_xy, gy_xy = run_bwd(be, d_x, d_y, xy, patch, dil)
    gx_yx, gy_yx = run_bwd(be, d_y, d_x, yx, patch, dil)
    moved = np.abs(dm_xy.astype(np.float64) - dm_yx.astype(np.float64)).max()
    print("mind symmetry %s patch %d dil %d: loss(x,y) %.9g  loss(y,x) %.9g  bound %.3e;  map differs by %.3e  bound %.3e"
          % (size, patch, dil, loss_xy, loss_yx, ref.loss_bound, moved, MARGIN * ref.yard_dm))
    assert abs(float(loss_xy) - float(loss_yx)) <= ref.loss_bound
    assert moved <= MARGIN * ref.yard_dm
    _check("%s patch %d dil %d (x, y)" % (size, patch, dil), ref, loss_xy, dm_xy, gx_xy, gy_xy)
    _check("%s patch %d dil %d (y, x)" % (size, patch, dil), fer, loss_yx, dm_yx, gx_yx, gy_yx)
    # across: d / d(second argument) of the (y, x) call is d / dx of the truth of (x, y), and the other way round
    for name, got, want, yard in (("gy(y,x) vs gx64(x,y)", gy_yx, ref.gx, ref.yard_gx), ("gx(y,x) vs gy64(x,y)", gx_yx, ref.gy, ref.yard_gy)):
        e = np.abs(got.astype(np.float64) - want).max()
        print("mind symmetry %s patch %d dil %d: %s  kernel %.3e  torch-fp32 %.3e  ratio %.2f" % (size, patch, dil, name, e, yard, _ratio(e, yard)))
        assert e <= MARGIN * yard, (name, e, yard)


def case_shift_invariance(be, size, patch, dil, seed=3, shift=(0.5, -0.25)):
    """x + 0.5 and y - 0.25: the shifted pair is held to the rules against its OWN truth and yardstick (float32 x + 0.5 is a rounded
    number: what the rounding moves is in both), and the two maps and gradients differ by no more than the two bounds together plus
    what the truth itself moved by"""
    H, W = size
    shape = (2, 3, 1, H, W)
    x, y = images(size, seed)
    xs, ys = _shifted(x, y, shift)
    ref, fer = reference(size, patch, dil, seed), reference(size, patch, dil, seed, shift=shift)
    d_x, d_y, d_xs, d_ys = be.dev(x), be.dev(y), be.dev(xs), be.dev(ys)
    loss0, dm0 = run_fwd(be, d_x, d_y, shape, patch, dil)
    gx0, gy0 = run_bwd(be, d_x, d_y, shape, patch, dil)
    loss1, dm1 = run_fwd(be, d_xs, d_ys, shape, patch, dil)
    gx1, gy1 = run_bwd(be, d_xs, d_ys, shape, patch, dil)
    _check("%s patch %d dil %d unshifted" % (size, patch, dil), ref, loss0, dm0, gx0, gy0)
    _check("%s patch %d dil %d shifted" % (size, patch, dil), fer, loss1, dm1, gx1, gy1)
    for name, a, b, t0, t1, y0, y1 in (("dm", dm0, dm1, ref.dm, fer.dm, ref.yard_dm, fer.yard_dm), ("gx", gx0, gx1, ref.gx, fer.gx, ref.yard_gx, fer.yard_gx),
                                       ("gy", gy0, gy1, ref.gy, fer.gy, ref.yard_gy, fer.yard_gy)):
        moved, truth = np.abs(a.astype(np.float64) - b).max(), np.abs(t0 - t1).max()
        bound = MARGIN * (y0 + y1) + truth
        print("mind shift    %s patch %d dil %d: %s moved by %.3e  (the truth by %.3e)  bound %.3e" % (size, patch, dil, name, moved, truth, bound))
        assert moved <= bound, (name, moved, bound)


# ---- channels ------------------------------------------------------------------------------------------------------------------------------
def case_channels(be, size, patch, dil, seed=4):
    """Cx = 1 against three copies of the same plane: the same loss and map within the rules (the mean of three equal floats is that float
    in float64, so one truth serves both); gx is one value for every channel, and the channels sum to the 1-channel gradient"""
    H, W = size
    x, y = images(size, seed, Cx=1)
    x3 = np.repeat(x, 3, axis=1)
    ref1, ref3 = reference(size, patch, dil, seed, Cx=1), reference(size, patch, dil, seed, Cx=1, plane3=True)
    d_y = be.dev(y)
    loss1, dm1 = run_fwd(be, be.dev(x), d_y, (2, 1, 1, H, W), patch, dil)
    gx1, gy1 = run_bwd(be, be.dev(x), d_y, (2, 1, 1, H, W), patch, dil)
    loss3, dm3 = run_fwd(be, be.dev(x3), d_y, (2, 3, 1, H, W), patch, dil)
    gx3, gy3 = run_bwd(be, be.dev(x3), d_y, (2, 3, 1, H, W), patch, dil)
    _check("%s patch %d dil %d Cx 1" % (size, patch, dil), ref1, loss1, dm1, gx1, gy1)
    _check("%s patch %d dil %d Cx 3 copies" % (size, patch, dil), ref3, loss3, dm3, gx3, gy3)
    print("mind channels %s: loss Cx 1 %.9g  Cx 3 %.9g  (same bits: %s)" % (size, loss1, loss3, np.float32(loss1).view(np.uint32) == np.float32(loss3).view(np.uint32)))
    assert abs(float(loss1) - float(loss3)) <= ref1.loss_bound + ref3.loss_bound
    for c in (1, 2):
        assert np.array_equal(gx3[:, c].view(np.uint32), gx3[:, 0].view(np.uint32)), "gx differs between channels"
    # the sum of the three channels' gradients is the gradient towards the one plane: three kernel values, three yardstick errors
    e = np.abs(gx3.astype(np.float64).sum(axis=1, keepdims=True) - ref1.gx).max()
    print("mind channels %s: sum_c gx vs the 1-channel gx64  kernel %.3e  torch-fp32 3 x %.3e  ratio %.2f" % (size, e, ref3.yard_gx, _ratio(e, 3 * ref3.yard_gx)))
    assert e <= MARGIN * 3 * ref3.yard_gx


# ---- repeatable, accumulated, optional outputs ------------------------------------------------------------------------------------------
def case_repeatable_accumulate_optional(be, size, patch, dil, seed=4):
    H, W = size
    shape = (2, 3, 1, H, W)
    x, y = images(size, seed)
    d_x, d_y = be.dev(x), be.dev(y)
    bits = lambda a: np.asarray(a).view(np.uint32)
    loss, dm = run_fwd(be, d_x, d_y, shape, patch, dil, EPS, 0.5)
    gx, gy = run_bwd(be, d_x, d_y, shape, patch, dil, EPS, 0.5, 3.0)
    # (the outputs were pre-filled with the poison in force: an element that was not written would show as a NaN)
    assert np.isfinite(loss) and all(np.all(np.isfinite(a)) for a in (dm, gx, gy)), "an output element was not written"
    assert 0 < loss <= 0.5 and np.abs(gx).max() > 0 and np.abs(gy).max() > 0
    loss2, dm2 = run_fwd(be, d_x, d_y, shape, patch, dil, EPS, 0.5)
    gx2, gy2 = run_bwd(be, d_x, d_y, shape, patch, dil, EPS, 0.5, 3.0)
    assert bits(loss) == bits(loss2) and np.array_equal(bits(dm), bits(dm2)) and np.array_equal(bits(gx), bits(gx2)) \
        and np.array_equal(bits(gy), bits(gy2)), "two calls, different bits"
    # without the optional outputs: no other output bit changes
    loss3, none = run_fwd(be, d_x, d_y, shape, patch, dil, EPS, 0.5, want_map=False)
    gx3, none2 = run_bwd(be, d_x, d_y, shape, patch, dil, EPS, 0.5, 3.0, want_gy=False)
    assert none is None and none2 is None
    assert bits(loss) == bits(loss3), "dm_map = NULL changes the loss"
    assert np.array_equal(bits(gx), bits(gx3)), "gy = NULL changes gx"
    # the accumulate flags add to what was there (one float32 addition)
    loss4, _ = run_fwd(be, d_x, d_y, shape, patch, dil, EPS, 0.5, accumulate=1, d_loss=be.full((1,), 2.5))
    assert bits(loss4) == bits(np.float32(2.5) + loss)
    rng = np.random.default_rng(seed)
    before_x = rng.standard_normal(gx.shape).astype(np.float32) * np.float32(1e-3)
    before_y = rng.standard_normal(gy.shape).astype(np.float32) * np.float32(1e-3)
    gx4, gy4 = run_bwd(be, d_x, d_y, shape, patch, dil, EPS, 0.5, 3.0, accumulate=1, d_gx=be.dev(before_x), d_gy=be.dev(before_y))
    assert np.array_equal(bits(gx4), bits(before_x + gx)) and np.array_equal(bits(gy4), bits(before_y + gy)), \
        "accumulate: the gradient buffers are not what was there plus the gradient"


# ---- non-finite input -------------------------------------------------------------------------------------------------------------------
def case_nonfinite(be, patch, dil, size=(35, 131)):
    """a NaN and an Inf pixel in x: NEMAR_OK, intact guards (checked after every call), and the outputs more than 2 (p + dil) away from
    every bad pixel — the backward's reach — are the bits of the clean run"""
    H, W = size
    shape = (2, 3, 1, H, W)
    x, y = images(size, 5)
    d_y = be.dev(y)
    _, dm0 = run_fwd(be, be.dev(x), d_y, shape, patch, dil)
    gx0, gy0 = run_bwd(be, be.dev(x), d_y, shape, patch, dil)
    reach = 2 * (patch // 2 + dil)
    spots = {0: [(17, 70)], 1: [(0, 0), (H - 1, W - 1)]}
    hh, ww = np.arange(H)[:, None], np.arange(W)[None, :]
    far = np.stack([np.all([np.maximum(abs(hh - h), abs(ww - w)) > reach for h, w in spots[n]], axis=0) for n in (0, 1)])[:, None]
    assert far.mean() > 0.5
    for bad in (np.nan, np.inf, -np.inf):
        xb = x.copy()
        xb[0, 1, 17, 70] = bad
        xb[1, 0, 0, 0] = bad
        xb[1, 2, H - 1, W - 1] = bad
        d_xb = be.dev(xb)
        loss, dm = run_fwd(be, d_xb, d_y, shape, patch, dil)
        gx, gy = run_bwd(be, d_xb, d_y, shape, patch, dil)
        assert not np.isfinite(loss)
        assert not np.isfinite(dm[0, 0, 17, 70]) and not np.isfinite(gx[0, 1, 17, 70]) and not np.isfinite(gx[0, 0, 17, 70])
        for got, want in ((dm, dm0), (gx, gx0), (gy, gy0)):
            m = np.broadcast_to(far, got.shape)
            assert np.array_equal(got[m].view(np.uint32), want[m].view(np.uint32)), "a pixel out of the bad pixels' reach changed"
    ally = np.full((2, 3, H, W), np.nan)
    run_fwd(be, be.dev(ally), be.dev(ally[:, :1]), shape, patch, dil)
    run_bwd(be, be.dev(ally), be.dev(ally[:, :1]), shape, patch, dil)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def case_refusals(be):
    """NEMAR_EINVAL (-1), a message, and nothing launched: the outputs keep their fill"""
    from nemar_amd._lib import NemarHipError
    N, Cx, Cy, H, W, patch, dil = 2, 3, 1, 12, 16, 5, 2
    x, y = images((H, W), 6)
    d_x, d_y, d_gs = be.dev(x), be.dev(y), be.dev(np.array([1.0]))
    d_loss, d_map, d_gx, d_gy = be.full((1,), 7.0), be.full((N, 1, H, W), 7.0), be.full((N, Cx, H, W), 7.0), be.full((N, Cy, H, W), 7.0)
    wsq = be.lib.mind_loss_workspace
    wsb = int(wsq(N, H, W, patch, dil))
    assert wsb > 0
    for bad in ((N, H, 0, patch, dil), (0, H, W, patch, dil), (N, -1, W, patch, dil), (65536, H, W, patch, dil), (N, 1 << 16, 1 << 15, patch, dil),
                (N, H, W, 4, dil), (N, H, W, 7, dil), (N, H, W, 1, dil), (N, H, W, patch, 0), (N, H, W, patch, 3)):
        assert int(wsq(*bad)) == 0, bad
    ws = be.bytes_buf(wsb + 4)
    off2 = lambda p: ctypes.c_void_p(p.value + 2)
    f_names = ("x", "Cx", "y", "Cy", "patch", "dil", "eps", "factor", "loss", "acc", "dm_map", "ws", "wsb", "N", "H", "W")
    f_good = [be.ptr(d_x), Cx, be.ptr(d_y), Cy, patch, dil, EPS, 1.0, be.ptr(d_loss), 0, be.ptr(d_map), be.ptr(ws), wsb, N, H, W]
    b_names = ("x", "Cx", "y", "Cy", "patch", "dil", "eps", "gscale", "factor", "gx", "gy", "acc", "N", "H", "W")
    b_good = [be.ptr(d_x), Cx, be.ptr(d_y), Cy, patch, dil, EPS, be.ptr(d_gs), 1.0, be.ptr(d_gx), be.ptr(d_gy), 0, N, H, W]

    def refused(which, **change):
        names, good, fn = (f_names, f_good, be.lib.mind_loss_fwd) if which == "fwd" else (b_names, b_good, be.lib.mind_loss_bwd)
        args = [change.get(k, v) for k, v in zip(names, good)]
        with pytest.raises(NemarHipError, match=r"failed \(-1\): mind_loss_%s: \S" % which):
            fn(*args, be.stream)

    for which, names, good, required, optional in (("fwd", f_names, f_good, ("x", "y", "loss", "ws"), ("dm_map",)),
                                                   ("bwd", b_names, b_good, ("x", "y", "gscale", "gx"), ("gy",))):
        for k in required:                                        # required pointers: null, not even 4-byte aligned
            refused(which, **{k: None})
            refused(which, **{k: off2(good[names.index(k)])})
        for k in optional:                                        # optional pointers: misaligned
            refused(which, **{k: off2(good[names.index(k)])})
        for p in (0, 1, 2, 4, 7, 9, -3):                          # patch: 3 or 5
            refused(which, patch=p)
        for d in (0, 3, 4, -1):                                   # dil: 1 or 2
            refused(which, dil=d)
        for e in (0.0, -1e-5, float('nan')):                      # eps
            refused(which, eps=e)
        for k in ("N", "Cx", "Cy", "H", "W"):                     # non-positive sizes
            refused(which, **{k: 0})
            refused(which, **{k: -3})
        refused(which, N=65536)
        refused(which, H=1 << 16, W=1 << 15)                      # H * W = 2^31
    refused("fwd", wsb=wsb - 1)                                   # a short workspace
    refused("fwd", wsb=0)
    refused("fwd", dm_map=f_good[0])                              # the map over an input
    refused("fwd", dm_map=f_good[2])
    refused("fwd", dm_map=ctypes.c_void_p(f_good[0].value + 4 * (N * Cx * H * W - 1)))      # ... over its last float
    for out in ("gx", "gy"):                                      # a gradient over an input
        refused("bwd", **{out: b_good[0]})
        refused("bwd", **{out: b_good[2]})
    refused("bwd", gy=b_good[9])                                  # gy over gx
    refused("bwd", gy=ctypes.c_void_p(b_good[9].value + 4 * (N * Cx * H * W - 1)))
    be.sync()
    assert all(np.all(be.np(d) == 7.0) for d in (d_loss, d_map, d_gx, d_gy))
    # and the good arguments are good
    be.lib.mind_loss_fwd(*f_good, be.stream)
    be.lib.mind_loss_bwd(*b_good, be.stream)
    assert all(np.all(np.isfinite(be.np(d))) and not np.any(be.np(d) == 7.0) for d in (d_loss, d_map, d_gx, d_gy))
