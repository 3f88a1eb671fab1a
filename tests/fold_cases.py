"""Backend-agnostic test bodies of nemar_fold_penalty_fwd / _bwd (csrc/fold.hip: the hinge max(0, margin - det) on the forward-difference
Jacobian determinant of a UNet offset field, as a loss with its gradient), driven through tests/backends.py (EmuBackend: host-emulated
kernels, CPU tier; HipBackend: the gfx950 library, `-m gpu` tier).  Every buffer is guard-banded and poisoned there, the workspace
included (exactly the queried bytes).

The truth is the definition of include/nemar_hip.h in float64 torch on the CPU with autograd (ref_fold), on register_cases.ref_grid's
coordinates; the same code in float32 is the yardstick.  The rules (why each bound is what it is):
  BAND      1e-3 in units of det: >= 9 x the float32 error of det at every size here (1.1e-4 at 256 x 256).  A pixel is AMBIGUOUS when
            |det64 - margin| <= BAND: two float32 evaluations may disagree on which side of the hinge it lies.  A texel is EXCLUDED from
            the gradient comparison when one of the up to three pixels it hears from (its own, the left one, the upper one) is ambiguous;
            the float64 reference alone keeps the excluded texels <= EXCLUDED_SHARE of all texels.
  gradient  on the kept texels, max-abs error against float64 <= MARGIN (register_cases: 4) x the yardstick's on the same texels — two
            fp32 evaluations of one formula in different rounding orders.  Where the yardstick's error is 0 because nothing is active,
            the kernel's gradient is exactly zero everywhere.
  loss      |loss - loss64| <= MARGIN x |loss32 - loss64| + factor / M x (CHAIN x 2^-24 x sum |term| + n_ambiguous x 2 x BAND): the
            yardstick's own error, the roundings a term passes through on its way into the sum, and per ambiguous pixel a term of at
            most 2 BAND that one side has and the other has not.
            CHAIN = 26: in the tile kernel a term is one rounded subtraction (margin - det), then at most 4 additions in its lane (one
            pixel in each of four rows), 6 in the wave's xor tree and 3 across the four waves: 14; in the finish kernel
            ceil(records / 256) = 1 addition per thread (records = N x tiles <= 128 at every size here), 6 + 3 in the workgroup tree:
            10; then the product with factor / M, itself rounded to float32: 2.
  active    #(det64 < margin - BAND) <= active[n] <= #(det64 <= margin + BAND)."""
import ctypes

import numpy as np
import pytest
import torch

from backends import both_poisons
from register_cases import GRID_UNET, MARGIN, ref_grid, smooth_field
from regularity_cases import run_jac

BAND = 1e-3
EXCLUDED_SHARE = 0.01
CHAIN = 26
MIN_ACTIVE = 0.05          # amp 1.0: the float64 reference finds 14 - 45 % of the pixels active; below this a case would show nothing

#         (H, W)
SIZES = [(35, 131), (40, 56), (67, 131)]       # tile edges inside both axes; one tile row; five tile rows and three tile columns
NETWORK = (256, 256)                           # the network's own size: 64 tiles per sample
EDGES = [(h, 40) for h in (2, 3, 16, 17, 33)] + [(20, w) for w in (2, 63, 64, 65, 129)]      # 17 and 65: the smallest sizes with a neighbour
                                                                                            # in the next tile; 2: the smallest with an interior pixel
THIN = [(1, 77), (50, 1)]                      # no interior pixel


# ---- the float64 truth, and (dtype float32) the yardstick -------------------------------------------------------------------------------
def ref_fold(pred, margin, factor=1.0, gscale=1.0, dtype=torch.float64):
    """-> (det [N,H-1,W-1], loss, gd [N,2,H,W]) as float64 numpy / a Python float, evaluated in `dtype`: include/nemar_hip.h's definition
    written out on ref_grid's coordinates, the gradient by autograd (relu: slope 0 at det == margin)"""
    N, _, H, W = pred.shape
    d = torch.tensor(pred, dtype=dtype, requires_grad=True)
    # ref_grid(pred) is identity + offsets, one addition: the identity is ref_grid of a zero field, bit for bit
    g = ref_grid(np.zeros_like(pred), GRID_UNET, H, W, dtype) + d.permute(0, 2, 3, 1)
    px = ((g[..., 0] + 1) * W - 1) / 2
    py = ((g[..., 1] + 1) * H - 1) / 2
    ax, ay = px[:, :-1, 1:] - px[:, :-1, :-1], py[:, :-1, 1:] - py[:, :-1, :-1]
    bx, by = px[:, 1:, :-1] - px[:, :-1, :-1], py[:, 1:, :-1] - py[:, :-1, :-1]
    det = ax * by - bx * ay
    M = N * (H - 1) * (W - 1)
    if M == 0:
        return det.detach().numpy().astype(np.float64), 0.0, np.zeros(pred.shape, dtype=np.float64)
    loss = (factor / M) * torch.relu(margin - det).sum()
    assert loss.dtype == dtype
    (loss * gscale).backward()
    return det.detach().numpy().astype(np.float64), float(loss.detach()), d.grad.numpy().astype(np.float64)


def excluded_texels(det64, margin, shape):
    """-> (ambiguous pixels [N,H-1,W-1], excluded texels [N,H,W]): texel (h, w) hears from pixels (h, w), (h, w-1) and (h-1, w)"""
    N, _, H, W = shape
    amb = np.abs(det64 - margin) <= BAND
    own = np.zeros((N, H, W), dtype=bool)
    own[:, :-1, :-1] = amb
    ex = own.copy()
    ex[:, :, 1:] |= own[:, :, :-1]
    ex[:, 1:, :] |= own[:, :-1, :]
    return amb, ex


# ---- drivers ----------------------------------------------------------------------------------------------------------------------------------
def _fill_value(be):
    """what outputs hold before a call: the float the poison in force reads as (a NaN, or 1e38)"""
    return np.array([be.poison], dtype=np.uint32).view(np.float32)[0]


def run_fwd(be, d_pred, shape, margin, factor=1.0, accumulate=0, d_loss=None, d_active=None):
    """-> (loss float32, active [N] uint32) on the host, bit for bit; outputs pre-filled"""
    N, _, H, W = shape
    d_loss = be.full((1,), _fill_value(be)) if d_loss is None else d_loss
    d_active = be.dev_i32(np.full((N,), -7)) if d_active is None else d_active
    wsb = int(be.lib.fold_penalty_workspace(N, H, W))
    ws = be.bytes_buf(wsb)
    be.lib.fold_penalty_fwd(be.ptr(d_pred), margin, factor, be.ptr(d_loss), accumulate, be.ptr(d_active), be.ptr(ws), wsb, N, H, W, be.stream)
    return be.raw(d_loss).view(np.float32)[0], be.raw(d_active).view(np.uint32)


def run_bwd(be, d_pred, shape, margin, factor=1.0, gscale=1.0, accumulate=0, d_gd=None):
    """-> gd [N,2,H,W] float32 on the host, bit for bit; pre-filled"""
    N, _, H, W = shape
    d_gd = be.full(shape, _fill_value(be)) if d_gd is None else d_gd
    d_gs = be.dev(np.array([gscale]))
    be.lib.fold_penalty_bwd(be.ptr(d_pred), margin, be.ptr(d_gs), factor, be.ptr(d_gd), accumulate, N, H, W, be.stream)
    return be.raw(d_gd).view(np.float32).reshape(shape)


def _what(size, amp, seed, margin):
    return "%s amp %g seed %d margin %g" % (size, amp, seed, margin)


# ---- 1. / 3. against float64 ----------------------------------------------------------------------------------------------------------------
def case_against_float64(be, size, amp, seed, margin, factor=1.0, gscale=1.0, N=2):
    H, W = size
    shape = (N, 2, H, W)
    pred = smooth_field(seed, N, H, W, amp)
    what = _what(size, amp, seed, margin)
    det64, loss64, gd64 = ref_fold(pred, margin, factor, gscale)
    _, loss32, gd32 = ref_fold(pred, margin, factor, gscale, torch.float32)
    M = N * (H - 1) * (W - 1)
    amb, ex = excluded_texels(det64, margin, shape)
    share = ex.mean()
    active64 = (det64 < margin).reshape(N, -1).sum(1)
    print("fold %-44s float64 active %s of %d, ambiguous %d, excluded texels %.4f" % (what, active64, M // N, amb.sum(), share))
    assert share <= EXCLUDED_SHARE, (what, share)
    if amp >= 1.0:
        assert active64.sum() >= MIN_ACTIVE * M, "the float64 reference finds too few active pixels: the case would show nothing (%s)" % what

    d_pred = be.dev(pred)
    loss, active = run_fwd(be, d_pred, shape, margin, factor)
    gd = run_bwd(be, d_pred, shape, margin, factor, gscale).astype(np.float64)
    assert np.isfinite(loss) and np.all(np.isfinite(gd)), what

    # gradient
    keep = np.broadcast_to(~ex[:, None], shape)
    yard = np.abs(gd32 - gd64)[keep].max()
    err = np.abs(gd - gd64)[keep].max()
    print("fold gradient %-35s kernel %.3e  torch-fp32 %.3e  ratio %.2f" % (what, err, yard, err / yard if yard else (0.0 if err == 0 else float('inf'))))
    if yard == 0 and active64.sum() == 0 and amb.sum() == 0:
        assert np.all(gd == 0), (what, "nothing is active: the gradient is exactly zero everywhere")
    assert err <= MARGIN * yard, (what, err, yard)

    # loss
    terms = np.maximum(0.0, margin - det64)
    bound_sum = factor / M * CHAIN * 2.0 ** -24 * terms.sum()
    bound = MARGIN * abs(loss32 - loss64) + bound_sum + factor / M * amb.sum() * 2 * BAND
    e = abs(float(loss) - loss64)
    print("fold loss %-39s kernel %.9g  float64 %.9g  error %.3e  torch-fp32 error %.3e  bound %.3e  share of the sum bound %.3f"
          % (what, loss, loss64, e, abs(loss32 - loss64), bound, e / bound_sum if bound_sum else 0.0))
    assert e <= bound, (what, loss, loss64, e, bound)
    if active64.sum() == 0 and amb.sum() == 0:
        assert loss == 0 and np.all(active == 0), (what, loss, active)

    # active
    lo, hi = (det64 < margin - BAND).reshape(N, -1).sum(1), (det64 <= margin + BAND).reshape(N, -1).sum(1)
    print("fold active %-37s float64 %s  kernel %s" % (what, (det64 <= margin).reshape(N, -1).sum(1), active))
    assert np.all(lo <= active) and np.all(active <= hi), (what, lo, active, hi)
    return err, yard


# ---- 2. against nemar_jacobian_stats at the same size ----------------------------------------------------------------------------------------
def case_agrees_with_jacobian_stats(be, size, seed, factor=1.0, N=2, amp=1.0):
    """margin 0: `active` is its fold count integer for integer, and the loss is the hinge of the map that kernel wrote, summed"""
    H, W = size
    shape = (N, 2, H, W)
    d_pred = be.dev(smooth_field(seed, N, H, W, amp))
    det, counts, _ = run_jac(be, d_pred, GRID_UNET, ((H, W), (H, W)), N)
    loss, active = run_fwd(be, d_pred, shape, 0.0, factor)
    assert counts[:, 1].sum() > 0, "no fold: the case would show nothing"
    assert np.array_equal(active, counts[:, 1]), (size, active, counts[:, 1])
    M = N * (H - 1) * (W - 1)
    terms = np.maximum(0.0, -det[:, :-1, :-1].astype(np.float64))
    want, bound = factor / M * terms.sum(), factor / M * CHAIN * 2.0 ** -24 * terms.sum()
    print("fold vs jacobian_stats %s seed %d: active %s  loss %.9g  hinge of its map %.9g  error %.3e  bound %.3e"
          % (size, seed, active, loss, want, abs(loss - want), bound))
    assert abs(float(loss) - want) <= bound, (size, loss, want, bound)


# ---- 4. no interior pixel --------------------------------------------------------------------------------------------------------------------
@both_poisons
def case_thin(be, size, N=2, seed=4):
    H, W = size
    shape = (N, 2, H, W)
    d_pred = be.dev(smooth_field(seed, N, H, W, 1.0))
    for margin in (0.0, 0.5):
        loss, active = run_fwd(be, d_pred, shape, margin)
        gd = run_bwd(be, d_pred, shape, margin)
        assert loss == 0 and np.all(active == 0) and np.all(gd == 0), (size, margin, loss, active)


# ---- 5. repeatable, overwritten, unaligned, accumulated --------------------------------------------------------------------------------------
def _off_by_4_bytes(be, a, dtype=np.float32):
    """`a` in a buffer that starts 4 bytes past a 16-byte boundary (a view of a guarded block one element longer)"""
    flat = np.concatenate([[0], np.asarray(a, dtype=dtype).ravel()])
    d_buf = be.dev(flat) if dtype is np.float32 else be.dev_i32(flat)
    return be.sub(d_buf, 1, d_buf.shape[0])


@both_poisons
def case_repeatable_unaligned_accumulate(be, size, margin, N=2, seed=3, amp=1.0):
    H, W = size
    shape = (N, 2, H, W)
    pred = smooth_field(seed, N, H, W, amp)
    d_pred = be.dev(pred)
    bits = lambda a: np.asarray(a).view(np.uint32)
    fill = _fill_value(be)
    loss, active = run_fwd(be, d_pred, shape, margin, 0.5)
    gd = run_bwd(be, d_pred, shape, margin, 0.5, 3.0)
    # (the outputs were pre-filled with the poison in force: an element that was not written would show — as a NaN, or as 1e38)
    assert np.isfinite(loss) and np.all(np.isfinite(gd)) and not np.any(gd == fill) and loss != fill, "an output element was not written"
    assert np.all(active <= (H - 1) * (W - 1)) and active.sum() > 0
    loss2, active2 = run_fwd(be, d_pred, shape, margin, 0.5)
    gd2 = run_bwd(be, d_pred, shape, margin, 0.5, 3.0)
    assert bits(loss) == bits(loss2) and np.array_equal(active, active2) and np.array_equal(bits(gd), bits(gd2)), "two calls, different bits"
    # every pointer 4 bytes off the 16-byte grid
    d_off = _off_by_4_bytes(be, pred)
    loss3, active3 = run_fwd(be, d_off, shape, margin, 0.5, d_loss=_off_by_4_bytes(be, [fill]), d_active=_off_by_4_bytes(be, [-7] * N, np.int32))
    gd3 = run_bwd(be, d_off, shape, margin, 0.5, 3.0, d_gd=_off_by_4_bytes(be, np.full(shape, fill)))
    assert bits(loss) == bits(loss3) and np.array_equal(active, active3) and np.array_equal(bits(gd), bits(gd3.reshape(shape))), \
        "views 4 bytes off the 16-byte grid: different bits"
    # the accumulate flags add to what was there (one float32 addition)
    loss4, active4 = run_fwd(be, d_pred, shape, margin, 0.5, accumulate=1, d_loss=be.full((1,), 2.5))
    assert bits(loss4) == bits(np.float32(2.5) + loss) and np.array_equal(active, active4)
    before = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    gd4 = run_bwd(be, d_pred, shape, margin, 0.5, 3.0, accumulate=1, d_gd=be.dev(before))
    assert np.array_equal(bits(gd4), bits(before + gd)), "accumulate: gd is not what was there plus the gradient"


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------
def case_refusals(be):
    """NEMAR_EINVAL (-1), a message, and nothing launched: the outputs keep their fill"""
    from nemar_amd._lib import NemarHipError
    N, H, W = 2, 12, 16
    d_pred, d_gs = be.zeros(N, 2, H, W), be.dev(np.array([1.0]))
    d_loss, d_active, d_gd = be.full((1,), 7.0), be.dev_i32(np.full((N,), 7)), be.full((N, 2, H, W), 7.0)
    wsb = int(be.lib.fold_penalty_workspace(N, H, W))
    assert wsb > 0 and int(be.lib.fold_penalty_workspace(N, H, 0)) == 0 and int(be.lib.fold_penalty_workspace(0, H, W)) == 0
    ws = be.bytes_buf(wsb + 4)
    off2 = lambda p: ctypes.c_void_p(p.value + 2)
    f_names = ("d", "margin", "factor", "loss", "acc", "active", "ws", "wsb", "N", "H", "W")
    f_good = [be.ptr(d_pred), 0.0, 1.0, be.ptr(d_loss), 0, be.ptr(d_active), be.ptr(ws), wsb, N, H, W]
    b_names = ("d", "margin", "gscale", "factor", "gd", "acc", "N", "H", "W")
    b_good = [be.ptr(d_pred), 0.0, be.ptr(d_gs), 1.0, be.ptr(d_gd), 0, N, H, W]

    def refused(which, **change):
        names, good, fn = (f_names, f_good, be.lib.fold_penalty_fwd) if which == "fwd" else (b_names, b_good, be.lib.fold_penalty_bwd)
        args = [change.get(k, v) for k, v in zip(names, good)]
        with pytest.raises(NemarHipError, match=r"failed \(-1\): fold_penalty_%s: \S" % which):
            fn(*args, be.stream)

    for which, names, good, ptrs in (("fwd", f_names, f_good, ("d", "loss", "active", "ws")), ("bwd", b_names, b_good, ("d", "gscale", "gd"))):
        for k in ptrs:                                            # required pointers: null, not even 4-byte aligned
            refused(which, **{k: None})
            refused(which, **{k: off2(good[names.index(k)])})
        for k in ("N", "H", "W"):                                 # non-positive sizes
            refused(which, **{k: 0})
            refused(which, **{k: -3})
        refused(which, N=65536)
        refused(which, H=1 << 16, W=1 << 15)                      # H * W = 2^31
    refused("fwd", wsb=wsb - 1)                                   # a short workspace
    refused("fwd", wsb=0)
    refused("bwd", gd=b_good[0])                                  # gd is the operand
    be.sync()
    assert np.all(be.np(d_loss) == 7.0) and np.all(be.np(d_gd) == 7.0) and np.all(be.raw(d_active).view(np.int32) == 7)
    # and the good arguments are good: a zero field is the reference's slight zoom, det = W H / ((W-1)(H-1)) > 1 at every pixel
    be.lib.fold_penalty_fwd(*f_good, be.stream)
    be.lib.fold_penalty_bwd(*b_good, be.stream)
    assert np.all(be.np(d_loss) == 0) and np.all(be.np(d_gd) == 0) and np.all(be.raw(d_active).view(np.int32) == 0)
