"""Backend-agnostic test bodies of nemar_dice_sums / nemar_dice_loss_fwd / _bwd (csrc/dice.hip: per-class soft overlap of a bilinearly
warped label map with the fixed map, as a Dice loss with its gradient towards the prediction), driven through tests/backends.py
(EmuBackend: host-emulated kernels, CPU tier; HipBackend: the gfx950 library, `-m gpu` tier).  Every buffer is guard-banded and
poisoned there, the workspace included (exactly the queried bytes).

The truth is the definition of include/nemar_hip.h in float64 torch on the CPU: the K one-hot planes of the moving map through
torch.nn.functional.grid_sample (bilinear, zeros, align_corners=False) on the oracle's own grids (the positions are checked against
deform_cases.ref_positions), autograd for the gradient (ref_dice); the same code in float32 is the yardstick.  MARGIN = 4
(register_cases).  The rules, and why each bound is what it is:
  sums      F exactly.  For I and M, per entry (n, k):  |sum - sum64| <= MARGIN x yard + pixels(n, k) x 2^-DICE_FIX_BITS, where yard is the
            yardstick's largest error over the I and M entries of the case (epe_cases' rule for element-wise results: the largest error
            against the largest error — a single entry's yardstick error can be 0 by cancellation) and pixels(n, k) the number of
            pixels with p_k > 0: each rounds its (class-folded) weights to the fixed-point grid once.  A soft sum is continuous in the
            positions, so no pixel is left out.
  loss      |loss - loss64| <= MARGIN x |loss32 - loss64| + LOSS_ULPS x 2^-24 x c x (number of terms): a term 1 - dice is in [0, 1] and
            is formed in double; the float32 roundings are the thread's partial -> float (1), the 6 + 4 additions of the workgroup tree,
            the product with c and c's own rounding (2), the accumulate addition (1): 14, each at most 2^-24 of a partial sum that is
            at most the number of terms.  Plus the sums' own error passed on: |d loss / d sum| x the sums bound, from coef's a and b.
  BAND      1e-3 px.  A pixel is AMBIGUOUS when its float64 ix (iy) lies within BAND of an integer in [-1, W] ([-1, H]): a cell boundary of
            the zero-padded read, the only places where the slope of the bilinear read jumps and two float32 evaluations may take
            different sides (epe_cases.ambiguous with the range of the zeros padding).
  UNET gradient   ambiguous pixels are left out, capped at EXCLUDED_SHARE = 1 % of the pixels: the float64 reference alone keeps them
            under the cap, or the draw is redrawn from the next seed before the kernel is looked at.  On the rest the max-abs error
            against float64 is <= MARGIN x the yardstick's on the same elements + GRAD_ULPS x 2^-24 x max |gradient64| (epe_cases' rule;
            the floor is for closed forms where the yardstick's error is 0: q (2: a [..] + b from float coef), the slope (4), the
            products with gscale and W/2 (2), coef's own rounding (2): 10 <= GRAD_ULPS = 16).
  AFFINE gradient   the sum cannot leave pixels out: the float64 reference is evaluated twice more with every ambiguous pixel moved by
            -BAND and by +BAND (to either side of its boundary).  Per component |gpred - gpred64| <= MARGIN x yardstick +
            chain' x 2^-24 x sum |per-pixel contribution| + |difference of the two| (epe_cases.chain_affine: the launch arithmetic is
            the EPE loss's).
"""
import ctypes

import numpy as np
import pytest
import torch

import deform_cases as D
import epe_cases as E
from oracle import ops_np as O
from register_cases import GRID_AFFINE, GRID_UNET, MARGIN

DICE_FIX_BITS = 30
BAND = E.BAND
EXCLUDED_SHARE = 0.01
GRAD_ULPS = 16
LOSS_ULPS = 14
TILE_W, TILE_H = 64, 16

#         (H, W): smaller than a tile with W % 4 != 0; past a 64 x 16 tile in both axes by a few and by one; whole tiles on the
#         16-byte route; a partial tile on the 16-byte route
SHAPES = [(11, 13), (19, 70), (35, 67), (17, 65), (32, 64), (17, 68)]
CLASSES = [2, 5, 257]                          # 257 crosses the 256-class table of dice_sums_kernel
DESCENT = [(24, 56), (40, 18)]                 # non-square: a swapped W/2 / H/2 changes the steps


# ---- the float64 truth, and (dtype float32) the yardstick -------------------------------------------------------------------------------
def ref_dice(pred, mode, lm, lf, K, eps=1.0, k0=1, factor=1.0, gscale=1.0, dtype=torch.float64, shift=None, drop=None):
    """include/nemar_hip.h's definition written out, the gradient by autograd.  lm, lf [N,H,W].  -> dict of float64 numpy arrays / floats:
    sums [N,K,3] (I, M, F in pixels), pixels [N,K] (pixels with p_k > 0), loss, gpred (d (gscale loss) / d pred), gpix [N,2,H,W] (the
    same towards each pixel's normalised grid coordinate), base, ix, iy [N,H,W], dice [N,K].
    shift = (sx, sy) [N,H,W] in pixels: added to the sampling positions (a constant).  drop [N,H,W] bool: pixels whose p_k is removed
    (what a non-finite position does)."""
    npdt = np.float64 if dtype == torch.float64 else np.float32
    lm, lf = np.asarray(lm), np.asarray(lf)
    N, H, W = lm.shape
    p = torch.tensor(np.asarray(pred), dtype=dtype, requires_grad=True)
    ident = O.affine_grid(np.array([[[1, 0, 0], [0, 1, 0]]], dtype=npdt), H, W)[0]
    xs, ys = torch.from_numpy(np.ascontiguousarray(ident[..., 0])), torch.from_numpy(np.ascontiguousarray(ident[..., 1]))
    if mode == GRID_UNET:
        grid = torch.from_numpy(O.unet_identity_grid(H, W, npdt)) + p
    else:
        th = p + torch.tensor([1, 0, 0, 0, 1, 0], dtype=dtype)
        c = lambda i: th[:, i, None, None]
        grid = torch.stack([c(0) * xs + c(1) * ys + c(2), c(3) * xs + c(4) * ys + c(5)], dim=1)
    grid.retain_grad()
    ix, iy = ((grid[:, 0] + 1) * W - 1) / 2, ((grid[:, 1] + 1) * H - 1) / 2
    g = grid
    if shift is not None:
        s = torch.stack([torch.as_tensor(shift[0], dtype=dtype) * (2.0 / W), torch.as_tensor(shift[1], dtype=dtype) * (2.0 / H)], dim=1)
        g = grid + s
    ks = np.arange(K, dtype=np.float64)[None, :, None, None]
    onehot = lambda a: torch.tensor((np.asarray(a, dtype=np.float64)[:, None] == ks), dtype=dtype)
    P = torch.nn.functional.grid_sample(onehot(lm), g.permute(0, 2, 3, 1), mode='bilinear', padding_mode='zeros', align_corners=False)
    if drop is not None:
        P = P * torch.tensor(~np.asarray(drop), dtype=dtype)[:, None]
    Fk = onehot(lf)
    I, M, F = (P * Fk).sum((2, 3)), P.sum((2, 3)), Fk.sum((2, 3))
    dice = (2 * I + eps) / (M + F + eps)
    loss = (factor / (N * (K - k0))) * (1 - dice[:, k0:]).sum()
    assert loss.dtype == dtype
    (loss * gscale).backward()
    f64 = lambda t: t.detach().numpy().astype(np.float64)
    return {'sums': f64(torch.stack([I, M, F], dim=2)), 'pixels': f64((P > 0).sum((2, 3))), 'loss': float(loss.detach()),
            'gpred': f64(p.grad), 'gpix': f64(grid.grad), 'base': (f64(xs[0]), f64(ys[:, 0])), 'ix': f64(ix), 'iy': f64(iy), 'dice': f64(dice)}


def ambiguous(r64, H, W):
    """-> (ax, ay) [N,H,W] bool"""
    near = lambda v, size: (np.abs(v - np.round(v)) <= BAND) & (v >= -1 - BAND) & (v <= size + BAND)
    return near(r64['ix'], W), near(r64['iy'], H)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def label_maps(rng, N, H, W, K):
    """-> (lm, lf) float32 [N,H,W]: the K-level quantisation of a smooth function (blocky for a small K, nearly per-pixel for a large one),
    and for the fixed map the same function moved by a few pixels"""
    f = D._smooth(rng, N, H + 6, W + 6, 3.0)[:, 0]
    f = (f - f.min()) / (f.max() - f.min() + 1e-9)
    q = np.minimum(np.floor(f * K), K - 1).astype(np.float32)
    return np.ascontiguousarray(q[:, 3:3 + H, 3:3 + W]), np.ascontiguousarray(q[:, 1:1 + H, 5:5 + W])


def draw(seed, mode, N, H, W, K, kind, **kw):
    """-> (pred, lm, lf, r64, (ax, ay)).  kinds 'smooth': offsets of a few pixels (deform_cases._draw_meter_inputs); 'leaving': a prediction
    that sends part of the image outside.  A draw whose float64 reference finds more than EXCLUDED_SHARE of the pixels ambiguous is
    redrawn from the next seed."""
    for attempt in range(8):
        rng = np.random.default_rng(seed + attempt)
        pred, _ = D._draw_meter_inputs(rng, mode, N, H, W, 'smooth')
        if kind == 'leaving':
            if mode == GRID_UNET:
                pred = D._smooth(rng, N, H, W, 1.5).astype(np.float32)              # normalised units: the image is 2 wide
            else:
                pred[:, 2] += np.where(np.arange(N) % 2 == 0, 0.6, -0.5)
                pred[:, 5] += np.where(np.arange(N) % 2 == 0, -0.4, 0.55)
        lm, lf = label_maps(rng, N, H, W, K)
        r64 = ref_dice(pred, mode, lm, lf, K, **kw)
        ax, ay = ambiguous(r64, H, W)
        if (ax | ay).mean() <= EXCLUDED_SHARE:
            return pred, lm, lf, r64, (ax, ay)
    raise AssertionError("no draw in 8 keeps the ambiguous pixels of the float64 reference <= %g" % EXCLUDED_SHARE)


# ---- drivers ----------------------------------------------------------------------------------------------------------------------------------
_fill_value = E._fill_value
_off_by_4_bytes = E._off_by_4_bytes


def _workspace(be, N, H, W):
    wsb = int(be.lib.dice_loss_workspace(N, H, W))
    return be.bytes_buf(wsb), wsb


def _sums_buf(be, N, K):
    return be.dev_i64(np.full((N, K, 3), -77, dtype=np.int64))


def _raw_sums(be, d_sums, N, K):
    return be.raw(d_sums).view(np.uint64).reshape(N, K, 3).copy()


def to_pixels(raw):
    """sums as the library writes them -> float64 [N,K,3] in pixels"""
    s = raw.astype(np.float64)
    s[..., :2] *= 2.0 ** -DICE_FIX_BITS
    return s


def run_sums(be, d_pred, mode, d_lm, d_lf, shape, K):
    """-> uint64 [N,K,3], bit for bit; pre-filled"""
    N, H, W = shape
    d_sums = _sums_buf(be, N, K)
    be.lib.dice_sums(be.ptr(d_pred), mode, be.ptr(d_lm), be.ptr(d_lf), be.ptr(d_sums), N, K, H, W, be.stream)
    return _raw_sums(be, d_sums, N, K)


def run_fwd(be, d_pred, mode, d_lm, d_lf, shape, K, k0=1, eps=1.0, factor=1.0, accumulate=0, d_loss=None, d_coef=None):
    """-> (loss float32 bit for bit, sums uint64 [N,K,3], the coef handle [N,K,2]); pre-filled"""
    N, H, W = shape
    d_loss = be.full((1,), _fill_value(be)) if d_loss is None else d_loss
    d_coef = be.full((N, K, 2), _fill_value(be)) if d_coef is None else d_coef
    d_sums = _sums_buf(be, N, K)
    be.lib.dice_loss_fwd(be.ptr(d_pred), mode, be.ptr(d_lm), be.ptr(d_lf), K, k0, eps, factor, be.ptr(d_loss), accumulate, be.ptr(d_sums),
                         be.ptr(d_coef), N, H, W, be.stream)
    return be.raw(d_loss).view(np.float32)[0], _raw_sums(be, d_sums, N, K), d_coef


def run_bwd(be, d_pred, mode, d_lm, d_lf, d_coef, shape, K, gscale=1.0, accumulate=0, d_gpred=None):
    """-> gpred float32 in the prediction's shape on the host, bit for bit; pre-filled"""
    N, H, W = shape
    pshape = (N, 2, H, W) if mode == GRID_UNET else (N, 6)
    d_gpred = be.full(pshape, _fill_value(be)) if d_gpred is None else d_gpred
    d_gs = be.dev(np.array([gscale]))
    ws, wsb = _workspace(be, N, H, W)
    be.lib.dice_loss_bwd(be.ptr(d_pred), mode, be.ptr(d_lm), be.ptr(d_lf), be.ptr(d_coef), K, be.ptr(d_gs), be.ptr(d_gpred), accumulate,
                         be.ptr(ws), wsb, N, H, W, be.stream)
    return be.raw(d_gpred).view(np.float32).reshape(pshape)


def run_all(be, pred, mode, lm, lf, K, k0=1, eps=1.0, factor=1.0, gscale=1.0):
    """-> (loss, sums in pixels, gpred, coef [N,K,2] float64)"""
    N, H, W = lm.shape
    d_pred, d_lm, d_lf = be.dev(pred), be.dev(lm), be.dev(lf)
    loss, raw, d_coef = run_fwd(be, d_pred, mode, d_lm, d_lf, (N, H, W), K, k0, eps, factor)
    gpred = run_bwd(be, d_pred, mode, d_lm, d_lf, d_coef, (N, H, W), K, gscale)
    return loss, to_pixels(raw), gpred, be.np(d_coef)


def _what(mode, size, K, kind, N):
    return "%s %s N=%d K=%d %s" % ("unet" if mode == GRID_UNET else "affine", size, N, K, kind)


# ---- the rules --------------------------------------------------------------------------------------------------------------------------------
def sums_bound(r64, r32):
    """[N,K,3]: 0 for F"""
    yard = np.abs(r32['sums'][..., :2] - r64['sums'][..., :2]).max()
    b = np.zeros_like(r64['sums'])
    b[..., :2] = (MARGIN * yard + r64['pixels'] * 2.0 ** -DICE_FIX_BITS)[..., None]
    return b, yard


def check_sums(sums, r64, r32, what):
    bound, yard = sums_bound(r64, r32)
    err = np.abs(sums - r64['sums'])
    print("dice sums %-40s kernel %.3e  torch-fp32 %.3e  fixed-point share %.3e" % (what, err[..., :2].max(), yard, (bound[..., 0] - MARGIN * yard).max()))
    assert np.array_equal(sums[..., 2], r64['sums'][..., 2]), (what, "F")
    assert np.all(err <= bound), (what, err.max(), bound.max())


def check_loss(loss, r64, r32, K, k0, eps, factor, what):
    N = r64['sums'].shape[0]
    c = abs(factor) / (N * (K - k0))
    I, M, F = (r64['sums'][..., i] for i in range(3))
    Dn = M + F + eps
    sb, _ = sums_bound(r64, r32)
    passed_on = (c * (2.0 / Dn + (2 * I + eps) / Dn ** 2) * sb[..., 0])[:, k0:].sum()            # |dL/dI| + |dL/dM|, times the sums bound
    bound = MARGIN * abs(r32['loss'] - r64['loss']) + LOSS_ULPS * 2.0 ** -24 * c * N * (K - k0) + passed_on
    e = abs(float(loss) - r64['loss'])
    print("dice loss %-40s kernel %.9g  float64 %.9g  error %.3e  torch-fp32 error %.3e  bound %.3e" % (what, loss, r64['loss'], e, abs(r32['loss'] - r64['loss']), bound))
    assert np.isfinite(loss) and e <= bound, (what, loss, r64['loss'], e, bound)


def check_unet_gradient(gpred, r64, r32, amb, what):
    assert amb.mean() <= EXCLUDED_SHARE, (what, amb.mean())
    sel = np.broadcast_to(~amb[:, None], gpred.shape)
    yard, err = np.abs(r32['gpred'] - r64['gpred'])[sel].max(), np.abs(gpred.astype(np.float64) - r64['gpred'])[sel].max()
    floor = GRAD_ULPS * 2.0 ** -24 * np.abs(r64['gpred']).max()
    print("dice gradient %-36s kernel %.3e  torch-fp32 %.3e  floor %.3e  largest %.3e  left out %.4f" % (what, err, yard, floor, np.abs(r64['gpred']).max(), amb.mean()))
    assert err <= MARGIN * yard + floor, (what, err, yard, floor)


def check_affine_gradient(gpred, r64, r32, ref_again, amb_xy, N, H, W, what):
    """ref_again(shift) -> the float64 reference's gpred with the positions moved by shift"""
    ax, ay = amb_xy
    lo, hi = ref_again((-BAND * ax, -BAND * ay)), ref_again((BAND * ax, BAND * ay))
    bound = (MARGIN * np.abs(r32['gpred'] - r64['gpred']) + E.chain_affine(N, H, W) * 2.0 ** -24 * E.affine_contributions(r64, N)
             + np.abs(hi - lo))
    err = np.abs(gpred.astype(np.float64) - r64['gpred'])
    print("dice gradient %-36s worst error / bound %.3f  (error %.3e, torch-fp32 %.3e, either side %.3e)"
          % (what, (err / np.maximum(bound, 1e-300)).max(), err.max(), np.abs(r32['gpred'] - r64['gpred']).max(), np.abs(hi - lo).max()))
    assert np.all(err <= bound), (what, err, bound)


# ---- 1. against float64 -------------------------------------------------------------------------------------------------------------------------
def case_against_float64(be, mode, size, K, kind, seed=1, N=2, k0=1, eps=1.0, factor=0.5, gscale=3.0):
    H, W = size
    what = _what(mode, size, K, kind, N)
    kw = dict(eps=eps, k0=k0, factor=factor, gscale=gscale)
    pred, lm, lf, r64, (ax, ay) = draw(seed, mode, N, H, W, K, kind, **kw)
    sx, sy = D.ref_positions(pred, mode, H, W)
    assert np.allclose(r64['ix'], sx, rtol=0, atol=1e-9) and np.allclose(r64['iy'], sy, rtol=0, atol=1e-9), "the grids are the oracle's"
    if kind == 'leaving':
        out = (r64['ix'] < -1) | (r64['ix'] > W) | (r64['iy'] < -1) | (r64['iy'] > H)
        print("dice leaving %s: %.3f of the samples read nothing" % (what, out.mean()))
        assert 0.05 <= out.mean() <= 0.95, out.mean()
    r32 = ref_dice(pred, mode, lm, lf, K, dtype=torch.float32, **kw)
    loss, sums, gpred, _ = run_all(be, pred, mode, lm, lf, K, k0, eps, factor, gscale)
    assert np.all(np.isfinite(gpred)), what
    check_sums(sums, r64, r32, what)
    check_loss(loss, r64, r32, K, k0, eps, factor, what)
    if mode == GRID_UNET:
        check_unet_gradient(gpred, r64, r32, ax | ay, what)
    else:
        again = lambda shift: ref_dice(pred, mode, lm, lf, K, shift=shift, **kw)['gpred']
        check_affine_gradient(gpred, r64, r32, again, (ax, ay), N, H, W, what)
    # the sums alone are the same bits
    d_pred, d_lm, d_lf = be.dev(pred), be.dev(lm), be.dev(lf)
    assert np.array_equal(to_pixels(run_sums(be, d_pred, mode, d_lm, d_lf, (N, H, W), K)), sums), "dice_sums and dice_loss_fwd differ"


# ---- 2. closed forms ----------------------------------------------------------------------------------------------------------------------------
def _blocks(N, H, W, K, seed=0):
    """a blocky map with every class of 0..K-1 present: vertical bands, jittered per sample"""
    w = np.arange(W)[None, None, :] + np.arange(N)[:, None, None]
    return np.ascontiguousarray(np.broadcast_to((w * K // (W + N)) % K, (N, H, W))).astype(np.float32)


def case_identity(be, size, K=4, N=2, eps=1.0):
    """AFFINE, dtheta = 0, power-of-two sides, lm == lf: S(x) = x exactly, every weight is 1 or 0: M = F = I exactly, dice = 1, loss = 0"""
    H, W = size
    assert (H & (H - 1)) == 0 and (W & (W - 1)) == 0
    lm = _blocks(N, H, W, K)
    pred = np.zeros((N, 6), dtype=np.float32)
    r64, r32 = ref_dice(pred, GRID_AFFINE, lm, lm, K, eps), ref_dice(pred, GRID_AFFINE, lm, lm, K, eps, dtype=torch.float32)
    assert abs(r64['loss']) <= 1e-15
    loss, sums, gpred, _ = run_all(be, pred, GRID_AFFINE, lm, lm, K, 1, eps)
    check_sums(sums, r64, r32, "identity %s" % (size,))
    assert np.array_equal(sums[..., 0], sums[..., 2]) and np.array_equal(sums[..., 1], sums[..., 2]), "M = F = I at the identity"
    check_loss(loss, r64, r32, K, 1, eps, 1.0, "identity %s" % (size,))
    assert abs(float(loss)) <= LOSS_ULPS * 2.0 ** -24


def case_disjoint(be, mode, size, K=3, N=2, eps=0.75):
    """the moving map holds class 1 only, the fixed map class 2 only: I = 0 and dice = eps / (M + F + eps) for both; class 0 is in neither"""
    H, W = size
    pred, _ = D._draw_meter_inputs(np.random.default_rng(5), mode, N, H, W, 'smooth')
    lm, lf = np.full((N, H, W), 1.0, dtype=np.float32), np.full((N, H, W), 2.0, dtype=np.float32)
    loss, sums, gpred, _ = run_all(be, pred, mode, lm, lf, K, 0, eps)
    r64, r32 = ref_dice(pred, mode, lm, lf, K, eps, 0), ref_dice(pred, mode, lm, lf, K, eps, 0, dtype=torch.float32)
    check_sums(sums, r64, r32, "disjoint %s" % (size,))
    assert np.all(sums[..., 0] == 0) and np.all(sums[:, 0] == 0) and np.all(sums[:, 1, 2] == 0) and np.all(sums[:, 2, 1] == 0)
    dice = eps / (sums[..., 1] + sums[..., 2] + eps)
    dice[:, 0] = 1.0                                                  # absent from both: eps / eps
    want = (1 - dice).sum() / (N * K)
    assert abs(float(loss) - want) <= LOSS_ULPS * 2.0 ** -24 * 1.0, (loss, want)
    check_loss(loss, r64, r32, K, 0, eps, 1.0, "disjoint %s" % (size,))


def case_absent_class_and_background(be, mode, size, N=2, eps=1.0):
    """K = 5 with classes 2 and 3 in neither map: no sums, dice exactly 1, no term in the loss, and no pixel meets their coef rows.  And
    background=False (k0 = 1) leaves class 0 out of the loss AND of the gradient: its coef row is exactly 0, the loss is the mean of the
    other classes' terms, and the sums are the same."""
    H, W = size
    K = 5
    rng = np.random.default_rng(11)
    pred, _ = D._draw_meter_inputs(rng, mode, N, H, W, 'smooth')
    lm, lf = label_maps(rng, N, H, W, 3)
    lm[lm == 2], lf[lf == 2] = 4.0, 4.0                                # classes 0, 1, 4 present; 2 and 3 absent
    out = {}
    for k0 in (0, 1):
        loss, sums, gpred, coef = run_all(be, pred, mode, lm, lf, K, k0, eps)
        r64 = ref_dice(pred, mode, lm, lf, K, eps, k0)
        r32 = ref_dice(pred, mode, lm, lf, K, eps, k0, dtype=torch.float32)
        check_sums(sums, r64, r32, "absent class k0=%d" % k0)
        check_loss(loss, r64, r32, K, k0, eps, 1.0, "absent class k0=%d" % k0)
        assert np.all(sums[:, 2:4] == 0) and np.all(r64['dice'][:, 2:4] == 1.0), "a class in neither map: no sums, dice 1"
        out[k0] = (float(loss), sums, gpred, coef, r64)
    assert np.all(out[1][3][:, 0] == 0), "k0 = 1: class 0's coefficients are exactly 0"
    assert np.all(out[0][3][:, 0, 0] < 0) and np.all(out[0][3][:, 0, 1] > 0)
    assert np.array_equal(out[0][1], out[1][1]), "the sums do not depend on k0"
    # the absent classes are two terms of value 0 among the K (K - 1) that the mean is taken over
    d0 = out[0][4]['dice']
    assert abs(out[0][0] - (1 - d0).sum() / (N * K)) <= 1e-6 and abs(out[1][0] - (1 - d0[:, 1:]).sum() / (N * (K - 1))) <= 1e-6
    if mode == GRID_UNET:
        # where the reference's gradient is exactly 0 (a cell of one class: every q is the same float) the kernel's is exactly 0
        r64 = out[1][4]
        bg = np.abs(r64['gpix']).sum(1) == 0
        assert bg.mean() > 0.1 and np.all(out[1][2][np.broadcast_to(bg[:, None], out[1][2].shape)] == 0)


def case_non_class_values(be, mode, size, K=4, N=2):
    """-1, 2.5, K, NaN, Inf in either map are no class: the same sums, loss and gradient bits as with any other non-class value there"""
    H, W = size
    rng = np.random.default_rng(13)
    pred, _ = D._draw_meter_inputs(rng, mode, N, H, W, 'smooth')
    lm, lf = label_maps(rng, N, H, W, K)
    sel_m, sel_f = rng.random((N, H, W)) < 0.15, rng.random((N, H, W)) < 0.15
    junk = np.array([-1.0, 2.5, float(K), np.nan, np.inf, 1e30, -0.5], dtype=np.float32)
    results = []
    for variant in range(2):
        a, b = lm.copy(), lf.copy()
        a[sel_m] = junk[rng.integers(0, junk.size, sel_m.sum())] if variant else -1.0
        b[sel_f] = junk[rng.integers(0, junk.size, sel_f.sum())] if variant else -1.0
        results.append(run_all(be, pred, mode, a, b, K))
    bits = lambda x: np.asarray(x, dtype=np.float32).view(np.uint32)
    assert bits(results[0][0]) == bits(results[1][0]) and np.array_equal(results[0][1], results[1][1])
    assert np.array_equal(bits(results[0][2]), bits(results[1][2]))
    a, b = lm.copy(), lf.copy()
    a[sel_m], b[sel_f] = -1.0, -1.0
    r64, r32 = ref_dice(pred, mode, a, b, K), ref_dice(pred, mode, a, b, K, dtype=torch.float32)
    check_sums(results[1][1], r64, r32, "non-class values")
    check_loss(results[1][0], r64, r32, K, 1, 1.0, 1.0, "non-class values")


# ---- 3. a non-finite prediction at a few pixels ---------------------------------------------------------------------------------------------
def case_non_finite(be, mode, size, K=4, N=2, seed=1):
    """those pixels contribute nothing to I and M (their f_k still counts) and get gradient exactly 0; everything else is what it is for
    the same map with these pixels removed — the float64 reference with their p_k dropped, and bit for bit a prediction that sends
    them far outside (where every corner is outside the image)"""
    H, W = size
    pred, lm, lf, _, _ = draw(seed, mode, N, H, W, K, 'smooth')
    bits = lambda x: np.asarray(x, dtype=np.float32).view(np.uint32)
    drop = np.zeros((N, H, W), dtype=bool)
    for bad in (np.nan, np.inf, -np.inf):
        p, far = pred.copy(), pred.copy()
        if mode == GRID_UNET:
            where = [(1, 0, H // 2, W // 3), (0, 1, 1, W - 1), (1, 1, H - 1, 0)]
            for (n, c, y, x) in where:
                p[n, c, y, x], far[n, c, y, x] = bad, 1000.0
                drop[n, y, x] = True
        else:
            p[1, 4], far[1, 5] = bad, 1000.0
            drop[1] = True
        got, ref = run_all(be, p, mode, lm, lf, K), run_all(be, far, mode, lm, lf, K)
        assert np.isfinite(got[0]) and np.all(np.isfinite(got[2]))
        assert bits(got[0]) == bits(ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(bits(got[2]), bits(ref[2])), bad
        g = got[2]
        assert np.all(g[np.broadcast_to(drop[:, None], g.shape)] == 0) if mode == GRID_UNET else np.all(g[1] == 0), "gradient at a non-finite pixel"
        r64 = ref_dice(pred, mode, lm, lf, K, drop=drop)
        r32 = ref_dice(pred, mode, lm, lf, K, drop=drop, dtype=torch.float32)
        check_sums(got[1], r64, r32, "non-finite %r" % bad)
        check_loss(got[0], r64, r32, K, 1, 1.0, 1.0, "non-finite %r" % bad)
        clean = run_all(be, pred, mode, lm, lf, K)
        assert np.array_equal(got[1][..., 2], clean[1][..., 2]) and not np.array_equal(got[1][..., 1], clean[1][..., 1]), "F counts them, M does not"


# ---- 4. repeatable, unaligned, accumulated, grid-stride ---------------------------------------------------------------------------------------
def case_repeatable_unaligned_accumulate(be, mode, size, K=5, N=2, seed=3):
    H, W = size
    shape = (N, H, W)
    rng = np.random.default_rng(seed)
    pred, _ = D._draw_meter_inputs(rng, mode, N, H, W, 'smooth')
    lm, lf = label_maps(rng, N, H, W, K)
    d_pred, d_lm, d_lf = be.dev(pred), be.dev(lm), be.dev(lf)
    bits = lambda a: np.asarray(a).view(np.uint32)
    fill = _fill_value(be)

    def both(d_pred, d_lm, d_lf, **kw):
        loss, raw, d_coef = run_fwd(be, d_pred, mode, d_lm, d_lf, shape, K, factor=0.5, d_loss=kw.get('d_loss'), d_coef=kw.get('d_coef'))
        coef = be.raw(d_coef).view(np.uint32).copy()
        return loss, raw, coef, run_bwd(be, d_pred, mode, d_lm, d_lf, d_coef, shape, K, 3.0, d_gpred=kw.get('d_gpred')), d_coef
    loss, raw, coef, gpred, d_coef = both(d_pred, d_lm, d_lf)
    assert np.isfinite(loss) and np.all(np.isfinite(gpred)) and loss > 0 and np.any(gpred != 0) and np.all(raw[..., 2] < (1 << 40))
    loss2, raw2, coef2, gpred2, _ = both(d_pred, d_lm, d_lf)
    assert bits(loss) == bits(loss2) and np.array_equal(raw, raw2) and np.array_equal(coef, coef2) and np.array_equal(bits(gpred), bits(gpred2)), "two calls, different bits"
    # every float tensor 4 bytes off the 16-byte grid
    off = lambda a: _off_by_4_bytes(be, a)
    loss3, raw3, coef3, gpred3, _ = both(off(pred), off(lm), off(lf), d_loss=off([fill]), d_coef=off(np.full((N, K, 2), fill)),
                                         d_gpred=off(np.full(pred.shape, fill)))
    assert bits(loss) == bits(loss3) and np.array_equal(raw, raw3) and np.array_equal(coef, coef3), "views 4 bytes off the 16-byte grid: different bits"
    assert np.array_equal(bits(gpred), bits(gpred3.reshape(pred.shape))), "views 4 bytes off the 16-byte grid: different gradient bits"
    # the accumulate flags add to what was there (one float32 addition)
    loss4, _, _ = run_fwd(be, d_pred, mode, d_lm, d_lf, shape, K, factor=0.5, accumulate=1, d_loss=be.full((1,), 2.5))
    assert bits(loss4) == bits(np.float32(2.5) + loss)
    before = rng.standard_normal(pred.shape).astype(np.float32) * np.abs(gpred).max()
    gpred4 = run_bwd(be, d_pred, mode, d_lm, d_lf, d_coef, shape, K, 3.0, accumulate=1, d_gpred=be.dev(before))
    assert np.array_equal(bits(gpred4), bits(before + gpred)), "accumulate: gpred is not what was there plus the gradient"


def _sums_launch(N, H, W):
    """(workgroups per sample, tiles per sample) of dice_sums_kernel: resident_groups(N, 8, tiles)"""
    tiles = -(-W // TILE_W) * -(-H // TILE_H)
    share = max(256 * 8 // N, 1)
    return min(tiles, share), tiles


GRID_STRIDE = [(64, 2, 33 * 64 - 3), (683, 17, 65)]      # 33 tiles for 32 workgroups; 4 tiles for 2 (and gridDim.y = 683)


def case_grid_stride(be, N, H, W, mode=GRID_UNET, K=3, seed=2):
    """a batch at which the launch's workgroup share makes a workgroup walk more than one tile"""
    gx, tiles = _sums_launch(N, H, W)
    assert gx < tiles
    rng = np.random.default_rng(seed)
    pred = (rng.standard_normal((N, 2, H, W)) * (3.0 / max(H, W))).astype(np.float32)
    lm, lf = label_maps(rng, N, H, W, K)
    what = _what(mode, (H, W), K, 'grid-stride', N)
    r64, r32 = ref_dice(pred, mode, lm, lf, K), ref_dice(pred, mode, lm, lf, K, dtype=torch.float32)
    ax, ay = ambiguous(r64, H, W)
    loss, sums, gpred, _ = run_all(be, pred, mode, lm, lf, K)
    check_sums(sums, r64, r32, what)
    check_loss(loss, r64, r32, K, 1, 1.0, 1.0, what)
    check_unet_gradient(gpred, r64, r32, ax | ay, what)


# ---- 5. descent -----------------------------------------------------------------------------------------------------------------------------
DESCENT_STEPS, DESCENT_STEP = 25, 0.6            # a step moves the fastest pixel by DESCENT_STEP px


def descent_inputs(size, N=2, K=3):
    """-> (the starting offsets, lm, lf): lf two nested boxes, lm the same map translated by (+3, -2) px; the start is a constant offset of a
    fraction of a pixel, so that no position of the first step lies on a cell boundary"""
    H, W = size
    y, x = np.mgrid[0:H, 0:W]
    box = lambda m: ((np.abs(y - H / 2) < H / 2 - m) & (np.abs(x - W / 2) < W / 2 - m))
    lf = (box(4).astype(np.float32) + box(8).astype(np.float32))
    lf = np.ascontiguousarray(np.broadcast_to(lf, (N, H, W))).copy()
    lm = np.roll(lf, (-2, 3), axis=(1, 2))
    pred0 = np.zeros((N, 2, H, W), dtype=np.float32)
    pred0[:, 0], pred0[:, 1] = 0.37 * 2 / W, 0.21 * 2 / H
    return pred0, lm, lf


def descend(loss_and_grad, pred0, H, W):
    """plain gradient steps on the offsets: p -= t g, t such that the largest |g| in pixels moves DESCENT_STEP px.  -> (first, last) loss"""
    p = pred0.astype(np.float64)
    px = np.array([W / 2.0, H / 2.0])[None, :, None, None]
    first = None
    for _ in range(DESCENT_STEPS):
        loss, g = loss_and_grad(p.astype(np.float32))
        first = loss if first is None else first
        g = g.astype(np.float64) / px                                    # d loss / d (position in pixels)
        top = np.abs(g).max()
        if top == 0:
            break
        p = p - (DESCENT_STEP / top) * g / px
    return float(first), float(loss_and_grad(p.astype(np.float32))[0])


def case_descent(size, kernel_loss_and_grad, N=2, K=3):
    """the sign and the scale of the whole gradient: the kernel's descent recovers at least half of what the float64 truth's own descent
    recovers from the same start with the same step rule (loose on purpose: it catches sign and scale errors, not rounding)"""
    H, W = size
    pred0, lm, lf = descent_inputs(size, N, K)

    def reference(p):
        r = ref_dice(p, GRID_UNET, lm, lf, K)
        return r['loss'], r['gpred']
    first64, last64 = descend(reference, pred0, H, W)
    print("dice descent %s: float64 reference %.5f -> %.5f" % (size, first64, last64))
    assert first64 - last64 >= 0.02 * first64, "the reference's own descent goes nowhere: the case would show nothing"
    first, last = descend(lambda p: kernel_loss_and_grad(p, lm, lf, K), pred0, H, W)
    print("dice descent %s: kernel %.5f -> %.5f" % (size, first, last))
    assert np.isfinite(last) and first - last >= 0.5 * (first64 - last64), (first, last, first64, last64)


def entry_point_loss_and_grad(be):
    def f(p, lm, lf, K):
        loss, _, gpred, _ = run_all(be, p, GRID_UNET, lm, lf, K)
        return float(loss), gpred
    return f


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------
def case_refusals(be):
    """NEMAR_EINVAL (-1), a message, and nothing launched: the outputs keep their fill"""
    from nemar_amd._lib import NemarHipError
    N, H, W, K = 2, 12, 16, 4
    d_pred, d_th, d_lm, d_lf, d_gs = be.zeros(N, 2, H, W), be.zeros(N, 6), be.zeros(N, H, W), be.zeros(N, H, W), be.dev(np.array([1.0]))
    d_loss, d_gpred, d_gth, d_coef = be.full((1,), 7.0), be.full((N, 2, H, W), 7.0), be.full((N, 6), 7.0), be.full((N, K, 2), 7.0)
    d_sums = be.dev_i64(np.full((N, K, 3), 7, dtype=np.int64))
    wsb = int(be.lib.dice_loss_workspace(N, H, W))
    assert wsb > 0 and int(be.lib.dice_loss_workspace(N, H, 0)) == 0 and int(be.lib.dice_loss_workspace(0, H, W)) == 0
    ws = be.bytes_buf(wsb + 4)
    offb = lambda p, b: ctypes.c_void_p(p.value + b)
    names = {"sums": ("pred", "mode", "lm", "lf", "sums", "N", "K", "H", "W"),
             "loss_fwd": ("pred", "mode", "lm", "lf", "K", "k0", "eps", "factor", "loss", "acc", "sums", "coef", "N", "H", "W"),
             "loss_bwd": ("pred", "mode", "lm", "lf", "coef", "K", "gscale", "gpred", "acc", "ws", "wsb", "N", "H", "W")}

    def good(which, mode):
        p, gp = (d_pred, d_gpred) if mode == GRID_UNET else (d_th, d_gth)
        v = {"pred": be.ptr(p), "mode": mode, "lm": be.ptr(d_lm), "lf": be.ptr(d_lf), "sums": be.ptr(d_sums), "N": N, "K": K, "H": H, "W": W,
             "k0": 1, "eps": 1.0, "factor": 1.0, "loss": be.ptr(d_loss), "acc": 0, "coef": be.ptr(d_coef), "gscale": be.ptr(d_gs),
             "gpred": be.ptr(gp), "ws": be.ptr(ws), "wsb": wsb}
        return [v[k] for k in names[which]]

    def refused(which, layout, **change):
        args = [change.get(k, v) for k, v in zip(names[which], good(which, layout))]
        with pytest.raises(NemarHipError, match=r"failed \(-1\): dice_%s: \S" % which):
            getattr(be.lib, "dice_" + which)(*args, be.stream)

    pointers = {"sums": ("pred", "lm", "lf", "sums"), "loss_fwd": ("pred", "lm", "lf", "loss", "sums", "coef"),
                "loss_bwd": ("pred", "lm", "lf", "coef", "gscale", "gpred", "ws")}
    for mode in (GRID_UNET, GRID_AFFINE):
        for which in names:
            for k in pointers[which]:                                 # pointers: null, not even 4-byte aligned
                refused(which, mode, **{k: None})
                refused(which, mode, **{k: offb(good(which, mode)[names[which].index(k)], 2)})
            if "sums" in names[which]:                                # sums: 8 bytes
                refused(which, mode, sums=offb(be.ptr(d_sums), 4))
            for bad in (0, 3, -1):                                    # EXPLICIT is not a prediction layout; 3 and -1 are no modes at all
                refused(which, mode, mode=bad)
            for k in ("N", "H", "W"):                                 # non-positive sizes
                refused(which, mode, **{k: 0})
                refused(which, mode, **{k: -3})
            refused(which, mode, N=65536)
            refused(which, mode, H=1 << 16, W=1 << 15)                # H * W = 2^31
            for bad in (0, -1, 1025):
                refused(which, mode, K=bad)
        for bad in (-1, 2, K):                                        # k0: 0 or 1
            refused("loss_fwd", mode, k0=bad)
        refused("loss_fwd", mode, K=1, k0=1)                          # ... and below K
        for eps in (0.0, -0.01, float('inf'), float('nan')):
            refused("loss_fwd", mode, eps=eps)
        refused("loss_bwd", mode, wsb=wsb - 1)                        # a short workspace
        refused("loss_bwd", mode, wsb=0)
        refused("loss_bwd", mode, gpred=good("loss_bwd", mode)[0])    # gpred is the prediction
    be.sync()
    assert np.all(be.np(d_loss) == 7.0) and np.all(be.np(d_gpred) == 7.0) and np.all(be.np(d_gth) == 7.0) and np.all(be.np(d_coef) == 7.0)
    assert np.all(be.raw(d_sums).view(np.int64) == 7)
    # and the good arguments are good (K = 1 with k0 = 0 included)
    for mode in (GRID_UNET, GRID_AFFINE):
        be.lib.dice_sums(*good("sums", mode), be.stream)
        be.lib.dice_loss_fwd(*good("loss_fwd", mode), be.stream)
        assert np.isfinite(be.np(d_loss)[0]) and be.np(d_loss)[0] != 7.0 and not np.any(be.np(d_coef) == 7.0)
        be.lib.dice_loss_bwd(*good("loss_bwd", mode), be.stream)
    assert np.all(np.isfinite(be.np(d_gpred))) and np.all(np.isfinite(be.np(d_gth))) and not np.any(be.np(d_gpred) == 7.0)
    args = good("loss_fwd", GRID_UNET)
    args[names["loss_fwd"].index("K")], args[names["loss_fwd"].index("k0")] = 1, 0
    be.lib.dice_loss_fwd(*args, be.stream)
    assert np.isfinite(be.np(d_loss)[0])


# ---- 7. labels through the input pipeline: nemar_crop_flip_deform_labels ---------------------------------------------------------------------
TIE_BAND, TIE_SHARE = 1e-3, 0.01


def _crop_flip(pool, par, Hc, Wc):
    """[B,1,Hc,Wc]: the crop window and flip of every parameter row, in numpy"""
    out = np.empty((len(par), 1, Hc, Wc), dtype=np.float32)
    for b, (i, y0, x0, flip) in enumerate(par):
        c = pool[i, 0, y0:y0 + Hc, x0:x0 + Wc]
        out[b, 0] = c[:, ::-1] if flip else c
    return out


def run_labels(be, d_pool, d_par, d_g, shape, d_y=None):
    M, B, H, W, Hc, Wc = shape
    d_y = be.full((B, 1, Hc, Wc), np.nan) if d_y is None else d_y
    be.lib.crop_flip_deform_labels(be.ptr(d_pool), be.ptr(d_par), be.ptr(d_g), be.ptr(d_y), M, B, H, W, Hc, Wc, be.stream)
    return be.raw(d_y).view(np.float32).reshape(B, 1, Hc, Wc)


def case_labels(be, H, W, Hc, Wc, K=7, seed=0, M=3, unaligned=False):
    """crops at the pool's corners (both flips) and a random one: g = NULL and g = 0 are the crop / flip exactly; an integer translation is
    the shifted map, border-clamped; a smooth g agrees with the numpy nearest statement (round half to even of the clamped position) at
    the same positions, those within TIE_BAND of a rounding tie left out (capped at TIE_SHARE)"""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, K, (M, 1, H, W)).astype(np.float32)
    par = np.array([(0, 0, 0, 0), (M - 1, H - Hc, W - Wc, 1), (1, 0, W - Wc, 1), (1, H - Hc, 0, 0),
                    (rng.integers(M), rng.integers(H - Hc + 1), rng.integers(W - Wc + 1), 1)], dtype=np.int32)
    B = len(par)
    shape = (M, B, H, W, Hc, Wc)
    d_pool, d_par = be.dev(pool), be.dev_i32(par)
    place = (lambda a: E._off_by_4_bytes(be, a)) if unaligned else be.dev
    out = (lambda: E._off_by_4_bytes(be, np.full((B, 1, Hc, Wc), np.nan))) if unaligned else (lambda: None)
    plain = _crop_flip(pool, par, Hc, Wc)
    assert np.array_equal(run_labels(be, d_pool, d_par, None, shape, out()), plain), "g = NULL is the crop / flip"
    assert np.array_equal(run_labels(be, d_pool, d_par, place(np.zeros((B, 2, Hc, Wc))), shape, out()), plain), "g = 0 is the crop / flip"
    # an integer translation: the shifted map, border-clamped
    tx, ty = 3, -2
    g = np.empty((B, 2, Hc, Wc), dtype=np.float32)
    g[:, 0], g[:, 1] = tx, ty
    ys, xs = np.clip(np.arange(Hc) + ty, 0, Hc - 1), np.clip(np.arange(Wc) + tx, 0, Wc - 1)
    assert np.array_equal(run_labels(be, d_pool, d_par, place(g), shape, out()), plain[:, :, ys][:, :, :, xs]), "an integer translation"
    # a smooth field of a few pixels, leaving the window at the border
    g = D._smooth(rng, B, Hc, Wc, 0.3 * max(Hc, Wc)).astype(np.float32)
    px = np.clip(np.arange(Wc, dtype=np.float32)[None, None, :] + g[:, 0], 0, Wc - 1).astype(np.float64)
    py = np.clip(np.arange(Hc, dtype=np.float32)[None, :, None] + g[:, 1], 0, Hc - 1).astype(np.float64)
    tie = (np.abs(px - np.floor(px) - 0.5) <= TIE_BAND) | (np.abs(py - np.floor(py) - 0.5) <= TIE_BAND)
    assert tie.mean() <= TIE_SHARE, tie.mean()
    xn, yn = np.rint(px).astype(int), np.rint(py).astype(int)                # (np.rint: round half to even)
    want = plain[np.arange(B)[:, None, None], 0, yn, xn]
    got = run_labels(be, d_pool, d_par, place(g), shape, out())[:, 0]
    assert np.array_equal(got[~tie], want[~tie]), "nearest sampling at q + g(q)"
    assert np.all(np.isin(got, np.arange(K))), "class ids are copied, never blended"


def case_labels_refusals(be):
    from nemar_amd._lib import NemarHipError
    M, B, H, W, Hc, Wc = 2, 2, 12, 16, 8, 8
    d_pool, d_par, d_y = be.zeros(M, 1, H, W), be.dev_i32(np.zeros((B, 4), dtype=np.int32)), be.full((B, 1, Hc, Wc), 7.0)
    good = dict(pool=be.ptr(d_pool), par=be.ptr(d_par), g=None, y=be.ptr(d_y), M=M, B=B, H=H, W=W, Hc=Hc, Wc=Wc)
    for change in (dict(pool=None), dict(par=None), dict(y=None), dict(M=0), dict(B=0), dict(B=65536), dict(Hc=H + 1), dict(Wc=W + 1), dict(Hc=0),
                   dict(par=ctypes.c_void_p(be.ptr(d_par).value + 4)), dict(y=ctypes.c_void_p(be.ptr(d_y).value + 2))):
        with pytest.raises(NemarHipError, match=r"failed \(-1\): crop_flip_deform_labels: \S"):
            be.lib.crop_flip_deform_labels(*{**good, **change}.values(), be.stream)
    be.sync()
    assert np.all(be.np(d_y) == 7.0)
