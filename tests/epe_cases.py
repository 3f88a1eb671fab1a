"""Backend-agnostic test bodies of nemar_epe_loss_fwd / _bwd (csrc/epe.hip: the registration-error meter's residual against a known
ground-truth field as a Charbonnier loss with its gradient towards the prediction), driven through tests/backends.py (EmuBackend:
host-emulated kernels, CPU tier; HipBackend: the gfx950 library, `-m gpu` tier).  Every buffer is guard-banded and poisoned there, the
workspace included (exactly the queried bytes).

The truth is the definition of include/nemar_hip.h in float64 torch on the CPU with autograd (ref_epe), on the oracle's own grids as
deform_cases.ref_positions takes them; the same code in float32 is the yardstick.  MARGIN = 4 (register_cases).  The rules, and why each
bound is what it is:
  loss      |loss - loss64| <= MARGIN x |loss32 - loss64| + chain x 2^-24 x loss64.  Every term is positive, so sum |term| is the loss
            itself; an addition rounds its partial sum by at most 2^-24 of it, and a term lies in `chain` partial sums: in the forward
            kernel VEC x trips additions in its lane (VEC = 4 pixels per lane when W % 4 == 0 in UNET mode, else 1; trips = how often the
            grid-stride loop runs, 1 at every size here but case_grid_stride's), 6 in the wave's xor tree, 4 across the four waves; in the
            merge kernel ceil(partials / 256) = 1 addition per thread, 6 + 4 in the workgroup tree; then the product with
            factor / (N H W), itself rounded to float32: 2.  chain() counts this from the launch arithmetic of epe.hip: 27 on the 4-pixel
            route and 24 on the one-pixel route at the sizes here.
  BAND      1e-3 px.  A pixel is AMBIGUOUS when its float64 ix (iy) lies within BAND of an integer that the clamped position can reach,
            -BAND <= ix <= W-1+BAND: a cell boundary or a clamp limit, the only places where the derivative of the bilinear read jumps and
            two float32 evaluations may take different sides (the float32 error of a position is ~1e-5 px at the sizes here).
  UNET gradient   ambiguous texels are left out; the float64 reference alone keeps them <= EXCLUDED_SHARE of all pixels (a draw that does not
            is redrawn from the next seed before the kernel is looked at, as deform_cases.case_meter redraws).  On the rest the max-abs
            error against float64 is <= MARGIN x the yardstick's on the same texels + GRAD_ULPS x 2^-24 x max |gradient64|.  The floor is
            for the closed forms, where the yardstick's error is 0: an element is k (W/2) Dx after roundings in r (2), rho (4), u (1), the
            slopes (3), Dx (3) and the two products with k and W/2 (3): 16, each at most 2^-24 of a value no larger than the largest
            gradient's factors (|u| <= 1; the slopes are differences of the g the case chose).
  AFFINE gradient   the sum cannot leave pixels out: the float64 reference is evaluated twice more, with every ambiguous pixel's cell forced
            to the lower and to the upper side (the cell and the clamp decision are taken at ix -+ BAND).  Per component
            |gpred - gpred64| <= MARGIN x yardstick + chain' x 2^-24 x sum |per-pixel contribution| + |difference of the two|.
            chain' (chain_affine): trips additions in the lane, 6 + 4 in the workgroup; ceil(records / 256) + 6 + 4 in the merge; the
            contribution's own products with W/2 and the base coordinate and the product with k: 3, and 1 for k's rounding: 26 here.
"""
import ctypes

import numpy as np
import pytest
import torch

import deform_cases as D
from backends import both_poisons
from oracle import ops_np as O
from register_cases import GRID_AFFINE, GRID_UNET, MARGIN

BAND = 1e-3
EXCLUDED_SHARE = 0.01
GRAD_ULPS = 16
MIN_CLAMPED = 0.30

#         (H, W)
ONE_PIXEL = [(35, 131), (17, 65)]              # W % 4 != 0: one pixel per lane; several workgroups per sample at the first
FOUR_PIXEL = [(40, 56), (64, 64)]              # W % 4 == 0: four pixels per lane
EDGES = [(h, 40) for h in (1, 2, 3)] + [(20, w) for w in (1, 2, 3, 4, 5, 63, 64, 65)]      # thin planes, the 4 / 1 pixel switch, W = 1 (linspace is -1)
DESCENT = [(GRID_UNET, (40, 56)), (GRID_UNET, (17, 65)), (GRID_AFFINE, (32, 32))]
GRID_STRIDE = [(2, 520, 513), (2, 520, 2052)]  # more than 2048 x 256 lane items over the batch: the loop runs twice, on either route


# ---- the launch arithmetic of csrc/epe.hip, for the reduction chains ------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def _launch(mode, N, H, W):
    """(pixels per lane, workgroups per sample, loop trips) of the forward kernel"""
    vec = 4 if (mode == GRID_UNET and W % 4 == 0) else 1
    items = H * (W // vec)
    gx = max(1, min(_cdiv(items, 256), _cdiv(256 * 8, N)))
    return vec, gx, _cdiv(items, gx * 256)


def chain(mode, N, H, W):
    vec, gx, trips = _launch(mode, N, H, W)
    return vec * trips + 6 + 4 + _cdiv(N * gx, 256) + 6 + 4 + 2


def chain_affine(N, H, W):
    _, gx, trips = _launch(GRID_AFFINE, N, H, W)
    return trips + 6 + 4 + _cdiv(gx, 256) + 6 + 4 + 4


# ---- the float64 truth, and (dtype float32) the yardstick -------------------------------------------------------------------------------
def ref_epe(pred, mode, g, eps, factor=1.0, gscale=1.0, dtype=torch.float64, shift=None):
    """include/nemar_hip.h's definition written out, the gradient by autograd.  -> dict of float64 numpy arrays / Python floats: loss,
    gpred (d (gscale loss) / d pred), gpix [N,2,H,W] (the same towards each pixel's own normalised grid coordinate: the UNET gradient,
    and what an affine prediction sums against its base coordinates), base (xb [W], yb [H]: affine_grid's), ix, iy [N,H,W], ux, uy.
    shift = (sx, sy) [N,H,W]: the cell and the clamp decision of a pixel are taken at ix + sx, iy + sy (forcing a side)."""
    npdt = np.float64 if dtype == torch.float64 else np.float32
    g = np.asarray(g)
    N, _, H, W = g.shape
    p = torch.tensor(np.asarray(pred), dtype=dtype, requires_grad=True)
    G = torch.tensor(g, dtype=dtype)
    ident = O.affine_grid(np.array([[[1, 0, 0], [0, 1, 0]]], dtype=npdt), H, W)[0]          # affine_grid's base coordinates [H,W,2]
    xs, ys = torch.from_numpy(np.ascontiguousarray(ident[..., 0])), torch.from_numpy(np.ascontiguousarray(ident[..., 1]))
    if mode == GRID_UNET:
        lin = torch.from_numpy(O.unet_identity_grid(H, W, npdt))
        grid = lin + p
    else:
        th = p + torch.tensor([1, 0, 0, 0, 1, 0], dtype=dtype)
        c = lambda i: th[:, i, None, None]
        grid = torch.stack([c(0) * xs + c(1) * ys + c(2), c(3) * xs + c(4) * ys + c(5)], dim=1)
    grid.retain_grad()
    ix, iy = ((grid[:, 0] + 1) * W - 1) / 2, ((grid[:, 1] + 1) * H - 1) / 2

    def locate(pos, size, s):
        sel = pos.detach() if s is None else pos.detach() + torch.as_tensor(s, dtype=dtype)
        inside = (sel >= 0) & (sel <= size - 1)
        c = torch.where(inside, pos, pos.detach().clamp(0, size - 1))          # the clamp passes the gradient inside, limits included
        f = sel.clamp(0, size - 1).floor()
        a = f.long()
        return a, (a + 1).clamp(max=size - 1), c - f

    xa, xb, tx = locate(ix, W, None if shift is None else shift[0])
    ya, yb, ty = locate(iy, H, None if shift is None else shift[1])
    n = torch.arange(N)[:, None, None]

    def read(c):
        P = G[:, c]
        ex, ey = 1 - tx, 1 - ty
        return P[n, ya, xa] * (ex * ey) + P[n, ya, xb] * (tx * ey) + P[n, yb, xa] * (ex * ty) + P[n, yb, xb] * (tx * ty)

    X, Y = torch.arange(W, dtype=dtype)[None, None, :], torch.arange(H, dtype=dtype)[None, :, None]
    rx, ry = (ix - X) + read(0), (iy - Y) + read(1)
    rho = torch.sqrt(rx * rx + ry * ry + eps * eps)
    loss = (factor / (N * H * W)) * rho.sum()
    assert loss.dtype == dtype
    (loss * gscale).backward()
    f64 = lambda t: t.detach().numpy().astype(np.float64)
    return {'loss': float(loss.detach()), 'gpred': f64(p.grad), 'gpix': f64(grid.grad), 'base': (f64(xs[0]), f64(ys[:, 0])),
            'ix': f64(ix), 'iy': f64(iy), 'ux': f64(rx / rho), 'uy': f64(ry / rho)}


def ambiguous(r64, H, W):
    """-> (ax, ay) [N,H,W] bool"""
    near = lambda v, size: (np.abs(v - np.round(v)) <= BAND) & (v >= -BAND) & (v <= size - 1 + BAND)
    return near(r64['ix'], W), near(r64['iy'], H)


def clamped(r64, H, W):
    """-> (x clamped, y clamped) [N,H,W] bool"""
    return (r64['ix'] < 0) | (r64['ix'] > W - 1), (r64['iy'] < 0) | (r64['iy'] > H - 1)


def affine_contributions(r, N):
    """sum |per-pixel contribution| [N,6] of a reference evaluation"""
    xb, yb = r['base']
    gx, gy = np.abs(r['gpix'][:, 0]), np.abs(r['gpix'][:, 1])
    ax, ay = np.abs(xb)[None, None, :], np.abs(yb)[None, :, None]
    return np.stack([(gx * ax).sum((1, 2)), (gx * ay).sum((1, 2)), gx.sum((1, 2)), (gy * ax).sum((1, 2)), (gy * ay).sum((1, 2)),
                     gy.sum((1, 2))], axis=1)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def draw(seed, mode, N, H, W, kind, eps):
    """-> (pred, g, r64, (ax, ay)).  kinds 'smooth' and 'fold': deform_cases._draw_meter_inputs; 'rough': its smooth prediction against white
    noise of a few pixels (the slopes of g dominate the gradient: the cell choice matters); 'leaving': a prediction large enough that
    MIN_CLAMPED of the samples clamp.  A draw whose float64 reference finds more than EXCLUDED_SHARE of the pixels ambiguous is redrawn
    from the next seed."""
    for attempt in range(8):
        rng = np.random.default_rng(seed + attempt)
        pred, g = D._draw_meter_inputs(rng, mode, N, H, W, 'fold' if kind == 'fold' else 'smooth')
        if kind == 'rough':
            g = (rng.standard_normal((N, 2, H, W)) * 3.0).astype(np.float32)
        elif kind == 'leaving':
            if mode == GRID_UNET:
                pred = D._smooth(rng, N, H, W, 3.0).astype(np.float32)              # normalised units: the image is 2 wide
            else:
                pred[:, 2] += np.where(np.arange(N) % 2 == 0, 0.9, -0.8)
                pred[:, 5] += np.where(np.arange(N) % 2 == 0, -0.7, 0.85)
        r64 = ref_epe(pred, mode, g, eps)
        ax, ay = ambiguous(r64, H, W)
        if (ax | ay).mean() <= EXCLUDED_SHARE:
            return pred, g, r64, (ax, ay)
    raise AssertionError("no draw in 8 keeps the ambiguous pixels of the float64 reference <= %g" % EXCLUDED_SHARE)


# ---- drivers ----------------------------------------------------------------------------------------------------------------------------------
def _fill_value(be):
    """what outputs hold before a call: the float the poison in force reads as (a NaN, or 1e38)"""
    return np.array([be.poison], dtype=np.uint32).view(np.float32)[0]


def _workspace(be, N, H, W):
    wsb = int(be.lib.epe_loss_workspace(N, H, W))
    return be.bytes_buf(wsb), wsb


def run_fwd(be, d_pred, mode, d_g, shape, eps, factor=1.0, accumulate=0, d_loss=None):
    """-> loss float32 on the host, bit for bit; pre-filled"""
    N, H, W = shape
    d_loss = be.full((1,), _fill_value(be)) if d_loss is None else d_loss
    ws, wsb = _workspace(be, N, H, W)
    be.lib.epe_loss_fwd(be.ptr(d_pred), mode, be.ptr(d_g), eps, factor, be.ptr(d_loss), accumulate, be.ptr(ws), wsb, N, H, W, be.stream)
    return be.raw(d_loss).view(np.float32)[0]


def run_bwd(be, d_pred, mode, d_g, shape, eps, factor=1.0, gscale=1.0, accumulate=0, d_gpred=None):
    """-> gpred float32 in the prediction's shape on the host, bit for bit; pre-filled"""
    N, H, W = shape
    pshape = (N, 2, H, W) if mode == GRID_UNET else (N, 6)
    d_gpred = be.full(pshape, _fill_value(be)) if d_gpred is None else d_gpred
    d_gs = be.dev(np.array([gscale]))
    ws, wsb = _workspace(be, N, H, W)
    be.lib.epe_loss_bwd(be.ptr(d_pred), mode, be.ptr(d_g), eps, be.ptr(d_gs), factor, be.ptr(d_gpred), accumulate, be.ptr(ws), wsb, N, H, W,
                        be.stream)
    return be.raw(d_gpred).view(np.float32).reshape(pshape)


def _what(mode, size, kind, eps, N):
    return "%s %s N=%d %s eps %g" % ("unet" if mode == GRID_UNET else "affine", size, N, kind, eps)


# ---- the three rules ----------------------------------------------------------------------------------------------------------------------------
def check_loss(loss, r64, r32, mode, N, H, W, what):
    bound_sum = chain(mode, N, H, W) * 2.0 ** -24 * r64['loss']
    bound = MARGIN * abs(r32['loss'] - r64['loss']) + bound_sum
    e = abs(float(loss) - r64['loss'])
    print("epe loss %-42s kernel %.9g  float64 %.9g  error %.3e  torch-fp32 error %.3e  bound %.3e  share of the sum bound %.3f"
          % (what, loss, r64['loss'], e, abs(r32['loss'] - r64['loss']), bound, e / bound_sum if bound_sum else 0.0))
    assert np.isfinite(loss) and e <= bound, (what, loss, r64['loss'], e, bound)


def check_unet_gradient(gpred, r64, r32, amb, what, keep=None, want=None, channel=None):
    """keep: further texels to restrict the comparison to; want: what to compare with instead of the reference's gradient (on `channel`)"""
    sel = ~amb if keep is None else (~amb & keep)
    pick = (lambda a: a[:, channel][sel]) if channel is not None else (lambda a: a[np.broadcast_to(sel[:, None], a.shape)])
    truth = pick(r64['gpred']) if want is None else want[sel]
    if truth.size == 0:
        return
    yard, err = np.abs(pick(r32['gpred']) - pick(r64['gpred'])).max(), np.abs(pick(gpred.astype(np.float64)) - truth).max()
    floor = GRAD_ULPS * 2.0 ** -24 * np.abs(r64['gpred']).max()
    print("epe gradient %-38s kernel %.3e  torch-fp32 %.3e  floor %.3e  left out %.4f" % (what, err, yard, floor, amb.mean()))
    assert err <= MARGIN * yard + floor, (what, err, yard, floor)


def check_affine_gradient(gpred, r64, r32, pred, g, eps, factor, gscale, amb_xy, N, H, W, what):
    ax, ay = amb_xy
    lo = ref_epe(pred, GRID_AFFINE, g, eps, factor, gscale, shift=(-BAND * ax, -BAND * ay))['gpred']
    hi = ref_epe(pred, GRID_AFFINE, g, eps, factor, gscale, shift=(BAND * ax, BAND * ay))['gpred']
    bound = (MARGIN * np.abs(r32['gpred'] - r64['gpred']) + chain_affine(N, H, W) * 2.0 ** -24 * affine_contributions(r64, N)
             + np.abs(hi - lo))
    err = np.abs(gpred.astype(np.float64) - r64['gpred'])
    print("epe gradient %-38s worst error / bound %.3f  (error %.3e, torch-fp32 %.3e, either side %.3e)"
          % (what, (err / np.maximum(bound, 1e-300)).max(), err.max(), np.abs(r32['gpred'] - r64['gpred']).max(), np.abs(hi - lo).max()))
    assert np.all(err <= bound), (what, err, bound)


# ---- 1. / 3. against float64 ------------------------------------------------------------------------------------------------------------------
def case_against_float64(be, mode, size, kind, eps, seed=1, N=2, factor=0.5, gscale=3.0):
    H, W = size
    what = _what(mode, size, kind, eps, N)
    pred, g, r64, (ax, ay) = draw(seed, mode, N, H, W, kind, eps)
    r64 = ref_epe(pred, mode, g, eps, factor, gscale)
    r32 = ref_epe(pred, mode, g, eps, factor, gscale, torch.float32)
    d_pred, d_g = be.dev(pred), be.dev(g)
    loss = run_fwd(be, d_pred, mode, d_g, (N, H, W), eps, factor)
    gpred = run_bwd(be, d_pred, mode, d_g, (N, H, W), eps, factor, gscale)
    assert np.all(np.isfinite(gpred)), what
    check_loss(loss, r64, r32, mode, N, H, W, what)
    if mode == GRID_UNET:
        check_unet_gradient(gpred, r64, r32, ax | ay, what)
    else:
        check_affine_gradient(gpred, r64, r32, pred, g, eps, factor, gscale, (ax, ay), N, H, W, what)
    return pred, g, r64, r32, gpred, (ax, ay)


# ---- 2. leaving the image -----------------------------------------------------------------------------------------------------------------------
def case_leaving(be, mode, size, eps=0.01, seed=1, N=2, factor=0.5, gscale=3.0):
    """where a position is clamped the read no longer depends on it: the gradient is k (W/2) u.x (k (H/2) u.y) with no slope of g in it"""
    H, W = size
    pred, g, r64, r32, gpred, (ax, ay) = case_against_float64(be, mode, size, 'leaving', eps, seed, N, factor, gscale)
    cx, cy = clamped(r64, H, W)
    share = (cx | cy).mean()
    print("epe leaving %s: %.3f of the samples clamp" % (_what(mode, size, 'leaving', eps, N), share))
    assert share >= MIN_CLAMPED, share
    k = gscale * factor / (N * H * W)
    want_x, want_y = k * (W / 2) * r64['ux'], k * (H / 2) * r64['uy']
    # the reference itself: no slope term on the clamped texels
    assert np.allclose(r64['gpix'][:, 0][cx], want_x[cx], rtol=1e-12, atol=0) and np.allclose(r64['gpix'][:, 1][cy], want_y[cy], rtol=1e-12, atol=0)
    if mode == GRID_UNET:
        check_unet_gradient(gpred, r64, r32, ax | ay, "clamped in x", keep=cx, want=want_x, channel=0)
        check_unet_gradient(gpred, r64, r32, ax | ay, "clamped in y", keep=cy, want=want_y, channel=1)


# ---- 4. closed forms --------------------------------------------------------------------------------------------------------------------------
def case_zero_residual(be, size, eps, N=2, factor=0.5, gscale=3.0):
    """AFFINE, dtheta = 0, g = 0, power-of-two sides: S(x) = x exactly, every residual is exactly 0"""
    H, W = size
    assert (H & (H - 1)) == 0 and (W & (W - 1)) == 0
    pred, g = np.zeros((N, 6), dtype=np.float32), np.zeros((N, 2, H, W), dtype=np.float32)
    r64, r32 = ref_epe(pred, GRID_AFFINE, g, eps, factor, gscale), ref_epe(pred, GRID_AFFINE, g, eps, factor, gscale, torch.float32)
    assert abs(r64['loss'] - factor * eps) <= 1e-15 and np.all(r64['gpred'] == 0)
    d_pred, d_g = be.dev(pred), be.dev(g)
    check_loss(run_fwd(be, d_pred, GRID_AFFINE, d_g, (N, H, W), eps, factor), r64, r32, GRID_AFFINE, N, H, W, "zero residual %s" % (size,))
    assert np.all(run_bwd(be, d_pred, GRID_AFFINE, d_g, (N, H, W), eps, factor, gscale) == 0), "a zero residual has a zero gradient, exactly"


def case_translation(be, size, t=(3.0, -2.0), eps=0.01, N=2, factor=0.5, gscale=3.0):
    """g a constant translation t, dtheta = 0: no sample clamps, loss = factor sqrt(|t|^2 + eps^2), and the translation components of the
    gradient are k (W/2) H W t.x / rho and the y analogue"""
    H, W = size
    assert (H & (H - 1)) == 0 and (W & (W - 1)) == 0
    pred, g = np.zeros((N, 6), dtype=np.float32), np.empty((N, 2, H, W), dtype=np.float32)
    g[:, 0], g[:, 1] = t
    r64, r32 = ref_epe(pred, GRID_AFFINE, g, eps, factor, gscale), ref_epe(pred, GRID_AFFINE, g, eps, factor, gscale, torch.float32)
    assert not np.any(clamped(r64, H, W))
    rho = np.sqrt(t[0] ** 2 + t[1] ** 2 + eps ** 2)
    k = gscale * factor / (N * H * W)
    assert abs(r64['loss'] - factor * rho) <= 1e-12 * rho
    assert np.allclose(r64['gpred'][:, 2], k * (W / 2) * H * W * t[0] / rho, rtol=1e-12) and np.allclose(r64['gpred'][:, 5], k * (H / 2) * H * W * t[1] / rho, rtol=1e-12)
    d_pred, d_g = be.dev(pred), be.dev(g)
    what = "translation %s" % (size,)
    check_loss(run_fwd(be, d_pred, GRID_AFFINE, d_g, (N, H, W), eps, factor), r64, r32, GRID_AFFINE, N, H, W, what)
    gpred = run_bwd(be, d_pred, GRID_AFFINE, d_g, (N, H, W), eps, factor, gscale)
    # (every position is an integer, so every pixel is ambiguous — and g is constant: the two sides give the same gradient)
    check_affine_gradient(gpred, r64, r32, pred, g, eps, factor, gscale, ambiguous(r64, H, W), N, H, W, what)


# ---- 5. descent -----------------------------------------------------------------------------------------------------------------------------
DESCENT_STEPS, DESCENT_LR, DESCENT_BOUND = 120, 0.01, 0.1


def descent_inputs(mode, size, N=2, seed=3):
    """-> (a zero prediction, g): a smooth field; for an affine prediction an affine one, which it can undo"""
    H, W = size
    pred, g = D._draw_meter_inputs(np.random.default_rng(seed), mode, N, H, W, 'smooth')
    if mode == GRID_AFFINE:
        p = np.array([[1.03, 0.05, 2.5, -0.04, 0.97, -1.5], [0.98, -0.03, -2.0, 0.06, 1.02, 1.0]], dtype=np.float32)
        g = D.ref_field(p, N, H, W, 0, 0).astype(np.float32)
    return np.zeros_like(pred), g


def descend(loss_and_grad, pred0, pixels):
    """Adam (0.9, 0.999, 1e-8) on the prediction from pred0 for DESCENT_STEPS steps, lr DESCENT_LR, halved after 80 steps and x 0.2 after
    100; the gradient is taken of the sum (x pixels), so that Adam's epsilon does not matter.  -> (first loss, last loss)"""
    p = pred0.astype(np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    first = None
    for t in range(1, DESCENT_STEPS + 1):
        loss, gr = loss_and_grad(p.astype(np.float32))
        first = loss if first is None else first
        gr = gr.astype(np.float64) * pixels
        m, v = 0.9 * m + 0.1 * gr, 0.999 * v + 0.001 * gr * gr
        lr = DESCENT_LR * (0.5 if t > 80 else 1.0) * (0.2 if t > 100 else 1.0)
        p = p - lr * (m / (1 - 0.9 ** t)) / (np.sqrt(v / (1 - 0.999 ** t)) + 1e-8)
    return float(first), float(loss_and_grad(p.astype(np.float32))[0])


def case_descent(mode, size, kernel_loss_and_grad, eps=0.01, N=2):
    """the sign and the scale of the whole gradient, no network: the reference's own descent meets the bound before the kernel is judged"""
    H, W = size
    pred0, g = descent_inputs(mode, size, N)

    def reference(p):
        r = ref_epe(p, mode, g, eps)
        return r['loss'], r['gpred']
    first64, last64 = descend(reference, pred0, N * H * W)
    print("epe descent %s: float64 reference %.4f -> %.4f (%.4f of the start)" % (_what(mode, size, 'descent', eps, N), first64, last64, last64 / first64))
    assert last64 <= DESCENT_BOUND * first64, (first64, last64)
    first, last = descend(lambda p: kernel_loss_and_grad(p, g), pred0, N * H * W)
    print("epe descent %s: kernel %.4f -> %.4f (%.4f of the start)" % (_what(mode, size, 'descent', eps, N), first, last, last / first))
    assert np.isfinite(last) and last <= DESCENT_BOUND * first, (first, last)


def entry_point_loss_and_grad(be, mode, size, eps=0.01, N=2):
    H, W = size

    def f(p, g):
        d_pred, d_g = be.dev(p), be.dev(g)
        return run_fwd(be, d_pred, mode, d_g, (N, H, W), eps), run_bwd(be, d_pred, mode, d_g, (N, H, W), eps)
    return f


# ---- 6. repeatable, overwritten, unaligned, accumulated --------------------------------------------------------------------------------------
def _off_by_4_bytes(be, a):
    """`a` in a buffer that starts 4 bytes past a 16-byte boundary (a view of a guarded block one element longer)"""
    d_buf = be.dev(np.concatenate([[0], np.asarray(a, dtype=np.float32).ravel()]))
    return be.sub(d_buf, 1, d_buf.shape[0])


@both_poisons
def case_repeatable_unaligned_accumulate(be, mode, size, N=2, seed=3, eps=0.01):
    H, W = size
    shape = (N, H, W)
    pred, g = D._draw_meter_inputs(np.random.default_rng(seed), mode, N, H, W, 'smooth')
    d_pred, d_g = be.dev(pred), be.dev(g)
    bits = lambda a: np.asarray(a).view(np.uint32)
    fill = _fill_value(be)
    loss, gpred = run_fwd(be, d_pred, mode, d_g, shape, eps, 0.5), run_bwd(be, d_pred, mode, d_g, shape, eps, 0.5, 3.0)
    # (the outputs were pre-filled with the poison in force: an element that was not written would show — as a NaN, or as 1e38)
    assert np.isfinite(loss) and np.all(np.isfinite(gpred)) and not np.any(gpred == fill) and loss != fill, "an output element was not written"
    assert loss > 0 and np.any(gpred != 0)
    loss2, gpred2 = run_fwd(be, d_pred, mode, d_g, shape, eps, 0.5), run_bwd(be, d_pred, mode, d_g, shape, eps, 0.5, 3.0)
    assert bits(loss) == bits(loss2) and np.array_equal(bits(gpred), bits(gpred2)), "two calls, different bits"
    # every tensor 4 bytes off the 16-byte grid
    o_pred, o_g = _off_by_4_bytes(be, pred), _off_by_4_bytes(be, g)
    loss3 = run_fwd(be, o_pred, mode, o_g, shape, eps, 0.5, d_loss=_off_by_4_bytes(be, [fill]))
    gpred3 = run_bwd(be, o_pred, mode, o_g, shape, eps, 0.5, 3.0, d_gpred=_off_by_4_bytes(be, np.full(pred.shape, fill)))
    assert bits(loss) == bits(loss3) and np.array_equal(bits(gpred), bits(gpred3.reshape(pred.shape))), "views 4 bytes off the 16-byte grid: different bits"
    # the accumulate flags add to what was there (one float32 addition)
    loss4 = run_fwd(be, d_pred, mode, d_g, shape, eps, 0.5, accumulate=1, d_loss=be.full((1,), 2.5))
    assert bits(loss4) == bits(np.float32(2.5) + loss)
    before = np.random.default_rng(seed).standard_normal(pred.shape).astype(np.float32)
    gpred4 = run_bwd(be, d_pred, mode, d_g, shape, eps, 0.5, 3.0, accumulate=1, d_gpred=be.dev(before))
    assert np.array_equal(bits(gpred4), bits(before + gpred)), "accumulate: gpred is not what was there plus the gradient"


def case_grid_stride(be, N, H, W, mode=GRID_UNET, eps=0.01, seed=2):
    """a size at which the launch's workgroup cap makes the grid-stride loop run more than once"""
    vec, gx, trips = _launch(mode, N, H, W)
    assert trips > 1 and gx == _cdiv(256 * 8, N)
    rng = np.random.default_rng(seed)
    pred = (rng.standard_normal((N, 2, H, W)) * (3.0 / max(H, W))).astype(np.float32)      # rough offsets of ~1.5 px, as the meter's 'fold' kind
    g = (rng.standard_normal((N, 2, H, W)) * 2.0).astype(np.float32)
    what = _what(mode, (H, W), 'grid-stride', eps, N)
    r64, r32 = ref_epe(pred, mode, g, eps), ref_epe(pred, mode, g, eps, dtype=torch.float32)
    ax, ay = ambiguous(r64, H, W)
    assert (ax | ay).mean() <= EXCLUDED_SHARE
    d_pred, d_g = be.dev(pred), be.dev(g)
    check_loss(run_fwd(be, d_pred, mode, d_g, (N, H, W), eps), r64, r32, mode, N, H, W, what)
    check_unet_gradient(run_bwd(be, d_pred, mode, d_g, (N, H, W), eps), r64, r32, ax | ay, what)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------
def case_refusals(be):
    """NEMAR_EINVAL (-1), a message, and nothing launched: the outputs keep their fill"""
    from nemar_amd._lib import NemarHipError
    N, H, W = 2, 12, 16
    d_pred, d_th, d_g, d_gs = be.zeros(N, 2, H, W), be.zeros(N, 6), be.zeros(N, 2, H, W), be.dev(np.array([1.0]))
    d_loss, d_gpred, d_gth = be.full((1,), 7.0), be.full((N, 2, H, W), 7.0), be.full((N, 6), 7.0)
    wsb = int(be.lib.epe_loss_workspace(N, H, W))
    assert wsb > 0 and int(be.lib.epe_loss_workspace(N, H, 0)) == 0 and int(be.lib.epe_loss_workspace(0, H, W)) == 0
    ws = be.bytes_buf(wsb + 4)
    off2 = lambda p: ctypes.c_void_p(p.value + 2)
    f_names = ("pred", "mode", "g", "eps", "factor", "loss", "acc", "ws", "wsb", "N", "H", "W")
    b_names = ("pred", "mode", "g", "eps", "gscale", "factor", "gpred", "acc", "ws", "wsb", "N", "H", "W")

    def good(which, mode):
        p, gp = (d_pred, d_gpred) if mode == GRID_UNET else (d_th, d_gth)
        if which == "fwd":
            return [be.ptr(p), mode, be.ptr(d_g), 0.01, 1.0, be.ptr(d_loss), 0, be.ptr(ws), wsb, N, H, W]
        return [be.ptr(p), mode, be.ptr(d_g), 0.01, be.ptr(d_gs), 1.0, be.ptr(gp), 0, be.ptr(ws), wsb, N, H, W]

    def refused(which, layout, **change):
        names, fn = (f_names, be.lib.epe_loss_fwd) if which == "fwd" else (b_names, be.lib.epe_loss_bwd)
        args = [change.get(k, v) for k, v in zip(names, good(which, layout))]
        with pytest.raises(NemarHipError, match=r"failed \(-1\): epe_loss_%s: \S" % which):
            fn(*args, be.stream)

    for mode in (GRID_UNET, GRID_AFFINE):
        for which, names, ptrs in (("fwd", f_names, ("pred", "g", "loss", "ws")), ("bwd", b_names, ("pred", "g", "gscale", "gpred", "ws"))):
            for k in ptrs:                                            # pointers: null, not even 4-byte aligned
                refused(which, mode, **{k: None})
                refused(which, mode, **{k: off2(good(which, mode)[names.index(k)])})
            for bad in (0, 3, -1):                                    # EXPLICIT is not a prediction layout; 3 and -1 are no modes at all
                refused(which, mode, mode=bad)
            for k in ("N", "H", "W"):                                 # non-positive sizes
                refused(which, mode, **{k: 0})
                refused(which, mode, **{k: -3})
            refused(which, mode, N=65536)
            refused(which, mode, H=1 << 16, W=1 << 15)                # H * W = 2^31
            refused(which, mode, wsb=wsb - 1)                         # a short workspace
            refused(which, mode, wsb=0)
            for eps in (-0.01, float('inf'), float('nan')):
                refused(which, mode, eps=eps)
        refused("bwd", mode, gpred=good("bwd", mode)[0])              # gpred is the prediction
    be.sync()
    assert np.all(be.np(d_loss) == 7.0) and np.all(be.np(d_gpred) == 7.0) and np.all(be.np(d_gth) == 7.0)
    # and the good arguments are good (eps = 0 included, which the entry points accept)
    for mode in (GRID_UNET, GRID_AFFINE):
        be.lib.epe_loss_fwd(*good("fwd", mode), be.stream)
        assert np.isfinite(be.np(d_loss)[0]) and be.np(d_loss)[0] != 7.0
        be.lib.epe_loss_bwd(*good("bwd", mode), be.stream)
    assert np.all(np.isfinite(be.np(d_gpred))) and np.all(np.isfinite(be.np(d_gth))) and not np.any(be.np(d_gpred) == 7.0)
    args = good("fwd", GRID_UNET)
    args[f_names.index("eps")] = 0.0
    be.lib.epe_loss_fwd(*args, be.stream)
    assert np.isfinite(be.np(d_loss)[0])


# ---- 8. non-finite input ----------------------------------------------------------------------------------------------------------------------
def _hears(r64, n, y, x, H, W, reach):
    """[H,W] bool: the pixels of sample n whose clamped float64 position lies within `reach` of texel (y, x) in both axes — the read's
    four corners hold the texel exactly when the clamped position is in (x - 1, x + 1) x (y - 1, y + 1)"""
    cx, cy = np.clip(r64['ix'][n], 0, W - 1), np.clip(r64['iy'][n], 0, H - 1)
    return (np.abs(cx - x) < reach) & (np.abs(cy - y) < reach)


def case_non_finite(be, mode, size, N=2, seed=1, eps=0.01):
    """NEMAR_OK, guard bands intact (the backend checks them after every call), non-finite values only where they must be — and every other
    gradient element keeps the clean call's bits"""
    H, W = size
    shape = (N, H, W)
    pred, g, r64, _ = draw(seed, mode, N, H, W, 'smooth', eps)
    d_g = be.dev(g)
    clean = run_bwd(be, be.dev(pred), mode, d_g, shape, eps)
    bits = lambda a: np.asarray(a).view(np.uint32)
    n, y, x = 1, H // 2, W // 3
    for bad in (np.nan, np.inf):                                     # in the prediction
        p = pred.copy()
        if mode == GRID_UNET:
            p[n, 0, y, x] = bad
        else:
            p[n, 4] = bad
        d_p = be.dev(p)
        assert not np.isfinite(run_fwd(be, d_p, mode, d_g, shape, eps)), "the loss hears from every pixel"
        got = run_bwd(be, d_p, mode, d_g, shape, eps)
        if mode == GRID_UNET:
            must = np.zeros((N, 2, H, W), dtype=bool)
            must[n, :, y, x] = True
        else:
            must = np.zeros((N, 6), dtype=bool)
            must[n] = True
        assert not np.any(np.isfinite(got[must])), (bad, got[must])
        assert np.array_equal(bits(got[~must]), bits(clean[~must])), "a non-finite prediction value reached an element that does not hear from it"
    gb = g.copy()                                                    # in the field
    gb[n, 1, y, x] = np.nan
    d_gb = be.dev(gb)
    d_p = be.dev(pred)
    assert not np.isfinite(run_fwd(be, d_p, mode, d_gb, shape, eps))
    got = run_bwd(be, d_p, mode, d_gb, shape, eps)
    if mode == GRID_UNET:
        surely, maybe = _hears(r64, n, y, x, H, W, 1 - BAND), _hears(r64, n, y, x, H, W, 1 + BAND)
        assert surely.sum() > 0, "no pixel reads the texel: the case would show nothing"
        bad_px = ~np.isfinite(got).all(axis=1)                       # [N,H,W]
        assert np.all(bad_px[n][surely]) and not np.any(bad_px[n][~maybe]) and not np.any(np.delete(bad_px, n, axis=0))
        same = np.broadcast_to(~bad_px[:, None] & ~np.pad(maybe[None], ((n, N - 1 - n), (0, 0), (0, 0)))[:, None], got.shape)
        assert np.array_equal(bits(got[same]), bits(clean[same]))
    else:
        assert not np.any(np.isfinite(got[n])) and np.array_equal(bits(np.delete(got, n, axis=0)), bits(np.delete(clean, n, axis=0)))
