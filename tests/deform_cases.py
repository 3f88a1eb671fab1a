"""Backend-agnostic test bodies of the known-misalignment entry points (nemar_deform_field, nemar_crop_flip_deform_normalize,
nemar_registration_error: csrc/deform.hip), driven through tests/backends.py (EmuBackend: host-emulated kernels, CPU tier; HipBackend:
the gfx950 library, `-m gpu` tier) and compared with the float64 numpy restatements written here.

Conventions (include/nemar_hip.h): pixel coordinates, integer values at pixel centres; a field g is [B,2,H,W] in pixels, channel 0 = x;
A'(q) = A_crop(q + g(q)); the meter's residual is r(x) = S(x) + g(S(x)) - x with S(x) the warp kernel's sampling position."""
import numpy as np
import pytest

from kernel_cases import _assert_close
from oracle import ops_np as O

GRID_UNET, GRID_AFFINE = 1, 2
FIELD_TOL = 16 * 2.0 ** -24        # x max(Hc, Wc) pixels: ~20 fp32 operations on values bounded by the image side
MARGIN = 1e-3                      # the float64 restatement keeps S(x) / the determinant this far from the counts' discontinuities


# ---- float64 restatements ---------------------------------------------------------------------------------------------------------------
def _bspline(t):
    t2, t3, u = t * t, t * t * t, 1.0 - t
    return np.stack([u * u * u / 6.0, (3 * t3 - 6 * t2 + 4) / 6.0, (-3 * t3 + 3 * t2 + 3 * t + 1) / 6.0, t3 / 6.0])


def _segments(size, gn):
    i = np.arange(size, dtype=np.float64)
    u = i * (gn - 3) / (size - 1) if size > 1 else np.zeros(size)
    j = np.minimum(np.floor(u), gn - 4).astype(np.int64)
    return j, _bspline(u - j)                       # [size], [4, size]


def ref_field(params, B, Hc, Wc, gh, gw):
    p = np.asarray(params, dtype=np.float64).reshape(B, -1)
    x, y = np.meshgrid(np.arange(Wc, dtype=np.float64) - (Wc - 1) / 2.0, np.arange(Hc, dtype=np.float64) - (Hc - 1) / 2.0)
    g = np.empty((B, 2, Hc, Wc))
    for b in range(B):
        a11, a12, tx, a21, a22, ty = p[b, :6]
        g[b, 0] = (a11 - 1.0) * x + a12 * y + tx
        g[b, 1] = a21 * x + (a22 - 1.0) * y + ty
        if gh:
            lat = p[b, 6:].reshape(2, gh, gw)
            jy, wy = _segments(Hc, gh)
            jx, wx = _segments(Wc, gw)
            for c in range(2):
                e = np.zeros((Hc, Wc))
                for a in range(4):
                    for k in range(4):
                        e += wy[a][:, None] * wx[k][None, :] * lat[c][(jy + a)[:, None], (jx + k)[None, :]]
                g[b, c] += e
    return g


def _bilinear_clamped(img, px, py):
    """img [..., H, W] read at (px, py) [H', W'] with the position clamped into the image"""
    H, W = img.shape[-2:]
    cx, cy = np.clip(px, 0, W - 1), np.clip(py, 0, H - 1)
    xa, ya = np.floor(cx).astype(np.int64), np.floor(cy).astype(np.int64)
    xb, yb = np.minimum(xa + 1, W - 1), np.minimum(ya + 1, H - 1)
    tx, ty = cx - xa, cy - ya
    return (img[..., ya, xa] * (1 - tx) * (1 - ty) + img[..., ya, xb] * tx * (1 - ty) + img[..., yb, xa] * (1 - tx) * ty +
            img[..., yb, xb] * tx * ty)


def ref_sample(pool, crop_params, g, Hc, Wc, scale):
    pool, g = np.asarray(pool, dtype=np.float64), np.asarray(g, dtype=np.float64)
    X, Y = np.meshgrid(np.arange(Wc, dtype=np.float64), np.arange(Hc, dtype=np.float64))
    out = np.empty((len(crop_params), pool.shape[1], Hc, Wc))
    for b, (idx, y0, x0, flip) in enumerate(crop_params):
        crop = pool[idx, :, y0:y0 + Hc, x0:x0 + Wc]
        if flip:
            crop = crop[:, :, ::-1]
        out[b] = (_bilinear_clamped(crop, X + g[b, 0], Y + g[b, 1]) * scale - 0.5) / 0.5
    return out


def ref_positions(pred, mode, H, W):
    """S(x) in pixels, [N,H,W] each, from the oracle's own grids"""
    pred = np.asarray(pred, dtype=np.float64)
    grid = O.unet_grid(pred) if mode == GRID_UNET else O.affine_grid(O.affine_theta(pred), H, W)
    return ((grid[..., 0] + 1) * W - 1) / 2, ((grid[..., 1] + 1) * H - 1) / 2


def ref_meter(pred, mode, g):
    """-> rows [N,6] (valid_count, sum|r|, max|r|, sum|g|, fold_count, interior_count), margin of the validity test, margin of the determinants"""
    g = np.asarray(g, dtype=np.float64)
    N, _, H, W = g.shape
    sx, sy = ref_positions(pred, mode, H, W)
    X, Y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rows = np.zeros((N, 6))
    m_valid, m_det = np.inf, np.inf
    for n in range(N):
        valid = (sx[n] >= 0) & (sx[n] <= W - 1) & (sy[n] >= 0) & (sy[n] <= H - 1)
        m_valid = min(m_valid, np.min(np.abs(np.stack([sx[n], sx[n] - (W - 1), sy[n], sy[n] - (H - 1)]))))
        gs = _bilinear_clamped(g[n], sx[n], sy[n])
        r = np.hypot(sx[n] + gs[0] - X, sy[n] + gs[1] - Y)
        det = ((sx[n][:-1, 1:] - sx[n][:-1, :-1]) * (sy[n][1:, :-1] - sy[n][:-1, :-1]) -
               (sx[n][1:, :-1] - sx[n][:-1, :-1]) * (sy[n][:-1, 1:] - sy[n][:-1, :-1]))
        if det.size:
            m_det = min(m_det, np.min(np.abs(det)))
        rows[n] = (valid.sum(), r[valid].sum(), r[valid].max() if valid.any() else 0.0, np.hypot(g[n, 0], g[n, 1]).sum(),
                   (det <= 0).sum(), det.size)
    return rows, m_valid, m_det


# ---- drivers ------------------------------------------------------------------------------------------------------------------------------
def run_field(be, params, B, Hc, Wc, gh, gw):
    d_g = be.full((B, 2, Hc, Wc), np.nan)
    d_p = be.dev(params)
    be.lib.deform_field(be.ptr(d_p), be.ptr(d_g), B, Hc, Wc, gh, gw, be.stream)
    return d_g


def run_sample(be, d_pool, d_par, d_g, shape, scale=1.0):
    M, B, C, H, W, Hc, Wc = shape
    d_y = be.full((B, C, Hc, Wc), np.nan)
    be.lib.crop_flip_deform_normalize(be.ptr(d_pool), be.ptr(d_par), be.ptr(d_g), be.ptr(d_y), M, B, C, H, W, Hc, Wc, scale, be.stream)
    return d_y


def run_meter(be, d_pred, mode, d_g, N, H, W, ws=None):
    wsb = int(be.lib.registration_error_workspace(N, H, W))
    ws = be.bytes_buf(wsb) if ws is None else ws
    d_out = be.full((N, 6), np.nan)
    be.lib.registration_error(be.ptr(d_pred), mode, be.ptr(d_g), be.ptr(d_out), be.ptr(ws), wsb, N, H, W, be.stream)
    return d_out


def draw_params(rng, B, Hc, Wc, gh, gw, affine=True, lattice=True):
    """parameter rows whose displacements stay below the image side (what the field tolerance assumes)"""
    side = max(Hc, Wc)
    p = np.zeros((B, 6 + 2 * gh * gw), dtype=np.float32)
    p[:, 0] = p[:, 4] = 1.0
    if affine:
        th, sc = rng.uniform(-0.15, 0.15, B), 1.0 + rng.uniform(-0.1, 0.1, B)
        p[:, 0], p[:, 1], p[:, 3], p[:, 4] = sc * np.cos(th), -sc * np.sin(th), sc * np.sin(th), sc * np.cos(th)
        p[:, 2], p[:, 5] = rng.uniform(-0.2 * side, 0.2 * side, B), rng.uniform(-0.2 * side, 0.2 * side, B)
    if lattice and gh:
        p[:, 6:] = rng.uniform(-0.25 * side, 0.25 * side, (B, 2 * gh * gw))
    return p


# ---- 1. field ---------------------------------------------------------------------------------------------------------------------------------
def case_field(be, Hc, Wc, gh, gw, affine=True, lattice=True, B=3, seed=0):
    rng = np.random.default_rng(seed)
    p = draw_params(rng, B, Hc, Wc, gh, gw, affine, lattice)
    got = be.np(run_field(be, p, B, Hc, Wc, gh, gw))
    _assert_close(got, ref_field(p, B, Hc, Wc, gh, gw), atol=FIELD_TOL * max(Hc, Wc), what="deform_field %dx%d lattice %dx%d" % (Hc, Wc, gh, gw))


def case_field_identities(be, Hc, Wc, gh, gw):
    p = draw_params(np.random.default_rng(0), 2, Hc, Wc, gh, gw, affine=False, lattice=False)
    assert np.all(be.np(run_field(be, p, 2, Hc, Wc, gh, gw)) == 0.0)            # identity, zero translation, zero lattice: exactly 0
    if gh:
        const = np.array([0.37 * max(Hc, Wc), -0.21 * max(Hc, Wc)])
        p[:, 6:] = np.repeat(const, gh * gw)[None, :]
        got = be.np(run_field(be, p, 2, Hc, Wc, gh, gw))
        want = np.broadcast_to(p[0, 6::gh * gw].astype(np.float64)[None, :, None, None], got.shape)
        _assert_close(got, want, atol=FIELD_TOL * max(Hc, Wc), what="constant lattice (partition of unity)")


# ---- 2. sampling ------------------------------------------------------------------------------------------------------------------------------
def case_sample(be, C, H, W, Hc, Wc, amplitude, seed=0, M=3, unaligned=False):
    """crops at the pool's corners (both flips) and a random one; `amplitude` x the crop side bounds the field (1.5: everything clamps)"""
    rng = np.random.default_rng(seed)
    pool = rng.random((M, C, H, W)).astype(np.float32)
    par = np.array([(0, 0, 0, 0), (M - 1, H - Hc, W - Wc, 1), (1, 0, W - Wc, 1), (1, H - Hc, 0, 0),
                    (rng.integers(M), rng.integers(H - Hc + 1), rng.integers(W - Wc + 1), 1)], dtype=np.int32)
    B = len(par)
    g = (rng.uniform(-1, 1, (B, 2, Hc, Wc)) * amplitude * max(Hc, Wc)).astype(np.float32)
    g[0, :, :2] = 0.0                                      # some pixels exactly on their own texel
    d_pool, d_par = be.dev(pool), be.dev_i32(par)
    if unaligned:                                          # a field 4 bytes off a 16-byte boundary: the scalar route must serve it
        d_buf = be.dev(np.concatenate([[0.0], g.ravel()]))
        d_g = d_buf[1:]
    else:
        d_g = be.dev(g)
    got = be.np(run_sample(be, d_pool, d_par, d_g, (M, B, C, H, W, Hc, Wc)))
    _assert_close(got, ref_sample(pool, par, g, Hc, Wc, 1.0), atol=4e-6 * max(H, W, 16), what="crop_flip_deform_normalize")
    # g == 0: nemar_crop_flip_normalize's output, bit for bit
    d_zero = be.zeros(B, 2, Hc, Wc)
    d_y0 = run_sample(be, d_pool, d_par, d_zero, (M, B, C, H, W, Hc, Wc))
    d_plain = be.full((B, C, Hc, Wc), np.nan)
    be.lib.crop_flip_normalize(be.ptr(d_pool), be.ptr(d_par), be.ptr(d_plain), M, B, C, H, W, Hc, Wc, 1.0, be.stream)
    assert np.array_equal(be.raw(d_y0), be.raw(d_plain)), "g == 0 must reproduce crop_flip_normalize bitwise"


# ---- 3. meter ---------------------------------------------------------------------------------------------------------------------------------
def _smooth(rng, N, H, W, amp):
    """a smooth 2-channel field of amplitude ~amp: a few random low-frequency waves"""
    X, Y = np.meshgrid(np.arange(W) / max(W - 1, 1), np.arange(H) / max(H - 1, 1))
    f = np.zeros((N, 2, H, W))
    for n in range(N):
        for c in range(2):
            for _ in range(3):
                kx, ky, ph = rng.uniform(0.5, 2.5), rng.uniform(0.5, 2.5), rng.uniform(0, 6.28)
                f[n, c] += rng.uniform(-1, 1) * np.sin(6.28 * (kx * X + ky * Y) + ph)
    return f * (amp / 3.0)


def _draw_meter_inputs(rng, mode, N, H, W, kind):
    g = _smooth(rng, N, H, W, 0.08 * max(H, W)).astype(np.float32)
    if mode == GRID_AFFINE:
        pred = (rng.uniform(-1, 1, (N, 6)) * 0.12).astype(np.float32)
        if kind == "fold":                                 # a reflection in x: every determinant is negative
            pred[:, 0] -= 2.0
    elif kind == "fold":                                   # rough offsets of ~1.5 px: the sampling positions cross
        pred = (rng.standard_normal((N, 2, H, W)) * (3.0 / max(H, W))).astype(np.float32)
    else:                                                  # smooth offsets of a few pixels (normalised units: 2 / side per pixel)
        pred = (_smooth(rng, N, H, W, 0.04 * max(H, W)) * np.array([2.0 / W, 2.0 / H])[None, :, None, None]).astype(np.float32)
    return pred, g


def check_meter(got, want, pixels, what):
    """counts exactly; the sums as count-normalised values (what smoothness_fwd is held to: rtol 2e-5, atol 1e-6); the maximum rtol 1e-5"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    for col, name in ((0, "valid_count"), (4, "fold_count"), (5, "interior_count")):
        assert np.array_equal(got[:, col], want[:, col]), (what, name, got[:, col], want[:, col])
    nv = np.maximum(want[:, 0], 1.0)
    _assert_close(got[:, 1] / nv, want[:, 1] / nv, atol=1e-6, rtol=2e-5, what=what + " sum|r| / valid")
    _assert_close(got[:, 3] / pixels, want[:, 3] / pixels, atol=1e-6, rtol=2e-5, what=what + " sum|g| / pixels")
    _assert_close(got[:, 2], want[:, 2], atol=0.0, rtol=1e-5, what=what + " max|r|")


def case_meter(be, mode, N, H, W, kind="smooth", seed=0):
    """kind 'smooth': no folds; 'fold': a prediction with real folds (fold fraction > 5 %)"""
    for attempt in range(8):                               # a draw that lands within MARGIN of a discontinuity is redrawn from the next seed
        pred, g = _draw_meter_inputs(np.random.default_rng(seed + attempt), mode, N, H, W, kind)
        want, m_valid, m_det = ref_meter(pred, mode, g)
        if m_valid >= MARGIN and m_det >= MARGIN:
            break
    else:
        raise AssertionError("no draw in 8 keeps the float64 positions / determinants %g away from the counts' discontinuities" % MARGIN)
    assert m_valid >= MARGIN and m_det >= MARGIN
    fold_frac = want[:, 4].sum() / max(want[:, 5].sum(), 1.0)
    assert fold_frac > 0.05 if kind == "fold" else fold_frac == 0.0, fold_frac
    got = be.np(run_meter(be, be.dev(pred), mode, be.dev(g), N, H, W))
    check_meter(got, want, H * W, "registration_error mode %d %s %dx%d" % (mode, kind, H, W))


def case_meter_identity(be, H, W):
    """pred identity, g == 0.  Affine mode: S(x) = x and every residual is 0 — exactly, at power-of-two sides, where (2i + 1) / n - 1 and
    the unnormalisation are exact in fp32.  UNet mode: the reference's linspace identity stretches, |r| = |x W/(W-1) - 0.5 - x| per axis."""
    N = 2
    d_g = be.zeros(N, 2, H, W)
    got = be.np(run_meter(be, be.zeros(N, 6), GRID_AFFINE, d_g, N, H, W))
    assert (H & (H - 1)) == 0 and (W & (W - 1)) == 0
    assert np.array_equal(got, np.tile([H * W, 0.0, 0.0, 0.0, 0.0, (H - 1) * (W - 1)], (N, 1))), got
    pred = np.zeros((N, 2, H, W), dtype=np.float32)
    want, m_valid, m_det = ref_meter(pred, GRID_UNET, np.zeros((N, 2, H, W)))
    assert m_valid >= MARGIN and m_det >= MARGIN
    x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    rx, ry = x * W / (W - 1) - 0.5 - x, y * H / (H - 1) - 0.5 - y
    sx, sy = x + rx, y + ry
    ok = ((sy >= 0) & (sy <= H - 1))[:, None] & ((sx >= 0) & (sx <= W - 1))[None, :]
    r = np.hypot(rx[None, :], ry[:, None])
    assert want[0, 0] == ok.sum() and abs(want[0, 1] - r[ok].sum()) < 1e-9 * r[ok].sum()          # the restatement is the closed form
    check_meter(be.np(run_meter(be, be.dev(pred), GRID_UNET, d_g, N, H, W)), want, H * W, "identity, UNet mode")


def case_meter_inverse_translation(be, H, W, shift=(3.5, -2.5)):
    """g a pure translation, dtheta its exact inverse: mean residual <= 1e-4 px, valid_count = the overlap area in closed form"""
    N = 2
    g = np.empty((N, 2, H, W), dtype=np.float32)
    g[:, 0], g[:, 1] = shift
    dtheta = np.zeros((N, 6), dtype=np.float32)
    dtheta[:, 2], dtheta[:, 5] = -2.0 * shift[0] / W, -2.0 * shift[1] / H                         # S(x) = x - shift
    want, m_valid, m_det = ref_meter(dtheta, GRID_AFFINE, g)
    assert m_valid >= MARGIN and m_det >= MARGIN
    area = (W - int(np.ceil(abs(shift[0])))) * (H - int(np.ceil(abs(shift[1]))))
    assert want[0, 0] == area
    got = be.np(run_meter(be, be.dev(dtheta), GRID_AFFINE, be.dev(g), N, H, W))
    assert np.all(got[:, 0] == area), (got[:, 0], area)
    assert np.all(got[:, 1] / got[:, 0] <= 1e-4), got[:, 1] / got[:, 0]
    _assert_close(got[:, 3] / (H * W), np.full(N, np.hypot(*shift)), atol=1e-6, rtol=2e-5, what="error before registration")


# ---- 4. repeatability ---------------------------------------------------------------------------------------------------------------------------
def case_repeatable(be, H=24, W=20, seed=5):
    rng = np.random.default_rng(seed)
    N, gh = 3, 5
    p = draw_params(rng, N, H, W, gh, gh)
    f1, f2 = run_field(be, p, N, H, W, gh, gh), run_field(be, p, N, H, W, gh, gh)
    assert np.array_equal(be.raw(f1), be.raw(f2))
    pool = rng.random((2, 3, H + 3, W + 5)).astype(np.float32)
    par = np.array([(0, 1, 2, 0), (1, 3, 5, 1), (1, 0, 0, 1)], dtype=np.int32)
    shape = (2, N, 3, H + 3, W + 5, H, W)
    d_pool, d_par = be.dev(pool), be.dev_i32(par)
    assert np.array_equal(be.raw(run_sample(be, d_pool, d_par, f1, shape)), be.raw(run_sample(be, d_pool, d_par, f2, shape)))
    for mode in (GRID_UNET, GRID_AFFINE):
        pred, _ = _draw_meter_inputs(rng, mode, N, H, W, "smooth")
        d_pred = be.dev(pred)
        wsb = max(int(be.lib.registration_error_workspace(N, H, W)), int(be.lib.smoothness_workspace(N, H, W)))
        ws = be.bytes_buf(wsb)
        a = be.raw(run_meter(be, d_pred, mode, f1, N, H, W, ws=ws))
        loss = be.zeros(1)                                  # an unrelated kernel leaves its own partials in the workspace
        be.lib.smoothness_fwd(be.ptr(f1), None, 0, 0.0, 1.0, be.ptr(loss), 0, be.ptr(ws), wsb, N, H, W, be.stream)
        b = be.raw(run_meter(be, d_pred, mode, f1, N, H, W, ws=ws))
        assert np.array_equal(a, b) and np.all(np.isfinite(np.frombuffer(a.tobytes(), dtype=np.float32)))


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
def case_refusals(be):
    """NEMAR_EINVAL (-1) and nothing launched: the output buffers keep their fill"""
    from nemar_amd._lib import NemarHipError
    einval = r"failed \(-1\)"
    B, H, W = 2, 8, 8
    d_p, d_g = be.dev(np.zeros((B, 6 + 2 * 16))), be.full((B, 2, H, W), 7.0)
    for gh, gw in ((1, 4), (4, 3), (2, 2), (3, 3), (0, 4)):
        with pytest.raises(NemarHipError, match=einval):
            be.lib.deform_field(be.ptr(d_p), be.ptr(d_g), B, H, W, gh, gw, be.stream)
    with pytest.raises(NemarHipError, match=einval):
        be.lib.deform_field(None, be.ptr(d_g), B, H, W, 4, 4, be.stream)
    with pytest.raises(NemarHipError, match=einval):
        be.lib.deform_field(be.ptr(d_p), None, B, H, W, 4, 4, be.stream)
    d_pool, d_par, d_y = be.dev(np.zeros((1, 1, H, W))), be.dev_i32(np.zeros((B, 4))), be.full((B, 1, H, W), 7.0)
    for args in ((None, be.ptr(d_par), be.ptr(d_g), be.ptr(d_y)), (be.ptr(d_pool), None, be.ptr(d_g), be.ptr(d_y)),
                 (be.ptr(d_pool), be.ptr(d_par), None, be.ptr(d_y)), (be.ptr(d_pool), be.ptr(d_par), be.ptr(d_g), None)):
        with pytest.raises(NemarHipError, match=einval):
            be.lib.crop_flip_deform_normalize(*args, 1, B, 1, H, W, H, W, 1.0, be.stream)
    wsb = int(be.lib.registration_error_workspace(B, H, W))
    assert wsb > 0
    ws, d_out, d_pred = be.bytes_buf(wsb), be.full((B, 6), 7.0), be.zeros(B, 2, H, W)
    for mode in (0, 3, -1):                                 # EXPLICIT is not a prediction layout; 3 and -1 are no modes at all
        with pytest.raises(NemarHipError, match=einval):
            be.lib.registration_error(be.ptr(d_pred), mode, be.ptr(d_g), be.ptr(d_out), be.ptr(ws), wsb, B, H, W, be.stream)
    with pytest.raises(NemarHipError, match=einval):
        be.lib.registration_error(be.ptr(d_pred), GRID_UNET, be.ptr(d_g), be.ptr(d_out), be.ptr(ws), wsb - 1, B, H, W, be.stream)
    for args in ((None, GRID_UNET, be.ptr(d_g), be.ptr(d_out), be.ptr(ws)), (be.ptr(d_pred), GRID_UNET, None, be.ptr(d_out), be.ptr(ws)),
                 (be.ptr(d_pred), GRID_UNET, be.ptr(d_g), None, be.ptr(ws)), (be.ptr(d_pred), GRID_UNET, be.ptr(d_g), be.ptr(d_out), None)):
        with pytest.raises(NemarHipError, match=einval):
            be.lib.registration_error(*args, wsb, B, H, W, be.stream)
    be.sync()
    assert np.all(be.np(d_g) == 7.0) and np.all(be.np(d_y) == 7.0) and np.all(be.np(d_out) == 7.0)
