"""nemar_grid_sample_bwd WITH a workspace (csrc/warp.hip: tile_offset_kernel -> gather pass -> far_scatter_kernel -> far_fold_kernel) at its
numeric and geometric limits.  The bodies drive the C ABI directly, on small ragged planes (at least 2 x 2 destination tiles of 64 x 16),
and compare with oracle/ops_np.py in float64; the sampling coordinates are built in float32 with the kernel's operation order
(kernel_cases.case_grid_sample), so the oracle makes the kernel's floor() decisions.  Driven by tests/test_warp_limits_emu.py and
tests/test_warp_limits_gpu.py; every case runs on the default route and, in the measurement build, on nemar_grid_sample_tune(16)
(256-thread gather) and (32) (windows centred on the tiles).

THE BOUND (include/nemar_hip.h, nemar_grid_sample_bwd).  For a texel of grad_input that receives P contributions w_k * gout,
S = sum |w_k * gout| in float64:

    |gin - float64| <= ROUND * S + P * quantum(gmax),        quantum(g) = max(2^-40 * g, 2^-120),  gmax = max |gout| of the call

  first term   fp32 rounding: a contribution is (1 - tx) * (1 - ty) * gout = four roundings of 2^-24 relative (1 - t is exact for
               t >= 1/2 and relative 2^-24 otherwise), i.e. 2^-22 of |w_k * gout|; the fp32 additions of the gathered part and the final
               add of the folded far part are covered by the distance between this worst case and what roundings do on average.
  second term  the fixed-point scatter: a far contribution is rounded to a multiple of 2^(e - 40), max |gout| < 2^e, half of which is
               at most 2^-40 * gmax; e is clamped at -80, below which the multiple is 2^-120 whatever gmax is.  The scale is the maximum
               over the tiles that HAVE far pixels, which is at most the call's.
d loss / d grid_src has no fixed-point part.  Per output pixel it is sum_c g_c * ((b - a) * ey + (d - c) * ty) * W / 2: about 6 + C
roundings of 2^-24 relative to A = sum_c |g_c| * (|b - a| * ey + |d - c| * ty) * W / 2, bounded here by GG_ROUND = 2^-20 of A (C <= 4);
the affine form sums those over the plane — per-lane partial sums, a 512-lane tree, the tiles in order: fewer than 32 further roundings
of the sum of |terms|, bounded by 2^-18 of it."""
import contextlib

import numpy as np

import kernel_cases as K
from kernel_cases import GRID_EXPLICIT, GRID_UNET, GRID_AFFINE
from oracle import ops_np as O

f32, f64 = np.float32, np.float64
ROUND = 2.0 ** -22
GG_ROUND, GG_ROUND_AFFINE = 2.0 ** -20, 2.0 ** -18
MODES = (GRID_UNET, GRID_AFFINE, GRID_EXPLICIT)
HW = ((17, 65), (40, 150), (33, 130))
HW_3COL = ((40, 150), (33, 130))          # three tile columns: two that stay near next to one with far pixels
GT_W, GT_H = 64, 16                       # destination tile of the gather pass


def quantum(gmax):
    return max(2.0 ** -40 * gmax, 2.0 ** -120)


def variants(be):
    return (0, 16, 32) if getattr(be.lib, "has_switches", False) else (0,)


@contextlib.contextmanager
def variant(be, v):
    if v:
        be.lib.grid_sample_tune(v)
    try:
        yield
    finally:
        if v:
            be.lib.grid_sample_tune(0)


# ---- fields ------------------------------------------------------------------------------------------------------------------------------
def px(v, n):
    """v pixels as a normalised offset on an axis of n pixels"""
    return v * 2.0 / n


def noise_offsets(rng, N, H, W, scale):
    return (rng.standard_normal((N, 2, H, W)) * scale).astype(f32)


def smooth_offsets(rng, N, H, W, sx=9.3, sy=-4.6, wave=2.0):
    """a translation plus a slow wave (the smooth_px field of kernel_cases.case_grid_sample): the windows follow it"""
    o = rng.standard_normal((N, 2, H, W)) * 0.001
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    o[:, 0] += px(sx + wave * np.sin(2 * np.pi * yy / H + 0.3) * np.cos(2 * np.pi * xx / W), W)
    o[:, 1] += px(sy + wave * np.cos(2 * np.pi * xx / W + 0.7), H)
    return o.astype(f32)


def split_offsets(rng, N, H, W):
    """tile columns 0 and 1 (x < 128): 0.3 px of noise — every corner in the centred window, no far pixel in column 0 (its pixels' corners
    reach column 1 at most); x >= 128: noise of half the plane — far and out-of-range pixels"""
    o = rng.standard_normal((N, 2, H, W))
    near = np.arange(W) < 2 * GT_W
    o[:, 0] *= np.where(near, px(0.3, W), 0.5)[None, None, :]
    o[:, 1] *= np.where(near, px(0.3, H), 0.5)[None, None, :]
    return o.astype(f32)


def src_of(mode, offsets):
    return offsets if mode == GRID_UNET else O.unet_grid(offsets)


def grid_of(mode, src, H, W):
    """float32 grid [N,H,W,2] with the kernel's operation order"""
    if mode == GRID_UNET:
        return O.unet_grid(src)
    if mode == GRID_AFFINE:
        return K.affine_grid_f32(src, H, W)
    return src


def magnitudes(rng, shape, lo=2.0 ** -4, hi=4.0):
    return (rng.uniform(lo, hi, shape) * rng.choice([-1.0, 1.0], shape)).astype(f32)


# ---- the float64 reference and the ingredients of the bound ----------------------------------------------------------------------------
class Ref:
    pass


def reference(mode, inp, src, gout):
    """oracle gradients in float64 + S, P of every texel + the magnitude A of every grid-gradient element (module docstring)"""
    N, C, H, W = inp.shape
    grid = grid_of(mode, src, H, W)
    inp64, gout64 = inp.astype(f64), gout.astype(f64)
    r = Ref()
    r.gin, gg = O.grid_sample_bwd(inp64, grid, gout64)
    x0, y0, tx, ty = O._locate(grid, H, W)
    tx, ty = tx.astype(f64), ty.astype(f64)
    ex, ey = 1.0 - tx, 1.0 - ty
    n_idx = np.arange(N)
    nn = np.broadcast_to(n_idx[:, None, None], x0.shape)
    r.x0, r.y0 = x0, y0
    r.S, r.P = np.zeros((N, C, H, W)), np.zeros((N, 1, H, W))
    r.contrib_min = np.inf
    vals = []
    for yy, xx, wgt in ((y0, x0, ex * ey), (y0, x0 + 1, tx * ey), (y0 + 1, x0, ex * ty), (y0 + 1, x0 + 1, tx * ty)):
        v, m = O._gather(inp64, n_idx, yy, xx)
        vals.append(v)
        np.add.at(r.P[:, 0], (nn[m], yy[m], xx[m]), 1.0)
        for ch in range(C):
            t = np.abs(gout64[:, ch] * wgt)[m]
            np.add.at(r.S[:, ch], (nn[m], yy[m], xx[m]), t)
            if np.any(t > 0):
                r.contrib_min = min(r.contrib_min, t[t > 0].min())
    a, b, c, d = vals
    g = np.abs(gout64)
    ax = np.sum(g * (np.abs(b - a) * ey[:, None] + np.abs(d - c) * ty[:, None]), axis=1) * W / 2
    ay = np.sum(g * (np.abs(c - a) * ex[:, None] + np.abs(d - b) * tx[:, None]), axis=1) * H / 2
    A = np.stack([ax, ay], axis=-1)
    if mode == GRID_UNET:
        r.gsrc, r.A, r.gg_round = gg.transpose(0, 3, 1, 2), A.transpose(0, 3, 1, 2), GG_ROUND
    elif mode == GRID_EXPLICIT:
        r.gsrc, r.A, r.gg_round = gg, A, GG_ROUND
    else:
        xs, ys = (2.0 * np.arange(W) + 1.0) / W - 1.0, (2.0 * np.arange(H) + 1.0) / H - 1.0
        base = np.stack([np.broadcast_to(xs[None, :], (H, W)), np.broadcast_to(ys[:, None], (H, W)), np.ones((H, W))], axis=-1)
        r.gsrc = np.einsum('nhwi,hwk->nik', gg, base).reshape(-1, 6)
        r.A, r.gg_round = np.einsum('nhwi,hwk->nik', A, np.abs(base)).reshape(-1, 6), GG_ROUND_AFFINE
    return r


def _report(what, err, lim, got, want):
    i = np.unravel_index(np.argmax(err - lim), err.shape)
    raise AssertionError("%s: |err| %.3e > bound %.3e at %s (got %.9g want %.9g)" % (what, err[i], lim[i], i, got[i], want[i]))


def check_gin(got, r, gmax, what, clean=None):
    """the bound of the module docstring on every texel (`clean`: only where that mask holds — and those must be finite)"""
    got = np.asarray(got, dtype=f64)
    q = quantum(gmax)
    with np.errstate(invalid="ignore"):
        lim = ROUND * r.S + np.where(r.P > 0, r.P * q, 0.0)
    err = np.abs(got - r.gin)
    ok = (err <= lim) & np.isfinite(got)
    if clean is not None:
        ok |= ~clean
    if np.isfinite(q):      # measured, printed before the assertion: the rounding part of the error as a multiple of 2^-24 * S
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where((r.S > 0) & (clean if clean is not None else True), (err - r.P * q) / r.S, 0.0)
        print("%s: worst (|err| - P * quantum) / S = %.3f * 2^-24" % (what, np.nanmax(ratio) * 2.0 ** 24))
    if not np.all(ok):
        _report(what + " gin", np.where(ok, 0.0, np.where(np.isfinite(err), err, np.inf)), np.where(ok, 0.0, lim), got, r.gin)


def check_gsrc(got, r, what, clean=None):
    got = np.asarray(got, dtype=f64)
    lim = r.gg_round * r.A
    err = np.abs(got - r.gsrc)
    ok = (err <= lim) & np.isfinite(got)
    if clean is not None:
        ok |= ~clean
    if not np.all(ok):
        _report(what + " ggrid", np.where(ok, 0.0, np.where(np.isfinite(err), err, np.inf)), np.where(ok, 0.0, lim), got, r.gsrc)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---- one operator call --------------------------------------------------------------------------------------------------------------------
class Call:
    """the device buffers of one nemar_grid_sample_bwd call (same-size, with a workspace); run() returns (gin, ggrid) as float32 arrays,
    bit for bit, after checking the return code and that the leading zeroed_bytes of the workspace came back all-zero"""

    def __init__(self, be, mode, inp, src, gout):
        self.be, self.mode, self.shape, self.src_shape = be, mode, inp.shape, src.shape
        N, C, H, W = inp.shape
        self.d_in, self.d_src, self.d_gout = be.dev(inp), be.dev(src), be.dev(gout)
        self.wsb = be.lib.grid_sample_bwd_workspace(N, C, H, W)
        self.zb = be.lib.grid_sample_bwd_zeroed_bytes(N, C, H, W)
        assert 0 < self.zb <= self.wsb
        self.ws = self.fresh_workspace()

    def fresh_workspace(self):
        return self.be.bytes_buf(self.wsb)

    def run(self, gout=None, src=None, ws=None):
        be = self.be
        N, C, H, W = self.shape
        d_gout = self.d_gout if gout is None else be.dev(gout)
        d_src = self.d_src if src is None else be.dev(src)
        ws = self.ws if ws is None else ws
        d_gin, d_gsrc = be.full(self.shape, np.nan), be.full(self.src_shape, np.nan)
        rc = be.lib.grid_sample_bwd(be.ptr(self.d_in), be.ptr(d_src), self.mode, be.ptr(d_gout), be.ptr(d_gin), 0, be.ptr(d_gsrc), 0,
                                    N, C, H, W, H, W, be.ptr(ws), self.wsb, be.stream)
        assert rc == 0, "nemar_grid_sample_bwd returned %d" % rc
        assert not np.any(be.raw(ws)[:self.zb]), "grid_sample_bwd must return the accumulator part of its workspace zero-filled"
        return be.raw(d_gin).view(f32).reshape(self.shape), be.raw(d_gsrc).view(f32).reshape(self.src_shape)


def run_checked(be, mode, inp, src, gout, what, gmax=None, twice=True, plane_sums=False):
    """reference once; on every variant: the call, the bound, and (twice) a second call on the same workspace, bit-identical"""
    r = reference(mode, inp, src, gout)
    gmax = float(np.abs(gout).max()) if gmax is None else gmax
    for v in variants(be):
        with variant(be, v):
            call = Call(be, mode, inp, src, gout)
            gin, gsrc = call.run()
            w = "%s, variant %d" % (what, v)
            check_gin(gin, r, gmax, w)
            check_gsrc(gsrc, r, w)
            if plane_sums:
                lim = (ROUND * r.S + r.P * quantum(gmax)).sum(axis=(2, 3))
                err = np.abs(gin.astype(f64).sum(axis=(2, 3)) - r.gin.sum(axis=(2, 3)))
                assert np.all(err <= lim), "%s: plane sums of gin off by %s (bound %s)" % (w, err, lim)
            if twice:
                gin2, gsrc2 = call.run()
                assert same_bits(gin, gin2) and same_bits(gsrc, gsrc2), "%s: the second call on the same workspace differs" % w
    return r


def image(rng, N, C, H, W):
    return rng.uniform(-1, 1, (N, C, H, W)).astype(f32)


# ---- 1 + 2: the bound at unit scale, then power-of-two equivariance, bit for bit -------------------------------------------------------
SCALE_EXPONENTS = (-32, 32, 80)


def case_equivariance(be, mode, field, H, W, N=2, C=3):
    """gout -> gout * 2^k on the same workspace right after the unscaled call: gin and ggrid are 2^k times the first result, bit for bit
    (the scale exponent of the fixed-point path moves with max |gout|; nothing else may).  |gout| in [2^-4, 4]: no contribution of the
    unscaled call is below 2^-94, so none is subnormal at 2^-32 either."""
    rng = np.random.default_rng(H * W + 7 * mode + (field == "noise"))
    inp = image(rng, N, C, H, W)
    if mode == GRID_AFFINE:
        src = (rng.standard_normal((N, 6)) * (0.5 if field == "noise" else 0.02)).astype(f32)
        if field != "noise":
            src[:, 2] += f32(0.12)
            src[:, 5] -= f32(0.23)
    else:
        src = src_of(mode, noise_offsets(rng, N, H, W, 0.5) if field == "noise" else smooth_offsets(rng, N, H, W))
    gout = magnitudes(rng, (N, C, H, W))
    r = reference(mode, inp, src, gout)
    assert r.contrib_min >= 2.0 ** -94, "a contribution of %.3e would be subnormal at 2^-32" % r.contrib_min
    for v in variants(be):
        with variant(be, v):
            call = Call(be, mode, inp, src, gout)
            gin, gsrc = call.run()
            what = "mode %d, %s field, %dx%d, variant %d" % (mode, field, H, W, v)
            check_gin(gin, r, float(np.abs(gout).max()), what)
            check_gsrc(gsrc, r, what)
            for k in SCALE_EXPONENTS:
                s = f32(2.0) ** f32(k)
                gin_k, gsrc_k = call.run(gout=gout * s)
                assert same_bits(gin_k, gin * s), "%s: gin(gout * 2^%d) != gin(gout) * 2^%d" % (what, k, k)
                assert same_bits(gsrc_k, gsrc * s), "%s: ggrid(gout * 2^%d) != ggrid(gout) * 2^%d" % (what, k, k)


# ---- 3: heterogeneous magnitudes under ONE scale word ------------------------------------------------------------------------------------
HETEROGENEOUS = ("samples", "channels", "outlier", "zero", "above_clamp", "below_clamp")


def case_heterogeneous(be, which, mode, H, W):
    """the scale of the fixed-point path is one word for the call: (samples) 1 : 1e-6 : 1e4 per sample, (channels) 1e-3 : 1 : 1e3 per channel,
    (outlier) 1e4 on one pixel of a tile without far pixels next to O(1) far tiles, (zero) gout = 0, (above_clamp / below_clamp)
    max |gout| = 2^-79 / 2^-100 — either side of the exponent clamp; the bound with the call-wide max |gout|"""
    rng = np.random.default_rng(H + W + len(which))
    N, C = 3, 3
    inp = image(rng, N, C, H, W)
    src = src_of(mode, split_offsets(rng, N, H, W))
    gout = magnitudes(rng, (N, C, H, W), 0.25, 1.0)
    if which == "samples":
        gout *= np.array([1, 1e-6, 1e4], dtype=f32)[:, None, None, None]
    elif which == "channels":
        gout *= np.array([1e-3, 1, 1e3], dtype=f32)[None, :, None, None]
    elif which == "outlier":
        gout[0, 1, H // 2, 30] = 1e4
    elif which == "zero":
        gout[...] = 0
    else:
        gout *= f32(2.0 ** (-79 if which == "above_clamp" else -100)) / np.abs(gout).max()
        assert float(np.abs(gout).max()) == 2.0 ** (-79 if which == "above_clamp" else -100)
    r = run_checked(be, mode, inp, src, gout, "%s, mode %d, %dx%d" % (which, mode, H, W))
    far = ((np.abs(r.x0 - np.arange(W)[None, None, :]) > 4) | (np.abs(r.y0 - np.arange(H)[None, :, None]) > 4)) & \
          (r.x0 >= 0) & (r.x0 + 1 < W) & (r.y0 >= 0) & (r.y0 + 1 < H)
    assert far[:, :, 2 * GT_W:].any() and not far[:, :, :GT_W].any(), "the field must have far pixels, and none in tile column 0"


# ---- 4: collapse and large linear maps ---------------------------------------------------------------------------------------------------
LINEAR = {                      # theta of GRID_AFFINE (dtheta = theta - identity)
    "collapse": (0, 0, 0, 0, 0, 0),             # every output pixel samples the image centre: H * W contributions on four texels
    "rot180": (-1, 0, 0, 0, -1, 0),
    "rot90": (0, -1, 0, 1, 0, 0),               # (on a square plane)
    "zoom2": (0.5, 0, 0, 0, 0.5, 0),
    "zoom05": (2, 0, 0, 0, 2, 0),
    "shear": (1, 0.5, 0, 0, 1, 0),
}


def case_linear(be, which, H, W, N=2, C=3):
    """theta far from the identity: the window offsets differ from tile to tile; float64 bound, two calls on one workspace bit-identical.
    (Every product theta * base is exact here, so the float32 coordinates do not depend on how the compiler contracts them.)"""
    rng = np.random.default_rng(H * W + len(which))
    inp, gout = image(rng, N, C, H, W), magnitudes(rng, (N, C, H, W), 0.25, 2.0)
    if which == "collapse_unet":                 # offsets = -identity: gx = gy = 0 exactly
        src = np.broadcast_to(-O.unet_identity_grid(H, W, f32), (N, 2, H, W)).copy()
        mode = GRID_UNET
    else:
        src = np.tile(np.array(LINEAR[which], dtype=f32) - np.array([1, 0, 0, 0, 1, 0], dtype=f32), (N, 1))
        mode = GRID_AFFINE
    r = run_checked(be, mode, inp, src, gout, "%s %dx%d" % (which, H, W))
    if which.startswith("collapse"):
        assert np.count_nonzero(r.P) <= 4 * N and r.P.sum() == 4 * N * H * W      # (the test's own geometry)


# ---- 5: fields with jumps -----------------------------------------------------------------------------------------------------------------
JUMP_T = (0, -1, 3, 4, 9, -17)                   # px: around the dead zone (ox in [-1, 0] -> 0) and the window radius 3
JUMPS = ("edge", "inside1", "inside3", "cross")


def jump_translations(where, H, W, N):
    """piecewise-constant whole-pixel translations [N,2,H,W], in pixels.  edge / inside1 / inside3: one vertical and one horizontal
    discontinuity at x = 64 + {0, 1, 3}, y = 16 + {0, 1, 3}, another four pairs out of JUMP_T per sample; cross: four different translations
    around the point where four tiles meet — one pixel lands with one corner in each of them"""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    t = np.zeros((N, 2, H, W))
    k = {"edge": 0, "inside1": 1, "inside3": 3, "cross": 0}[where]
    q = (xx >= GT_W + k) * 1 + (yy >= GT_H + k) * 2
    for n in range(N):
        if where == "cross":
            quad = ((3, 4), (-1, 9), (9, -1), (-17, 0))
        else:
            j = JUMP_T[2 * n % 6:] + JUMP_T[:2 * n % 6]
            quad = ((j[0], j[1]), (j[1], j[2]), (j[3], j[0]), (j[4], j[5]))
        for i, (sx, sy) in enumerate(quad):
            t[n, 0][q == i] = sx
            t[n, 1][q == i] = sy
    return t


def case_jumps(be, where, mode, H, W, N=3, C=2):
    rng = np.random.default_rng(H * W + len(where))
    inp, gout = image(rng, N, C, H, W), magnitudes(rng, (N, C, H, W), 0.25, 2.0)
    t = jump_translations(where, H, W, N)
    if mode == GRID_EXPLICIT:      # exactly whole pixels: grid = (2 (w + t) + 1) / W - 1, sampled at (or an ulp below) integer coordinates
        yy, xx = np.meshgrid(np.arange(H, dtype=f64), np.arange(W, dtype=f64), indexing='ij')
        src = np.stack([(2 * (xx[None] + t[:, 0]) + 1) / W - 1, (2 * (yy[None] + t[:, 1]) + 1) / H - 1], axis=-1).astype(f32)
    else:
        src = np.stack([px(t[:, 0], W), px(t[:, 1], H)], axis=1).astype(f32)
    r = run_checked(be, mode, inp, src, gout, "jump %s, mode %d, %dx%d" % (where, mode, H, W), plane_sums=True)
    if where == "cross" and mode == GRID_UNET:
        four = (r.x0 == GT_W - 1) & (r.y0 == GT_H - 1)
        assert four.any(), "no pixel with its four corners in four tiles"


# ---- 6: non-finite data must not poison the workspace ----------------------------------------------------------------------------------
def _far_pixel(r, n, W):
    """an output pixel of sample n in the far part of split_offsets: displaced by more than 4 px, all four corners in the image"""
    H = r.x0.shape[1]
    ok = (np.abs(r.x0[n] - np.arange(W)[None, :]) > 4) & (r.x0[n] >= 0) & (r.x0[n] + 1 < W) & (r.y0[n] >= 0) & (r.y0[n] + 1 < H)
    ok[:, :2 * GT_W] = False
    h, w = np.argwhere(ok)[0]
    return int(h), int(w)


def _after_poison(be, call, gout, what):
    """a clean call on the workspace the poisoned call used == the same call on a fresh zeroed workspace, bit for bit"""
    a = call.run(gout=gout)
    b = call.run(gout=gout, ws=call.fresh_workspace())
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]), "%s: the call after the poisoned one differs from one on a fresh workspace" % what


def case_nonfinite_gout(be, inf_is_far, mode, H=40, W=150, N=2, C=3):
    """one +Inf and one NaN in gout, one on a far pixel and one in tile column 0 (no far pixels).  Everything that does not depend on
    the two pixels is finite and within the bound — with max |gout| over the FINITE values when the far one is the NaN (a NaN never
    enters the scale, and the Inf sits in a tile whose maximum is not taken); with the Inf on a far pixel the call's max |gout| is
    infinite and so is the fixed-point term of the bound: texels with contributions must be finite, the others exactly zero."""
    rng = np.random.default_rng(11 + mode + inf_is_far)
    inp, gout = image(rng, N, C, H, W), magnitudes(rng, (N, C, H, W), 0.25, 2.0)
    src = src_of(mode, split_offsets(rng, N, H, W))
    r = reference(mode, inp, src, gout)
    fh, fw = _far_pixel(r, 1, W)
    spots = {"far": (1, 2, fh, fw), "near": (0, 1, 5, 20)}
    bad = gout.copy()
    bad[spots["far" if inf_is_far else "near"]] = np.inf
    bad[spots["near" if inf_is_far else "far"]] = np.nan
    clean_gin = np.ones((N, C, H, W), dtype=bool)
    clean_gg = np.ones((N, H, W), dtype=bool)
    for n, c, h, w in spots.values():
        clean_gg[n, h, w] = False
        for dy in (0, 1):
            for dx in (0, 1):
                y, x = r.y0[n, h, w] + dy, r.x0[n, h, w] + dx
                if 0 <= y < H and 0 <= x < W:
                    clean_gin[n, c, y, x] = False
    clean_gsrc = np.broadcast_to(clean_gg[:, None] if mode == GRID_UNET else clean_gg[..., None], src.shape)
    zeroed = np.where(np.isfinite(bad), bad, 0).astype(f32)
    rz = reference(mode, inp, src, zeroed)          # what the clean elements must hold
    gmax = np.inf if inf_is_far else float(np.abs(zeroed).max())
    for v in variants(be):
        with variant(be, v):
            what = "Inf %s, mode %d, variant %d" % ("far" if inf_is_far else "near", mode, v)
            call = Call(be, mode, inp, src, gout)
            gin, gsrc = call.run(gout=bad)
            # observed, for the header's account of such a call: what the poisoned elements hold, how far the clean ones are off
            print("%s: poisoned texels %s, poisoned ggrid %s, clean texels off by at most %.3e" %
                  (what, gin[~clean_gin], gsrc[~clean_gsrc], np.abs(gin - rz.gin)[clean_gin].max()))
            check_gin(gin, rz, gmax, what, clean=clean_gin)
            check_gsrc(gsrc, rz, what, clean=clean_gsrc)
            _after_poison(be, call, gout, what)


def case_nonfinite_offsets(be, H=40, W=150, N=2, C=3):
    """a NaN (x offset, on the centre pixel of tile (1, 1), which tile_offset_kernel samples) and an Inf (y offset) in the GRID_UNET field:
    locate() clamps before the int conversion, so both pixels sample outside the plane and contribute nothing — grad_input is within the
    bound EVERYWHERE, the grid gradient everywhere but at the two pixels; no address leaves the plane (guard bands)"""
    rng = np.random.default_rng(13)
    inp, gout = image(rng, N, C, H, W), magnitudes(rng, (N, C, H, W), 0.25, 2.0)
    off = split_offsets(rng, N, H, W)
    spots = ((0, 0, GT_H + GT_H // 2, GT_W + GT_W // 2, np.nan), (1, 1, 5, 140, np.inf))
    bad, outside = off.copy(), off.copy()
    clean = np.ones((N, 2, H, W), dtype=bool)
    for n, ch, h, w, v in spots:
        bad[n, ch, h, w] = v
        outside[n, ch, h, w] = 8.0               # the reference's stand-in: far outside the plane, no valid corner
        clean[n, :, h, w] = False
    r = reference(GRID_UNET, inp, outside, gout)
    gmax = float(np.abs(gout).max())
    for v in variants(be):
        with variant(be, v):
            what = "non-finite offsets, variant %d" % v
            call = Call(be, GRID_UNET, inp, off, gout)
            gin, gsrc = call.run(src=bad)
            print("%s: ggrid at the two pixels %s" % (what, gsrc[~clean]))
            check_gin(gin, r, gmax, what)
            check_gsrc(gsrc, r, what, clean=clean)
            _after_poison(be, call, gout, what)
