"""Backend-agnostic test bodies for the normalisation kernels on ILL-CONDITIONED planes (csrc/norm.hip, csrc/norm_planes.hip; the
BatchNorm side lives in tests/bn_cases.py and takes its plane families from here), driven through tests/backends.py and compared with
float64 numpy restatements written in this file.

The pass criterion (every family but `plain`, which keeps the assertions of kernel_cases.case_instnorm unchanged):

    err <= max(today's tolerance for the quantity, F * max(e_ref, e_np)),   F = 4

where e_ref is the error against float64 of torch's own fp32 layer on the CPU (F.instance_norm, its backward through autograd) and e_np
the error of a plain numpy fp32 exact two-pass restatement (np32_*), both on the same input.  The yardsticks and the kernels differ only
in summation order (numpy pairwise: 128 sequential + a tree; torch: Welford in a wider accumulator; the kernels: <= 64 sequential + 6
shuffles + 16 across waves), which under a random-walk model is at most a factor 2; F = 4 doubles that for an unlucky draw.  F is a
condition of the test, not a knob.  Every check appends its figures to RECORD (profiles/norm_conditioning.txt is made from them)."""
import numpy as np

from backends import POISON_BIG
from kernel_cases import _assert_close, _decode_planes, _decode_pixel_planes, _dgrad_plane_content

ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
EPS, SLOPE, F = 1e-5, 0.2, 4.0
f32 = np.float32

RECORD = []        # dicts: route, family, quantity, err, yard, ratio (err / yard), backend


def _both_poisons(case):
    """The max-word forms and the plane producers skip NaN by design: their cases run once with the large finite poison in the guard
    bands (tests/backends.py; that pass leaves no RECORD rows) and once, as before, with the NaN poison."""
    import functools

    @functools.wraps(case)
    def run(be, *a, **k):
        n = len(RECORD)
        with be.poisoned(POISON_BIG):
            case(be, *a, **k)
        del RECORD[n:]
        return case(be, *a, **k)
    return run


# ---- the plane families: (rng, planes, HW) -> fp32 [planes, HW] --------------------------------------------------------------------------
def _plain(rng, planes, HW):
    return (rng.standard_normal((planes, HW)) * 2 + rng.standard_normal((planes, 1)) * 3).astype(f32)


def _offset(rng, planes, HW):
    return (rng.standard_normal((planes, HW)) + 1000.0).astype(f32)


def _first_outlier(rng, planes, HW):
    x = rng.standard_normal((planes, HW)).astype(f32)
    x[:, 0] = 30.0
    return x


def _first_outlier_far(rng, planes, HW):
    x = rng.standard_normal((planes, HW)).astype(f32)
    x[:, 0] = 1000.0
    return x


def _last_outlier(rng, planes, HW):
    x = rng.standard_normal((planes, HW)).astype(f32)
    x[:, -1] = -30.0
    return x


def _spike(rng, planes, HW):
    x = np.zeros((planes, HW), dtype=f32)
    x[np.arange(planes), (np.arange(planes) * 7919 + HW // 3) % HW] = 5.0
    return x


def _constant(rng, planes, HW):
    return np.full((planes, HW), 0.7, dtype=f32)


def _tiny(rng, planes, HW):
    return (1e-4 * rng.standard_normal((planes, HW)) + 1e-2).astype(f32)


def _mixed(rng, planes, HW):
    scales = 10.0 ** (((np.arange(planes) * 5) % 7) - 3.0)             # 1e-3 ... 1e3, neighbours far apart
    return (rng.standard_normal((planes, HW)) * scales.reshape(planes, 1)).astype(f32)


FAMILIES = {"plain": _plain, "offset": _offset, "first_outlier": _first_outlier, "first_outlier_far": _first_outlier_far,
            "last_outlier": _last_outlier, "spike": _spike, "constant": _constant, "tiny": _tiny, "mixed": _mixed}
FAMILY_NAMES = list(FAMILIES)
NO_ACT_BACKWARD = ("constant", "spike")        # xhat == 0 on all but one pixel: the backward runs with ACT_NONE only


def make_planes(seed, planes, HW, family):
    """-> x fp32 [planes, HW], the family name of every plane.  family "cycle": plane p is of family (seed + p) mod 9 (the planes of one
    call cycle through the families); a family name: every plane the same."""
    rng = np.random.default_rng(seed)
    if family != "cycle":
        return FAMILIES[family](rng, planes, HW), [family] * planes
    names = [FAMILY_NAMES[(seed + p) % len(FAMILY_NAMES)] for p in range(planes)]
    x = np.empty((planes, HW), dtype=f32)
    for p, nm in enumerate(names):
        x[p] = FAMILIES[nm](rng, planes, HW)[p]
    return x, names


# ---- float64 and the two fp32 yardsticks -------------------------------------------------------------------------------------------------
def ref64_fwd(x):
    x = x.astype(np.float64)
    m = x.mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(x.var(axis=1, keepdims=True) + EPS)
    return (x - m) * rstd, m[:, 0], rstd[:, 0]


def ref64_bwd(x, mean, rstd, g):
    """gx from GIVEN statistics (float64 arithmetic): rstd (g - mean g - xhat mean(g xhat))"""
    x, g = x.astype(np.float64), g.astype(np.float64)
    r = np.asarray(rstd, dtype=np.float64).reshape(-1, 1)
    xh = (x - np.asarray(mean, dtype=np.float64).reshape(-1, 1)) * r
    return r * (g - g.mean(axis=1, keepdims=True) - xh * (g * xh).mean(axis=1, keepdims=True))


def np32_fwd(x):
    """plain numpy fp32 exact two-pass InstanceNorm -> xhat, mean, rstd (all float32)"""
    HW = f32(x.shape[1])
    m = (x.sum(axis=1, keepdims=True, dtype=f32) / HW).astype(f32)
    d = (x - m).astype(f32)
    var = ((d * d).sum(axis=1, keepdims=True, dtype=f32) / HW).astype(f32)
    rstd = (f32(1.0) / np.sqrt(var + f32(EPS), dtype=f32)).astype(f32)
    return (d * rstd).astype(f32), m[:, 0], rstd[:, 0]


def np32_bwd(x, g):
    """the same for the backward, from its own fp32 statistics"""
    xh, _, rstd = np32_fwd(x)
    HW = f32(x.shape[1])
    g = g.astype(f32)
    m1 = (g.sum(axis=1, keepdims=True, dtype=f32) / HW).astype(f32)
    m2 = ((g * xh).sum(axis=1, keepdims=True, dtype=f32) / HW).astype(f32)
    return (rstd.reshape(-1, 1) * (g - m1 - xh * m2)).astype(f32)


def torch32(x, g=None):
    """torch's fp32 layer on the CPU: F.instance_norm, and its backward through autograd -> xhat[, gx]"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).reshape(1, *x.shape).requires_grad_(g is not None)
    y = torch.nn.functional.instance_norm(t, eps=EPS)
    if g is None:
        return y.detach().numpy()[0]
    y.backward(torch.from_numpy(np.ascontiguousarray(g.astype(f32))).reshape(1, *x.shape))
    return y.detach().numpy()[0], t.grad.numpy()[0]


def _plane_max(a):
    return np.abs(a).reshape(a.shape[0], -1).max(axis=1)


def check(be, route, names, quantity, got, want, atol, rtol, yard):
    """per plane: every element within today's tolerance (atol + rtol |want|; atol a scalar or one value per plane), or — any family but
    `plain` — the plane's largest error within F x its yardstick (`yard`: one value per plane)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    P = got.shape[0]
    got, want = got.reshape(P, -1), want.reshape(P, -1)
    err = np.abs(got - want)
    lim = np.broadcast_to(np.asarray(atol, dtype=np.float64).reshape(-1, 1), (P, 1)) + rtol * np.abs(want)
    today = np.all(err <= lim, axis=1)
    emax = err.max(axis=1)
    yard = np.asarray(yard, dtype=np.float64).reshape(P)
    bad = []
    for p in range(P):
        ratio = float(emax[p] / yard[p]) if yard[p] > 0 else (0.0 if emax[p] == 0 else float("inf"))
        RECORD.append(dict(backend=be.name, route=route, family=names[p], quantity=quantity, err=float(emax[p]), yard=float(yard[p]),
                           ratio=ratio, today=bool(today[p])))
        ok = today[p] or (names[p] != "plain" and emax[p] <= F * yard[p])
        if not ok:
            bad.append("plane %d (%s): max|err|=%.3e, yardstick %.3e (ratio %.1f), today's atol=%.3g rtol=%g" %
                       (p, names[p], emax[p], yard[p], ratio, float(np.asarray(atol).reshape(-1)[min(p, np.asarray(atol).size - 1)]), rtol))
    print("%-44s %-9s worst ratio %8.3f  worst err %.3e" % (route, quantity, max([r["ratio"] for r in RECORD[-P:] if np.isfinite(r["ratio"])] + [0.0]),
                                                         emax.max()))
    assert not bad, "%s %s: %s" % (route, quantity, "; ".join(bad))


def place(be, a, misalign):
    """`a` flattened into device memory that starts on a 16-byte boundary, or (misalign) 4 bytes past one"""
    a = np.ascontiguousarray(a, dtype=f32).ravel()
    o = 1 if misalign else 0                     # (a backend buffer starts on a 16-byte boundary and ends flush against its back guard)
    buf = be.full((a.size + o,), np.nan)
    v = be.sub(buf, o, o + a.size)
    v[:] = be.dev(a)
    assert be.ptr(v).value % 16 == (4 if misalign else 0)
    return v


def _words(be, buf, n):
    return be.raw(buf)[:4 * n].view(np.uint32).copy()


def _want_words(a, samples):
    a = np.abs(np.asarray(a, dtype=f32).reshape(samples, -1))
    return np.where(np.isfinite(a), a, 0).max(axis=1).astype(f32).view(np.uint32)


# The HW of every instance of the two dispatch chains of norm.hip (instnorm_fwd_impl / instnorm_bwd_impl), aligned pointers:
#   (HW, forward instance, backward instance, vectorised: repeated with misaligned pointers, which sends the row to the scalar or
#   streaming instance of the same size)
ROUTES = [
    (448, "fwd<64,8>", "bwd<64,8>", False),
    (961, "fwd<256,16>", "bwd<256,16>", False),                       # 31 x 31
    (1024, "fwd4<256,4>", "bwd4<256,4>", True),                       # misaligned: fwd<256,16> / bwd<256,16>
    (4096, "fwd4<256,4>", "bwd4<256,4>", True),
    (4098, "fwd<1024,16>", "bwd<1024,16>", False),                    # % 4 != 0
    (4100, "fwd4<1024,4> masked tail", "bwd4<1024,4> masked tail", True),   # misaligned: fwd<1024,16> / bwd<1024,16>
    (16384, "fwd4<1024,4>", "bwd4<1024,4>", True),
    (16386, "fwd<1024,0> streaming", "bwd<1024,32>", False),
    (16388, "fwd4<1024,8> masked tail", "bwd4<1024,8> masked tail", True),  # misaligned: streaming / bwd<1024,32>
    (32768, "fwd4<1024,8>", "bwd4<1024,8>", True),
    (40000, "fwd4<1024,12>", "bwd<1024,0> streaming", True),          # misaligned: streaming both ways
    (50176, "fwd4<1024,14>", "bwd<1024,0> streaming", True),
    (61488, "fwd<1024,0> streaming", "bwd<1024,0> streaming", False),      # 244 x 252
    (65536, "fwd4<1024,16,FULL>", "bwd4s<1024,16>", True),
    (110592, "fwd<1024,0> streaming", "bwd<1024,0> streaming", False),     # 288 x 384, the default geometry
    (1048576, "fwd<1024,0> streaming", "bwd<1024,0> streaming", False),    # 1024 x 1024: GPU tier only
]


def route_name(HW, misalign):
    row = [r for r in ROUTES if r[0] == HW]
    if not row:
        return "HW=%d%s" % (HW, " +4B" if misalign else "")
    _, fw, bw, _ = row[0]
    if misalign:
        per = 8 if HW <= 512 else 16
        thr = 64 if HW <= 512 else (256 if HW <= 4096 else 1024)
        fw = "fwd<%d,%d>" % (thr, per) if HW <= 16384 else "fwd<1024,0> streaming"
        bw = "bwd<%d,%d>" % (thr, per) if HW <= 16384 else ("bwd<1024,32>" if HW <= 32768 else "bwd<1024,0> streaming")
    return "HW=%d%s %s | %s" % (HW, " +4B" if misalign else "", fw, bw)


@_both_poisons
def case_instnorm_conditioned(be, planes, HW, family, act, residual, misalign, pps=1, seed=0):
    """nemar_instnorm_fwd (output, stats), nemar_instnorm_bwd from the kernel's own stats, their _max forms (same bits, words == numpy's
    per-sample finite maximum) and two identical calls bit for bit, on `planes` planes of `HW` elements of one family (or "cycle")."""
    route = route_name(HW, misalign)
    x, names = make_planes(seed, planes, HW, family)
    rng = np.random.default_rng(seed + 1000)
    res = rng.standard_normal((planes, HW)).astype(f32) if residual else None
    gy = rng.standard_normal((planes, HW)).astype(f32)
    plain_call = family == "plain"

    xhat64, m64, r64 = ref64_fwd(x)
    xh_np, m_np, r_np = np32_fwd(x)
    xh_t = torch32(x)
    yard_y = np.maximum(_plane_max(xh_np - xhat64), _plane_max(xh_t - xhat64))
    yard_m, yard_r = np.abs(m_np - m64), np.abs(r_np - r64)
    a64 = np.where(xhat64 > 0, xhat64, 0.0 if act == ACT_RELU else SLOPE * xhat64) if act != ACT_NONE else xhat64
    want_y = a64 + (res.astype(np.float64) if residual else 0.0)

    d_x, d_gy = place(be, x, misalign), place(be, gy, misalign)
    d_res = place(be, res, misalign) if residual else None
    nan = np.full(planes * HW, np.nan, dtype=f32)

    def fwd(maxw=None):
        y, st = place(be, nan, misalign), be.full((planes, 2), np.nan)
        if maxw is None:
            be.lib.instnorm_fwd(be.ptr(d_x), be.ptr(d_res), be.ptr(y), be.ptr(st), planes, HW, EPS, act, SLOPE, be.stream)
        else:
            be.lib.instnorm_fwd_max(be.ptr(d_x), be.ptr(d_res), be.ptr(y), be.ptr(st), planes, HW, EPS, act, SLOPE, be.ptr(maxw), pps, be.stream)
        be.sync()
        return y, st

    y, st = fwd()
    stn = be.np(st)
    yn = be.np(y).reshape(planes, HW)
    assert np.all(np.isfinite(yn)) and np.all(np.isfinite(stn)), route
    check(be, route, names, "y", yn, want_y, 3e-5, 1e-5, yard_y)
    check(be, route, names, "mean", stn[:, 0], m64, 1e-5, 1e-5, yard_m)
    check(be, route, names, "rstd", stn[:, 1], r64, 0.0, 3e-5, yard_r)
    y2, st2 = fwd()
    assert be.raw(y2).tobytes() == be.raw(y).tobytes() and be.raw(st2).tobytes() == be.raw(st).tobytes(), route + ": forward repeat"
    samples = planes // pps
    w = be.bytes_buf(4 * samples * 2049)
    y3, st3 = fwd(w)
    assert be.raw(y3).tobytes() == be.raw(y).tobytes() and be.raw(st3).tobytes() == be.raw(st).tobytes(), route + ": fwd_max != fwd"
    assert np.array_equal(_words(be, w, samples), _want_words(yn, samples)), route + ": forward max words"

    # backward from the kernel's own stats; the activation mask from xhat recomputed in fp32 exactly as the kernels do
    bact = ACT_NONE if any(n in NO_ACT_BACKWARD for n in names) else act
    st32 = np.asarray(stn, dtype=f32)
    xh32 = ((x - st32[:, :1]).astype(f32) * st32[:, 1:]).astype(f32)
    mask = np.ones_like(xh32) if bact == ACT_NONE else np.where(xh32 > 0, f32(1), f32(0.0 if bact == ACT_RELU else SLOPE)).astype(f32)
    g = (gy * mask).astype(f32)                          # (a product with 0, 1 or the slope: the kernels' own fp32 value)
    want_gx = ref64_bwd(x, stn[:, 0], stn[:, 1], g)
    gx64 = ref64_bwd(x, m64, r64, g)                     # the exact layer's gradient: what the yardsticks are measured against
    yard_g = np.maximum(_plane_max(np32_bwd(x, g) - gx64), _plane_max(torch32(x, g)[1] - gx64))

    def bwd(maxw=None):
        gx = place(be, nan, misalign)
        if maxw is None:
            be.lib.instnorm_bwd(be.ptr(d_x), be.ptr(st), be.ptr(d_gy), be.ptr(gx), planes, HW, bact, SLOPE, be.stream)
        else:
            be.lib.instnorm_bwd_max(be.ptr(d_x), be.ptr(st), be.ptr(d_gy), be.ptr(gx), planes, HW, bact, SLOPE, be.ptr(maxw), pps, be.stream)
        be.sync()
        return gx

    gx = bwd()
    gxn = be.np(gx).reshape(planes, HW)
    assert np.all(np.isfinite(gxn)), route
    atol_g = 3e-5 * (np.abs(want_gx).max() if plain_call else _plane_max(want_gx))
    check(be, route, names, "gx", gxn, want_gx, atol_g, 1e-4, yard_g)
    assert be.raw(bwd()).tobytes() == be.raw(gx).tobytes(), route + ": backward repeat"
    w = be.bytes_buf(4 * samples * 2049)
    assert be.raw(bwd(w)).tobytes() == be.raw(gx).tobytes(), route + ": bwd_max != bwd"
    assert np.array_equal(_words(be, w, samples), _want_words(gxn, samples)), route + ": backward max words"
    return be.raw(y), be.raw(st), be.raw(gx)


# ---- the plane producers (csrc/norm_planes.hip) ---------------------------------------------------------------------------------------------
PRODUCER_FAMILIES = ("spike", "constant", "offset", "first_outlier")


@_both_poisons
def case_producers_conditioned(be, H, W, family, res_max=None, drop_p=0.0, N=2, C=64, seed=0):
    """nemar_instnorm_fwd_planes / nemar_instnorm_bwd_planes on ill-conditioned planes: stats and the fp32 outputs against float64 by the
    criterion above, the decoded hi + lo planes == the fp32 output within the split's own bound (the one case_instnorm_planes uses), every
    decoded value finite, the published scale word >= the true maximum.  res_max: None = no residual; 0, 1, 1e3 = the residual's largest
    magnitude (its max word)."""
    HW, P = H * W, N * C
    route = "planes %dx%d%s%s" % (H, W, "" if res_max is None else " res %g" % res_max, " drop" if drop_p else "")
    x, names = make_planes(seed, P, HW, family)
    rng = np.random.default_rng(seed + 2000)
    res = None
    if res_max is not None:
        res = rng.uniform(-1, 1, (P, HW)).astype(f32) * f32(res_max)
        if res_max:
            res[::C, 0] = res_max                                    # every sample's word is exactly res_max
    xhat64, m64, r64 = ref64_fwd(x)
    xh_np, m_np, r_np = np32_fwd(x)
    yard_y = np.maximum(_plane_max(xh_np - xhat64), _plane_max(torch32(x) - xhat64))
    keep, dscale = np.ones((P, HW), dtype=bool), 1.0
    if drop_p > 0:
        ones, m = be.dev(np.ones(P * HW)), be.full((P * HW,), np.nan)
        be.lib.dropout(be.ptr(ones), be.ptr(m), P * HW, drop_p, 424242, 5, be.stream)
        keep, dscale = (be.np(m) != 0).reshape(P, HW), 1.0 / (1 - drop_p)
    want = np.where(keep, xhat64 * dscale, 0.0) + (res.astype(np.float64) if res is not None else 0.0)
    d_x, d_res = be.dev(x), (be.dev(res) if res is not None else None)
    resmax = be.dev(np.abs(res).reshape(N, -1).max(axis=1).astype(f32)) if res is not None else None
    d_y, d_st = be.full((P, HW), np.nan), be.full((P, 2), np.nan)
    pbytes = 2 * N * (C // 8) * (H + 4) * (W + 4) * 16
    planes, scale_w, max_w = be.bytes_buf(pbytes), be.bytes_buf(4 * N), be.bytes_buf(4 * N * 2049)
    be.lib.instnorm_fwd_planes(be.ptr(d_x), be.ptr(d_res), be.ptr(resmax), be.ptr(d_y), be.ptr(d_st), N, C, H, W, EPS, ACT_NONE, SLOPE,
                               drop_p, 424242, 5, be.ptr(planes), be.ptr(scale_w), be.ptr(max_w), None, be.stream)
    be.sync()
    y, st = be.np(d_y), be.np(d_st)
    assert np.all(np.isfinite(y)) and np.all(np.isfinite(st)), route
    # today's tolerance of case_instnorm_planes: 2e-5 max(1, max |want|) on y, 1e-5 on the mean, 1e-5 relative on rstd
    check(be, route + " fwd", names, "y", y, want, 2e-5 * max(1.0, np.abs(want).max()), 0.0, yard_y * dscale)
    check(be, route + " fwd", names, "mean", st[:, 0], m64, 1e-5, 0.0, np.abs(m_np - m64))
    check(be, route + " fwd", names, "rstd", st[:, 1], r64, 0.0, 1e-5, np.abs(r_np - r64))
    bound = _words(be, scale_w, N).view(f32).astype(np.float64)
    ymax = np.abs(y).reshape(N, -1).max(axis=1)
    assert np.all(bound >= ymax), (route, "the published scale word is below the true maximum", bound, ymax)
    assert np.array_equal(_words(be, max_w, N), _want_words(y, N)), route + ": max words"
    scale = (2.0 ** (11 - np.floor(np.log2(bound)))).reshape(N, 1, 1, 1)
    pl = _decode_planes(be.raw(planes)[:pbytes], N, C, H, W)
    assert np.all(np.isfinite(pl)), route + ": a decoded plane value is inf or NaN"
    val = (pl[0] + pl[1]) / scale
    ypad = np.pad(y.reshape(N, C, H, W), ((0, 0), (0, 0), (1, 1), (1, 1)), mode='reflect')
    err = np.abs(val[:, :, :H + 2, :W + 2] - ypad)
    assert np.all(err <= 2.0 ** -21 * np.abs(ypad) + 2.0 ** -24 / scale), (route, "hi + lo planes", float(err.max()))

    # ---- the backward producer, from the forward's own stats ----
    gy = rng.standard_normal((P, HW)).astype(f32)
    g = np.where(keep, gy.astype(np.float64) * dscale, 0.0) if drop_p > 0 else gy.astype(np.float64)
    want_gx = ref64_bwd(x, st[:, 0], st[:, 1], g)
    gx64 = ref64_bwd(x, m64, r64, g)
    g32 = g.astype(f32)                                     # (gy * 2 under dropout 0.5: exact)
    yard_g = np.maximum(_plane_max(np32_bwd(x, g32) - gx64), _plane_max(torch32(x, g32)[1] - gx64))
    d_gy = be.dev(gy)
    gymax = be.dev(np.abs(gy).reshape(N, -1).max(axis=1).astype(f32))
    d_gx = be.full((P, HW), np.nan)
    CPR, Hg = (W + 2 + 7) // 8, (H + 3) // 4 * 4
    dbytes, gbytes = pbytes, 2 * N * C * Hg * CPR * 16
    dplanes, gplanes, bscale = be.bytes_buf(dbytes), be.bytes_buf(gbytes), be.bytes_buf(4 * N)
    be.lib.instnorm_bwd_planes(be.ptr(d_x), be.ptr(d_st), be.ptr(d_gy), be.ptr(gymax), N, C, H, W, ACT_NONE, SLOPE, drop_p, 424242, 5, 1,
                               be.ptr(d_gx), be.ptr(dplanes), be.ptr(gplanes), be.ptr(bscale), None, be.stream)
    be.sync()
    gx = be.np(d_gx)
    assert np.all(np.isfinite(gx)), route
    # today's tolerance of case_resblock_planes_chain: 2e-5 x the sample's largest |gx|
    smax = np.repeat(np.abs(want_gx).reshape(N, -1).max(axis=1), C)
    check(be, route + " bwd", names, "gx", gx, want_gx, 2e-5 * smax, 0.0, yard_g)
    bb = _words(be, bscale, N).view(f32).astype(np.float64)
    assert np.all(bb >= np.abs(gx).reshape(N, -1).max(axis=1)), (route, "the backward scale word is below the true maximum")
    bs = (2.0 ** (11 - np.floor(np.log2(bb)))).reshape(N, 1, 1, 1)
    gx4 = gx.reshape(N, C, H, W)
    dp = _decode_planes(be.raw(dplanes)[:dbytes], N, C, H, W)
    gp = _decode_pixel_planes(be.raw(gplanes)[:gbytes], N, C, Hg, CPR)
    assert np.all(np.isfinite(dp)) and np.all(np.isfinite(gp)), route + ": a decoded gradient plane value is inf or NaN"
    want_dp, mag_dp = _dgrad_plane_content(gx4, True), _dgrad_plane_content(np.abs(gx4), True)
    err = np.abs((dp[0] + dp[1]) / bs - want_dp)
    assert np.all(err <= 2.0 ** -21 * mag_dp + 2.0 ** -23 / bs), (route, "data-gradient planes", float(err.max()))
    want_gp = np.zeros((N, C, Hg, CPR * 8))
    want_gp[:, :, :H, :W] = gx4
    err = np.abs((gp[0] + gp[1]) / bs - want_gp)
    assert np.all(err <= 2.0 ** -21 * np.abs(want_gp) + 2.0 ** -24 / bs), (route, "weight-gradient planes", float(err.max()))


def dump_record(path):
    import json
    with open(path, "w") as f:
        json.dump(RECORD, f)
