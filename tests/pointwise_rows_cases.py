"""The row-vector forms of the plain data-movement passes (nemar_tune key 47: csrc/pointwise.hip 2x resize forward / backward and max-pool
backward, csrc/conv.hip reflect fold; the bias sums have no row form — their case pins that the switch leaves them alone) against the one-element-per-lane kernels they stand in front of and against the
float64 oracle.  Written against tests/backends.py: tests/test_pointwise_rows_emu.py runs the bodies on the host emulator,
tests/test_pointwise_rows_gpu.py on the gfx950 library.

Every entry point is called three ways on the same data:
  rows       16-byte aligned tensors, switch at its default (1): the row-vector form where the shape allows it;
  displaced  every tensor one float past a 16-byte boundary: the alignment test of the dispatch sends the call to the general form;
  switch 0   aligned tensors, nemar_tune(47, 0): the general form everywhere.
The three results must agree BIT FOR BIT (the raw bytes are compared, so NaN payloads and signed zeros count), the first one with the
oracle at the tolerances of kernel_cases.case_pointwise, and every call runs under the guard bands of the backend — each case under both
poisons (max-pool's comparisons and the conv kernels' maxima skip NaN by design)."""
import contextlib
import ctypes

import numpy as np

import kernel_cases as KC
from backends import both_poisons
from kernel_cases import _assert_close
from oracle import ops_np as O

KEY = 47
WAYS = (("rows", False, 1), ("displaced", True, 1), ("switch 0", False, 0))

RESIZE_SHAPES = ((2, 4), (3, 8), (8, 12), (5, 16), (4, 6))       # border-only planes, one interior run, W % 8 == 4, odd H; (4, 6): W % 4 != 0, general form
RESIZE_PLANES = 3
POOL_SHAPES = ((2, 8), (4, 8), (5, 8), (6, 16), (4, 12))
POOL_PLANES = 6
BIAS_SHAPES = ((1, 2, 16), (2, 3, 4100), (3, 5, 8192))           # below one chunk of 4096, a ragged second chunk, whole chunks
FOLD_SIZES = tuple((h, w) for w in (8, 12) for h in (4, 5, 9))
# the 16-bit route takes no padded row narrower than 24 texels (csrc/conv_s16g.hip nemar_s16g_plan: OW >= 24, here W + 2), so widths 8 and 12
# stay on the exact route whatever the thresholds; its smallest widths with W % 4 == 0 are 24 (whole 8-float runs) and 28 (W % 8 == 4)
FOLD_SIZES_S16G = tuple((h, w) for w in (24, 28) for h in (4, 5, 9))
# (N, C, K): the smallest reflect 3x3 stride-1 data gradients whose plan ends in fold_padded (csrc/conv_route.h plan_dgrad) —
#   exact     C > 4 and a padded plane of <= 1296 texels: the padded-domain form of the exact-fp32 route (fold_small); K * 9 < 16 reduction
#             stages of 16, so the launch is not split and the plain fold pass (not the sum-and-fold pass) writes gx;
#   s16g      the work threshold of the 16-bit route lifted (kernel_cases.s16g_route): S16G_FOLD; one 16-channel chunk, 8 >= 5 output rows.
FOLD_ROUTES = {"exact": (1, 8, 8), "s16g": (1, 8, 16)}
FOLD_CASES = tuple(("exact", s) for s in FOLD_SIZES) + tuple(("s16g", s) for s in FOLD_SIZES_S16G)


@contextlib.contextmanager
def switch(be, value):
    be.lib.tune(KEY, value)
    try:
        yield
    finally:
        be.sync()
        be.lib.tune(KEY, 1)


class _Placed:
    """a float32 array on the device, 16-byte aligned or one float past a 16-byte boundary (`held` keeps the whole block)"""

    def __init__(self, be, a, displaced, role):
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        self.be, self.n, self.displaced = be, a.size, displaced
        if displaced:
            self.held = be.dev(np.concatenate([np.float32([0.625]), a]), role=role)
            self.h = be.sub(self.held, 1, a.size + 1)
        else:
            self.held = self.h = be.dev(a, role=role)

    @property
    def ptr(self):
        return self.be.ptr(self.h)

    def bits(self):
        """the payload's bytes; the float in front of a displaced payload must be what it was"""
        raw = self.be.raw(self.held)
        if self.displaced:
            assert np.array_equal(raw[:4], np.float32([0.625]).view(np.uint8)), "the float in front of a displaced tensor changed"
            raw = raw[4:]
        return raw


def three_ways(be, launch, inputs, out_init, what):
    """launch(in_ptr..., out_ptr) on `inputs` (float32 arrays; None = an absent optional tensor) three ways; out_init: the output's
    contents before the call.  Returns {way: float32 result}; asserts nothing but the guards."""
    res = {}
    for way, displaced, value in WAYS:
        ins = [None if a is None else _Placed(be, a, displaced, "%s in" % what) for a in inputs]
        out = _Placed(be, out_init, displaced, "%s out" % what)
        with switch(be, value):
            launch(*[None if p is None else p.ptr for p in ins], out.ptr)
        res[way] = out.bits().view(np.float32)
    return res


def same_bits(res, what, ways=("displaced", "switch 0")):
    for way in ways:
        a, b = res["rows"].view(np.uint32), res[way].view(np.uint32)
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, "%s: rows and %s differ at %d of %d elements, first at %d (%r / %r)" % (
            what, way, bad.size, a.size, bad[0], res["rows"][bad[0]], res[way][bad[0]])


# ---- resize, exactly 2x up ------------------------------------------------------------------------------------------------------------
@both_poisons
def case_resize_up2(be, H, W, seed=0, planes=RESIZE_PLANES):
    rng = np.random.default_rng(seed)
    Ho, Wo = 2 * H, 2 * W
    x = rng.standard_normal((1, planes, H, W)).astype(np.float32)
    nan_out = np.full(planes * Ho * Wo, np.nan, np.float32)
    res = three_ways(be, lambda px, py: be.lib.bilinear_fwd(px, py, planes, H, W, Ho, Wo, be.stream), [x], nan_out, "bilinear_fwd")
    same_bits(res, "bilinear_fwd %dx%d" % (H, W))
    _assert_close(res["rows"].astype(np.float64).reshape(1, planes, Ho, Wo), O.bilinear_resize_fwd(x.astype(np.float64), Ho, Wo), atol=2e-6,
                  what="bilinear_fwd %dx%d" % (H, W))
    gy = rng.standard_normal((1, planes, Ho, Wo)).astype(np.float32)
    nan_in = np.full(planes * H * W, np.nan, np.float32)
    res = three_ways(be, lambda pg, pgx: be.lib.bilinear_bwd(pg, pgx, planes, H, W, Ho, Wo, be.stream), [gy], nan_in, "bilinear_bwd")
    same_bits(res, "bilinear_bwd %dx%d" % (H, W))
    _assert_close(res["rows"].astype(np.float64).reshape(1, planes, H, W), O.bilinear_resize_bwd(gy.astype(np.float64), H, W), atol=5e-6,
                  what="bilinear_bwd %dx%d" % (H, W))


# ---- max-pool backward ------------------------------------------------------------------------------------------------------------------
@both_poisons
def case_maxpool_bwd(be, H, W, with_addend, seed=0, planes=POOL_PLANES):
    rng = np.random.default_rng(seed)
    Ho, Wo = H // 2, W // 2
    x = (rng.integers(-2, 3, (1, planes, H, W)) * 0.25).astype(np.float32)        # five values over four texels: ties in most windows (tie_positions)
    gy = rng.standard_normal((1, planes, Ho, Wo)).astype(np.float32)
    add = rng.standard_normal((1, planes, H, W)).astype(np.float32) if with_addend else None
    nan_out = np.full(planes * H * W, np.nan, np.float32)
    res = three_ways(be, lambda px, pg, pa, po: be.lib.maxpool2_bwd(px, pg, pa, po, planes, H, W, be.stream), [x, gy, add], nan_out,
                     "maxpool2_bwd")
    same_bits(res, "maxpool2_bwd %dx%d addend %d" % (H, W, with_addend))
    want = O.maxpool2_bwd(x.astype(np.float64), gy.astype(np.float64))
    got = res["rows"].astype(np.float64).reshape(1, planes, H, W)
    if with_addend:
        _assert_close(got, want + add, atol=1e-6, what="maxpool2_bwd+addend %dx%d" % (H, W))
    else:
        _assert_close(got, want, atol=0, what="maxpool2_bwd %dx%d" % (H, W))


def tie_positions(H, W, seed=0, planes=POOL_PLANES):
    """which (row, column) of a window is tied with the window's maximum, over the case's data: all four must occur"""
    rng = np.random.default_rng(seed)
    x = (rng.integers(-2, 3, (1, planes, H, W)) * 0.25)[0, :, :H // 2 * 2, :W // 2 * 2]
    win = x.reshape(planes, H // 2, 2, W // 2, 2).transpose(0, 1, 3, 2, 4).reshape(-1, 4)
    tied = (win == win.max(axis=1, keepdims=True)) & ((win == win.max(axis=1, keepdims=True)).sum(axis=1, keepdims=True) > 1)
    return tied.any(axis=0)


# ---- bias sums ------------------------------------------------------------------------------------------------------------------------------
@both_poisons
def case_bias_sums(be, N, C, HW, seed=0):
    """nemar_bias_grad: gb[c] += sum over samples and texels (one kernel, whatever the switch says).  The kernel itself adds in another order when the planes are not
    16-byte aligned (one accumulator, one float per lane), so the displaced call is held to the oracle only — at
    guard_cases.case_bias_grad's tolerance — and rows / switch 0 to each other bit for bit."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((N, C, HW)).astype(np.float32)
    wsb = be.lib.bias_grad_workspace(N, C, HW)
    ws = be.bytes_buf(wsb)
    res = three_ways(be, lambda pg, pgb: be.lib.bias_grad(pg, pgb, N, C, HW, be.ptr(ws), wsb, be.stream), [g], np.full(C, -0.25, np.float32),
                     "bias_grad")
    same_bits(res, "bias_grad %r" % ((N, C, HW),), ways=("switch 0",))
    want = g.astype(np.float64).sum(axis=(0, 2)) - 0.25
    for way in res:
        _assert_close(res[way].astype(np.float64), want, atol=2e-5 * np.sqrt(N * HW), rtol=2e-5, what="bias_grad %r %s" % ((N, C, HW), way))


# ---- reflect fold behind the padded-domain data gradient ---------------------------------------------------------------------------------------
def _dgrad_three_ways(be, N, C, K, H, W, R, pad, with_addend, seed):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((K, C, R, R)) / np.sqrt(K * R * R)).astype(np.float32)
    gy = rng.standard_normal((N, K, H, W)).astype(np.float32)
    add = rng.standard_normal((N, C, H, W)).astype(np.float32) if with_addend else None
    want, _, _ = O.conv2d_bwd(np.zeros((N, C, H, W)), w.astype(np.float64), gy.astype(np.float64), 1, pad, "reflect")
    d_gy, d_w = be.dev(gy), be.dev(w)
    wsb = be.lib.conv2d_bwd_data_workspace(N, C, H, W, K, R, R, 1, pad, KC.PAD_REFLECT)
    ws = be.bytes_buf(wsb)
    if with_addend:
        assert be.lib.conv2d_bwd_data_addend_ok(N, C, H, W, K, R, R, 1, pad, KC.PAD_REFLECT) == 1, "the plan does not end in a fold pass"
    routes = []

    def launch(padd, pgx):
        from nemar_amd._lib import ConvExtras
        e = ConvExtras()
        e.addend = padd.value if padd is not None else None
        be.lib.conv2d_bwd_data_ex(be.ptr(d_gy), be.ptr(d_w), None, 0, 0.0, pgx, C, None, 0, N, H, W, K, H, W, R, R, 1, pad, KC.PAD_REFLECT,
                                  be.ptr(ws), wsb, 0, be.stream, ctypes.byref(e))
        routes.append(be.lib.last_route())

    res = three_ways(be, launch, [add], np.full(N * C * H * W, np.nan, np.float32), "conv2d_bwd_data (fold)")
    return res, (want + add if with_addend else want), routes


@both_poisons
def case_fold(be, route, H, W, with_addend, seed=0):
    N, C, K = FOLD_ROUTES[route]
    what = "fold %s %dx%d addend %d" % (route, H, W, with_addend)
    if route == "s16g":
        with KC.s16g_route(be):
            res, want, routes = _dgrad_three_ways(be, N, C, K, H, W, 3, 1, with_addend, seed)
        assert routes == [3, 3, 3], "%s: routes %r, not the general 16-bit-pipe route" % (what, routes)
    else:
        res, want, routes = _dgrad_three_ways(be, N, C, K, H, W, 3, 1, with_addend, seed)
        assert routes == [0, 0, 0], "%s: routes %r, not the exact-fp32 route" % (what, routes)
    same_bits(res, what)
    _assert_close(res["rows"].astype(np.float64).reshape(want.shape), want, atol=2e-5, rtol=2e-5, what=what)


@both_poisons
def case_fold_pad3(be, H=9, W=12, seed=0):
    """7x7 / pad 3 reflect on the padded domain (4 reduction channels: an unsplit launch, then the plain fold pass): pad != 1 stays on the
    general kernel, whatever the switch says"""
    res, want, routes = _dgrad_three_ways(be, 1, 8, 4, H, W, 7, 3, False, seed)
    assert len(set(routes)) == 1, routes
    same_bits(res, "fold pad 3")
    _assert_close(res["rows"].astype(np.float64).reshape(want.shape), want, atol=2e-5, rtol=2e-5, what="fold pad 3")
