"""Backend-agnostic test bodies of nemar_svf_step_fwd / _bwd (csrc/integrate.hip: one scaling-and-squaring step on a displacement field,
forward and backward, and the chain of K steps that integrates a stationary velocity field), driven through tests/backends.py
(EmuBackend: host-emulated kernels, CPU tier; HipBackend: the gfx950 library, `-m gpu` tier).  Every buffer is guard-banded and
poisoned there, the workspace included (exactly the queried bytes; its scratch tail is filled with 0xA5 before every call, its zeroed
prefix must be zero after every call).

The truth is the definition of include/nemar_hip.h in float64 torch on the CPU (ref_step), written with explicit floor / clamp / gather
indexing so that H = 1 and W = 1 work; its gradient comes from autograd (clamp passes the gradient on min <= x <= max: zero along an axis
whose raw position was clamped).  The same code in float32 is the yardstick.  The rules (why each bound is what it is):
  forward   continuous, nothing excluded: max error in PIXELS (channel 0 times W/2, channel 1 times H/2) against float64 <= MARGIN
            (register_cases: 4) x the yardstick's — two fp32 evaluations of one formula in different rounding orders.
  backward  the position path is discontinuous where a raw (unclamped) position lies within BAND = 1e-3 px of an integer in [0, size-1],
            the clamp edges included (fp32 positions err by ~1e-5 px at these sizes: two evaluations may floor differently).  Such a texel
            is EXCLUDED from the comparison, and only that texel: the scatter weights are continuous.  Positions clamped from further out
            than BAND are unambiguous and stay in.  The float64 reference alone keeps the excluded share below the cap (0.01 at SIZES and
            the network's size, 0.03 at EDGES and THIN, used with amp 1.0 there) before the kernel is looked at.  Those caps describe
            s = 1 (float64, seeds 1 - 3: 0.003 - 0.006 at SIZES and the network's size, <= 0.020 at EDGES / THIN).  A scale |s| < 1
            shrinks the displacement to A = |s| amp size / 2 pixels along an axis, below one pixel at most of these cases (0.05 px
            at (35, 131), amp 0.1, s = -1/64): every texel then sits next to the integer it started from, and a smooth field spread over
            [-A, A] leaves about BAND / A of them inside the band per axis — a property of the case that no kernel changes (float64:
            up to 0.22 at SIZES, 0.27 at (1, 77)).  There the reference asserts SHARE_SCALED = 0.30 instead: more than two thirds of the
            texels are compared, and what s does to the excluded ones is covered bit for bit by case_bits (the call with (u, s) is
            s times the call with (s u, 1): s is a power of two, every product with it is exact).  On the kept texels
            max-abs error <= MARGIN x the yardstick's; where the yardstick's is 0 the kernel is exact.  The fixed-point image path
            rounds each contribution to 2^-40 of max |gout|: 2^-16 of an fp32 rounding, far inside the rule.
            accumulate = 1: truth = pre-fill + float64 gradient, yardstick = fp32(pre-fill + fp32 gradient): both sides add once.
  chain     forward of K steps against the float64 chain by the same MARGIN rule (the yardstick walks the same K steps in float32).
            The chain's gradient is proven by `backward` per step plus the bitwise identity of ops.integrate_velocity's backward with K
            manual step calls (tests/test_integrate_gpu.py): a direct float64 comparison would need exclusions that spread through the steps.
  folds     the float64 reference first shows that the case means something: the raw field folds on >= 10 % of the interior pixels and
            the float64 integrated field's smallest determinant (fold_cases.ref_fold: jacobian_tile.h's expression) is >= 0.03; only then
            the kernel's integrated field must show 0 folds under nemar_jacobian_stats and the raw field >= 10 %.
  inverse   r = u_- + u_+ o (id + u_-), evaluated in float64 on the host from the kernel's two fields, max over the interior
            amp max(H, W) / 2 + 2 pixels from the border, in pixels: <= 2 x the value the float64 reference gives for the same K (slack
            for fp32 against float64 on a quantity ~1e4 x the fp32 error), and the reference's value at K = 6 <= a quarter of K = 2's."""
import ctypes

import numpy as np
import pytest
import torch

from backends import both_poisons
from fold_cases import EDGES, SIZES, THIN, NETWORK, ref_fold
from register_cases import GRID_UNET, MARGIN, smooth_field
from regularity_cases import run_jac

BAND = 1e-3                                    # px
SHARE_SIZES, SHARE_EDGES = 0.01, 0.03          # s = 1
SHARE_SCALED = 0.30                            # |s| < 1: sub-pixel displacements (see above)
SCALES = (1.0, 1.0 / 16, -1.0 / 64)
AMPS = (0.1, 0.3, 1.0)
MIN_RAW_FOLDS, MIN_DET = 0.10, 0.03


def share_cap(size, s=1.0):
    if abs(s) != 1.0:
        return SHARE_SCALED
    return SHARE_SIZES if tuple(size) in [tuple(s) for s in SIZES] + [tuple(NETWORK)] else SHARE_EDGES


# ---- the float64 truth, and (dtype float32) the yardstick -------------------------------------------------------------------------------
def _step(u, s):
    """one step on a torch tensor u [N,2,H,W] in its own dtype -> (out, raw x, raw y)"""
    N, _, H, W = u.shape
    dt = u.dtype
    a = u * s
    rx = torch.arange(W, dtype=dt)[None, None, :] + a[:, 0] * (W / 2)
    ry = torch.arange(H, dtype=dt)[None, :, None] + a[:, 1] * (H / 2)
    px, py = rx.clamp(0, W - 1), ry.clamp(0, H - 1)
    x0, y0 = px.detach().floor().long(), py.detach().floor().long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    tx, ty = px - x0.to(dt), py - y0.to(dt)
    flat = a.reshape(N, 2, H * W)
    at = lambda yy, xx: flat.gather(2, (yy * W + xx).reshape(N, 1, H * W).expand(N, 2, H * W)).reshape(N, 2, H, W)
    ex, ey = 1 - tx, 1 - ty
    bil = at(y0, x0) * (ex * ey)[:, None] + at(y0, x1) * (tx * ey)[:, None] + at(y1, x0) * (ex * ty)[:, None] + at(y1, x1) * (tx * ty)[:, None]
    return a + bil, rx.detach(), ry.detach()


def ref_step(u, s, gout=None, dtype=torch.float64):
    """-> (out, gu or None, raw x, raw y) as float64 numpy, evaluated in `dtype`"""
    t = torch.tensor(np.asarray(u), dtype=dtype, requires_grad=gout is not None)
    out, rx, ry = _step(t, s)
    assert out.dtype == dtype
    gu = None
    if gout is not None:
        (out * torch.tensor(np.asarray(gout), dtype=dtype)).sum().backward()
        gu = t.grad.numpy().astype(np.float64)
    f64 = lambda x: x.detach().numpy().astype(np.float64)
    return f64(out), gu, f64(rx), f64(ry)


def scales_of(K, sign):
    return [sign / float(1 << K)] + [1.0] * (K - 1) if K > 0 else []


def ref_chain(v, K, sign=1.0, dtype=torch.float64):
    """integrate(v, K, sign) -> float64 numpy, evaluated in `dtype`; K = 0: sign * v"""
    u = torch.tensor(np.asarray(v), dtype=dtype)
    if K == 0:
        u = u * sign
    for s in scales_of(K, sign):
        u = _step(u, s)[0]
    return u.numpy().astype(np.float64)


def excluded_texels(rx, ry, H, W):
    """[N,H,W] True where the raw position lies within BAND of an integer in [0, size-1] along either axis"""
    def near(r, size):
        k = np.rint(r)
        return (np.abs(r - k) <= BAND) & (k >= 0) & (k <= size - 1)
    return near(rx, W) | near(ry, H)


def to_px(a, H, W):
    """offset units -> pixels, per channel"""
    return np.asarray(a, dtype=np.float64) * np.array([W / 2.0, H / 2.0])[None, :, None, None]


# ---- drivers ----------------------------------------------------------------------------------------------------------------------------------
def _fill_value(be):
    return np.array([be.poison], dtype=np.uint32).view(np.float32)[0]


def run_fwd(be, d_u, s, shape, d_out=None):
    """-> (out [N,2,H,W] float32 on the host, bit for bit; the device handle); pre-filled"""
    N, _, H, W = shape
    d_out = be.full(shape, _fill_value(be)) if d_out is None else d_out
    be.lib.svf_step_fwd(be.ptr(d_u), s, be.ptr(d_out), N, H, W, be.stream)
    return be.raw(d_out).view(np.float32).reshape(shape), d_out


def run_bwd(be, d_u, s, d_gout, shape, accumulate=0, d_gu=None):
    """-> gu [N,2,H,W] float32 on the host, bit for bit; pre-filled.  The workspace: exactly the queried bytes, guard-banded, the zeroed
    prefix zero, the scratch tail 0xA5; the prefix must come back zero"""
    N, _, H, W = shape
    d_gu = be.full(shape, _fill_value(be)) if d_gu is None else d_gu
    wsb, zb = int(be.lib.svf_step_bwd_workspace(N, H, W)), int(be.lib.svf_step_bwd_zeroed_bytes(N, H, W))
    assert 0 < zb <= wsb
    ws = be.bytes_buf(wsb)
    ws[zb:] = 0xA5
    be.lib.svf_step_bwd(be.ptr(d_u), s, be.ptr(d_gout), be.ptr(d_gu), accumulate, be.ptr(ws), wsb, N, H, W, be.stream)
    assert not be.raw(ws)[:zb].any(), "the zeroed part of the workspace is not zero after the call"
    return be.raw(d_gu).view(np.float32).reshape(shape)


def run_chain(be, v, K, sign=1.0):
    """integrate(v, K, sign) through K step calls -> (result float32 on the host, the K step inputs as device handles, the scales)"""
    shape = v.shape
    d_u = be.dev(v)
    inputs, scales = [], scales_of(K, sign)
    host = (np.float32(sign) * v).astype(np.float32)
    for s in scales:
        inputs.append(d_u)
        host, d_u = run_fwd(be, d_u, s, shape)
    return host, inputs, scales


def gaussian(seed, shape):
    return np.random.default_rng(1000 + seed).standard_normal(shape).astype(np.float32)


def _ratio(err, yard):
    return err / yard if yard else (0.0 if err == 0 else float('inf'))


# ---- 1. step forward ---------------------------------------------------------------------------------------------------------------------
def case_step_fwd(be, size, amp, seed=1, N=2):
    H, W = size
    shape = (N, 2, H, W)
    u = smooth_field(seed, N, H, W, amp)
    d_u = be.dev(u)
    for s in SCALES:
        want = ref_step(u, s)[0]
        yard = np.abs(to_px(ref_step(u, s, dtype=torch.float32)[0] - want, H, W)).max()
        got = run_fwd(be, d_u, s, shape)[0]
        assert np.all(np.isfinite(got)), (size, amp, s)
        err = np.abs(to_px(got.astype(np.float64) - want, H, W)).max()
        print("svf fwd %s amp %g s %g: kernel %.3e px  torch-fp32 %.3e px  ratio %.2f" % (size, amp, s, err, yard, _ratio(err, yard)))
        assert err <= MARGIN * yard, (size, amp, s, err, yard)


# ---- 2. step backward --------------------------------------------------------------------------------------------------------------------
def case_step_bwd(be, size, amp, seed=1, N=2):
    H, W = size
    shape = (N, 2, H, W)
    u = smooth_field(seed, N, H, W, amp)
    gout = gaussian(seed, shape)
    before = gaussian(seed + 7, shape)
    d_u, d_gout = be.dev(u), be.dev(gout)
    for s in SCALES:
        _, gu64, rx, ry = ref_step(u, s, gout)
        ex = excluded_texels(rx, ry, H, W)
        share = ex.mean()
        print("svf bwd %s amp %g s %g: float64 excludes %.4f of the texels (cap %.2f)" % (size, amp, s, share, share_cap(size, s)))
        assert share <= share_cap(size, s), (size, amp, s, share)
        gu32 = ref_step(u, s, gout, torch.float32)[1]
        keep = np.broadcast_to(~ex[:, None], shape)
        for accumulate in (0, 1):
            if accumulate:
                want = before.astype(np.float64) + gu64
                yard32 = (before + gu32.astype(np.float32)).astype(np.float64)
                got = run_bwd(be, d_u, s, d_gout, shape, 1, d_gu=be.dev(before))
            else:
                want, yard32 = gu64, gu32
                got = run_bwd(be, d_u, s, d_gout, shape)
            assert np.all(np.isfinite(got)), (size, amp, s, accumulate)
            yard = np.abs(yard32 - want)[keep].max()
            err = np.abs(got.astype(np.float64) - want)[keep].max()
            print("svf bwd %s amp %g s %g accumulate %d: kernel %.3e  torch-fp32 %.3e  ratio %.2f" % (size, amp, s, accumulate, err, yard, _ratio(err, yard)))
            assert err <= MARGIN * yard, (size, amp, s, accumulate, err, yard)


# ---- 3. bits -------------------------------------------------------------------------------------------------------------------------------
@both_poisons
def case_bits(be, size, amp=1.0, seed=3, N=2, K=4):
    H, W = size
    shape = (N, 2, H, W)
    u = smooth_field(seed, N, H, W, amp)
    gout = gaussian(seed, shape)
    d_u, d_gout = be.dev(u), be.dev(gout)
    bits = lambda a: np.asarray(a).view(np.uint32)
    fill = _fill_value(be)
    for s in (1.0, -1.0 / 64):
        out, out2 = run_fwd(be, d_u, s, shape)[0], run_fwd(be, d_u, s, shape)[0]
        gu, gu2 = run_bwd(be, d_u, s, d_gout, shape), run_bwd(be, d_u, s, d_gout, shape)
        # (the outputs were pre-filled with the poison in force: an element that was not written would show — as a NaN, or as 1e38)
        assert np.all(np.isfinite(out)) and np.all(np.isfinite(gu)) and not np.any(out == fill) and not np.any(gu == fill), "an output element was not written"
        assert np.array_equal(bits(out), bits(out2)) and np.array_equal(bits(gu), bits(gu2)), "two calls, different bits"
        before = gaussian(seed + 7, shape)
        gu3 = run_bwd(be, d_u, s, d_gout, shape, 1, d_gu=be.dev(before))
        assert np.array_equal(bits(gu3), bits(before + gu)), "accumulate: gu is not what was there plus the gradient, rounded once"
        if s != 1.0:                               # s is a power of two: the call with (u, s) is s times the call with (s u, 1), exactly
            d_su = be.dev(np.float32(s) * u)
            assert np.array_equal(bits(out), bits(run_fwd(be, d_su, 1.0, shape)[0])), "step_fwd(u, s) is not step_fwd(s u, 1)"
            assert np.array_equal(bits(gu), bits(np.float32(s) * run_bwd(be, d_su, 1.0, d_gout, shape))), "step_bwd(u, s) is not s step_bwd(s u, 1)"
    plus = run_chain(be, -u, K, 1.0)[0]
    minus = run_chain(be, u, K, -1.0)[0]
    assert np.array_equal(bits(plus), bits(minus)), "integrate(v, K, -1) is not integrate(-v, K, +1) bit for bit"
    # a zero field samples its own texel: the true identity, exactly
    zero = run_fwd(be, be.zeros(*shape), 1.0, shape)[0]
    assert not zero.any()


# ---- 4. bounds -----------------------------------------------------------------------------------------------------------------------------
@both_poisons
def case_bounds(be, size=(17, 65), N=2, seed=5):
    """NaN, +-inf and +-1e30 entries in the field and in gout: both calls return NEMAR_OK and every guard band is intact (be.lib checks
    them after each call; the reads are bounded by the clamp before the integer conversion).  Values are not compared"""
    H, W = size
    shape = (N, 2, H, W)
    rng = np.random.default_rng(seed)
    u = smooth_field(seed, N, H, W, 1.0)
    gout = gaussian(seed, shape)
    odd = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], dtype=np.float32)
    for a in (u, gout):
        idx = rng.choice(a.size, size=a.size // 8, replace=False)
        a.reshape(-1)[idx] = odd[rng.integers(0, odd.size, idx.size)]
    d_u, d_gout = be.dev(u), be.dev(gout)
    for s in (1.0, -1.0 / 64, 0.0):
        run_fwd(be, d_u, s, shape)
        run_bwd(be, d_u, s, d_gout, shape)
        run_bwd(be, d_u, s, d_gout, shape, 1, d_gu=be.dev(gaussian(seed + 1, shape)))
    # and the workspace serves a clean call afterwards as a fresh one does (run_bwd asserts its zeroed bytes)
    be.check_guards("case_bounds")


def case_refusals(be):
    """NEMAR_EINVAL (-1), a message, and nothing launched: the outputs keep their fill"""
    from nemar_amd._lib import NemarHipError
    N, H, W = 2, 12, 16
    d_u, d_gout = be.zeros(N, 2, H, W), be.full((N, 2, H, W), 1.0)
    d_out, d_gu = be.full((N, 2, H, W), 7.0), be.full((N, 2, H, W), 7.0)
    wsb, zb = int(be.lib.svf_step_bwd_workspace(N, H, W)), int(be.lib.svf_step_bwd_zeroed_bytes(N, H, W))
    assert 0 < zb <= wsb and zb >= 8 * N * 2 * H * W
    for q in (be.lib.svf_step_bwd_workspace, be.lib.svf_step_bwd_zeroed_bytes):
        assert int(q(N, H, 0)) == 0 and int(q(0, H, W)) == 0 and int(q(N, -1, W)) == 0
    ws = be.bytes_buf(wsb + 8)
    off2 = lambda p: ctypes.c_void_p(p.value + 2)
    f_names = ("u", "s", "out", "N", "H", "W")
    f_good = [be.ptr(d_u), 1.0, be.ptr(d_out), N, H, W]
    b_names = ("u", "s", "gout", "gu", "acc", "ws", "wsb", "N", "H", "W")
    b_good = [be.ptr(d_u), 1.0, be.ptr(d_gout), be.ptr(d_gu), 0, be.ptr(ws), wsb, N, H, W]

    def refused(which, **change):
        names, good, fn = (f_names, f_good, be.lib.svf_step_fwd) if which == "fwd" else (b_names, b_good, be.lib.svf_step_bwd)
        args = [change.get(k, v) for k, v in zip(names, good)]
        with pytest.raises(NemarHipError, match=r"failed \(-1\): svf_step_%s: \S" % which):
            fn(*args, be.stream)

    for which, names, good, ptrs in (("fwd", f_names, f_good, ("u", "out")), ("bwd", b_names, b_good, ("u", "gout", "gu", "ws"))):
        for k in ptrs:                                            # required pointers: null, misaligned
            refused(which, **{k: None})
            refused(which, **{k: off2(good[names.index(k)])})
        for k in ("N", "H", "W"):                                 # non-positive sizes
            refused(which, **{k: 0})
            refused(which, **{k: -3})
        refused(which, N=65536)
        refused(which, H=1 << 16, W=1 << 15)                      # H * W = 2^31
    refused("fwd", out=f_good[0])                                 # out is the operand
    refused("bwd", gu=b_good[0])                                  # gu is u
    refused("bwd", gu=b_good[2])                                  # gu is gout
    refused("bwd", wsb=wsb - 1)                                   # a short workspace
    refused("bwd", wsb=0)
    refused("bwd", ws=ctypes.c_void_p(be.ptr(ws).value + 4))      # the accumulator is 64-bit
    be.sync()
    assert np.all(be.np(d_out) == 7.0) and np.all(be.np(d_gu) == 7.0) and not be.raw(ws).any()
    # and the good arguments are good: a zero field is the identity, its gradient is gout itself (direct term; the image path lands
    # on the texel's own corner with weight 1; the position path differences a zero field) = 2 gout
    be.lib.svf_step_fwd(*f_good, be.stream)
    be.lib.svf_step_bwd(*b_good, be.stream)
    assert np.all(be.np(d_out) == 0) and np.all(be.np(d_gu) == 2.0) and not be.raw(ws)[:zb].any()


# ---- 5. chain (forward) --------------------------------------------------------------------------------------------------------------------
def check_chain_fwd(got, v, K, sign, what):
    """the MARGIN rule on a chain's result `got` (float32 numpy) against the float64 chain, in pixels"""
    H, W = v.shape[2:]
    want = ref_chain(v, K, sign)
    yard = np.abs(to_px(ref_chain(v, K, sign, torch.float32) - want, H, W)).max()
    err = np.abs(to_px(got.astype(np.float64) - want, H, W)).max()
    print("svf chain %s: kernel %.3e px  torch-fp32 %.3e px  ratio %.2f" % (what, err, yard, _ratio(err, yard)))
    assert np.all(np.isfinite(got)), what
    assert err <= MARGIN * yard, (what, err, yard)


def case_chain_fwd(be, size, K, amp=0.3, seed=2, N=2):
    H, W = size
    v = smooth_field(seed, N, H, W, amp)
    for sign in (1.0, -1.0):
        got = run_chain(be, v, K, sign)[0]
        check_chain_fwd(got, v, K, sign, "%s amp %g K %d sign %+g" % (size, amp, K, sign))


# ---- 6. what it is for ---------------------------------------------------------------------------------------------------------------------
def reference_says_it_matters(v, K, what):
    """the float64 statement alone: the raw field folds, the integrated one does not, with room"""
    det_raw = ref_fold(v, 0.0)[0]
    raw_share = (det_raw <= 0).mean()
    det_int = ref_fold(ref_chain(v, K).astype(np.float32), 0.0)[0]
    print("svf folds %s: float64 raw field folds on %.3f of the interior pixels; integrated: min det %.4f" % (what, raw_share, det_int.min()))
    assert raw_share >= MIN_RAW_FOLDS, (what, raw_share)
    assert det_int.min() >= MIN_DET, (what, det_int.min())


def case_no_folds(be, size, seed, K=6, amp=1.0, N=2):
    H, W = size
    what = "%s seed %d amp %g K %d" % (size, seed, amp, K)
    v = smooth_field(seed, N, H, W, amp)
    reference_says_it_matters(v, K, what)
    got = run_chain(be, v, K)[0]
    counts_raw = run_jac(be, be.dev(v), GRID_UNET, ((H, W), (H, W)), N, det_map=False)[1]
    counts_int = run_jac(be, be.dev(got), GRID_UNET, ((H, W), (H, W)), N, det_map=False)[1]
    print("svf folds %s: nemar_jacobian_stats raw %s, integrated %s of %s interior pixels" % (what, counts_raw[:, 1], counts_int[:, 1], counts_raw[:, 0]))
    assert counts_raw[:, 1].sum() >= MIN_RAW_FOLDS * counts_raw[:, 0].sum(), (what, counts_raw)
    assert counts_int[:, 1].sum() == 0, (what, counts_int)


# ---- 7. inverse ----------------------------------------------------------------------------------------------------------------------------
def inverse_residual_px(u_plus, u_minus, amp):
    """max over the interior of |u_- + u_+ o (id + u_-)| in pixels, float64 on the host"""
    up, um = np.asarray(u_plus, dtype=np.float64), np.asarray(u_minus, dtype=np.float64)
    H, W = up.shape[2:]
    composed = _step_compose(torch.tensor(up), torch.tensor(um)).numpy()
    r = to_px(composed, H, W)
    b = int(np.ceil(amp * max(H, W) / 2 + 2))
    assert H > 2 * b and W > 2 * b
    return np.sqrt((r ** 2).sum(1))[:, b:H - b, b:W - b].max()


def _step_compose(up, um):
    """u_- + u_+ o (id + u_-): the step's own sampling rule with two different fields, float64"""
    N, _, H, W = up.shape
    dt = up.dtype
    px = (torch.arange(W, dtype=dt)[None, None, :] + um[:, 0] * (W / 2)).clamp(0, W - 1)
    py = (torch.arange(H, dtype=dt)[None, :, None] + um[:, 1] * (H / 2)).clamp(0, H - 1)
    x0, y0 = px.floor().long(), py.floor().long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    tx, ty = px - x0.to(dt), py - y0.to(dt)
    flat = up.reshape(N, 2, H * W)
    at = lambda yy, xx: flat.gather(2, (yy * W + xx).reshape(N, 1, H * W).expand(N, 2, H * W)).reshape(N, 2, H, W)
    ex, ey = 1 - tx, 1 - ty
    return um + at(y0, x0) * (ex * ey)[:, None] + at(y0, x1) * (tx * ey)[:, None] + at(y1, x0) * (ex * ty)[:, None] + at(y1, x1) * (tx * ty)[:, None]


def case_inverse(be, size, amp=0.1, seed=1, N=2):
    H, W = size
    v = smooth_field(seed, N, H, W, amp)
    ref = {K: inverse_residual_px(ref_chain(v, K, 1.0), ref_chain(v, K, -1.0), amp) for K in (2, 6)}
    print("svf inverse %s amp %g: float64 residual %.4f px at K = 2, %.4f px at K = 6" % (size, amp, ref[2], ref[6]))
    assert ref[6] <= 0.25 * ref[2], ref
    for K in (2, 6):
        got = inverse_residual_px(run_chain(be, v, K, 1.0)[0], run_chain(be, v, K, -1.0)[0], amp)
        print("svf inverse %s amp %g K %d: kernel residual %.4f px, float64 %.4f px" % (size, amp, K, got, ref[K]))
        assert got <= 2.0 * ref[K], (size, K, got, ref[K])
