"""Backend-agnostic test bodies of the BatchNorm entry points (nemar_batchnorm_*, csrc/batchnorm.hip), driven through tests/backends.py
(EmuBackend: host-emulated kernels, CPU tier; HipBackend: the gfx950 library, `-m gpu` tier) and compared with float64 numpy
restatements of nn.BatchNorm2d(affine=True, track_running_stats=True) written here."""
import numpy as np

from backends import both_poisons
from kernel_cases import _assert_close

ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
EPS, MOM, SLOPE = 1e-5, 0.1, 0.2


def _i64(be, v):
    return be.dev_i64(np.array([v], dtype=np.int64))


def _i64_value(be, t):
    return int(be.np(t)[0])


def _act(z, act):
    if act == ACT_RELU:
        return np.maximum(z, 0.0)
    if act == ACT_LRELU:
        return np.where(z > 0, z, z * SLOPE)
    return z


def _act_d(z, act):
    if act == ACT_RELU:
        return (z > 0).astype(np.float64)
    if act == ACT_LRELU:
        return np.where(z > 0, 1.0, SLOPE)
    return np.ones_like(z)


def ref_forward(x, gamma, beta, rm, rv, S, act, residual=None):
    """float64 BatchNorm2d training forward per segment (S separate calls of the reference's layer) -> y, mean[S,C], rstd[S,C], rm, rv"""
    x = x.astype(np.float64)
    N = x.shape[0]
    Ns = N // S
    rm, rv = rm.astype(np.float64).copy(), rv.astype(np.float64).copy()
    y = np.empty_like(x)
    means, rstds = [], []
    for s in range(S):
        xs = x[s * Ns:(s + 1) * Ns]
        m = xs.mean(axis=(0, 2, 3))
        v = xs.var(axis=(0, 2, 3))
        M = xs.size // xs.shape[1]
        rstd = 1.0 / np.sqrt(v + EPS)
        z = (xs - m[None, :, None, None]) * (rstd * gamma)[None, :, None, None] + beta[None, :, None, None]
        y[s * Ns:(s + 1) * Ns] = _act(z, act)
        rm = (1 - MOM) * rm + MOM * m
        rv = (1 - MOM) * rv + MOM * v * M / (M - 1)
        means.append(m)
        rstds.append(rstd)
    if residual is not None:
        y = y + residual
    return y, np.array(means), np.array(rstds), rm, rv


def ref_backward(x, gy, gamma, mean, rstd, S, act_mask, training=True):
    """-> gx, dgamma, dbeta; act_mask: act'(z) per element (taken from z recomputed in float32 as the kernel does, so the two sides agree
    on which side of zero every element is)"""
    x, gy = x.astype(np.float64), gy.astype(np.float64)
    N = x.shape[0]
    Ns = N // S
    gx = np.empty_like(x)
    dg = np.zeros(x.shape[1])
    db = np.zeros(x.shape[1])
    for s in range(S):
        sl = slice(s * Ns, (s + 1) * Ns)
        r = rstd[s][None, :, None, None]
        xh = (x[sl] - mean[s][None, :, None, None]) * r
        g = gy[sl] * act_mask[sl]
        sg, sgx = g.sum(axis=(0, 2, 3)), (g * xh).sum(axis=(0, 2, 3))
        dg += sgx
        db += sg
        M = g.size // g.shape[1]
        if training:
            gx[sl] = gamma[None, :, None, None] * r * (g - (sg / M)[None, :, None, None] - xh * (sgx / M)[None, :, None, None])
        else:
            gx[sl] = gamma[None, :, None, None] * r * g
    return gx, dg, db


def _z32(x, gamma, beta, mean, rstd, S):
    """z = (x - mean) * scale + beta in float32 with the kernel's operation order (scale = gamma * rstd)"""
    f = np.float32
    N = x.shape[0]
    Ns = N // S
    z = np.empty_like(x, dtype=f)
    for s in range(S):
        sc = (gamma.astype(f) * rstd[s].astype(f)).astype(f)
        d = (x[s * Ns:(s + 1) * Ns] - mean[s].astype(f)[None, :, None, None]).astype(f)
        z[s * Ns:(s + 1) * Ns] = (d * sc[None, :, None, None]).astype(f) + beta.astype(f)[None, :, None, None]
    return z


BN_FAMILIES = ("plain", "offset", "first_outlier", "first_outlier_far", "last_outlier", "spike", "constant", "tiny", "mixed")


def _family_x(rng, N, C, H, W, family):
    """the plane families of tests/norm_cases.py with the statistics per channel over (N, H, W)"""
    if family == "plain":
        return rng.standard_normal((N, C, H, W)) * 1.5 + rng.standard_normal((1, C, 1, 1)) * 2
    if family == "constant":                                # uneven over the samples: sample 0 is 0, every other sample 1 — the merge of
        return np.broadcast_to((np.arange(N) > 0).astype(np.float64).reshape(N, 1, 1, 1), (N, C, H, W)).copy()   # per-piece (mean, M2) pairs
    if family == "spike":
        x = np.zeros((N, C, H, W))
        x[N - 1, np.arange(C), (np.arange(C) * 3 + H // 3) % H, (np.arange(C) * 5 + W // 2) % W] = 5.0
        return x
    x = rng.standard_normal((N, C, H, W))
    if family == "offset":                                  # a different offset per channel
        x += (1000.0 / (1 + np.arange(C)) * (-1.0) ** np.arange(C)).reshape(1, C, 1, 1)
    elif family == "first_outlier":                         # element 0 of sample 0
        x[0, :, 0, 0] = 30.0
    elif family == "first_outlier_far":
        x[0, :, 0, 0] = 1000.0
    elif family == "last_outlier":
        x[-1, :, -1, -1] = -30.0
    elif family == "tiny":
        x = 1e-4 * x + 1e-2
    elif family == "mixed":
        x *= (10.0 ** (((np.arange(C) * 5) % 7) - 3.0)).reshape(1, C, 1, 1)
    else:
        raise ValueError(family)
    return x


def _inputs(N, C, H, W, seed, family="plain"):
    rng = np.random.default_rng(seed)
    x = _family_x(rng, N, C, H, W, family).astype(np.float32)
    gamma = (1.0 + 0.3 * rng.standard_normal(C)).astype(np.float32)
    gamma[0] = -abs(gamma[0])                       # a negative scale: the sign of xhat is not the sign of z
    beta = (0.2 * rng.standard_normal(C)).astype(np.float32)
    rm = (0.1 * rng.standard_normal(C)).astype(np.float32)
    rv = (1.0 + 0.5 * rng.uniform(size=C)).astype(np.float32)
    gy = rng.standard_normal((N, C, H, W)).astype(np.float32)
    res = rng.standard_normal((N, C, H, W)).astype(np.float32)
    return x, gamma, beta, rm, rv, gy, res


def _ws(be, N, C, HW, S):
    return be.bytes_buf(int(be.lib.batchnorm_workspace(N, C, HW, S)))


def run_train(be, d_x, d_res, d_g, d_b, d_rm, d_rv, cnt, N, C, HW, S, act, p=0.0, seed=0, off=0, words=None, ws=None):
    d_y = be.full((N, C, HW), np.nan)
    saved = be.full((2, S, C), np.nan)
    ws = ws if ws is not None else _ws(be, N, C, HW, S)
    be.lib.batchnorm_fwd_train(be.ptr(d_x), be.ptr(d_res), be.ptr(d_y), be.ptr(d_g), be.ptr(d_b), be.ptr(d_rm), be.ptr(d_rv), be.ptr(cnt),
                               be.ptr(saved), N, C, HW, S, EPS, MOM, act, SLOPE, p, seed, off, be.ptr(words), be.ptr(ws),
                               int(be.lib.batchnorm_workspace(N, C, HW, S)), be.stream)
    return d_y, saved


def run_bwd(be, d_x, d_gy, d_g, d_b, saved, gw, gb, N, C, HW, S, training, act, p=0.0, seed=0, off=0, want_gx=True):
    d_gx = be.full((N, C, HW), np.nan) if want_gx else None
    ws = _ws(be, N, C, HW, S)
    be.lib.batchnorm_bwd(be.ptr(d_x), be.ptr(d_gy), be.ptr(d_gx), be.ptr(d_g), be.ptr(d_b), be.ptr(saved), be.ptr(gw), be.ptr(gb),
                         N, C, HW, S, int(training), act, SLOPE, p, seed, off, be.ptr(ws), int(be.lib.batchnorm_workspace(N, C, HW, S)),
                         be.stream)
    return d_gx


def case_batchnorm_train(be, N, C, H, W, S, act, residual=False, seed=0):
    """training forward (statistics, running statistics, counter, output) and backward (gx, accumulated dgamma / dbeta) against float64"""
    x, gamma, beta, rm, rv, gy, res = _inputs(N, C, H, W, seed)
    HW = H * W
    d_x, d_gy, d_g, d_b = be.dev(x), be.dev(gy), be.dev(gamma), be.dev(beta)
    d_res = be.dev(res) if residual else None
    d_rm, d_rv, cnt = be.dev(rm.copy()), be.dev(rv.copy()), _i64(be, 7)
    d_y, saved = run_train(be, d_x, d_res, d_g, d_b, d_rm, d_rv, cnt, N, C, HW, S, act)
    want, m, rstd, wrm, wrv = ref_forward(x, gamma.astype(np.float64), beta.astype(np.float64), rm, rv, S, act,
                                          res.astype(np.float64) if residual else None)
    sv = be.np(saved)
    _assert_close(sv[0], m, atol=2e-5, rtol=1e-5, what="batchnorm mean")
    _assert_close(sv[1], rstd, atol=0, rtol=3e-5, what="batchnorm rstd")
    _assert_close(be.np(d_y).reshape(x.shape), want, atol=5e-5, rtol=3e-5, what="batchnorm_fwd_train")
    _assert_close(be.np(d_rm), wrm, atol=2e-6, rtol=1e-5, what="running_mean")
    _assert_close(be.np(d_rv), wrv, atol=2e-6, rtol=3e-5, what="running_var")
    assert _i64_value(be, cnt) == 7 + S
    # backward, accumulating into non-zero gradients
    gw0 = np.linspace(-1, 1, C).astype(np.float32)
    gb0 = np.linspace(2, 3, C).astype(np.float32)
    gw, gb = be.dev(gw0.copy()), be.dev(gb0.copy())
    d_gx = run_bwd(be, d_x, d_gy, d_g, d_b, saved, gw, gb, N, C, HW, S, True, act)
    mask = _act_d(_z32(x, gamma, beta, sv[0], sv[1], S), act)
    wgx, wdg, wdb = ref_backward(x, gy, gamma.astype(np.float64), sv[0], sv[1], S, mask)
    _assert_close(be.np(d_gx).reshape(x.shape), wgx, atol=3e-5 * np.abs(wgx).max(), rtol=1e-4, what="batchnorm_bwd gx")
    scale = np.sqrt(x.size / C)
    _assert_close(be.np(gw), gw0 + wdg, atol=2e-5 * scale, rtol=1e-5, what="dgamma")
    _assert_close(be.np(gb), gb0 + wdb, atol=2e-5 * scale, rtol=1e-5, what="dbeta")


def case_batchnorm_eval(be, N, C, H, W, act, residual=False, seed=1):
    """eval forward from the running statistics (left untouched) and its backward (fixed statistics)"""
    x, gamma, beta, rm, rv, gy, res = _inputs(N, C, H, W, seed)
    HW = H * W
    d_x, d_gy, d_g, d_b, d_rm, d_rv = be.dev(x), be.dev(gy), be.dev(gamma), be.dev(beta), be.dev(rm.copy()), be.dev(rv.copy())
    d_res = be.dev(res) if residual else None
    d_y = be.full((N, C, HW), np.nan)
    saved = be.full((2, 1, C), np.nan)
    be.lib.batchnorm_fwd_eval(be.ptr(d_x), be.ptr(d_res), be.ptr(d_y), be.ptr(d_g), be.ptr(d_b), be.ptr(d_rm), be.ptr(d_rv), be.ptr(saved),
                              N, C, HW, EPS, act, SLOPE, 0.0, 0, 0, None, be.stream)
    rstd = 1.0 / np.sqrt(rv.astype(np.float64) + EPS)
    z = (x - rm[None, :, None, None]) * (rstd * gamma)[None, :, None, None] + beta[None, :, None, None]
    want = _act(z, act) + (res if residual else 0.0)
    _assert_close(be.np(d_y).reshape(x.shape), want, atol=5e-5, rtol=3e-5, what="batchnorm_fwd_eval")
    assert np.array_equal(be.np(d_rm), rm.astype(np.float64)) and np.array_equal(be.np(d_rv), rv.astype(np.float64))
    sv = be.np(saved)
    _assert_close(sv[1][0], rstd, atol=0, rtol=3e-6, what="eval rstd")
    gw, gb = be.zeros(C), be.zeros(C)
    d_gx = run_bwd(be, d_x, d_gy, d_g, d_b, saved, gw, gb, N, C, HW, 1, False, act)
    mask = _act_d(_z32(x, gamma, beta, sv[0], sv[1], 1), act)
    wgx, wdg, wdb = ref_backward(x, gy, gamma.astype(np.float64), sv[0], sv[1], 1, mask, training=False)
    _assert_close(be.np(d_gx).reshape(x.shape), wgx, atol=3e-5 * np.abs(wgx).max(), rtol=1e-4, what="eval bwd gx")
    scale = np.sqrt(x.size / C)
    _assert_close(be.np(gw), wdg, atol=2e-5 * scale, rtol=1e-5, what="eval dgamma")
    _assert_close(be.np(gb), wdb, atol=2e-5 * scale, rtol=1e-5, what="eval dbeta")


def case_batchnorm_segments(be, N=6, C=5, H=7, W=9, S=3, act=ACT_LRELU, seed=2):
    """one call over S segments == S separate calls on the segments in order, bit for bit: output, saved statistics, running statistics,
    counter, gx, and dgamma / dbeta (summed over the segments in order)"""
    x, gamma, beta, rm, rv, gy, _ = _inputs(N, C, H, W, seed)
    HW, Ns = H * W, N // S
    d_g, d_b = be.dev(gamma), be.dev(beta)
    d_rm, d_rv, cnt = be.dev(rm.copy()), be.dev(rv.copy()), _i64(be, 0)
    y, saved = run_train(be, be.dev(x), None, d_g, d_b, d_rm, d_rv, cnt, N, C, HW, S, act)
    gw, gb = be.zeros(C), be.zeros(C)
    gx = run_bwd(be, be.dev(x), be.dev(gy), d_g, d_b, saved, gw, gb, N, C, HW, S, True, act)
    e_rm, e_rv, e_cnt = be.dev(rm.copy()), be.dev(rv.copy()), _i64(be, 0)
    ys, gxs, sv = [], [], be.np(saved)
    sums_w, sums_b = [], []
    for s in range(S):
        xs, gys = x[s * Ns:(s + 1) * Ns], gy[s * Ns:(s + 1) * Ns]
        y1, saved1 = run_train(be, be.dev(xs), None, d_g, d_b, e_rm, e_rv, e_cnt, Ns, C, HW, 1, act)
        s1 = be.np(saved1)
        assert np.array_equal(s1[:, 0], sv[:, s]), "segment %d statistics" % s
        w1, b1 = be.zeros(C), be.zeros(C)
        gx1 = run_bwd(be, be.dev(xs), be.dev(gys), d_g, d_b, saved1, w1, b1, Ns, C, HW, 1, True, act)
        ys.append(be.np(y1))
        gxs.append(be.np(gx1))
        sums_w.append(np.asarray(be.np(w1), dtype=np.float32))
        sums_b.append(np.asarray(be.np(b1), dtype=np.float32))
    assert np.array_equal(be.np(y), np.concatenate(ys)), "segmented output"
    assert np.array_equal(be.np(gx), np.concatenate(gxs)), "segmented gx"
    assert np.array_equal(be.np(d_rm), be.np(e_rm)) and np.array_equal(be.np(d_rv), be.np(e_rv)), "running statistics in segment order"
    assert _i64_value(be, cnt) == S and _i64_value(be, e_cnt) == S
    tw = sums_w[0]
    tb = sums_b[0]
    for s in range(1, S):
        tw = (tw + sums_w[s]).astype(np.float32)
        tb = (tb + sums_b[s]).astype(np.float32)
    assert np.array_equal(np.asarray(be.np(gw), dtype=np.float32), tw) and np.array_equal(np.asarray(be.np(gb), dtype=np.float32), tb)


@both_poisons
def case_batchnorm_dropout_and_max(be, N=2, C=128, H=6, W=10, seed=3, act=ACT_RELU):
    """dropout fused into the BatchNorm pass == BatchNorm followed by nemar_dropout with the same (p, seed, offset), bit for bit, forward and
    backward; the published max words == nemar_absmax_samples of the output; two identical calls are bit-identical"""
    x, gamma, beta, rm, rv, gy, _ = _inputs(N, C, H, W, seed)
    HW = H * W
    d_x, d_gy, d_g, d_b = be.dev(x), be.dev(gy), be.dev(gamma), be.dev(beta)
    p, sd, off = 0.5, 987654321, 11
    y0, sv0 = run_train(be, d_x, None, d_g, d_b, be.dev(rm.copy()), be.dev(rv.copy()), _i64(be, 0), N, C, HW, 1, act)
    yd = be.full((N, C, HW), np.nan)
    be.lib.dropout(be.ptr(y0), be.ptr(yd), x.size, p, sd, off, be.stream)
    words = be.bytes_buf(4 * N * 2049)
    y1, sv1 = run_train(be, d_x, None, d_g, d_b, be.dev(rm.copy()), be.dev(rv.copy()), _i64(be, 0), N, C, HW, 1, act, p, sd, off, words=words)
    assert be.raw(y1).tobytes() == be.raw(yd).tobytes(), "fused dropout != BatchNorm + nemar_dropout"
    ref_words = be.bytes_buf(4 * N)
    be.lib.absmax_samples(be.ptr(y1), N, C * HW, be.ptr(ref_words), be.stream)
    assert be.raw(words)[:4 * N].tobytes() == be.raw(ref_words)[:4 * N].tobytes(), "max words"
    y2, sv2 = run_train(be, d_x, None, d_g, d_b, be.dev(rm.copy()), be.dev(rv.copy()), _i64(be, 0), N, C, HW, 1, act, p, sd, off)
    assert be.raw(y2).tobytes() == be.raw(y1).tobytes() and be.raw(sv2).tobytes() == be.raw(sv1).tobytes(), "repeat"
    # backward: mask regenerated == nemar_dropout on gy, then the plain backward
    gd = be.full((N, C, HW), np.nan)
    be.lib.dropout(be.ptr(d_gy), be.ptr(gd), x.size, p, sd, off, be.stream)
    w0, b0, w1, b1 = be.zeros(C), be.zeros(C), be.zeros(C), be.zeros(C)
    gx0 = run_bwd(be, d_x, gd, d_g, d_b, sv0, w0, b0, N, C, HW, 1, True, act)
    gx1 = run_bwd(be, d_x, d_gy, d_g, d_b, sv1, w1, b1, N, C, HW, 1, True, act, p, sd, off)
    assert be.raw(gx0).tobytes() == be.raw(gx1).tobytes(), "backward with the regenerated mask"
    assert be.raw(w0).tobytes() == be.raw(w1).tobytes() and be.raw(b0).tobytes() == be.raw(b1).tobytes()
    gx2 = run_bwd(be, d_x, d_gy, d_g, d_b, sv1, be.zeros(C), be.zeros(C), N, C, HW, 1, True, act, p, sd, off)
    assert be.raw(gx2).tobytes() == be.raw(gx1).tobytes(), "repeat backward"


def case_batchnorm_single_value(be):
    """one value per channel in training (N * H * W == 1, or N / S * H * W == 1) is refused, as PyTorch refuses it"""
    from nemar_amd._lib import NemarHipError
    import pytest
    C = 3
    d_g, d_b = be.dev(np.ones(C)), be.dev(np.zeros(C))
    for N, S in ((1, 1), (2, 2)):
        with pytest.raises(NemarHipError, match="more than 1 value"):
            run_train(be, be.dev(np.ones((N, C, 1, 1))), None, d_g, d_b, be.dev(np.zeros(C)), be.dev(np.ones(C)), _i64(be, 0), N, C, 1, S,
                      ACT_NONE)


# ---- ill-conditioned channels (the families of tests/norm_cases.py) --------------------------------------------------------------------
def _np32_bn(x, g, gamma, beta, rv, S):
    """plain numpy fp32 exact two-pass BatchNorm2d (training) per segment -> y, mean[S,C], rstd[S,C], running_var, gx, dgamma, dbeta"""
    f = np.float32
    N, C = x.shape[:2]
    Ns = N // S
    y, gx = np.empty_like(x), np.empty_like(x)
    rv = rv.astype(f).copy()
    dg, db = np.zeros(C, dtype=f), np.zeros(C, dtype=f)
    means, rstds = [], []
    ga, be_ = gamma.astype(f).reshape(1, C, 1, 1), beta.astype(f).reshape(1, C, 1, 1)
    for s in range(S):
        sl = slice(s * Ns, (s + 1) * Ns)
        xs, gs = x[sl], g[sl].astype(f)
        M = f(xs.size // C)
        m = (xs.sum(axis=(0, 2, 3), keepdims=True, dtype=f) / M).astype(f)
        d = (xs - m).astype(f)
        var = ((d * d).sum(axis=(0, 2, 3), keepdims=True, dtype=f) / M).astype(f)
        rstd = (f(1) / np.sqrt(var + f(EPS), dtype=f)).astype(f)
        xh = (d * rstd).astype(f)
        y[sl] = xh * ga + be_
        rv = (f(1 - MOM) * rv + f(MOM) * (var.reshape(C) * (M / (M - f(1))))).astype(f)
        sg, sgx = gs.sum(axis=(0, 2, 3), keepdims=True, dtype=f), (gs * xh).sum(axis=(0, 2, 3), keepdims=True, dtype=f)
        gx[sl] = ga * rstd * (gs - sg / M - xh * (sgx / M))
        dg, db = dg + sgx.reshape(C), db + sg.reshape(C)
        means.append(m.reshape(C))
        rstds.append(rstd.reshape(C))
    return y, np.array(means), np.array(rstds), rv, gx, dg, db


def _torch32_bn(x, g, gamma, beta, rm, rv, S):
    """torch's fp32 layer on the CPU, one F.batch_norm call per segment, the backward through autograd -> y, running_var, gx, dgamma, dbeta"""
    import torch
    N = x.shape[0]
    Ns = N // S
    w, b = torch.tensor(gamma, requires_grad=True), torch.tensor(beta, requires_grad=True)
    trm, trv = torch.tensor(rm.copy()), torch.tensor(rv.copy())
    ys, gxs = [], []
    for s in range(S):
        t = torch.tensor(x[s * Ns:(s + 1) * Ns], requires_grad=True)
        y = torch.nn.functional.batch_norm(t, trm, trv, w, b, True, MOM, EPS)
        y.backward(torch.tensor(np.ascontiguousarray(g[s * Ns:(s + 1) * Ns], dtype=np.float32)))
        ys.append(y.detach().numpy())
        gxs.append(t.grad.numpy())
    return np.concatenate(ys), trv.numpy(), np.concatenate(gxs), w.grad.numpy(), b.grad.numpy()


def case_batchnorm_conditioned(be, N, C, H, W, S, family, seed=5):
    """case_batchnorm_train on one family of ill-conditioned channels: saved mean / rstd, output, running variance, gx, dgamma, dbeta.
    `plain` keeps case_batchnorm_train's assertions; every other family passes a quantity within max(that tolerance, F x the larger
    error against float64 of torch's fp32 F.batch_norm and of a numpy fp32 two-pass restatement) — norm_cases.check, per channel."""
    import norm_cases as NC
    act = ACT_NONE if family in NC.NO_ACT_BACKWARD else ACT_LRELU
    x, gamma, beta, rm, rv, gy, _ = _inputs(N, C, H, W, seed, family)
    HW, Ns = H * W, N // S
    route = "batchnorm N=%d HW=%d S=%d" % (N, HW, S)
    names = [family] * (S * C)

    def ch(a):                                   # [N, C, H, W] -> one row per (segment, channel)
        return np.asarray(a, dtype=np.float64).reshape(S, Ns, C, HW).transpose(0, 2, 1, 3).reshape(S * C, Ns * HW)

    d_x, d_gy, d_g, d_b = be.dev(x), be.dev(gy), be.dev(gamma), be.dev(beta)
    d_rm, d_rv, cnt = be.dev(rm.copy()), be.dev(rv.copy()), _i64(be, 0)
    d_y, saved = run_train(be, d_x, None, d_g, d_b, d_rm, d_rv, cnt, N, C, HW, S, act)
    g64, b64 = gamma.astype(np.float64), beta.astype(np.float64)
    want, m, rstd, _, wrv = ref_forward(x, g64, b64, rm, rv, S, act)
    pre64 = ref_forward(x, g64, b64, rm, rv, S, ACT_NONE)[0]
    sv = be.np(saved)
    assert np.all(np.isfinite(sv)) and np.all(np.isfinite(be.np(d_y)))
    mask = _act_d(_z32(x, gamma, beta, sv[0], sv[1], S), act)
    g = (gy * mask).astype(np.float32)
    ny, nm, nr, nrv, ngx, ndg, ndb = _np32_bn(x, g, gamma, beta, rv, S)
    ty, trv, tgx, tdg, tdb = _torch32_bn(x, g, gamma, beta, rm, rv, S)
    ex_gx, ex_dg, ex_db = ref_backward(x, g, g64, m, rstd, S, np.ones_like(x, dtype=np.float64))     # the exact layer: the yardsticks' target
    pm = lambda a: np.abs(a).reshape(a.shape[0], -1).max(axis=1)
    NC.check(be, route, names, "mean", sv[0].reshape(-1), m.reshape(-1), 2e-5, 1e-5, np.abs(nm - m).reshape(-1))
    NC.check(be, route, names, "rstd", sv[1].reshape(-1), rstd.reshape(-1), 0.0, 3e-5, np.abs(nr - rstd).reshape(-1))
    NC.check(be, route, names, "y", ch(be.np(d_y).reshape(x.shape)), ch(want), 5e-5, 3e-5, np.maximum(pm(ch(ny) - ch(pre64)), pm(ch(ty) - ch(pre64))))
    NC.check(be, route, [family] * C, "running_var", be.np(d_rv), wrv, 2e-6, 3e-5, np.maximum(np.abs(nrv - wrv), np.abs(trv - wrv)))
    assert _i64_value(be, cnt) == S
    gw, gb = be.zeros(C), be.zeros(C)
    d_gx = run_bwd(be, d_x, d_gy, d_g, d_b, saved, gw, gb, N, C, HW, S, True, act)
    wgx, wdg, wdb = ref_backward(x, gy, g64, sv[0], sv[1], S, mask)
    atol = 3e-5 * (np.abs(wgx).max() if family == "plain" else pm(ch(wgx)))
    NC.check(be, route, names, "gx", ch(be.np(d_gx).reshape(x.shape)), ch(wgx), atol, 1e-4, np.maximum(pm(ch(ngx) - ch(ex_gx)), pm(ch(tgx) - ch(ex_gx))))
    scale = np.sqrt(x.size / C)
    NC.check(be, route, [family] * C, "dgamma", be.np(gw), wdg, 2e-5 * scale, 1e-5, np.maximum(np.abs(ndg - ex_dg), np.abs(tdg - ex_dg)))
    NC.check(be, route, [family] * C, "dbeta", be.np(gb), wdb, 2e-5 * scale, 1e-5, np.maximum(np.abs(ndb - ex_db), np.abs(tdb - ex_db)))
