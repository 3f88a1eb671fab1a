"""Backend-agnostic test bodies of nemar_jacobian_stats (csrc/regularity.hip: the forward-difference Jacobian determinant of a
prediction's transformation at any output size, as a map and as fold / log-Jacobian statistics, in one pass), driven through
tests/backends.py (EmuBackend: host-emulated kernels, CPU tier; HipBackend: the gfx950 library, `-m gpu` tier).  Every buffer is
guard-banded there, the workspace included (exactly the queried bytes).

The truth is the definition of include/nemar_hip.h written out in float64 numpy (ref_det) on register_cases.ref_grid: the position
((g + 1) * size - 1) / 2 of every output pixel in an image of the output's own size, then the forward differences.  The same function
with dtype float32 is the yardstick.  The rules (why each bound is what it is):
  map         interior max-abs error <= MARGIN x the yardstick's on the same case (register_cases.MARGIN: two fp32 evaluations of one
              formula in different rounding orders); the last row and column are NaN, everything else finite.
  closed form the same rule against a constant: theta's 2 x 2 determinant (affine; the aspect factors cancel), Wo Ho / ((Wo-1)(Ho-1))
              for a zero UNet field (the reference's linspace identity is a slight zoom).
  reduction   counts and stats against the map THE KERNEL WROTE: interior, folds, min and max exactly (the same bits); each sum within
              CHAIN x 2^-24 x sum |term| of the float64 sum.  CHAIN = 64 bounds the additions a term passes through: one tile per
              workgroup at every size — 4 pixels per lane, 6 wave steps, 3 workgroup steps — then ceil(tiles / 256) + 6 + 3 in the merge
              (tiles <= 64 at the sizes tested here: 23 in all), plus 2 ulp of logf and the rounding of its square.
  folds       #(det64 < -FOLD_BAND) <= folds <= #(det64 <= FOLD_BAND); the float64 reference alone keeps the band's share <= BAND_SHARE
              of the interior pixels.  FOLD_BAND = 1e-3 is >= 8 x the yardstick's error up to 256 x 256."""
import ctypes

import numpy as np
import pytest
import torch

from backends import both_poisons
from deform_cases import run_meter
from register_cases import GRID_AFFINE, GRID_EXPLICIT, GRID_UNET, MARGIN, draw, ref_grid

U, A = GRID_UNET, GRID_AFFINE
#        (hf, wf),  (Ho, Wo)
RAGGED = ((32, 48), (35, 131))          # tile edges inside both axes, the field coarser than the output
EQUAL = ((40, 56), (40, 56))            # no resampling
DOWN = ((64, 64), (24, 40))             # down-sampling: the un-staged global path
ONE_TEXEL = ((1, 1), (20, 36))          # a one-texel field
TALL = ((16, 24), (67, 131))            # five tile rows, three tile columns
NETWORK = ((64, 64), (256, 256))        # the network's own output size: 64 tiles per sample
SIZES = [RAGGED, EQUAL, DOWN, ONE_TEXEL, TALL]
FOLDING = [RAGGED, EQUAL, DOWN, TALL]   # (a one-texel field is a constant offset and cannot fold: its reduction is checked with its map)
THIN = [((8, 12), (1, 77)), ((8, 12), (50, 1))]                  # no interior pixel
EDGES = [((8, 12), (h, 40)) for h in (2, 3, 16, 17, 33)] + [((8, 12), (20, w)) for w in (2, 63, 64, 65, 129)]      # 17 and 65: the smallest
                                                                                                                    # sizes with a neighbour in the next tile
CHAIN = 64
FOLD_BAND = 1e-3
BAND_SHARE = 0.005
MIN_FOLDS = 0.05


# ---- the float64 truth, and (dtype float32) the yardstick -------------------------------------------------------------------------------
def ref_det(pred, mode, Ho, Wo, dtype=np.float64):
    """det [N,Ho-1,Wo-1] of include/nemar_hip.h nemar_jacobian_stats at the interior pixels, written out"""
    tdtype = torch.float64 if dtype is np.float64 else torch.float32
    g = ref_grid(pred, mode, Ho, Wo, tdtype).numpy()                       # [N,Ho,Wo,2]
    one, two = dtype(1), dtype(2)
    px = ((g[..., 0] + one) * dtype(Wo) - one) / two
    py = ((g[..., 1] + one) * dtype(Ho) - one) / two
    ax, ay = px[:, :-1, 1:] - px[:, :-1, :-1], py[:, :-1, 1:] - py[:, :-1, :-1]
    bx, by = px[:, 1:, :-1] - px[:, :-1, :-1], py[:, 1:, :-1] - py[:, :-1, :-1]
    det = ax * by - bx * ay
    assert det.dtype == dtype
    return det.astype(np.float64)


# ---- drivers ----------------------------------------------------------------------------------------------------------------------------------
def _fill_value(be):
    """what outputs hold before a call: the float the poison in force reads as (a NaN, or 1e38 — the map's border is NaN by contract, so
    only the finite poison shows that it was written)"""
    return np.array([be.poison], dtype=np.uint32).view(np.float32)[0]


def run_jac(be, d_pred, mode, size, N, det_map=True, d_det=None):
    """-> (det [N,Ho,Wo] float32 or None, counts [N,2] uint32, stats [N,5] float32) on the host, bit for bit; outputs pre-filled"""
    (hf, wf), (Ho, Wo) = size
    fill = _fill_value(be)
    if det_map and d_det is None:
        d_det = be.full((N, Ho, Wo), fill)
    d_counts, d_stats = be.dev_i32(np.full((N, 2), -7)), be.full((N, 5), fill)
    wsb = int(be.lib.jacobian_stats_workspace(N, Ho, Wo))
    ws = be.bytes_buf(wsb)
    be.lib.jacobian_stats(be.ptr(d_pred), mode, be.ptr(d_det) if det_map else None, be.ptr(d_counts), be.ptr(d_stats), be.ptr(ws), wsb, N, hf, wf,
                          Ho, Wo, be.stream)
    det = be.raw(d_det).view(np.float32).reshape(N, Ho, Wo) if det_map else None
    return det, be.raw(d_counts).view(np.uint32).reshape(N, 2), be.raw(d_stats).view(np.float32).reshape(N, 5)


def _what(mode, size, amp):
    return "%s %s -> %s amp %g" % ("UA"[mode == A], *size, amp)


def check_map(got, pred, mode, Ho, Wo, what, want=None):
    """the map rule; -> (kernel error, yardstick error).  `want`: a closed form in place of the float64 reference"""
    assert np.all(np.isnan(got[:, -1, :])) and np.all(np.isnan(got[:, :, -1])), "the last row and column are NaN: " + what
    inner = got[:, :-1, :-1].astype(np.float64)
    assert np.all(np.isfinite(inner)), what
    if inner.size == 0:
        return 0.0, 0.0
    ref32 = ref_det(pred, mode, Ho, Wo, np.float32)
    want = ref_det(pred, mode, Ho, Wo) if want is None else want
    yard = np.abs(ref32 - want).max()
    err = np.abs(inner - want).max()
    print("regularity map %-44s kernel %.3e  numpy-fp32 %.3e  ratio %.2f" % (what, err, yard, err / yard if yard else (0.0 if err == 0 else float('inf'))))
    assert err <= MARGIN * yard, (what, err, yard)
    return err, yard


def check_reduction(det, counts, stats, what):
    """counts and stats are a faithful reduction of the map the kernel wrote"""
    N, Ho, Wo = det.shape
    for n in range(N):
        m = det[n, :-1, :-1].ravel()
        assert int(counts[n, 0]) == (Ho - 1) * (Wo - 1), (what, n, counts[n])
        assert int(counts[n, 1]) == int((m <= 0).sum()), (what, n, counts[n], int((m <= 0).sum()))
        if m.size == 0:
            assert stats[n, 0] == np.inf and stats[n, 1] == -np.inf and np.all(stats[n, 2:] == 0), (what, n, stats[n])
            continue
        assert stats[n, 0].view(np.uint32) == m.min().view(np.uint32) and stats[n, 1].view(np.uint32) == m.max().view(np.uint32), (what, n, stats[n])
        logs = np.log(m[m > 0].astype(np.float64))
        for k, terms in ((2, m.astype(np.float64)), (3, logs), (4, logs * logs)):
            want, bound = terms.sum(), CHAIN * 2.0 ** -24 * np.abs(terms).sum()
            print("regularity sum %-44s n %d column %d  kernel %.9g  float64 %.9g  error %.3e  bound %.3e" % (what, n, k, stats[n, k], want, abs(stats[n, k] - want), bound))
            assert abs(float(stats[n, k]) - want) <= bound, (what, n, k, stats[n, k], want, bound)


# ---- 1. the map against float64 ------------------------------------------------------------------------------------------------------------
def case_map(be, size, mode, amp, N=2, seed=1):
    (hf, wf), (Ho, Wo) = size
    _, pred = draw(seed, mode, N, 1, hf, wf, 1, 1, amp)
    det, counts, stats = run_jac(be, be.dev(pred), mode, size, N)
    check_reduction(det, counts, stats, _what(mode, size, amp))
    return check_map(det, pred, mode, Ho, Wo, _what(mode, size, amp))


# ---- 2. closed forms -----------------------------------------------------------------------------------------------------------------------
def case_affine_closed_form(be, size, amp, N=2, seed=1):
    (hf, wf), (Ho, Wo) = size
    _, dtheta = draw(seed, A, N, 1, hf, wf, 1, 1, amp)
    th = dtheta.astype(np.float64) + np.array([1, 0, 0, 0, 1, 0], dtype=np.float64)[None]
    want = (th[:, 0] * th[:, 4] - th[:, 1] * th[:, 3])[:, None, None]
    det, counts, _ = run_jac(be, be.dev(dtheta), A, size, N)
    assert np.all(want > 0) and np.all(counts[:, 1] == 0), "an affine draw does not fold"
    check_map(det, dtheta, A, Ho, Wo, "closed form " + _what(A, size, amp), want=np.broadcast_to(want, (N, Ho - 1, Wo - 1)))


def case_zero_field_closed_form(be, size, N=2):
    (hf, wf), (Ho, Wo) = size
    pred = np.zeros((N, 2, hf, wf), dtype=np.float32)
    want = Wo * Ho / ((Wo - 1.0) * (Ho - 1.0))
    det, _, stats = run_jac(be, be.dev(pred), U, size, N)
    check_map(det, pred, U, Ho, Wo, "zero field " + _what(U, size, 0), want=np.full((N, Ho - 1, Wo - 1), want))
    assert np.all(np.abs(stats[:, :2] - want) < 1e-3)


# ---- 3. / 4. the statistics: a faithful reduction of the map, and the folds against float64 ------------------------------------------------
def case_statistics(be, size, N=2, seed=1, amp=1.0):
    (hf, wf), (Ho, Wo) = size
    _, pred = draw(seed, U, N, 1, hf, wf, 1, 1, amp)
    what = "statistics " + _what(U, size, amp)
    want = ref_det(pred, U, Ho, Wo)
    interior = (Ho - 1) * (Wo - 1)
    assert (want <= 0).mean() >= MIN_FOLDS, "the float64 reference shows too few folds: the case would show nothing (%s: %.4f)" % (what, (want <= 0).mean())
    band = (np.abs(want) <= FOLD_BAND).reshape(N, -1).sum(1)
    assert np.all(band <= BAND_SHARE * interior), (what, band, interior)
    det, counts, stats = run_jac(be, be.dev(pred), U, size, N)
    check_reduction(det, counts, stats, what)
    lo, hi = (want < -FOLD_BAND).reshape(N, -1).sum(1), (want <= FOLD_BAND).reshape(N, -1).sum(1)
    print("regularity folds %-42s float64 %s  kernel %s  band %s of %d" % (what, (want <= 0).reshape(N, -1).sum(1), counts[:, 1], band, interior))
    assert np.all(lo <= counts[:, 1]) and np.all(counts[:, 1] <= hi), (what, lo, counts[:, 1], hi)


# ---- 5. agreement with the existing meter ----------------------------------------------------------------------------------------------------
def case_agrees_with_meter(be, size=EQUAL, N=2, seed=2, amp=1.0):
    """nemar_registration_error with g = 0 counts folds over the same positions at the field's own size"""
    (hf, wf), (Ho, Wo) = size
    assert (hf, wf) == (Ho, Wo)
    _, pred = draw(seed, U, N, 1, hf, wf, 1, 1, amp)
    d_pred = be.dev(pred)
    det, counts, _ = run_jac(be, d_pred, U, size, N)
    meter = be.np(run_meter(be, d_pred, U, be.zeros(N, 2, Ho, Wo), N, Ho, Wo))
    near = (np.abs(det[:, :-1, :-1]) < FOLD_BAND).reshape(N, -1).sum(1)
    print("regularity meter: folds %s, registration_error %s, |det| < %g at %s pixels" % (counts[:, 1], meter[:, 4], FOLD_BAND, near))
    assert np.array_equal(meter[:, 5], counts[:, 0].astype(np.float64))
    assert counts[:, 1].sum() > 0 and np.all(np.abs(meter[:, 4] - counts[:, 1]) <= near)


# ---- 6. edges -----------------------------------------------------------------------------------------------------------------------------
@both_poisons
def case_thin(be, size, mode, N=2, seed=4):
    (hf, wf), (Ho, Wo) = size
    _, pred = draw(seed, mode, N, 1, hf, wf, 1, 1, 1.0)
    det, counts, stats = run_jac(be, be.dev(pred), mode, size, N)
    assert np.all(np.isnan(det)), "no pixel has both forward neighbours: the map is all NaN"
    assert np.all(counts == 0), counts
    assert np.all(stats[:, 0] == np.inf) and np.all(stats[:, 1] == -np.inf) and np.all(stats[:, 2:] == 0), stats


@both_poisons
def case_edges(be, size, mode, N=2, seed=4, amp=1.0):
    (hf, wf), (Ho, Wo) = size
    _, pred = draw(seed, mode, N, 1, hf, wf, 1, 1, amp)
    det, counts, stats = run_jac(be, be.dev(pred), mode, size, N)
    check_map(det, pred, mode, Ho, Wo, "edges " + _what(mode, size, amp))
    check_reduction(det, counts, stats, "edges " + _what(mode, size, amp))


# ---- 7. repeatable, overwritten, unaligned, optional map, refusals ----------------------------------------------------------------------------
def _off_by_4_bytes(be, a):
    """`a` in a buffer that starts 4 bytes past a 16-byte boundary (a view of a guarded block one element longer)"""
    d_buf = be.dev(np.concatenate([[0.0], np.asarray(a, dtype=np.float32).ravel()]))
    return be.sub(d_buf, 1, d_buf.shape[0])


@both_poisons
def case_repeatable_unaligned(be, size, mode, N=2, seed=3, amp=1.0):
    (hf, wf), (Ho, Wo) = size
    _, pred = draw(seed, mode, N, 1, hf, wf, 1, 1, amp)
    d_pred = be.dev(pred)
    det, counts, stats = run_jac(be, d_pred, mode, size, N)
    bits = lambda a: a.view(np.uint32)
    # (the outputs were pre-filled with the poison in force: under the finite one, an element that was not written would show)
    fill = _fill_value(be)
    if np.isfinite(fill):
        assert not np.any(det == fill) and not np.any(stats == fill), "an output element was not written"
    assert np.all(counts[:, 0] == (Ho - 1) * (Wo - 1))
    det2, counts2, stats2 = run_jac(be, d_pred, mode, size, N)
    assert np.array_equal(bits(det), bits(det2)) and np.array_equal(counts, counts2) and np.array_equal(bits(stats), bits(stats2)), "two calls, different bits"
    det3, counts3, stats3 = run_jac(be, _off_by_4_bytes(be, pred), mode, size, N, d_det=_off_by_4_bytes(be, np.full(N * Ho * Wo, fill)))
    assert np.array_equal(bits(det), bits(det3)) and np.array_equal(counts, counts3) and np.array_equal(bits(stats), bits(stats3)), \
        "views 4 bytes off the 16-byte grid: different bits"
    none, counts4, stats4 = run_jac(be, d_pred, mode, size, N, det_map=False)
    assert none is None and np.array_equal(counts, counts4) and np.array_equal(bits(stats), bits(stats4)), "counts / stats differ without det_out"


def case_refusals(be):
    """NEMAR_EINVAL (-1), a message, and nothing launched: the outputs keep their fill"""
    from nemar_amd._lib import NemarHipError
    N, hf, wf, Ho, Wo = 2, 6, 8, 12, 16
    d_pred, d_th = be.zeros(N, 2, hf, wf), be.zeros(N, 6)
    d_det, d_counts, d_stats = be.full((N, Ho, Wo), 7.0), be.dev_i32(np.full((N, 2), 7)), be.full((N, 5), 7.0)
    wsb = int(be.lib.jacobian_stats_workspace(N, Ho, Wo))
    assert wsb > 0 and int(be.lib.jacobian_stats_workspace(N, Ho, 0)) == 0
    ws = be.bytes_buf(wsb + 4)
    off2 = lambda p: ctypes.c_void_p(p.value + 2)
    names = ("pred", "mode", "det", "counts", "stats", "ws", "wsb", "N", "hf", "wf", "Ho", "Wo")
    good = [be.ptr(d_pred), U, be.ptr(d_det), be.ptr(d_counts), be.ptr(d_stats), be.ptr(ws), wsb, N, hf, wf, Ho, Wo]

    def refused(**change):
        args = [change.get(k, v) for k, v in zip(names, good)]
        with pytest.raises(NemarHipError, match=r"failed \(-1\): jacobian_stats: \S"):
            be.lib.jacobian_stats(*args, be.stream)

    for m in (GRID_EXPLICIT, 3, -1):                              # an explicit grid has one resolution; 3 and -1 are no modes at all
        refused(mode=m)
    for k in ("pred", "counts", "stats", "ws"):                   # required pointers: null, not even 4-byte aligned
        refused(**{k: None})
        refused(**{k: off2(good[names.index(k)])})
    refused(det=off2(good[2]))                                    # (a null det_out is the stats-only call)
    for k in ("N", "Ho", "Wo"):                                   # non-positive sizes
        refused(**{k: 0})
        refused(**{k: -3})
    for k in ("hf", "wf"):                                        # UNET without a field
        refused(**{k: 0})
        refused(**{k: -1})
    refused(N=65536)
    refused(Ho=1 << 16, Wo=1 << 15)                               # Ho * Wo = 2^31
    refused(wsb=wsb - 1)                                          # a short workspace
    refused(wsb=0)
    refused(det=good[0])                                          # det_out is the operand
    be.sync()
    assert np.all(be.np(d_det) == 7.0) and np.all(be.np(d_stats) == 7.0) and np.all(be.raw(d_counts).view(np.int32) == 7)
    # hf, wf of an affine prediction are ignored; the identity has determinant 1
    be.lib.jacobian_stats(be.ptr(d_th), A, None, be.ptr(d_counts), be.ptr(d_stats), be.ptr(ws), wsb, N, 0, -1, Ho, Wo, be.stream)
    assert np.all(be.np(d_det) == 7.0)
    assert np.array_equal(be.raw(d_counts).view(np.uint32).reshape(N, 2), np.array([[(Ho - 1) * (Wo - 1), 0]] * N, dtype=np.uint32))
    stats = be.np(d_stats)
    assert np.all(np.abs(stats[:, :2] - 1) < 1e-5) and np.all(np.abs(stats[:, 2] - (Ho - 1) * (Wo - 1)) < 1e-2)


# ---- 9. the host-side summary ------------------------------------------------------------------------------------------------------------------
def case_summary():
    from nemar_amd import ops
    counts = np.array([[100, 10], [300, 0]], dtype=np.uint32)
    #                 min   max  sum det  sum log  sum log^2
    stats = np.array([[-0.5, 2.0, 90.0, 9.0, 45.0], [0.25, 3.0, 330.0, -30.0, 120.0]], dtype=np.float32)
    s = ops.regularity_summary(counts, stats)
    assert s['interior'] == 400 and s['folds'] == 10 and isinstance(s['interior'], int) and isinstance(s['folds'], int)
    assert s['fold_frac'] == 10 / 400                             # counts added, then divided (not the mean of 0.1 and 0)
    assert s['det_min'] == -0.5 and s['det_max'] == 3.0 and s['det_mean'] == 420.0 / 400
    k = 390
    assert s['log_det_mean'] == pytest.approx(-21.0 / k, rel=1e-15)
    assert s['log_det_std'] == pytest.approx(np.sqrt(165.0 / k - (21.0 / k) ** 2), rel=1e-12)        # SDlogJ from the two sums, in float64
    assert all(isinstance(s[key], float) for key in ('fold_frac', 'det_min', 'det_max', 'det_mean', 'log_det_mean', 'log_det_std'))
    # float64: a difference that float32 would lose
    big = ops.regularity_summary(np.array([[1 << 24, 0]], dtype=np.uint32), np.array([[1, 1, 1 << 24, 4096.0, 1.5]], dtype=np.float32))
    assert big['log_det_mean'] == 4096.0 / (1 << 24) and big['log_det_std'] == pytest.approx(np.sqrt(1.5 / (1 << 24) - (4096.0 / (1 << 24)) ** 2), rel=1e-12)
    # every pixel folds: nothing to take a logarithm of; no pixel at all: nothing to average
    s = ops.regularity_summary(np.array([[6, 6]], dtype=np.uint32), np.array([[-2, -1, -9, 0, 0]], dtype=np.float32))
    assert s['fold_frac'] == 1.0 and s['det_mean'] == -1.5 and s['log_det_mean'] is None and s['log_det_std'] is None
    s = ops.regularity_summary(np.zeros((2, 2), dtype=np.uint32), np.array([[np.inf, -np.inf, 0, 0, 0]] * 2, dtype=np.float32))
    assert s['interior'] == 0 and s['folds'] == 0
    assert all(s[key] is None for key in ('fold_frac', 'det_min', 'det_max', 'det_mean', 'log_det_mean', 'log_det_std'))
    # torch tensors (what ops.jacobian_stats returns, brought to the host) are taken as well
    t = ops.regularity_summary(torch.from_numpy(counts.astype(np.int64)), torch.from_numpy(stats))
    assert t == ops.regularity_summary(counts, stats)
