"""Backend-agnostic test bodies of nemar_joint_histogram (csrc/similarity.hip: the joint histogram and the moments of the registered
moving image against the fixed image, in one pass), driven through tests/backends.py (EmuBackend: host-emulated kernels, CPU tier;
HipBackend: the gfx950 library, `-m gpu` tier).  Every buffer is guard-banded there, the workspace included (exactly the queried bytes);
`counts` is an int32 buffer read back bit for bit.

The grid has ONE truth, tests/register_cases.py (draw, smooth_field, ref_grid, ref_warp, tie_mask); what is new is written out here in
numpy (truth()): the channel means, which pixels count, the bin rule and the sums.  The rules (why each bound is what it is):
  values    a64 = the float64 channel mean of ref_warp(BILINEAR); the kernel's a lies within E_a = MARGIN x the max-abs error of torch's
            own float32 grid_sample against float64 on that case (check_bilinear's yardstick).  b is a float32 statement by definition —
            (sum of the channels, ascending) * (1.f / Cf) — and is evaluated as such in numpy float32: no allowance at all (the issue
            grants one float32 rounding of the mean; asking for the bits asks more).
  bins      the bin rule is a float32 statement too, clamp((int)floorf((v - lo) * (bins / (hi - lo))), 0, bins - 1), monotone in v: a
            pixel is BIN-AMBIGUOUS where that rule, evaluated in numpy float32, gives different bins at the two ends of
            [a64 - E_a, a64 + E_a] (rounded outwards), i.e. where a64 lies within E_a of a bin edge; its candidates are the bins between.
  border    register_cases.tie_mask marks the pixels whose float64 sampling position lies within TIE_BAND px of a rounding tie; the
            float64 reference alone keeps them <= TIE_SHARE.  Whether the nearest texel is inside can differ only for those of them
            whose tie IS the source's border (rounding the other way crosses it): these are the BORDER-AMBIGUOUS pixels — a subset of
            tie_mask, so the rules below ask more than they would with all of it.
  counts    per sample and cell, sure[cell] <= got[cell] <= sure[cell] + could[cell]: `sure` counts the counted pixels that are in
            neither set in their cell, `could` the ambiguous ones in every cell they might land in; the sample's total lies between the
            sure pixels and those plus the ambiguous ones.  The float64 reference alone keeps either set <= TIE_SHARE of the pixels.
  moments   each sum against float64 over the float64-counted pixels, within
              (D + 3) 2^-24 sum |term|  +  sum over the counted pixels of (E_a |d term / da| + E_b |d term / db|)  +  max |term| per
              border-ambiguous pixel,
            D the addition depth csrc/similarity.hip states: 4 T + ceil(G / 256) + 18 with G workgroups per sample and T tiles per
            workgroup (depth()); E_b = 2^-24 max |b|, one float32 rounding of the mean."""
import ctypes

import numpy as np
import pytest
import torch

from backends import both_poisons
from register_cases import (ALL_SIZES, BILINEAR, GRID_AFFINE, GRID_EXPLICIT, GRID_UNET, MARGIN, TIE_BAND, TIE_SHARE, ref_grid, ref_warp, run_fused,
                            smooth_field, tie_mask)
from score_cases import _off_by_4_bytes

U, A = GRID_UNET, GRID_AFFINE
GARBAGE = 0x5a5a5a5a
#          (hf, wf), (Ho, Wo), (Hs, Ws) or None = the output size
SIZES = [s[:3] for s in ALL_SIZES]                           # a different source size and down-sampling among them
THIN = [((8, 12), (1, 77), (9, 13)), ((8, 12), (50, 1), (9, 13))]
THIN_SEED = {GRID_UNET: 4, GRID_AFFINE: 7}                   # 77 and 50 pixels: ONE pixel near a rounding tie is more than TIE_SHARE
ONE_TEXEL_FIELD = ((1, 1), (20, 36), None)
LEAVES_SOURCE = ((16, 24), (67, 45), (30, 41))               # with amp = 1.5: the field leaves the source, those pixels do not count
RAGGED = SIZES[4]                                            # 131 x 203 from a 90 x 120 source: odd sizes, three tile columns, nine tile rows
EDGES = [((8, 12), (20, w), None) for w in (63, 64, 65)] + [((8, 12), (h, 40), None) for h in (16, 17)]      # where a tile ends
TWO_TRIPS = ((32, 48), (1300, 1290), (90, 120))              # 1722 tiles for 1536 workgroups (64 bins): the grid-stride loop runs twice (GPU tier)
CHANNELS = [(1, 1), (3, 1), (2, 5)]
BINS = [2, 32, 64]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _shape(size, N, Cm, Cf):
    (hf, wf), (Ho, Wo), src = size
    Hs, Ws = src or (Ho, Wo)
    return (N, Cm, Cf, Hs, Ws, hf, wf, Ho, Wo)


def draw_pair(seed, mode, shape, amp=0.15, nans=5, fade=False):
    """moving [N,Cm,Hs,Ws]: a texture in [0, 1] (noise on a lattice of at most 8 x 10 points, bicubic in between: per-pixel noise has
    gradients of order one per pixel, and the yardstick E_a — position error, which grows with the image, times gradient — would then put
    more than TIE_SHARE of the pixels within E_a of one of 64 bin edges); fixed [N,Cf,Ho,Wo] uniform in [0, 1) (it is not interpolated),
    `nans` NaN pixels in one channel of every sample; different content per sample; and the prediction of register_cases.draw's kind.
    fade: the texture falls linearly to zero over the outer tenth of the source.  Without it E_a is set by the pixels that blend with the
    zero padding, where the value changes by |value| per pixel; position error grows with the image, and from about 256 x 256 those few
    pixels push E_a past 1 % of a bin's width times the bins.  (The smaller cases keep the cliff at the border.)"""
    N, Cm, Cf, Hs, Ws, hf, wf, Ho, Wo = shape
    rng = np.random.default_rng(seed)
    pred = smooth_field(seed, N, hf, wf, amp) if mode == U else (rng.uniform(-1, 1, (N, 6)) * amp).astype(np.float32)
    lattice = torch.from_numpy(rng.random((N, Cm, min(8, max(2, Hs // 3)), min(10, max(2, Ws // 3)))))
    moving = torch.nn.functional.interpolate(lattice, size=(Hs, Ws), mode='bicubic', align_corners=False).clamp_(0, 1).numpy().astype(np.float32)
    if fade:
        ramp = lambda n: np.minimum(np.minimum(np.arange(n), n - 1 - np.arange(n)) / max(0.1 * n, 1.0), 1.0).astype(np.float32)
        moving = moving * ramp(Hs)[:, None] * ramp(Ws)[None, :]
    fixed = rng.random((N, Cf, Ho, Wo)).astype(np.float32)
    for n in range(N):
        at = rng.choice(Ho * Wo, min(nans, Ho * Wo), replace=False)
        fixed[n, rng.integers(0, Cf)].reshape(-1)[at] = np.nan
    return moving, fixed, pred


# ---- the truth ----------------------------------------------------------------------------------------------------------------------------
def bin32(v, lo, hi, bins):
    """the bin rule as the header states it, in float32 (v: float32, no NaN)"""
    lo, hi = np.float32(lo), np.float32(hi)
    scale = np.float32(bins) / (hi - lo)
    assert scale.dtype == np.float32 and np.asarray(v).dtype == np.float32
    with np.errstate(over='ignore'):
        return np.clip(np.floor((v - lo) * scale), 0, bins - 1).astype(np.int64)


def mean32(x):
    """(sum of the channels, ascending) * (1.f / C) of x [N,C,H,W] in float32"""
    s = np.zeros(x[:, 0].shape, dtype=np.float32)
    for c in range(x.shape[1]):
        s = s + x[:, c]
    return s * (np.float32(1) / np.float32(x.shape[1]))


class Truth:
    pass


def truth(moving, fixed, pred, mode, Ho, Wo):
    """everything the rules need that does not depend on bins and ranges"""
    t = Truth()
    N, Cm, Hs, Ws = moving.shape
    g = ref_grid(pred, mode, Ho, Wo, torch.float64).numpy()
    ix, iy = ((g[..., 0] + 1) * Ws - 1) / 2, ((g[..., 1] + 1) * Hs - 1) / 2
    def inside(x, y):
        xn, yn = np.rint(x), np.rint(y)                                # round half to even, as F.grid_sample(mode='nearest')
        return (xn >= 0) & (xn <= Ws - 1) & (yn >= 0) & (yn <= Hs - 1)
    t.inside = inside(ix, iy)
    t.tie = tie_mask(pred, mode, Ho, Wo, Hs, Ws)
    # of the pixels near a tie, those where the tie is the source's border: rounding the other way moves the nearest texel across it
    moved = [inside(ix + dx, iy + dy) for dx in (-TIE_BAND, TIE_BAND) for dy in (-TIE_BAND, TIE_BAND)]
    t.border = t.tie & np.logical_or.reduce([m != t.inside for m in moved])
    w64 = ref_warp(moving, pred, mode, Ho, Wo, BILINEAR)
    t.E_a = MARGIN * float(np.abs(ref_warp(moving, pred, mode, Ho, Wo, BILINEAR, torch.float32) - w64).max())
    t.a = w64.sum(1) / Cm
    t.b32 = mean32(fixed)
    t.b = fixed.astype(np.float64).sum(1) / fixed.shape[1]
    t.b_ok = ~np.isnan(t.b)
    assert np.array_equal(t.b_ok, ~np.isnan(t.b32))
    t.E_b = 2.0 ** -24 * float(np.abs(t.b[t.b_ok]).max()) if t.b_ok.any() else 0.0
    t.counted = t.inside & t.b_ok                                      # the float64 statement of "counts"
    return t


def quantile_range(v, outside=0.05):
    """(lo, hi) as float32 that leave about `outside` of the values v beyond them, half on either side"""
    lo, hi = np.quantile(v, [outside / 2, 1 - outside / 2])
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    return (lo, hi) if hi > lo else (lo - 0.5, lo + 0.5)


def expected_counts(t, bins, range_m, range_f):
    """-> sure [N,B,B], could [N,B,B], ambiguous pixels per sample [N], share of bin-ambiguous pixels"""
    N = t.a.shape[0]
    down = np.nextafter((t.a - t.E_a).astype(np.float32), np.float32(-np.inf))
    up = np.nextafter((t.a + t.E_a).astype(np.float32), np.float32(np.inf))
    ka0, ka1 = bin32(down, *range_m, bins), bin32(up, *range_m, bins)
    kb = bin32(np.where(t.b_ok, t.b32, np.float32(0)), *range_f, bins)
    bin_amb = ka0 != ka1
    sure_px = t.counted & ~t.border & ~bin_amb
    amb_px = (t.border | bin_amb) & t.b_ok & (t.inside | t.border)     # (outside and clear of the border, or NaN: certainly not counted)
    sure, could = np.zeros((N, bins, bins), dtype=np.int64), np.zeros((N, bins, bins), dtype=np.int64)
    n_of = np.broadcast_to(np.arange(N)[:, None, None], t.a.shape)
    np.add.at(sure, (n_of[sure_px], ka0[sure_px], kb[sure_px]), 1)
    for d in range(int((ka1 - ka0)[amb_px].max()) + 1 if amb_px.any() else 0):
        m = amb_px & (ka0 + d <= ka1)
        np.add.at(could, (n_of[m], (ka0 + d)[m], kb[m]), 1)
    return sure, could, amb_px.reshape(N, -1).sum(1), float(bin_amb.mean())


def depth(N, bins, Ho, Wo):
    """D of csrc/similarity.hip's header comment"""
    tiles = -(-Wo // 64) * -(-Ho // 16)
    G = min(tiles, max(256 * (8 if bins <= 32 else 6) // N, 1))
    T = -(-tiles // G)
    return 4 * T + -(-G // 256) + 18, G, T


def moment_terms(a, b):
    """the six terms and, per term, (|d/da|, |d/db|)"""
    one, zero = np.ones_like(a), np.zeros_like(a)
    return [(a, one, zero), (b, zero, one), (a * a, 2 * np.abs(a), zero), (b * b, zero, 2 * np.abs(b)), (a * b, np.abs(b), np.abs(a)),
            (np.abs(a - b), one, one)]


def check_moments(got, t, D, what):
    N = t.a.shape[0]
    for n in range(N):
        keep, known = t.counted[n], t.b_ok[n]
        ties = int((t.border[n] & known).sum())
        all_terms = moment_terms(t.a[n][known], t.b[n][known])
        for k, (term, da, db) in enumerate(moment_terms(t.a[n][keep], t.b[n][keep])):
            want = term.sum()
            tol = (D + 3) * 2.0 ** -24 * np.abs(term).sum() + (t.E_a * da + t.E_b * db).sum() + \
                ties * (np.abs(all_terms[k][0]).max() if all_terms[k][0].size else 0.0)
            print("similarity moment %-52s n %d column %d  kernel %.9g  float64 %.9g  error %.3e  bound %.3e" %
                  (what, n, k, got[n, k], want, abs(got[n, k] - want), tol))
            assert abs(float(got[n, k]) - want) <= tol, (what, n, k, got[n, k], want, tol)


# ---- drivers ----------------------------------------------------------------------------------------------------------------------------------
def _fill_value(be):
    return np.array([be.poison], dtype=np.uint32).view(np.float32)[0]


def run_hist(be, d_m, d_f, d_pred, mode, shape, bins, range_m, range_f, moments=True, d_counts=None, d_mom=None):
    """-> (counts [N,B,B] int64, moments [N,6] float32 or None) on the host, bit for bit; outputs pre-filled"""
    N, Cm, Cf, Hs, Ws, hf, wf, Ho, Wo = shape
    d_counts = be.dev_i32(np.full((N, bins, bins), GARBAGE, dtype=np.int32)) if d_counts is None else d_counts
    ws, wsb = None, 0
    if moments:
        d_mom = be.full((N, 6), _fill_value(be)) if d_mom is None else d_mom
        wsb = int(be.lib.joint_histogram_workspace(N, Ho, Wo))
        ws = be.bytes_buf(wsb)
    be.lib.joint_histogram(be.ptr(d_m), be.ptr(d_f), be.ptr(d_pred), mode, be.ptr(d_counts), be.ptr(d_mom) if moments else None, be.ptr(ws), wsb,
                           N, Cm, Cf, bins, range_m[0], range_m[1], range_f[0], range_f[1], Hs, Ws, hf, wf, Ho, Wo, be.stream)
    counts = be.raw(d_counts).view(np.uint32).reshape(N, bins, bins).astype(np.int64)
    return counts, (be.raw(d_mom).view(np.float32).reshape(N, 6) if moments else None)


def _what(mode, size, amp, Cm, Cf, bins):
    return "%s %s -> %s source %s amp %g C %d/%d bins %d" % ("UA"[mode == A], size[0], size[1], size[2] or size[1], amp, Cm, Cf, bins)


# ---- 1. counts and moments against float64 -----------------------------------------------------------------------------------------------------
def case_float64(be, size, mode=U, amp=0.15, channels=(3, 1), bins=32, N=2, seed=2, outside=0.05, fade=False):
    Cm, Cf = channels
    shape = _shape(size, N, Cm, Cf)
    N, Cm, Cf, Hs, Ws, hf, wf, Ho, Wo = shape
    moving, fixed, pred = draw_pair(seed, mode, shape, amp, fade=fade)
    what = _what(mode, size, amp, Cm, Cf, bins)
    t = truth(moving, fixed, pred, mode, Ho, Wo)
    # ranges that put about 5 % of the values outside, from the float64 reference's own values
    range_m = quantile_range(t.a[t.counted] if t.counted.any() else t.a.ravel(), outside)
    range_f = quantile_range(t.b[t.b_ok], outside)
    if t.counted.sum() > 1000:
        beyond = ((t.a[t.counted] < range_m[0]) | (t.a[t.counted] > range_m[1])).mean()
        assert 0.02 < beyond < 0.10, (what, beyond)
    sure, could, n_amb, bin_share = expected_counts(t, bins, range_m, range_f)
    print("similarity counts %-52s E_a %.3e  border-ambiguous %.5f  bin-ambiguous %.5f  counted %.3f" %
          (what, t.E_a, t.tie.mean(), bin_share, t.counted.mean()))
    assert t.tie.mean() <= TIE_SHARE and bin_share <= TIE_SHARE, (what, t.tie.mean(), bin_share)
    got, mom = run_hist(be, be.dev(moving), be.dev(fixed), be.dev(pred), mode, shape, bins, range_m, range_f)
    assert np.all(sure <= got) and np.all(got <= sure + could), (what, int((sure - got).max()), int((got - sure - could).max()))
    total, sure_total = got.reshape(N, -1).sum(1), sure.reshape(N, -1).sum(1)
    assert np.all(sure_total <= total) and np.all(total <= sure_total + n_amb), (what, sure_total, total, n_amb)
    D, G, T = depth(N, bins, Ho, Wo)
    check_moments(mom, t, D, what)
    return t, got, (G, T)


def case_leaves_source(be, mode=U):
    """amp 1.5: a good share of the pixels sample outside the source and do not count"""
    t, got, _ = case_float64(be, LEAVES_SOURCE, mode, amp=1.5, seed=4)
    assert (~t.inside).mean() > 0.05, "the field does not leave the source: the case would show nothing"
    assert np.all(got.reshape(got.shape[0], -1).sum(1) < t.a[0].size)


def case_two_trips(be):
    t, got, (G, T) = case_float64(be, TWO_TRIPS, U, channels=(1, 1), bins=64, N=1, seed=5, fade=True)
    assert T == 2 and G == 1536


# ---- 2. bitwise: repeatable, optional moments, unaligned, the two LDS-add variants --------------------------------------------------------------
@both_poisons
def case_bitwise(be, size, mode=U, channels=(3, 1), bins=32, N=2, seed=3):
    Cm, Cf = channels
    shape = _shape(size, N, Cm, Cf)
    N, Cm, Cf, Hs, Ws, hf, wf, Ho, Wo = shape
    moving, fixed, pred = draw_pair(seed, mode, shape)
    rm, rf = (0.1, 0.9), (0.05, 0.95)
    d_m, d_f, d_pred = be.dev(moving), be.dev(fixed), be.dev(pred)
    counts, mom = run_hist(be, d_m, d_f, d_pred, mode, shape, bins, rm, rf)
    fill = _fill_value(be)
    if np.isfinite(fill):
        assert not np.any(mom == fill), "a moment was not written"
    assert np.all(np.isfinite(mom)) and counts.sum() > 0
    counts2, mom2 = run_hist(be, d_m, d_f, d_pred, mode, shape, bins, rm, rf,
                             d_counts=be.dev_i32(np.full((N, bins, bins), -1, dtype=np.int32)))      # other garbage
    assert np.array_equal(counts, counts2) and np.array_equal(mom.view(np.uint32), mom2.view(np.uint32)), "two calls, different bits"
    counts3, none = run_hist(be, d_m, d_f, d_pred, mode, shape, bins, rm, rf, moments=False)
    assert none is None and np.array_equal(counts, counts3), "counts differ without moments"
    counts4, mom4 = run_hist(be, d_m, d_f, _off_by_4_bytes(be, pred, be.dev), mode, shape, bins, rm, rf,
                             d_counts=_off_by_4_bytes(be, np.full(N * bins * bins, GARBAGE, dtype=np.int32), be.dev_i32),
                             d_mom=_off_by_4_bytes(be, np.full(N * 6, fill, dtype=np.float32), be.dev))
    assert np.array_equal(counts, counts4) and np.array_equal(mom.view(np.uint32), mom4.view(np.uint32)), "views 4 bytes off the 16-byte grid: different bits"
    # measurement build: wave-aggregated adds (nemar_tune(46, 0)) / every lane adds for itself (the default)
    be.lib.tune(46, 0)
    try:
        counts5, mom5 = run_hist(be, d_m, d_f, d_pred, mode, shape, bins, rm, rf)
    finally:
        be.lib.tune(46, 1)
    assert np.array_equal(counts, counts5) and np.array_equal(mom.view(np.uint32), mom5.view(np.uint32)), "the two LDS-add variants differ"


# ---- 3. properties ------------------------------------------------------------------------------------------------------------------------------
def case_identity(be, hw=(67, 45), bins=32, N=2, seed=8):
    """dtheta = 0, equal sizes, the same single-channel image on both sides, every value on a bin centre: every pixel counts (whatever
    fp32 does to the last column's position), the table is diagonal and equals numpy's plain histogram"""
    H, W = hw
    lo, hi = -1.0, 1.0
    k = np.random.default_rng(seed).integers(0, bins, (N, 1, H, W))
    img = (lo + (k + 0.5) * ((hi - lo) / bins)).astype(np.float32)
    d_img = be.dev(img)
    got, mom = run_hist(be, d_img, d_img, be.zeros(N, 6), A, (N, 1, 1, H, W, 0, 0, H, W), bins, (lo, hi), (lo, hi))
    want = np.zeros((N, bins, bins), dtype=np.int64)
    for n in range(N):
        h = np.histogram(img[n].ravel().astype(np.float64), bins=bins, range=(lo, hi))[0]
        assert np.array_equal(h, np.bincount(k[n].ravel(), minlength=bins))
        want[n][np.arange(bins), np.arange(bins)] = h
    assert np.array_equal(got, want), int(np.abs(got - want).max())
    assert np.all(got.reshape(N, -1).sum(1) == H * W)
    assert np.all(np.abs(mom[:, 5]) <= 1e-3 * H * W)              # sum |a - b| of an image against itself: position rounding only


def case_ranking(be, size=RAGGED, mode=U, channels=(3, 1), bins=32, N=2, seed=9, amp=0.15):
    """fixed = g(the library's own warp of moving by pred) for a nonlinear monotone g of the channel mean: mutual information with pred
    must exceed the value with the identity prediction"""
    from nemar_amd import ops
    Cm, Cf = channels
    shape = _shape(size, N, Cm, Cf)
    N, Cm, Cf, Hs, Ws, hf, wf, Ho, Wo = shape
    moving, _, pred = draw_pair(seed, mode, shape, amp)
    up = lambda t: torch.nn.functional.interpolate(t, size=(Hs, Ws), mode='bicubic', align_corners=False)
    g = torch.Generator().manual_seed(seed)
    moving = up(torch.rand(N, Cm, 12, 16, generator=g)).clamp_(0, 1).numpy().astype(np.float32)       # a smooth texture: the identity scores above zero
    d_m, d_pred = be.dev(moving), be.dev(pred)
    warped = be.np(run_fused(be, d_m, d_pred, mode, BILINEAR, (N, Cm, Hs, Ws, hf, wf, Ho, Wo)))
    mean = warped.mean(1, keepdims=True)
    fixed = np.exp(2.0 * mean) / np.exp(2.0)                       # g: monotone, nonlinear, [0, 1] -> (0, 1]
    fixed = np.repeat(fixed, Cf, 1).astype(np.float32)
    d_f = be.dev(fixed)
    with_pred, m1 = run_hist(be, d_m, d_f, d_pred, mode, shape, bins, (0.0, 1.0), (0.0, 1.0))
    with_identity, m0 = run_hist(be, d_m, d_f, be.zeros(N, 6), A, shape, bins, (0.0, 1.0), (0.0, 1.0))
    s1, s0 = ops.similarity_summary(with_pred, m1), ops.similarity_summary(with_identity, m0)
    print("similarity ranking: MI %.4f with the prediction, %.4f with the identity; NCC %.4f / %.4f" % (s1['mi'], s0['mi'], s1['ncc'], s0['ncc']))
    assert s1['mi'] > s0['mi']


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------------
def case_refusals(be):
    """NEMAR_EINVAL (-1), a message, and nothing launched: `counts` and `moments` keep their fill"""
    from nemar_amd._lib import NemarHipError
    N, Cm, Cf, B, Hs, Ws, hf, wf, Ho, Wo = 2, 3, 1, 8, 12, 16, 6, 8, 10, 14
    d_m, d_f, d_pred, d_th = be.zeros(N, Cm, Hs, Ws), be.zeros(N, Cf, Ho, Wo), be.zeros(N, 2, hf, wf), be.zeros(N, 6)
    d_counts = be.dev_i32(np.full((N, 65, 65), GARBAGE, dtype=np.int32))        # (room for the 65-bin call, should it ever launch)
    d_mom = be.full((N, 6), 7.0)
    wsb = int(be.lib.joint_histogram_workspace(N, Ho, Wo))
    assert wsb > 0 and int(be.lib.joint_histogram_workspace(N, Ho, 0)) == 0
    ws = be.bytes_buf(wsb + 4)
    off2 = lambda p: ctypes.c_void_p(p.value + 2)
    names = ("m", "f", "pred", "mode", "counts", "mom", "ws", "wsb", "N", "Cm", "Cf", "bins", "lo_m", "hi_m", "lo_f", "hi_f", "Hs", "Ws", "hf", "wf",
             "Ho", "Wo")
    good = [be.ptr(d_m), be.ptr(d_f), be.ptr(d_pred), U, be.ptr(d_counts), be.ptr(d_mom), be.ptr(ws), wsb, N, Cm, Cf, B, -1.0, 1.0, -1.0, 1.0, Hs, Ws,
            hf, wf, Ho, Wo]

    def refused(**change):
        args = [change.get(k, v) for k, v in zip(names, good)]
        with pytest.raises(NemarHipError, match=r"failed \(-1\): joint_histogram: \S"):
            be.lib.joint_histogram(*args, be.stream)

    for k in ("m", "f", "pred", "counts"):                        # required pointers: null, not even 4-byte aligned
        refused(**{k: None})
        refused(**{k: off2(good[names.index(k)])})
    refused(mom=off2(good[5]))                                    # (a null `moments` is the counts-only call)
    refused(ws=None)                                              # moments without a workspace
    refused(ws=off2(good[6]))
    refused(wsb=wsb - 1)                                          # ... or with a short one
    refused(wsb=0)
    for side in ("m", "f"):                                       # hi <= lo, or no number at all
        refused(**{"lo_" + side: 1.0})
        refused(**{"lo_" + side: 2.0})
        refused(**{"hi_" + side: float('nan')})
        refused(**{"hi_" + side: float('inf')})
    for b in (1, 0, -4, 65):
        refused(bins=b)
    for k in ("Cm", "Cf"):
        for c in (0, -1, 65):
            refused(**{k: c})
    for m in (GRID_EXPLICIT, 3, -1):                              # an explicit grid has one resolution; 3 and -1 are no modes at all
        refused(mode=m)
    for k in ("N", "Hs", "Ws", "Ho", "Wo"):                       # non-positive sizes
        refused(**{k: 0})
        refused(**{k: -3})
    for k in ("hf", "wf"):                                        # UNET without a field
        refused(**{k: 0})
        refused(**{k: -1})
    refused(N=65536)
    refused(Ho=1 << 16, Wo=1 << 15)                               # Ho * Wo = 2^31
    refused(Hs=1 << 16, Ws=1 << 15)
    be.sync()
    assert np.all(be.raw(d_counts).view(np.uint32) == GARBAGE) and np.all(be.np(d_mom) == 7.0)
    # AFFINE ignores hf, wf; 64 bins and 64 channels are served; without moments the workspace is not looked at
    d_m64 = be.zeros(N, 64, Hs, Ws)
    be.lib.joint_histogram(be.ptr(d_m64), be.ptr(d_f), be.ptr(d_th), A, be.ptr(d_counts), None, None, 0, N, 64, Cf, 64, -1.0, 1.0, -1.0, 1.0, Hs, Ws,
                           0, -1, Ho, Wo, be.stream)
    got = be.raw(d_counts).view(np.uint32)[:N * 64 * 64].reshape(N, 64, 64)
    assert np.all(got[:, 32, 32] == Ho * Wo) and got.sum() == N * Ho * Wo          # two images of zeros: everything in the bin that starts at 0
    assert np.all(be.np(d_mom) == 7.0)
