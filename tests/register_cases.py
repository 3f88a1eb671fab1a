"""Backend-agnostic test bodies of nemar_warp_resampled_fwd (csrc/register.hip: the STN's prediction applied to an image of another
size, coarse field interpolated in registers), driven through tests/backends.py (EmuBackend: host-emulated kernels, CPU tier;
HipBackend: the gfx950 library, `-m gpu` tier).

The float64 truth is torch on the CPU, written out here: F.interpolate + torch.linspace / F.affine_grid + F.grid_sample in float64.
The rules (why each bound is what it is):
  bitwise   the bilinear result equals nemar_bilinear_fwd + nemar_grid_sample_fwd on the same backend bit for bit: one statement of
            the arithmetic (warp_grid.h, resize_taps.h), no contraction.
  bilinear  against float64: the yardstick of a case is the max-abs error of torch's OWN fp32 evaluation of the same formula on the CPU;
            the kernel's must be <= 4 x that — both are fp32 evaluations of one formula with different rounding orders, and the error is
            position error (~4e-5 px) times image gradient.
  nearest   against float64: exact (a source value or zero is copied), except pixels whose float64 sampling position lies within TIE_BAND
            px of a rounding tie in x or y; the float64 reference alone must exclude <= 1 % of a case's pixels."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from backends import both_poisons

GRID_EXPLICIT, GRID_UNET, GRID_AFFINE = 0, 1, 2
BILINEAR, NEAREST = 0, 1
TIE_BAND = 1e-3            # px
TIE_SHARE = 0.01
MARGIN = 4.0               # kernel error <= MARGIN x torch-fp32 error, both against float64

#           (hf, wf),  (Ho, Wo),   (Hs, Ws) or None = the output size,  C
UPSAMPLING = [((32, 48), (131, 203), None, 3), ((64, 64), (256, 256), None, 1), ((36, 48), (288, 384), None, 3),
              ((16, 24), (67, 45), None, 5), ((32, 48), (131, 203), (90, 120), 3)]
EQUAL = ((40, 56), (40, 56), None, 3)
DOWN = ((64, 64), (24, 40), (50, 70), 3)
ALL_SIZES = UPSAMPLING + [EQUAL, DOWN]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def smooth_field(seed, N, hf, wf, amp):
    """bicubic-upsampled 4 x 5 Gaussian noise, max |.| = amp normalised units"""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn(N, 2, 4, 5, generator=g, dtype=torch.float64)
    f = F.interpolate(coarse, size=(hf, wf), mode='bicubic', align_corners=False)
    return (f * (amp / f.abs().max())).numpy().astype(np.float32)


def draw(seed, mode, N, C, hf, wf, Hs, Ws, amp=0.15, labels=False):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 8, (N, C, Hs, Ws)).astype(np.float32) if labels else rng.random((N, C, Hs, Ws)).astype(np.float32)
    pred = smooth_field(seed, N, hf, wf, amp) if mode == GRID_UNET else (rng.uniform(-1, 1, (N, 6)) * amp).astype(np.float32)
    return img, pred


# ---- torch on the CPU: the float64 truth, and (dtype float32) the yardstick -----------------------------------------------------------------
def ref_grid(pred, mode, Ho, Wo, dtype):
    p = torch.as_tensor(np.asarray(pred), dtype=dtype)
    if mode == GRID_UNET:
        if tuple(p.shape[2:]) != (Ho, Wo):
            p = F.interpolate(p, size=(Ho, Wo), mode='bilinear', align_corners=False)
        x, y = torch.linspace(-1, 1, Wo, dtype=dtype), torch.linspace(-1, 1, Ho, dtype=dtype)
        return torch.stack([x[None, None, :] + p[:, 0], y[None, :, None] + p[:, 1]], dim=-1)
    theta = p + torch.tensor([1, 0, 0, 0, 1, 0], dtype=dtype)[None]
    return F.affine_grid(theta.view(-1, 2, 3), (p.shape[0], 1, Ho, Wo), align_corners=False)


def ref_warp(img, pred, mode, Ho, Wo, sample, dtype=torch.float64):
    grid = ref_grid(pred, mode, Ho, Wo, dtype)
    out = F.grid_sample(torch.as_tensor(np.asarray(img), dtype=dtype), grid, mode='nearest' if sample == NEAREST else 'bilinear',
                        padding_mode='zeros', align_corners=False)
    return out.numpy().astype(np.float64)


def tie_mask(pred, mode, Ho, Wo, Hs, Ws):
    """[N,Ho,Wo] True where the float64 sampling position is within TIE_BAND px of a rounding tie (x.5) in x or y"""
    g = ref_grid(pred, mode, Ho, Wo, torch.float64).numpy()
    ix, iy = ((g[..., 0] + 1) * Ws - 1) / 2, ((g[..., 1] + 1) * Hs - 1) / 2
    near = lambda v: np.abs(v - np.floor(v) - 0.5) < TIE_BAND
    return near(ix) | near(iy)


# ---- drivers ----------------------------------------------------------------------------------------------------------------------------------
def run_fused(be, d_img, d_pred, mode, sample, shape, d_out=None):
    N, C, Hs, Ws, hf, wf, Ho, Wo = shape
    d_out = be.full((N, C, Ho, Wo), np.nan) if d_out is None else d_out
    be.lib.warp_resampled_fwd(be.ptr(d_img), be.ptr(d_pred), mode, sample, be.ptr(d_out), N, C, Hs, Ws, hf, wf, Ho, Wo, be.stream)
    return d_out


def run_composed(be, d_img, d_pred, mode, shape):
    """what a caller had before: nemar_bilinear_fwd (the field at the output size, in memory), then nemar_grid_sample_fwd"""
    N, C, Hs, Ws, hf, wf, Ho, Wo = shape
    d_field = d_pred
    if mode == GRID_UNET and (hf, wf) != (Ho, Wo):
        d_field = be.full((N, 2, Ho, Wo), np.nan)
        be.lib.bilinear_fwd(be.ptr(d_pred), be.ptr(d_field), N * 2, hf, wf, Ho, Wo, be.stream)
    d_out = be.full((N, C, Ho, Wo), np.nan)
    be.lib.grid_sample_fwd(be.ptr(d_img), be.ptr(d_field), mode, be.ptr(d_out), N, C, Hs, Ws, Ho, Wo, be.stream)
    return d_out


def _shape(size, N):
    (hf, wf), (Ho, Wo), src, C = size
    Hs, Ws = src or (Ho, Wo)
    return (N, C, Hs, Ws, hf, wf, Ho, Wo)


# ---- the three comparisons ----------------------------------------------------------------------------------------------------------------
def check_bilinear(got, img, pred, mode, Ho, Wo, what):
    want = ref_warp(img, pred, mode, Ho, Wo, BILINEAR)
    yard = np.abs(ref_warp(img, pred, mode, Ho, Wo, BILINEAR, torch.float32) - want).max()
    err = np.abs(got - want).max()
    print("register bilinear %-46s kernel %.3e  torch-fp32 %.3e  ratio %.2f" % (what, err, yard, err / yard if yard else float('inf')))
    assert np.all(np.isfinite(got)), what
    assert err <= MARGIN * yard, (what, err, yard)
    return err, yard


def check_nearest(got, img, pred, mode, Ho, Wo, what):
    Hs, Ws = img.shape[2:]
    tie = tie_mask(pred, mode, Ho, Wo, Hs, Ws)
    share = tie.mean()
    print("register nearest  %-46s excluded %.4f" % (what, share))
    assert share <= TIE_SHARE, (what, share)
    want = ref_warp(img, pred, mode, Ho, Wo, NEAREST)
    keep = np.broadcast_to(~tie[:, None], want.shape)
    assert np.array_equal(got[keep], want[keep]), (what, int((got[keep] != want[keep]).sum()))
    assert np.all(np.isfinite(got)), what


# ---- 1. bitwise against the composed path ---------------------------------------------------------------------------------------------------
def case_bitwise(be, size, mode=GRID_UNET, N=2, seed=0, amp=0.15):
    shape = _shape(size, N)
    N, C, Hs, Ws, hf, wf, Ho, Wo = shape
    img, pred = draw(seed, mode, N, C, hf, wf, Hs, Ws, amp)
    d_img, d_pred = be.dev(img), be.dev(pred)
    fused = be.raw(run_fused(be, d_img, d_pred, mode, BILINEAR, shape))
    assert np.array_equal(fused, be.raw(run_composed(be, d_img, d_pred, mode, shape))), "fused != composed: %s mode %d" % (size, mode)


# ---- 2. bilinear against float64 ----------------------------------------------------------------------------------------------------------------
def case_bilinear(be, size, mode=GRID_UNET, N=2, seed=1, amp=0.15):
    shape = _shape(size, N)
    N, C, Hs, Ws, hf, wf, Ho, Wo = shape
    img, pred = draw(seed, mode, N, C, hf, wf, Hs, Ws, amp)
    got = be.np(run_fused(be, be.dev(img), be.dev(pred), mode, BILINEAR, shape))
    return check_bilinear(got, img, pred, mode, Ho, Wo, "mode %d field %s -> %s source %s C %d" % (mode, (hf, wf), (Ho, Wo), (Hs, Ws), C))


# ---- 3. nearest against float64 ------------------------------------------------------------------------------------------------------------------
def case_nearest(be, size, mode=GRID_UNET, N=2, seed=2, amp=0.15, labels=False):
    shape = _shape(size, N)
    N, C, Hs, Ws, hf, wf, Ho, Wo = shape
    img, pred = draw(seed, mode, N, C, hf, wf, Hs, Ws, amp, labels=labels)
    got = be.np(run_fused(be, be.dev(img), be.dev(pred), mode, NEAREST, shape))
    check_nearest(got, img, pred, mode, Ho, Wo, "mode %d field %s -> %s source %s%s" % (mode, (hf, wf), (Ho, Wo), (Hs, Ws), " labels" if labels else ""))
    if labels:
        assert set(np.unique(got)) <= set(np.unique(img)) | {0.0}, "nearest sampling made a value that is no label"


# ---- 4. routes and edges --------------------------------------------------------------------------------------------------------------------------
def _off_by_4_bytes(be, a):
    """`a` in a buffer that starts 4 bytes past a 16-byte boundary (a view of a guarded block one element longer)"""
    d_buf = be.dev(np.concatenate([[0.0], np.asarray(a, dtype=np.float32).ravel()]))
    return be.sub(d_buf, 1, d_buf.shape[0])


@both_poisons
def case_unaligned(be, size, mode=GRID_UNET, N=1, seed=3):
    """pred and out 4 bytes off the 16-byte grid (4-byte alignment is all the entry point asks for): the same bits as the aligned call"""
    shape = _shape(size, N)
    N, C, Hs, Ws, hf, wf, Ho, Wo = shape
    img, pred = draw(seed, mode, N, C, hf, wf, Hs, Ws)
    d_img = be.dev(img)
    aligned = be.raw(run_fused(be, d_img, be.dev(pred), mode, BILINEAR, shape))
    d_out = _off_by_4_bytes(be, np.full(N * C * Ho * Wo, np.nan))
    run_fused(be, d_img, _off_by_4_bytes(be, pred), mode, BILINEAR, shape, d_out=d_out)
    assert np.array_equal(be.raw(d_out), aligned)
    got = be.np(d_out).reshape(N, C, Ho, Wo)
    check_bilinear(got, img, pred, mode, Ho, Wo, "unaligned mode %d %s -> %s" % (mode, (hf, wf), (Ho, Wo)))


@both_poisons
def case_edges(be, size, mode=GRID_UNET, N=1, seed=4, amp=0.15):
    """bilinear and nearest against float64 at one shape (thin outputs, N = 1, fields that leave the source: zero padding)"""
    shape = _shape(size, N)
    N, C, Hs, Ws, hf, wf, Ho, Wo = shape
    img, pred = draw(seed, mode, N, C, hf, wf, Hs, Ws, amp)
    d_img, d_pred = be.dev(img), be.dev(pred)
    what = "edges mode %d %s -> %s source %s amp %g" % (mode, (hf, wf), (Ho, Wo), (Hs, Ws), amp)
    check_bilinear(be.np(run_fused(be, d_img, d_pred, mode, BILINEAR, shape)), img, pred, mode, Ho, Wo, what)
    got = be.np(run_fused(be, d_img, d_pred, mode, NEAREST, shape))
    check_nearest(got, img, pred, mode, Ho, Wo, what)
    if amp >= 1.0:           # the field really leaves the source: a good share of exact zeros, where float64 has them
        want = ref_warp(img, pred, mode, Ho, Wo, NEAREST)
        assert (want == 0).mean() > 0.05


def case_vector_route(be, size, mode=GRID_UNET, N=1, seed=6):
    """measurement build only: the 4-pixels-per-lane / 16-byte-store route (nemar_tune(44, 1)) gives the default route's bits, bilinear and
    nearest — on widths it takes (Wo % 4 == 0, aligned out) and on those that fall back"""
    shape = _shape(size, N)
    N, C, Hs, Ws, hf, wf, Ho, Wo = shape
    img, pred = draw(seed, mode, N, C, hf, wf, Hs, Ws)
    d_img, d_pred = be.dev(img), be.dev(pred)
    for sample in (BILINEAR, NEAREST):
        want = be.raw(run_fused(be, d_img, d_pred, mode, sample, shape))
        be.lib.tune(44, 1)
        try:
            got = be.raw(run_fused(be, d_img, d_pred, mode, sample, shape))
        finally:
            be.lib.tune(44, 0)
        assert np.array_equal(got, want), (size, mode, sample)


# ---- 5. repeatable, refusals ----------------------------------------------------------------------------------------------------------------
def case_repeatable(be, size=UPSAMPLING[0], seed=5):
    for mode in (GRID_UNET, GRID_AFFINE):
        shape = _shape(size, 2)
        N, C, Hs, Ws, hf, wf, Ho, Wo = shape
        img, pred = draw(seed, mode, N, C, hf, wf, Hs, Ws)
        d_img, d_pred = be.dev(img), be.dev(pred)
        for sample in (BILINEAR, NEAREST):
            a, b = run_fused(be, d_img, d_pred, mode, sample, shape), run_fused(be, d_img, d_pred, mode, sample, shape)
            assert np.array_equal(be.raw(a), be.raw(b))


def case_refusals(be):
    """NEMAR_EINVAL (-1), a message, and nothing launched: `out` keeps its fill"""
    from nemar_amd._lib import NemarHipError
    einval = r"failed \(-1\): warp_resampled_fwd: \S"
    N, C, Hs, Ws, hf, wf, Ho, Wo = 2, 3, 12, 16, 6, 8, 12, 16
    d_img, d_pred, d_th, d_out = be.zeros(N, C, Hs, Ws), be.zeros(N, 2, hf, wf), be.zeros(N, 6), be.full((N, C, Ho, Wo), 7.0)
    img, pred, th, out = be.ptr(d_img), be.ptr(d_pred), be.ptr(d_th), be.ptr(d_out)
    off2 = lambda p: ctypes.c_void_p(p.value + 2)
    good = [img, pred, GRID_UNET, BILINEAR, out, N, C, Hs, Ws, hf, wf, Ho, Wo]

    def refused(**change):
        names = ("inp", "pred", "mode", "sample", "out", "N", "C", "Hs", "Ws", "hf", "wf", "Ho", "Wo")
        args = [change.get(k, v) for k, v in zip(names, good)]
        with pytest.raises(NemarHipError, match=einval):
            be.lib.warp_resampled_fwd(*args, be.stream)

    for k in ("inp", "pred", "out"):
        refused(**{k: None})                                    # null pointers
        refused(**{k: off2(dict(inp=img, pred=pred, out=out)[k])})      # not even 4-byte aligned
    for k in ("N", "C", "Hs", "Ws", "Ho", "Wo"):                 # non-positive sizes
        refused(**{k: 0})
        refused(**{k: -3})
    for m in (GRID_EXPLICIT, 3, -1):                            # an explicit grid has one resolution; 3 and -1 are no modes at all
        refused(mode=m)
    for s in (2, -1):
        refused(sample=s)
    for k in ("hf", "wf"):                                      # UNET without a field
        refused(**{k: 0})
        refused(**{k: -1})
    be.sync()
    assert np.all(be.np(d_out) == 7.0)
    be.lib.warp_resampled_fwd(img, th, GRID_AFFINE, BILINEAR, out, N, C, Hs, Ws, 0, 0, Ho, Wo, be.stream)       # AFFINE ignores hf, wf
    assert np.all(be.np(d_out) == 0.0)                          # (a zero source, warped)
