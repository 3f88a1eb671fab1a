"""Backend-agnostic test bodies of nemar_surface_distance (csrc/surface.hip: the distances between the class boundaries of the warped
moving label map and of the fixed label map), driven through tests/backends.py (EmuBackend: host-emulated kernels, CPU tier;
HipBackend: the gfx950 library, `-m gpu` tier).  Every buffer is guard-banded there; counts, hist and dist2 are read back bit for bit.

ONE rule: exact, integer for integer.  The moving class map is the same backend's own nemar_warp_resampled_fwd(NEAREST, C = 1) output
(score_cases.library_warp, as score_cases.check_exact takes it); from there the truth is written out here in numpy — the boundary by a
padded 4-neighbour comparison, d2 by brute force over the two boundary point sets, the histogram by bincount — and counts, hist and
dist2 must equal it with no pixel excluded and no tolerance: squared pixel distances are integers and integer addition has no order.
There is no float64 tier: the warp's rounding is score_cases' and register_cases' subject, and one flipped pixel moves distances
non-locally."""
import ctypes

import numpy as np
import pytest

from backends import both_poisons
from register_cases import GRID_AFFINE, GRID_EXPLICIT, GRID_UNET, UPSAMPLING, EQUAL, DOWN
from score_cases import LEAVES_SOURCE, ONE_TEXEL_FIELD, _inputs, _off_by_4_bytes, _shape, class_np, label_map, library_warp

GARBAGE = 0x5a5a5a5a
COLS = ("boundary", "far", "max_d2")
# the routes of a prediction: (name, mode, field size as a function of the output size)
ROUTES = [("unet_equal", GRID_UNET, lambda hw: hw), ("unet_resampled", GRID_UNET, lambda hw: (8, 12)), ("affine", GRID_AFFINE, lambda hw: (8, 12))]
# output sizes where the 64 x 16 tile logic ends: one row, one column, one past the tile in both directions, exactly one tile
TILE_EDGES = [(1, 77), (50, 1), (17, 65), (16, 64)]
CONTENT_SIZE = UPSAMPLING[0]                              # 131 x 203: three tile columns, nine tile rows, odd sizes


def edge_size(hw, field):
    return (tuple(field(hw)), hw, (9, 13), 1)


# ---- the truth ------------------------------------------------------------------------------------------------------------------------
def boundary_np(S):
    """S ^ binary_erosion(S) with the 4-connected footprint and border_value = 0, by a padded neighbour comparison"""
    P = np.pad(S, 1, constant_values=False)
    return S & ~(P[:-2, 1:-1] & P[2:, 1:-1] & P[1:-1, :-2] & P[1:-1, 2:])


def nearest_d2(A, Bp):
    """for every point of A [a,2] the smallest squared distance to a point of Bp [b,2]: brute force, int64"""
    out = np.empty(len(A), dtype=np.int64)
    step = max(1, (1 << 22) // max(1, len(Bp)))
    for i in range(0, len(A), step):
        d = A[i:i + step, None, :].astype(np.int64) - Bp[None, :, :].astype(np.int64)
        out[i:i + step] = (d * d).sum(-1).min(1)
    return out


def truth(m, f, K, D):
    """(counts [N,K,2,3], hist [N,K,2,D*D], dist2 [N,2,Ho,Wo]) int64 of maps m, f [N,Ho,Wo] of label VALUES"""
    km, kf = class_np(m, K), class_np(f, K)
    N, Ho, Wo = km.shape
    B = D * D
    counts, hist = np.zeros((N, K, 2, 3), dtype=np.int64), np.zeros((N, K, 2, B), dtype=np.int64)
    dist2 = np.full((N, 2, Ho, Wo), -1, dtype=np.int64)
    for n in range(N):
        for k in np.union1d(km[n][km[n] >= 0], kf[n][kf[n] >= 0]):
            edges = [boundary_np(km[n] == k), boundary_np(kf[n] == k)]
            pts = [np.argwhere(e) for e in edges]
            counts[n, k, :, 0] = [len(p) for p in pts]
            for dr in (0, 1):
                if not len(pts[dr]):
                    continue
                if not len(pts[1 - dr]):
                    dist2[n, dr][edges[dr]] = -2
                    continue
                d2 = nearest_d2(pts[dr], pts[1 - dr])
                dist2[n, dr][edges[dr]] = d2                  # (argwhere and boolean indexing share the row-major order)
                hist[n, k, dr] = np.bincount(d2[d2 < B], minlength=B)
                counts[n, k, dr, 1:] = [(d2 >= B).sum(), d2.max()]
    return counts, hist, dist2


# ---- drivers ----------------------------------------------------------------------------------------------------------------------------
class Out:
    """the three results of one call as the buffers hold them, bit for bit"""

    def __init__(self, be, N, K, D, Ho, Wo, d_counts, d_hist, d_dist):
        self.counts = be.raw(d_counts).view(np.uint32).reshape(N, K, 2, 3).astype(np.int64)
        self.hist = be.raw(d_hist).view(np.uint32).reshape(N, K, 2, D * D).astype(np.int64)
        self.dist2 = None if d_dist is None else be.raw(d_dist).view(np.int32).reshape(N, 2, Ho, Wo).astype(np.int64)


def workspace_bytes(be, N, K, Ho, Wo):
    return int(be.lib.surface_distance_workspace(N, K, Ho, Wo))


def run_surface(be, d_lm, d_lf, d_pred, mode, K, D, shape, dist=True, fill=GARBAGE, bufs=None):
    """-> Out; every output (and the workspace) pre-filled with `fill` unless the caller brings buffers (counts, hist, dist2, ws)"""
    N, _, Hs, Ws, hf, wf, Ho, Wo = shape
    wsb = workspace_bytes(be, N, K, Ho, Wo)
    assert wsb >= 8 * N * Ho * Wo
    word = np.array(fill, dtype=np.uint32).view(np.int32)
    if bufs is None:
        bufs = (be.dev_i32(np.full(N * K * 6, word)), be.dev_i32(np.full(N * K * 2 * D * D, word)),
                be.dev_i32(np.full(N * 2 * Ho * Wo, word)) if dist else None, be.dev_i32(np.full((wsb + 3) // 4, word)))
    d_counts, d_hist, d_dist, d_ws = bufs
    be.lib.surface_distance(be.ptr(d_lm), be.ptr(d_lf), be.ptr(d_pred), mode, be.ptr(d_counts), be.ptr(d_hist), be.ptr(d_dist), be.ptr(d_ws),
                            wsb, N, K, D, Hs, Ws, hf, wf, Ho, Wo, be.stream)
    return Out(be, N, K, D, Ho, Wo, d_counts, d_hist, d_dist)


def assert_equal(got, want, what):
    counts, hist, dist2 = want
    for c, name in enumerate(COLS):
        assert np.array_equal(got.counts[..., c], counts[..., c]), (what, name, np.argwhere(got.counts[..., c] != counts[..., c])[:4].tolist())
    assert np.array_equal(got.hist, hist), (what, "hist", np.argwhere(got.hist != hist)[:4].tolist())
    if got.dist2 is not None:
        assert np.array_equal(got.dist2, dist2), (what, "dist2", np.argwhere(got.dist2 != dist2)[:4].tolist())
    # what the outputs owe each other
    assert np.array_equal(got.hist.sum(-1) + got.counts[..., 1], np.where(got.counts[..., 0].min(-1, keepdims=True) > 0, got.counts[..., 0], 0)), what


def check_exact(be, shape, lm, lf, pred, mode, K, D, what, dist=True):
    """against the truth over the library's own nearest warp"""
    d_lm, d_pred = be.dev(lm[:, None]), be.dev(pred)
    got = run_surface(be, d_lm, be.dev(lf), d_pred, mode, K, D, shape, dist=dist)
    m = library_warp(be, d_lm, d_pred, mode, shape)
    want = truth(m, lf, K, D)
    assert_equal(got, want, what)
    return got, want


# ---- 1. every route, the sizes where the tile logic ends -------------------------------------------------------------------------------------
def case_route(be, size, mode, N=2, seed=0, amp=0.15, D=16):
    """score_cases' inputs: an 8-class per-pixel random moving map, a blocky fixed map, register_cases' predictions"""
    shape, lm, lf, pred = _inputs(size, mode, N, seed, amp)
    got, _ = check_exact(be, shape, lm, lf, pred, mode, 8, D, "route %s mode %d amp %g" % (size, mode, amp))
    assert got.counts[..., 0].sum() > 0
    if min(shape[6:]) > 1 and amp < 1:
        assert (got.counts[..., 2] > 0).any(), "no distance but 0: the case would show nothing"


# ---- 2. label content ------------------------------------------------------------------------------------------------------------------------
@both_poisons
def case_content(be, kind, K, mode=GRID_UNET, size=CONTENT_SIZE, N=2, seed=7, junk=False, D=8):
    """moving and fixed of the same kind (different seeds): blocky, per-pixel random, one class filling the plane; junk: values of no
    class on either side, never boundary pixels"""
    shape, lm, lf, pred = _inputs(size, mode, N, seed, 0.15, K=K, moving=kind, fixed=kind, junk=junk)
    got, (counts, hist, dist2) = check_exact(be, shape, lm, lf, pred, mode, K, D, "content %s K %d junk %s mode %d" % (kind, K, junk, mode))
    Ho, Wo = shape[6:]
    if kind == "single" and not junk:                       # the fixed map's class fills the plane: its boundary is the plane's border
        assert np.all(got.counts[:, (K - 1) // 2, 1, 0] == 2 * (Ho + Wo) - 4)
    if junk:
        none = class_np(lf, K) < 0
        assert none.any() and np.all(got.dist2[:, 1][none] == -1)


def case_special(be, N=1):
    """a one-pixel class, a class touching all four plane borders, a class present in one map only (an undefined pair: -2), K = 1 and
    K = 1024 with classes 0, 511 and 1023 present — identity prediction, maps of different content"""
    H, W = 37, 70
    ident = be.zeros(N, 6)
    shape = (N, 1, H, W, 0, 0, H, W)

    def run(m, f, K, D=16):
        m, f = (np.broadcast_to(a, (N, H, W)).astype(np.float32) for a in (m, f))
        got = run_surface(be, be.dev(m), be.dev(f), ident, GRID_AFFINE, K, D, shape)
        want = truth(m, f, K, D)
        assert_equal(got, want, "special K %d" % K)
        return got

    # class 1: one pixel in m, a 3 x 3 block in f; class 2: a frame touching all four borders in m, a cross touching them in f;
    # class 3: in m only
    m, f = np.zeros((H, W)), np.zeros((H, W))
    m[[0, -1], :], m[:, [0, -1]] = 2, 2
    f[H // 2, :], f[:, W // 3] = 2, 2
    m[10, 20] = 1
    f[20:23, 40:43] = 1
    m[25:30, 50:60] = 3
    got = run(m, f, 4)
    assert got.counts[0, 1, 0].tolist() == [1, 1, (20 - 10) ** 2 + (40 - 20) ** 2]             # 500 >= 16^2: far, and max d2 exact
    assert got.counts[0, 3].tolist() == [[26, 0, 0], [0, 0, 0]] and got.hist[0, 3].sum() == 0
    assert np.all(got.dist2[0, 0][25:30, 50:60][[0, -1]] == -2) and got.dist2[0, 0, 27, 55] == -1
    # K = 1: everything that is 0 is the class, the rest belongs to no class
    got = run(np.where(m == 2, 0, 5), np.where(f == 2, 0, 5), 1)
    assert got.counts[0, 0, :, 0].tolist() == [2 * (H + W) - 4, H + W - 2]       # (the cross's centre has its four neighbours)
    # K = 1024: three classes present, 1021 absent; the classes as the largest ids and the middle one
    remap = np.array([0, 511, 1023, 1023])
    got = run(remap[m.astype(int)], remap[np.where(f == 1, 0, f).astype(int)], 1024)
    present = np.flatnonzero(got.counts[0, :, :, 0].sum(-1))
    assert present.tolist() == [0, 511, 1023]
    assert got.counts[0, 511, :, 0].tolist() == [1, 0] and got.dist2[0, 0, 10, 20] == -2       # the one pixel: in m only now


# ---- 3. analytic: no oracle ------------------------------------------------------------------------------------------------------------------
RECT = (15, 30)


def rect_pair(H=40, W=60):
    """a 15 x 30 rectangle of class 1 and the same rectangle shifted 4 rows and 3 columns"""
    m, f = np.zeros((1, H, W), np.float32), np.zeros((1, H, W), np.float32)
    m[0, 8:8 + RECT[0], 10:10 + RECT[1]] = 1
    f[0, 12:12 + RECT[0], 13:13 + RECT[1]] = 1
    return m, f


def _identity(be, m, f, K, D, dist=True):
    N, H, W = m.shape
    return run_surface(be, be.dev(m), be.dev(f), be.zeros(N, 6), GRID_AFFINE, K, D, (N, 1, H, W, 0, 0, H, W), dist=dist)


def case_analytic(be):
    m, f = rect_pair()
    got = _identity(be, m, f, 2, 64)
    assert got.counts[0, 1].tolist() == [[86, 0, 25], [86, 0, 25]]
    pooled = np.sqrt(np.repeat(np.arange(64 * 64), got.hist[0, 1].sum(0)))
    assert len(pooled) == 172 and np.percentile(pooled, 95) == 4.0
    assert_equal(got, truth(m, f, 2, 64), "rectangle")
    # a map against itself: every d2 is 0, all mass in bin 0
    lab = label_map("blocky", 4, 2, 45, 67, 5)
    got = _identity(be, lab, lab, 5, 4)
    assert np.all(got.counts[..., 1:] == 0) and np.all(got.hist[..., 1:] == 0)
    assert np.array_equal(got.hist[..., 0], got.counts[..., 0]) and got.hist.sum() > 0
    assert np.all((got.dist2 == 0) | (got.dist2 == -1)) and np.array_equal(got.dist2[:, 0], got.dist2[:, 1])


def case_far(be):
    m, f = rect_pair()
    want = truth(m, f, 2, 64)
    near, d64, d128 = _identity(be, m, f, 2, 2), _identity(be, m, f, 2, 64), _identity(be, m, f, 2, 128)
    assert_equal(near, truth(m, f, 2, 2), "max_dist 2")
    assert near.hist.shape[-1] == 4
    assert np.array_equal(near.counts[0, 1, :, 1], want[1][0, 1, :, 4:].sum(-1)) and np.all(near.counts[0, 1, :, 1] > 0)
    assert near.counts[0, 1, :, 2].tolist() == [25, 25]                                      # max d2 is exact beyond the histogram
    assert np.array_equal(near.dist2, d64.dist2)
    assert np.array_equal(d128.hist[..., :64 * 64], d64.hist) and np.all(d128.hist[..., 64 * 64:] == 0)
    assert np.array_equal(d128.counts, d64.counts)


# ---- 4. samples do not leak into each other ---------------------------------------------------------------------------------------------------
def case_samples(be, mode=GRID_UNET, size=UPSAMPLING[3], K=6, D=12):
    """N = 3 with different content per sample: blocky, one class, per-pixel random (classes absent in some samples, present in others)"""
    shape, _, _, pred = _inputs(size, mode, 3, 5, 0.15)
    N, _, Hs, Ws, hf, wf, Ho, Wo = shape
    lm = np.concatenate([label_map(kind, 30 + i, 1, Hs, Ws, K) for i, kind in enumerate(("blocky", "single", "random"))])
    lf = np.concatenate([label_map(kind, 40 + i, 1, Ho, Wo, K) for i, kind in enumerate(("blocky", "blocky", "single"))])
    got, _ = check_exact(be, shape, lm, lf, pred, mode, K, D, "samples mode %d" % mode)
    for n in range(N):                                     # every sample alone gives its own rows
        one = (1,) + shape[1:]
        alone, _ = check_exact(be, one, lm[n:n + 1], lf[n:n + 1], pred[n:n + 1], mode, K, D, "sample %d alone" % n)
        assert np.array_equal(alone.counts[0], got.counts[n]) and np.array_equal(alone.hist[0], got.hist[n])


def case_chunks(be, N=3, K=1024, D=6):
    """planes and a class count at which the vertical-distance planes of all classes exceed the entry point's bound: the classes are
    served in several chunks, with classes present in the first, a middle and the last of them, differently per sample"""
    (Ho, Wo), G = CONTENT_SIZE[1], 128 << 20
    chunk = G // (4 * N * Ho * Wo)
    assert 1 < chunk < K // 2 and workspace_bytes(be, N, K, Ho, Wo) == (8 + 4 * chunk) * N * Ho * Wo, "the case no longer spans several chunks"
    ids = np.array([0, chunk - 1, chunk, 2 * chunk + 3, K - 1])
    lm, lf = (np.stack([ids[(label_map("blocky", seed + n, 1, Ho, Wo, 5)[0].astype(int) + n) % (5 - n)] for n in range(N)]).astype(np.float32)
              for seed in (60, 70))
    lf[1][lf[1] == ids[2]] = ids[0]                                # sample 1: the first class of the second chunk in the moving map only
    shape = (N, 1, Ho, Wo, 0, 0, Ho, Wo)
    pred = np.zeros((N, 6), np.float32)
    pred[:, 2] = 0.05                                              # a shift of a few pixels
    got, _ = check_exact(be, shape, lm, lf, pred, GRID_AFFINE, K, D, "chunks")
    present = [np.flatnonzero(got.counts[n, :, :, 0].sum(-1)).tolist() for n in range(N)]
    assert present[0] == ids.tolist() and present[2] == ids[:3].tolist() and np.all(got.counts[1, ids[2], :, 0] == [got.counts[1, ids[2], 0, 0], 0])
    assert got.counts[..., 1].sum() > 0 and got.hist.sum() > 0


# ---- 5. repeatable, overwritten, unaligned, with and without the map ------------------------------------------------------------------------
@both_poisons
def case_repeatable_unaligned(be, size, mode=GRID_UNET, N=1, seed=3, K=8, D=8):
    shape, lm, lf, pred = _inputs(size, mode, N, seed, 0.15)
    N, _, Hs, Ws, hf, wf, Ho, Wo = shape
    d_lm, d_lf, d_pred = be.dev(lm), be.dev(lf), be.dev(pred)
    a = run_surface(be, d_lm, d_lf, d_pred, mode, K, D, shape)
    b = run_surface(be, d_lm, d_lf, d_pred, mode, K, D, shape, fill=0xffffffff)                # other garbage
    for x, y in ((a.counts, b.counts), (a.hist, b.hist), (a.dist2, b.dist2)):
        assert np.array_equal(x, y), "two calls, different bits"
    c = run_surface(be, d_lm, d_lf, d_pred, mode, K, D, shape, dist=False)
    assert c.dist2 is None and np.array_equal(a.counts, c.counts) and np.array_equal(a.hist, c.hist), "dist2 changed counts or hist"
    wsb = workspace_bytes(be, N, K, Ho, Wo)
    off = lambda n: _off_by_4_bytes(be, np.full(n, GARBAGE, dtype=np.int32), be.dev_i32)
    bufs = (off(N * K * 6), off(N * K * 2 * D * D), off(N * 2 * Ho * Wo), off((wsb + 3) // 4))
    d = run_surface(be, _off_by_4_bytes(be, lm, be.dev), _off_by_4_bytes(be, lf, be.dev), _off_by_4_bytes(be, pred, be.dev), mode, K, D, shape, bufs=bufs)
    for x, y in ((a.counts, d.counts), (a.hist, d.hist), (a.dist2, d.dist2)):
        assert np.array_equal(x, y), "views 4 bytes off the 16-byte grid: different bits"
    assert a.counts[..., 0].sum() > 0


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------------
def case_refusals(be):
    """NEMAR_EINVAL (-1), a message, and nothing written: counts, hist, dist2 and the workspace keep their fill"""
    from nemar_amd._lib import NemarHipError
    N, K, D, Hs, Ws, hf, wf, Ho, Wo = 2, 4, 3, 12, 16, 6, 8, 10, 14
    d_lm, d_lf, d_pred, d_th = be.zeros(N, Hs, Ws), be.zeros(N, Ho, Wo), be.zeros(N, 2, hf, wf), be.zeros(N, 6)
    wsb = workspace_bytes(be, N, K, Ho, Wo)
    assert wsb == 8 * N * Ho * Wo + K * 4 * N * Ho * Wo                  # small planes: one chunk holds every class
    outs = [be.dev_i32(np.full(n, GARBAGE, dtype=np.int32)) for n in (N * K * 6, N * K * 2 * D * D, N * 2 * Ho * Wo, wsb // 4)]
    d_counts, d_hist, d_dist, d_ws = outs
    off2 = lambda p: ctypes.c_void_p(p.value + 2)
    names = ("lm", "lf", "pred", "mode", "counts", "hist", "dist2", "ws", "wsb", "N", "K", "D", "Hs", "Ws", "hf", "wf", "Ho", "Wo")
    good = [be.ptr(d_lm), be.ptr(d_lf), be.ptr(d_pred), GRID_UNET, be.ptr(d_counts), be.ptr(d_hist), be.ptr(d_dist), be.ptr(d_ws), wsb,
            N, K, D, Hs, Ws, hf, wf, Ho, Wo]

    def refused(**change):
        args = [change.get(k, v) for k, v in zip(names, good)]
        with pytest.raises(NemarHipError, match=r"failed \(-1\): surface_distance: \S"):
            be.lib.surface_distance(*args, be.stream)

    for k in ("lm", "lf", "pred", "counts", "hist", "ws"):
        refused(**{k: None})                                      # null required pointers
    for k in ("lm", "lf", "pred", "counts", "hist", "dist2", "ws"):
        refused(**{k: off2(good[names.index(k)])})                # not 4-byte aligned
    for k in (0, -1, 1025):
        refused(K=k)
    for d in (0, -1, 129):
        refused(D=d)
    refused(Ho=32769, Wo=1)                                       # a side above 32768, whatever the plane's size
    refused(Ho=1, Wo=32769)
    for k in ("N", "Hs", "Ws", "Ho", "Wo"):                       # non-positive sizes
        refused(**{k: 0})
        refused(**{k: -3})
    for m in (GRID_EXPLICIT, 3, -1):                              # what pred_ok refuses
        refused(mode=m)
    for k in ("hf", "wf"):
        refused(**{k: 0})
        refused(**{k: -1})
    refused(N=65536)                                              # what tile_grid_ok refuses
    refused(wsb=wsb - 1)
    refused(wsb=0)
    be.sync()
    for h in outs:
        assert np.all(be.raw(h).view(np.uint32) == GARBAGE)
    assert workspace_bytes(be, N, 1025, Ho, Wo) == 0 and workspace_bytes(be, N, K, 32769, 1) == 0
    # the size query is honest about the chunks: planes too large for every class at once get fewer
    assert workspace_bytes(be, 4, 64, 1024, 1024) == (8 + 8 * 4) * 4 * 1024 * 1024
    assert workspace_bytes(be, 4, 2, 1024, 1024) == (8 + 2 * 4) * 4 * 1024 * 1024
    assert workspace_bytes(be, 1, 1024, 32768, 32768) == (8 + 4) * 32768 * 32768
    # AFFINE ignores hf, wf; K = 1024, max_dist = 128 and dist2 = NULL are served
    big = [be.dev_i32(np.full(n, GARBAGE, dtype=np.int32)) for n in (N * 1024 * 6, N * 1024 * 2 * 128 * 128, 1, workspace_bytes(be, N, 1024, Ho, Wo) // 4)]
    got = run_surface(be, d_lm, d_lf, d_th, GRID_AFFINE, 1024, 128, (N, 1, Hs, Ws, 0, 0, Ho, Wo), dist=False, bufs=(big[0], big[1], None, big[3]))
    edge = 2 * (Ho + Wo) - 4                                      # two maps of zeros: class 0 fills both planes
    assert np.all(got.counts[:, 0] == [edge, 0, 0]) and np.all(got.counts[:, 1:] == 0)
    assert np.all(got.hist[:, 0, :, 0] == edge) and got.hist.sum() == 2 * N * edge


# ---- 7. the truth itself (CPU tier only: scipy) ---------------------------------------------------------------------------------------------
def check_truth_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    K, D = 5, 64
    for kind, seed in (("blocky", 1), ("random", 2), ("single", 3)):
        m, f = label_map(kind, seed, 2, 45, 67, K), label_map(kind, seed + 50, 2, 45, 67, K)
        counts, hist, dist2 = truth(m, f, K, D)
        for n in range(2):
            for k in range(K):
                em, ef = ((a[n] == k) ^ ndi.binary_erosion(a[n] == k, structure=ndi.generate_binary_structure(2, 1), border_value=0) for a in (m, f))
                assert np.array_equal(em, boundary_np(m[n] == k)) and np.array_equal(ef, boundary_np(f[n] == k))
                assert counts[n, k, :, 0].tolist() == [em.sum(), ef.sum()]
                if em.any() and ef.any():
                    for dr, (a, b) in enumerate(((em, ef), (ef, em))):
                        d2 = np.rint(ndi.distance_transform_edt(~b)[a] ** 2).astype(np.int64)
                        assert np.array_equal(dist2[n, dr][a], d2)
                        assert np.array_equal(hist[n, k, dr], np.bincount(d2[d2 < D * D], minlength=D * D))
                        assert counts[n, k, dr, 2] == d2.max()
