"""`-m gpu` tier of the bounds cases (tests/guard_cases.py): self-tests of the guard bands of tests/backends.py (host-side stores through
ordinary torch indexing ops into the test's own allocation), then every kernel family at the shapes where its vector, chunk or tile logic
ends, on the gfx950 library — each library call followed by a device sync and a guard check."""
import re

import numpy as np
import pytest

import backends as B
import bn_cases as BN
import deform_cases as D
import guard_cases as G
import kernel_cases as K
from backends import HipBackend

pytestmark = pytest.mark.gpu

FLAT = G.FLAT_N + G.FLAT_N_LONG
GRID_HW = [(15, 63), (16, 64), (17, 65), (15, 127), (17, 129), (16, 65), (17, 64)]


@pytest.fixture(scope="module")
def be(hip_lib):
    return HipBackend(hip_lib)


# ---- the mechanism itself -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [1, 3, 17, 4096])
def test_payload_is_exact_and_aligned(be, nbytes):
    """the payload is exactly the requested bytes on a 16-byte boundary; the back guard starts at byte `nbytes`"""
    h = be.bytes_buf(nbytes)
    assert be.ptr(h).value % 16 == 0 and be.raw(h).size == nbytes and not be.raw(h).any()
    be.check_guards("untouched")
    be.poke(h, nbytes - 1, 0xEE)                     # the payload's last byte is the test's own
    be.check_guards("last payload byte written")
    assert be.raw(h)[-1] == 0xEE
    be.poke(h, nbytes, 0xEE)                         # ... the next one is not
    with pytest.raises(AssertionError, match=r"bytes_buf buffer.*%d bytes, back guard, first bad byte at payload offset \+%d " % (nbytes, nbytes)):
        be.check_guards("self-test")
    be.check_guards("reported once")                 # (a failed test's traceback keeps its buffers alive: the next call is not blamed)


@pytest.mark.parametrize("poison", B.POISONS)
def test_one_byte_either_side_is_reported(be, poison):
    """an ordinary in-allocation host-side store of one BIT at payload offset -1 / +nbytes (and at the far ends of the guards): reported
    with the buffer, the side, the offset and the call's name, by the explicit check and by a read-back; an untouched set passes; the
    other live buffers are not blamed"""
    with be.poisoned(poison):
        a, c = be.dev(np.arange(7)), be.dev_i32(np.arange(4))
    for off, side in ((-1, "front"), (60, "back"), (60 + B.GUARD_BYTES - 1, "back"), (-B.GUARD_BYTES, "front")):
        with be.poisoned(poison):
            b = be.full((3, 5), 1.0, role="victim")
        assert be.poison_of(b) & ~0xf00 == poison & ~0xf00
        be.check_guards("untouched")
        assert np.array_equal(be.np(a), np.arange(7)) and np.array_equal(be.np(c), np.arange(4)) and np.all(be.np(b) == 1.0)
        be.poke(b, off)
        what = r"victim buffer, shape \(3, 5\).*60 bytes, %s guard, .*offset %s " % (side, re.escape("%+d" % off))
        if side == "front":
            with pytest.raises(AssertionError, match="after nemar_self_test: " + what):
                be.check_guards("nemar_self_test")
        else:
            with pytest.raises(AssertionError, match="after read-back: " + what):
                be.np(a)
        be.check_guards("reported once")
        assert np.array_equal(be.np(a), np.arange(7))


def test_guard_words_poison_what_reads_them(be):
    """an aligned 32-bit read anywhere in a guard sees the whole poison word, also behind a payload that is not a multiple of 4; every
    per-allocation variant of the two poisons is still a quiet NaN / still ~1e38, and odd as an integer"""
    for nbytes in (16, 17, 18, 19):
        for poison in B.POISONS:
            with be.poisoned(poison):
                h = be.bytes_buf(nbytes)
            word = be.poison_of(h)
            pat = B._pattern(word, nbytes % 4)
            first = (-nbytes) % 4                    # first 4-byte boundary behind the payload
            assert int(pat[first:first + 4].copy().view(np.uint32)[0]) == word
            f = np.array([word], dtype=np.uint32).view(np.float32)[0]
            assert word % 2 == 1 and (np.isnan(f) if poison == B.POISON_NAN else (np.isfinite(f) and f > 9e37))
    x, y = be.dev(np.ones(3)), be.dev(np.ones(3))
    assert be.poison_of(x) != be.poison_of(y), "neighbouring allocations carry different poison words"


def test_every_launch_is_followed_by_a_check(be):
    """be.lib: an entry point that takes a stream is followed by a sync and a guard check under its own name; a freed buffer leaves the registry"""
    x, y = be.dev(np.ones(5)), be.full((5,), np.nan)
    n0 = be.checks
    be.lib.add2(be.ptr(x), be.ptr(x), be.ptr(y), 5, be.stream)
    assert be.checks == n0 + 1
    be.poke(y, 20)
    with pytest.raises(AssertionError, match="after nemar_add2: full buffer"):
        be.lib.add2(be.ptr(x), be.ptr(x), be.ptr(y), 5, be.stream)
    y2 = be.full((5,), np.nan)
    live = len(be.live_blocks())
    del y2
    assert len(be.live_blocks()) == live - 1, "a freed buffer leaves the registry"
    be.check_guards("nothing else is blamed")
    assert np.all(be.np(x) == 1.0)


# ---- flat kernels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", FLAT)
def test_flat_act_add(be, n):
    G.case_flat_act_add(be, n)


@pytest.mark.parametrize("n", FLAT)
def test_flat_dropout(be, n):
    G.case_flat_dropout(be, n)


@pytest.mark.parametrize("n", FLAT)
def test_flat_losses_adam(be, n):
    G.case_flat_losses_adam(be, n)


@pytest.mark.parametrize("n", FLAT)
def test_flat_absmax(be, n):
    G.case_flat_absmax(be, n)


@pytest.mark.parametrize("n", FLAT)
def test_flat_concat(be, n):
    G.case_flat_concat(be, n)


@pytest.mark.parametrize("shape", G.BIAS_GRAD)
def test_bias_grad(be, shape):
    G.case_bias_grad(be, *shape)


# ---- plane kernels --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", G.PLANE_W)
def test_pool_bilinear(be, W):
    G.case_pool_bilinear(be, W)


@pytest.mark.parametrize("W", G.PLANE_W)
def test_smoothness(be, W):
    G.case_smoothness(be, W)


@pytest.mark.parametrize("W", G.PLANE_W)
def test_crop_flip_normalize(be, W):
    G.case_crops(be, W)


@pytest.mark.parametrize("W", G.PLANE_W)
def test_instnorm(be, W):
    G.case_instnorm(be, W)


@pytest.mark.parametrize("W", G.PLANE_W)
def test_deform_field_sample_meter(be, W):
    """nemar_deform_field, nemar_crop_flip_deform_normalize (crops at the pool's corners, both flips: deform_cases.case_sample) and
    nemar_registration_error at heights 2 and 3"""
    for H in (2, 3):
        D.case_field(be, H, W, 4, 5, seed=W)
        D.case_sample(be, 2, H + 1, W + 1, H, W, 0.5, seed=W)
        D.case_sample(be, 1, H, W, H, W, 1.5, seed=W)
    if W >= 4:                    # (the meter's smooth test fields need a plane that is not a sliver)
        D.case_meter(be, D.GRID_UNET, 2, max(4, W // 2), W, seed=W)
        D.case_meter(be, D.GRID_AFFINE, 1, max(4, W // 2) + 1, W, seed=W)


@pytest.mark.parametrize("W", G.PLANE_W)
def test_batchnorm(be, W):
    for H in (1, 2, 3):
        BN.case_batchnorm_train(be, 2, 3, H, W, 1, BN.ACT_LRELU, residual=(H == 2), seed=W)
    BN.case_batchnorm_train(be, 4, 2, 1, W, 2, BN.ACT_RELU, seed=W)
    BN.case_batchnorm_eval(be, 2, 3, 2, W, BN.ACT_NONE, residual=True, seed=W)


# ---- grid sample ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [K.GRID_UNET, K.GRID_AFFINE, K.GRID_EXPLICIT])
@pytest.mark.parametrize("H,W", GRID_HW)
def test_grid_sample_ragged_tiles(be, mode, H, W):
    G.case_grid_edges(be, mode, H, W)


@pytest.mark.parametrize("H,W", GRID_HW[:3])
def test_grid_sample_ragged_tiles_without_workspace(be, H, W):
    for mode in (K.GRID_UNET, K.GRID_AFFINE, K.GRID_EXPLICIT):
        G.case_grid_edges(be, mode, H, W, workspace=False)


@pytest.mark.parametrize("workspace", [True, False])
@pytest.mark.parametrize("H,W", GRID_HW[:4])
def test_grid_sample_borders(be, H, W, workspace):
    G.case_grid_borders(be, H, W, workspace=workspace)


# ---- convolutions ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", G.CONV_EXACT)
def test_conv_exact(be, shape):
    G.case_conv_exact(be, shape)


@pytest.mark.parametrize("shape", G.CONV_NARROW)
def test_conv_narrow(be, shape):
    G.case_conv_narrow(be, shape)


@pytest.mark.parametrize("shape", G.CONV_S16G)
def test_conv_s16g(be, shape):
    G.case_conv_s16g(be, shape)


@pytest.mark.parametrize("shape", G.CONV_S16G_WGRAD)
def test_conv_s16g_weight_gradient(be, shape):
    K.case_conv_s16g_bwd_weight(be, *shape, seed=3)


@pytest.mark.parametrize("shape", G.CONV_S16G_DGRAD)
def test_conv_s16g_data_gradient(be, shape):
    G.case_conv_s16g_dgrad(be, shape)


@pytest.mark.parametrize("shape", G.CONV_K7_FWD)
def test_conv_k7_forward(be, shape):
    K.case_conv_k7_fwd(be, *shape, act=K.O.ACT_RELU, seed=1)


@pytest.mark.parametrize("shape", G.CONV_K7_DGRAD)
def test_conv_k7_data_gradient(be, shape):
    K.case_conv_k7_bwd_data(be, *shape, seed=2)


@pytest.mark.parametrize("shape", G.CONV_K7_WGRAD)
def test_conv_k7_weight_gradient(be, shape):
    K.case_conv_k7_bwd_weight(be, *shape, seed=3)


@pytest.mark.parametrize("what", ["fwd", "dgrad", "wgrad"])
def test_conv_split16(be, what):
    for shape in {"fwd": G.CONV_SPLIT16, "dgrad": G.CONV_SPLIT16_DGRAD, "wgrad": G.CONV_SPLIT16_WGRAD}[what]:
        G.case_conv_split16(be, shape, what)


@pytest.mark.parametrize("shape", G.CONV_TRANSPOSE)
def test_conv_transpose(be, shape):
    K.case_conv_transpose_fwd(be, *shape, seed=4)
    with K.s16g_route(be, on=False):
        K.case_conv_transpose_fwd(be, *shape, act=K.O.ACT_LRELU, seed=5)
