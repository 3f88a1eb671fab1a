"""`-m gpu`: nemar_compose_pred (csrc/compose.hip) on the gfx950 library — the bodies of tests/compose_cases.py that
tests/test_compose_emu.py runs on the emulator, and the network's own size (256 x 256 fields, more workgroups than the chip has CUs at
batch 8) — and ops.compose_predictions on top of it."""
import numpy as np
import pytest
import torch

import compose_cases as K
from backends import HipBackend

pytestmark = pytest.mark.gpu

NETWORK = ((256, 256), (256, 256), (256, 256))
UPSAMPLED = ((64, 64), (128, 96), (515, 770))


@pytest.fixture(scope="module")
def be(hip_lib):
    return HipBackend(hip_lib)


@pytest.mark.parametrize("m1,m2", K.MODE_PAIRS)
@pytest.mark.parametrize("size", K.SIZES + [NETWORK, UPSAMPLED], ids=str)
def test_against_float64(be, size, m1, m2):
    K.case_float64(be, size, m1, m2)


@pytest.mark.parametrize("m1,m2", K.MODE_PAIRS)
def test_against_float64_where_the_position_leaves_the_image(be, m1, m2):
    K.case_float64(be, K.RAGGED, m1, m2, amp=1.5)


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("m1,m2", K.MODE_PAIRS)
@pytest.mark.parametrize("size", [K.RAGGED, K.EQUAL, K.DOWN, K.THIN[0], NETWORK], ids=str)
def test_fused_warp_is_the_librarys_warp(be, size, m1, m2, C):
    K.case_fused_warp(be, size, m1, m2, C, N=8 if size is NETWORK else 2)


def test_fused_warp_where_the_position_leaves_the_image(be):
    K.case_fused_warp(be, K.RAGGED, K.U, K.U, 3, amp=1.5)


@pytest.mark.parametrize("m1,m2", K.MODE_PAIRS)
def test_composition_is_sequential_warping(be, m1, m2):
    K.case_sequential(be, m1, m2)


@pytest.mark.parametrize("size", [K.RAGGED, K.EQUAL, K.THIN[1]], ids=str)
def test_affine_closed_form(be, size):
    K.case_affine_closed_form(be, size)


@pytest.mark.parametrize("m1,m2", K.MODE_PAIRS)
@pytest.mark.parametrize("size", [K.RAGGED, ((9, 13), (9, 13), (9, 13)), K.DOWN, UPSAMPLED], ids=str)
def test_repeatable_overwritten_unaligned(be, size, m1, m2):
    K.case_repeatable_unaligned(be, size, m1, m2)


def test_refusals(be):
    K.case_refusals(be)


@pytest.mark.parametrize("m1,m2", K.MODE_PAIRS)
def test_ops_compose_predictions(be, m1, m2):
    """the Python layer hands the kernel what the test bodies hand it: the same bits, with and without the image; shapes are checked"""
    from nemar_amd import ops
    N, C, size = 2, 3, K.RAGGED
    H, W = size[2]
    first, second = K.draw_pair(6, m1, m2, N, size)
    img = np.random.default_rng(6).random((N, C, H, W)).astype(np.float32)
    d_field, d_out = K.run_compose(be, be.dev(first), m1, be.dev(second), m2, size, N, be.dev(img), C)
    t_first, t_second, t_img = (torch.from_numpy(a).cuda() for a in (first, second, img))
    field = ops.compose_predictions(t_first, m1, t_second, m2, (H, W))
    field2, warped = ops.compose_predictions(t_first, m1, t_second, m2, (H, W), image=t_img)
    assert field.shape == (N, 2, H, W) and torch.equal(field, field2) and torch.equal(field.cpu(), d_field.cpu())
    assert torch.equal(warped.cpu(), d_out.cpu())
    assert torch.equal(warped, ops.warp_resampled(field, ops.GRID_UNET, [t_img], None)[0])
    with pytest.raises(ValueError, match="compose_predictions"):
        ops.compose_predictions(t_first, m1, t_second[:1], m2, (H, W))
    with pytest.raises(ValueError, match="compose_predictions"):
        ops.compose_predictions(t_first, m1, t_second, m2, (H, W), image=t_img[:, :, :-1])
    with pytest.raises(ValueError, match="compose_predictions"):
        ops.compose_predictions(t_first, K.GRID_EXPLICIT, t_second, m2, (H, W))
