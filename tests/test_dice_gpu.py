"""`-m gpu`: nemar_dice_sums / nemar_dice_loss_fwd / _bwd (csrc/dice.hip) on the gfx950 library — the bodies of tests/dice_cases.py
that tests/test_dice_emu.py runs on the emulator."""
import pytest

import dice_cases as K
from backends import HipBackend
from register_cases import GRID_AFFINE, GRID_UNET

pytestmark = pytest.mark.gpu

MODES = [GRID_UNET, GRID_AFFINE]
mode_id = lambda m: "unet" if m == GRID_UNET else "affine"


@pytest.fixture(scope="module")
def be(hip_lib):
    return HipBackend(hip_lib)


@pytest.mark.parametrize("kind", ["smooth", "leaving"])
@pytest.mark.parametrize("classes", K.CLASSES)
@pytest.mark.parametrize("size", K.SHAPES, ids=str)
@pytest.mark.parametrize("mode", MODES, ids=mode_id)
def test_sums_loss_and_gradient_against_float64(be, mode, size, classes, kind):
    K.case_against_float64(be, mode, size, classes, kind)


@pytest.mark.parametrize("mode", MODES, ids=mode_id)
def test_background_included(be, mode):
    K.case_against_float64(be, mode, K.SHAPES[2], 5, "smooth", k0=0, eps=0.25)


@pytest.mark.parametrize("size", [(16, 32), (64, 64)], ids=str)
def test_identity_of_equal_maps_is_zero_loss(be, size):
    K.case_identity(be, size)


@pytest.mark.parametrize("mode", MODES, ids=mode_id)
def test_disjoint_maps_in_closed_form(be, mode):
    K.case_disjoint(be, mode, K.SHAPES[1])


@pytest.mark.parametrize("mode", MODES, ids=mode_id)
def test_absent_class_adds_nothing_and_background_is_left_out(be, mode):
    K.case_absent_class_and_background(be, mode, K.SHAPES[2])


@pytest.mark.parametrize("mode", MODES, ids=mode_id)
def test_non_class_values_are_ignored(be, mode):
    K.case_non_class_values(be, mode, K.SHAPES[1])


@pytest.mark.parametrize("size", [K.SHAPES[1], K.SHAPES[4]], ids=str)
@pytest.mark.parametrize("mode", MODES, ids=mode_id)
def test_non_finite_prediction(be, mode, size):
    K.case_non_finite(be, mode, size)


@pytest.mark.parametrize("size", [K.SHAPES[0], K.SHAPES[3], K.SHAPES[4], K.SHAPES[5]], ids=str)
@pytest.mark.parametrize("mode", MODES, ids=mode_id)
def test_repeatable_unaligned_accumulated(be, mode, size):
    K.case_repeatable_unaligned_accumulate(be, mode, size)


@pytest.mark.parametrize("shape", K.GRID_STRIDE, ids=str)
def test_a_workgroup_walks_more_than_one_tile(be, shape):
    K.case_grid_stride(be, *shape)


def test_refusals(be):
    K.case_refusals(be)


@pytest.mark.parametrize("size", K.DESCENT, ids=str)
def test_descent_on_the_offsets(be, size):
    K.case_descent(size, K.entry_point_loss_and_grad(be))


@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("shape", [(40, 48, 32, 32), (37, 45, 25, 31), (20, 70, 17, 65)], ids=str)
def test_labels_crop_flip_deform(be, shape, unaligned):
    K.case_labels(be, *shape, unaligned=unaligned)


def test_labels_crop_flip_deform_refusals(be):
    K.case_labels_refusals(be)
