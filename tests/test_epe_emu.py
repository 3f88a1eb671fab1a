"""CPU tier: nemar_epe_loss_fwd / _bwd (csrc/epe.hip) compiled for the host SIMT emulator (tests/emu), against the float64 statement of
their definition with autograd, where samples leave the image, at thin planes and the 4 / 1 pixel switch, at their closed forms, as the
gradient of a descent, and at their refusals (tests/epe_cases.py); tests/test_epe_gpu.py runs the same bodies on the gfx950 library."""
import pytest

import epe_cases as K
from backends import EmuBackend
from register_cases import GRID_AFFINE, GRID_UNET

MODES = [GRID_UNET, GRID_AFFINE]
mode_id = lambda m: "unet" if m == GRID_UNET else "affine"


@pytest.fixture(scope="module")
def be(emu_lib):
    return EmuBackend(emu_lib)


@pytest.mark.parametrize("eps", [0.01, 0.5])
@pytest.mark.parametrize("kind", ["smooth", "fold"])
@pytest.mark.parametrize("size", K.ONE_PIXEL + K.FOUR_PIXEL, ids=str)
@pytest.mark.parametrize("mode", MODES, ids=mode_id)
def test_against_float64(be, mode, size, kind, eps):
    K.case_against_float64(be, mode, size, kind, eps)


@pytest.mark.parametrize("size", [K.ONE_PIXEL[0], K.FOUR_PIXEL[0]], ids=str)
@pytest.mark.parametrize("mode", MODES, ids=mode_id)
def test_rough_field_the_cell_choice_matters(be, mode, size):
    K.case_against_float64(be, mode, size, 'rough', 0.01)


@pytest.mark.parametrize("size", [K.ONE_PIXEL[0], K.FOUR_PIXEL[0]], ids=str)
@pytest.mark.parametrize("mode", MODES, ids=mode_id)
def test_leaving_the_image(be, mode, size):
    K.case_leaving(be, mode, size)


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("size", K.EDGES, ids=str)
@pytest.mark.parametrize("mode", MODES, ids=mode_id)
def test_edges(be, mode, size, N):
    K.case_against_float64(be, mode, size, 'smooth', 0.01, N=N)


@pytest.mark.parametrize("eps", [0.01, 0.5])
@pytest.mark.parametrize("size", [(16, 32), (64, 64)], ids=str)
def test_zero_residual_is_eps_with_a_zero_gradient(be, size, eps):
    K.case_zero_residual(be, size, eps)


@pytest.mark.parametrize("size", [(16, 32), (64, 64)], ids=str)
def test_constant_translation_in_closed_form(be, size):
    K.case_translation(be, size)


@pytest.mark.parametrize("mode,size", K.DESCENT, ids=lambda v: mode_id(v) if isinstance(v, int) else str(v))
def test_descent_on_the_prediction(be, mode, size):
    K.case_descent(mode, size, K.entry_point_loss_and_grad(be, mode, size))


@pytest.mark.parametrize("size", [K.ONE_PIXEL[0], K.FOUR_PIXEL[0], (9, 13)], ids=str)
@pytest.mark.parametrize("mode", MODES, ids=mode_id)
def test_repeatable_overwritten_unaligned_accumulated(be, mode, size):
    K.case_repeatable_unaligned_accumulate(be, mode, size)


def test_refusals(be):
    K.case_refusals(be)


@pytest.mark.parametrize("size", [K.ONE_PIXEL[1], K.FOUR_PIXEL[0]], ids=str)
@pytest.mark.parametrize("mode", MODES, ids=mode_id)
def test_non_finite_input(be, mode, size):
    K.case_non_finite(be, mode, size)
