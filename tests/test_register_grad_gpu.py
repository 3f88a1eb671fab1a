"""`-m gpu`: nemar_warp_resampled_bwd (csrc/register.hip) on the gfx950 library — the bodies of tests/register_grad_cases.py that
tests/test_register_grad_emu.py runs on the emulator."""
import pytest

import register_grad_cases as K
from backends import HipBackend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(hip_lib):
    return HipBackend(hip_lib)


@pytest.mark.parametrize("size", K.SIZES, ids=str)
@pytest.mark.parametrize("mode", K.MODES, ids=K.mode_id)
def test_against_float64(be, mode, size):
    K.case_float64(be, mode, size)


@pytest.mark.parametrize("seed", [2, 3])
def test_equal_sizes_are_grid_sample_bwd_bit_for_bit(be, seed):
    K.case_equal_bitwise(be, seed=seed)


@pytest.mark.parametrize("size", [K.RESAMPLED[0], K.RESAMPLED[3], K.RESAMPLED[4], K.RESAMPLED[5], K.RESAMPLED[6], K.TILE_EDGES[2]], ids=str)
@pytest.mark.parametrize("mode", K.MODES, ids=K.mode_id)
def test_adjoint_of_the_fused_forward(be, mode, size):
    K.case_adjoint(be, mode, size)


@pytest.mark.parametrize("size", [K.RESAMPLED[0], K.RESAMPLED[3], K.EQUAL], ids=str)
@pytest.mark.parametrize("mode", K.MODES, ids=K.mode_id)
def test_repeatable_overwritten_accumulated(be, mode, size):
    K.case_repeat_accumulate(be, mode, size)


@pytest.mark.parametrize("size", [K.RESAMPLED[1], K.TILE_EDGES[3], K.EQUAL], ids=str)
@pytest.mark.parametrize("mode", K.MODES, ids=K.mode_id)
def test_unaligned(be, mode, size):
    K.case_unaligned(be, mode, size)


@pytest.mark.parametrize("size", [K.RESAMPLED[0], K.EQUAL], ids=str)
@pytest.mark.parametrize("mode", K.MODES, ids=K.mode_id)
def test_non_finite_prediction(be, mode, size):
    K.case_non_finite(be, mode, size)


def test_refusals(be):
    K.case_refusals(be)
