"""CPU tier: nemar_warp_resampled_bwd (csrc/register.hip) compiled for the host SIMT emulator (tests/emu) — against float64 with autograd,
against nemar_grid_sample_bwd at equal sizes, as the adjoint of the fused forward, repeatable, accumulating, off the 16-byte grid, with
non-finite predictions and at its refusals (tests/register_grad_cases.py); tests/test_register_grad_gpu.py runs the same bodies on the
gfx950 library."""
import pytest

import register_grad_cases as K
from backends import EmuBackend


@pytest.fixture(scope="module")
def be(emu_lib):
    return EmuBackend(emu_lib)


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
