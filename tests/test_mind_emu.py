"""CPU tier: nemar_mind_loss_fwd / _bwd (csrc/mind.hip) compiled for the host SIMT emulator (tests/emu), against the float64 statement
of their definition with autograd, at the tile edges, on planes smaller than the patch, on flat patches, on unaligned rows and at their
refusals (tests/mind_cases.py); tests/test_mind_gpu.py runs the same bodies on the gfx950 library."""
import pytest

import mind_cases as K
from backends import EmuBackend

TWO = [(3, 1), (5, 2)]


@pytest.fixture(scope="module")
def be(emu_lib):
    return EmuBackend(emu_lib)


@pytest.mark.parametrize("patch,dil", K.CONFIGS)
@pytest.mark.parametrize("size", K.SIZES, ids=str)
def test_against_float64(be, size, patch, dil):
    K.case_against_float64(be, size, patch, dil)


def test_factor_and_gscale_scale_the_result(be):
    K.case_against_float64(be, K.SIZES[1], 3, 2, factor=10.0, gscale=3.0)


@pytest.mark.parametrize("patch,dil", TWO)
@pytest.mark.parametrize("size", K.EDGES, ids=str)
def test_edges(be, size, patch, dil):
    K.case_against_float64(be, size, patch, dil)


@pytest.mark.parametrize("patch,dil", [(3, 2), (5, 2)])
@pytest.mark.parametrize("size", K.SMALL, ids=str)
def test_smaller_than_the_patch(be, size, patch, dil):
    K.case_against_float64(be, size, patch, dil)


@pytest.mark.parametrize("patch,dil", TWO)
@pytest.mark.parametrize("size", K.THIN, ids=str)
def test_one_dimensional_planes(be, size, patch, dil):
    K.case_against_float64(be, size, patch, dil)


@pytest.mark.parametrize("patch,dil", K.CONFIGS)
def test_flat_patches(be, patch, dil):
    K.case_against_float64(be, K.SIZES[0], patch, dil, flat=True)


@pytest.mark.parametrize("patch,dil", [(3, 2), (5, 2)])
@pytest.mark.parametrize("size", [K.SIZES[1], (17, 40)], ids=str)
def test_base_pointers_one_float_past_alignment(be, size, patch, dil):
    K.case_against_float64(be, size, patch, dil, off=1)


@pytest.mark.parametrize("patch,dil", TWO)
def test_symmetry(be, patch, dil):
    K.case_symmetry(be, K.SIZES[0], patch, dil)


@pytest.mark.parametrize("patch,dil", TWO)
def test_shift_invariance(be, patch, dil):
    K.case_shift_invariance(be, K.SIZES[0], patch, dil)


@pytest.mark.parametrize("patch,dil", [(3, 2), (5, 1)])
def test_channels(be, patch, dil):
    K.case_channels(be, K.SIZES[1], patch, dil)


@pytest.mark.parametrize("patch,dil", TWO)
@pytest.mark.parametrize("size", [K.SIZES[0], (17, 64)], ids=str)
def test_repeatable_accumulated_optional_outputs(be, size, patch, dil):
    K.case_repeatable_accumulate_optional(be, size, patch, dil)


@pytest.mark.parametrize("patch,dil", TWO)
def test_nonfinite_input(be, patch, dil):
    K.case_nonfinite(be, patch, dil)


def test_refusals(be):
    K.case_refusals(be)
