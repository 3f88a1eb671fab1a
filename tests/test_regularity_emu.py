"""CPU tier: nemar_jacobian_stats (csrc/regularity.hip) compiled for the host SIMT emulator (tests/emu), against the float64 statement
of its definition, against closed forms, against its own map and against the registration-error meter (tests/regularity_cases.py), and
the host-side ops.regularity_summary; tests/test_regularity_gpu.py runs the same bodies on the gfx950 library."""
import pytest

import regularity_cases as K
from backends import EmuBackend


@pytest.fixture(scope="module")
def be(emu_lib):
    return EmuBackend(emu_lib)


@pytest.mark.parametrize("amp", [0.15, 1.0])
@pytest.mark.parametrize("mode", [K.U, K.A])
@pytest.mark.parametrize("size", K.SIZES, ids=str)
def test_map_against_float64(be, size, mode, amp):
    K.case_map(be, size, mode, amp)


@pytest.mark.parametrize("amp", [0.15, 1.5])
@pytest.mark.parametrize("size", [K.RAGGED, K.ONE_TEXEL], ids=str)
def test_affine_closed_form(be, size, amp):
    K.case_affine_closed_form(be, size, amp)


@pytest.mark.parametrize("size", [K.ONE_TEXEL, K.RAGGED, K.EQUAL], ids=str)
def test_zero_field_closed_form(be, size):
    K.case_zero_field_closed_form(be, size)


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("size", K.FOLDING, ids=str)
def test_statistics_reduce_the_map_and_folds_match_float64(be, size, seed):
    K.case_statistics(be, size, seed=seed)


def test_agrees_with_the_registration_error_meter(be):
    K.case_agrees_with_meter(be)


@pytest.mark.parametrize("mode", [K.U, K.A])
@pytest.mark.parametrize("size", K.THIN, ids=str)
def test_no_interior_pixel(be, size, mode):
    K.case_thin(be, size, mode)


@pytest.mark.parametrize("mode", [K.U, K.A])
@pytest.mark.parametrize("size", K.EDGES, ids=str)
def test_edges(be, size, mode):
    K.case_edges(be, size, mode)


@pytest.mark.parametrize("mode", [K.U, K.A])
@pytest.mark.parametrize("size", [K.RAGGED, ((9, 13), (9, 13)), K.DOWN], ids=str)
def test_repeatable_overwritten_unaligned_optional_map(be, size, mode):
    K.case_repeatable_unaligned(be, size, mode)


def test_refusals(be):
    K.case_refusals(be)


def test_regularity_summary():
    K.case_summary()
