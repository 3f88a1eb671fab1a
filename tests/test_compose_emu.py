"""CPU tier: nemar_compose_pred (csrc/compose.hip) compiled for the host SIMT emulator (tests/emu), against float64, against the
library's own warp bit for bit and against two warps in sequence (tests/compose_cases.py); tests/test_compose_gpu.py runs the same bodies
on the gfx950 library."""
import pytest

import compose_cases as K
from backends import EmuBackend


@pytest.fixture(scope="module")
def be(emu_lib):
    return EmuBackend(emu_lib)


@pytest.mark.parametrize("m1,m2", K.MODE_PAIRS)
@pytest.mark.parametrize("size", K.SIZES, ids=str)
def test_against_float64(be, size, m1, m2):
    K.case_float64(be, size, m1, m2)


@pytest.mark.parametrize("m1,m2", K.MODE_PAIRS)
def test_against_float64_where_the_position_leaves_the_image(be, m1, m2):
    K.case_float64(be, K.RAGGED, m1, m2, amp=1.5)


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("m1,m2", K.MODE_PAIRS)
@pytest.mark.parametrize("size", [K.RAGGED, K.EQUAL, K.DOWN, K.THIN[0]], ids=str)
def test_fused_warp_is_the_librarys_warp(be, size, m1, m2, C):
    K.case_fused_warp(be, size, m1, m2, C)


def test_fused_warp_where_the_position_leaves_the_image(be):
    K.case_fused_warp(be, K.RAGGED, K.U, K.U, 3, amp=1.5)


@pytest.mark.parametrize("m1,m2", K.MODE_PAIRS)
def test_composition_is_sequential_warping(be, m1, m2):
    K.case_sequential(be, m1, m2)


@pytest.mark.parametrize("size", [K.RAGGED, K.EQUAL, K.THIN[1]], ids=str)
def test_affine_closed_form(be, size):
    K.case_affine_closed_form(be, size)


@pytest.mark.parametrize("m1,m2", K.MODE_PAIRS)
@pytest.mark.parametrize("size", [K.RAGGED, ((9, 13), (9, 13), (9, 13)), K.DOWN], ids=str)
def test_repeatable_overwritten_unaligned(be, size, m1, m2):
    K.case_repeatable_unaligned(be, size, m1, m2)


def test_refusals(be):
    K.case_refusals(be)
