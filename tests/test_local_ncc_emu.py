"""CPU tier: nemar_local_ncc_fwd / _bwd (csrc/local_ncc.hip) compiled for the host SIMT emulator (tests/emu), against the float64
statement of their definition with autograd, at the tile edges, on planes smaller than the window, on flat windows and at their refusals
(tests/local_ncc_cases.py); tests/test_local_ncc_gpu.py runs the same bodies on the gfx950 library."""
import pytest

import local_ncc_cases as K
from backends import EmuBackend


@pytest.fixture(scope="module")
def be(emu_lib):
    return EmuBackend(emu_lib)


@pytest.mark.parametrize("win", K.WINS)
@pytest.mark.parametrize("size", K.SIZES, ids=str)
def test_against_float64(be, size, win):
    K.case_against_float64(be, size, win)


@pytest.mark.parametrize("win", [5, 7])
def test_the_other_window_sizes(be, win):
    K.case_against_float64(be, K.SIZES[0], win, seed=2)


def test_factor_and_gscale_scale_the_result(be):
    K.case_against_float64(be, K.SIZES[1], 9, factor=10.0, gscale=3.0)


@pytest.mark.parametrize("win", [3, 9])
@pytest.mark.parametrize("size", K.EDGES, ids=str)
def test_edges(be, size, win):
    K.case_against_float64(be, size, win)


def test_smaller_than_the_window(be):
    K.case_against_float64(be, K.SMALL, 9)


@pytest.mark.parametrize("win", [3, 9])
@pytest.mark.parametrize("size", K.THIN, ids=str)
def test_one_dimensional_planes(be, size, win):
    K.case_against_float64(be, size, win)


@pytest.mark.parametrize("win", [3, 9])
def test_flat_windows(be, win):
    K.case_against_float64(be, K.SIZES[0], win, flat=True)


def test_the_steps_channel_count(be):
    K.case_against_float64(be, K.SIZES[1], 9, N=1, C=3)


@pytest.mark.parametrize("win", [3, 9])
def test_symmetry(be, win):
    K.case_symmetry(be, K.SIZES[0], win)


@pytest.mark.parametrize("win", [3, 9])
def test_shift_invariance(be, win):
    K.case_shift_invariance(be, K.SIZES[0], win)


@pytest.mark.parametrize("win", [3, 11])
@pytest.mark.parametrize("size", [K.SIZES[0], (17, 65)], ids=str)
def test_repeatable_accumulated_optional_outputs(be, size, win):
    K.case_repeatable_accumulate_optional(be, size, win)


def test_nonfinite_input(be):
    K.case_nonfinite(be)


def test_refusals(be):
    K.case_refusals(be)
