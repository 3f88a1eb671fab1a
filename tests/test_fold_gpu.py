"""`-m gpu`: nemar_fold_penalty_fwd / _bwd (csrc/fold.hip) on the gfx950 library — the bodies of tests/fold_cases.py that
tests/test_fold_emu.py runs on the emulator, and the network's own size (256 x 256: 64 tiles per sample)."""
import pytest

import fold_cases as K
from backends import HipBackend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(hip_lib):
    return HipBackend(hip_lib)


@pytest.mark.parametrize("margin", [0.0, 0.5])
@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("amp", [0.15, 1.0])
@pytest.mark.parametrize("size", K.SIZES + [K.NETWORK], ids=str)
def test_against_float64(be, size, amp, seed, margin):
    K.case_against_float64(be, size, amp, seed, margin)


def test_factor_and_gscale_scale_the_result(be):
    K.case_against_float64(be, K.SIZES[0], 1.0, 1, 0.5, factor=0.5, gscale=3.0)


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("size", K.SIZES + [K.NETWORK], ids=str)
def test_agrees_with_jacobian_stats(be, size, seed):
    K.case_agrees_with_jacobian_stats(be, size, seed)


@pytest.mark.parametrize("margin", [0.0, 0.5])
@pytest.mark.parametrize("size", K.EDGES, ids=str)
def test_edges(be, size, margin):
    K.case_against_float64(be, size, 1.0, 1, margin)


@pytest.mark.parametrize("size", K.THIN, ids=str)
def test_no_interior_pixel(be, size):
    K.case_thin(be, size)


@pytest.mark.parametrize("margin", [0.0, 0.5])
@pytest.mark.parametrize("size", [K.SIZES[0], (9, 13), (17, 65), K.NETWORK], ids=str)
def test_repeatable_overwritten_unaligned_accumulated(be, size, margin):
    K.case_repeatable_unaligned_accumulate(be, size, margin)


def test_refusals(be):
    K.case_refusals(be)
