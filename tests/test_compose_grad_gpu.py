"""`-m gpu`: nemar_compose_pred_bwd (csrc/compose.hip) on the gfx950 library — the bodies of tests/compose_grad_cases.py that
tests/test_compose_grad_emu.py runs on the emulator."""
import pytest

import compose_grad_cases as K
from backends import HipBackend

pytestmark = pytest.mark.gpu

pairs = pytest.mark.parametrize("pair", K.MODE_PAIRS, ids=K.pair_id)


@pytest.fixture(scope="module")
def be(hip_lib):
    return HipBackend(hip_lib)


@pytest.mark.parametrize("hw", K.ALL_HW, ids=str)
@pairs
def test_against_float64(be, pair, hw):
    K.case_float64(be, *pair, hw)


@pairs
def test_against_float64_where_the_position_leaves_the_image(be, pair):
    K.case_float64(be, *pair, (35, 131), amp=1.5)


@pytest.mark.parametrize("hw", [(40, 56), (17, 65), (50, 1)], ids=str)
@pairs
def test_adjoint_towards_first(be, pair, hw):
    K.case_adjoint(be, *pair, hw)


def test_anchor_zero_second_field(be):
    K.case_anchor(be)


@pytest.mark.parametrize("hw", [(40, 56), (33, 129), (1, 77)], ids=str)
@pairs
def test_repeatable_overwritten_accumulated(be, pair, hw):
    K.case_repeat_accumulate(be, *pair, hw)


@pytest.mark.parametrize("hw", [(35, 131), (16, 64)], ids=str)
@pairs
def test_unaligned(be, pair, hw):
    K.case_unaligned(be, *pair, hw)


@pytest.mark.parametrize("hw", [(40, 56), (17, 65)], ids=str)
@pairs
def test_non_finite_positions(be, pair, hw):
    K.case_non_finite(be, *pair, hw)


def test_refusals(be):
    K.case_refusals(be)
