"""`-m gpu`: the row-vector forms of max-pool backward, the 2x resize, the reflect fold (nemar_tune key 47; and the bias sums, which the switch leaves alone) on the gfx950
library — the bodies of tests/pointwise_rows_cases.py that tests/test_pointwise_rows_emu.py runs on the emulator."""
import pytest

import pointwise_rows_cases as K
from backends import HipBackend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(hip_lib):
    return HipBackend(hip_lib)


@pytest.mark.parametrize("size", K.RESIZE_SHAPES, ids=str)
def test_resize_up2(be, size):
    K.case_resize_up2(be, *size)


@pytest.mark.parametrize("with_addend", [False, True], ids=["plain", "addend"])
@pytest.mark.parametrize("size", K.POOL_SHAPES, ids=str)
def test_maxpool_bwd(be, size, with_addend):
    K.case_maxpool_bwd(be, *size, with_addend)


@pytest.mark.parametrize("shape", K.BIAS_SHAPES, ids=str)
def test_bias_sums(be, shape):
    K.case_bias_sums(be, *shape)


@pytest.mark.parametrize("with_addend", [False, True], ids=["plain", "addend"])
@pytest.mark.parametrize("route_size", K.FOLD_CASES, ids=str)
def test_fold(be, route_size, with_addend):
    route, size = route_size
    K.case_fold(be, route, *size, with_addend)


def test_fold_pad3_stays_general(be):
    K.case_fold_pad3(be)
