"""CPU tier: the BatchNorm kernels (csrc/batchnorm.hip) compiled for the host SIMT emulator (tests/emu), against float64 numpy
(tests/bn_cases.py); tests/test_batchnorm_gpu.py runs the same bodies on the gfx950 library."""
import pytest

import bn_cases as B
from backends import EmuBackend


@pytest.fixture(scope="module")
def be(emu_lib):
    return EmuBackend(emu_lib)


@pytest.mark.parametrize("act", [B.ACT_NONE, B.ACT_RELU, B.ACT_LRELU])
@pytest.mark.parametrize("residual", [False, True])
def test_train_forward_backward(be, act, residual):
    B.case_batchnorm_train(be, N=4, C=3, H=5, W=7, S=1, act=act, residual=residual)        # odd map: scalar route


@pytest.mark.parametrize("shape", [(2, 3, 1, 2, 1), (2, 4, 2, 2, 2), (6, 2, 4, 8, 3), (2, 2, 31, 31, 1), (2, 2, 35, 47, 2),
                                   (2, 2, 64, 64, 1)])
def test_train_maps_and_segments(be, shape):
    N, C, H, W, S = shape
    B.case_batchnorm_train(be, N, C, H, W, S, B.ACT_LRELU)


@pytest.mark.parametrize("act", [B.ACT_NONE, B.ACT_RELU, B.ACT_LRELU])
def test_eval(be, act):
    B.case_batchnorm_eval(be, N=3, C=4, H=6, W=8, act=act, residual=act == B.ACT_NONE)
    B.case_batchnorm_eval(be, N=2, C=3, H=5, W=5, act=act)


def test_segments_equal_separate_calls(be):
    B.case_batchnorm_segments(be)
    B.case_batchnorm_segments(be, N=4, C=3, H=8, W=8, S=2, act=B.ACT_RELU)


def test_dropout_max_words_and_repeat(be):
    B.case_batchnorm_dropout_and_max(be)


def test_single_value_per_channel_refused(be):
    B.case_batchnorm_single_value(be)
