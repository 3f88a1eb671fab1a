"""CPU tier: nemar_svf_step_fwd / _bwd (csrc/integrate.hip) compiled for the host SIMT emulator (tests/emu), against the float64 statement
of their definition with autograd, at the tile edges, at their limits and refusals, and as the chain of K steps that integrates a velocity
field (tests/integrate_cases.py); tests/test_integrate_gpu.py runs the same bodies on the gfx950 library."""
import pytest

import integrate_cases as K
from backends import EmuBackend


@pytest.fixture(scope="module")
def be(emu_lib):
    return EmuBackend(emu_lib)


@pytest.mark.parametrize("amp", K.AMPS)
@pytest.mark.parametrize("size", K.SIZES + K.EDGES + K.THIN, ids=str)
def test_step_forward_against_float64(be, size, amp):
    K.case_step_fwd(be, size, amp)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("amp", K.AMPS)
@pytest.mark.parametrize("size", K.SIZES, ids=str)
def test_step_backward_against_float64(be, size, amp, seed):
    K.case_step_bwd(be, size, amp, seed)


@pytest.mark.parametrize("size", K.EDGES + K.THIN, ids=str)
def test_step_backward_at_the_edges(be, size):
    K.case_step_bwd(be, size, 1.0)


@pytest.mark.parametrize("size", [K.SIZES[0], (9, 13), (17, 65)], ids=str)
def test_bits(be, size):
    K.case_bits(be, size)


def test_bounds(be):
    K.case_bounds(be)


def test_refusals(be):
    K.case_refusals(be)


@pytest.mark.parametrize("steps", [0, 1, 4, 6])
@pytest.mark.parametrize("size", [K.SIZES[0], K.SIZES[2]], ids=str)
def test_chain_forward_against_float64(be, size, steps):
    K.case_chain_fwd(be, size, steps)


@pytest.mark.parametrize("seed", [1, 3])
def test_the_integrated_field_has_no_folds(be, seed):
    K.case_no_folds(be, K.SIZES[2], seed)


def test_inverse(be):
    K.case_inverse(be, K.SIZES[2])
