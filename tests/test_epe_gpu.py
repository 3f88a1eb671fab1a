"""`-m gpu`: nemar_epe_loss_fwd / _bwd (csrc/epe.hip) on the gfx950 library — the bodies of tests/epe_cases.py that tests/test_epe_emu.py
runs on the emulator, the descent through ops.epe_loss, and sizes at which the launch's workgroup cap makes the grid-stride loop run
twice."""
import numpy as np
import pytest
import torch

import epe_cases as K
from backends import HipBackend
from register_cases import GRID_AFFINE, GRID_UNET

pytestmark = pytest.mark.gpu

MODES = [GRID_UNET, GRID_AFFINE]
mode_id = lambda m: "unet" if m == GRID_UNET else "affine"


@pytest.fixture(scope="module")
def be(hip_lib):
    return HipBackend(hip_lib)


@pytest.mark.parametrize("eps", [0.01, 0.5])
@pytest.mark.parametrize("kind", ["smooth", "fold"])
@pytest.mark.parametrize("size", K.ONE_PIXEL + K.FOUR_PIXEL, ids=str)
@pytest.mark.parametrize("mode", MODES, ids=mode_id)
def test_against_float64(be, mode, size, kind, eps):
    K.case_against_float64(be, mode, size, kind, eps)


@pytest.mark.parametrize("size", [K.ONE_PIXEL[0], K.FOUR_PIXEL[0]], ids=str)
@pytest.mark.parametrize("mode", MODES, ids=mode_id)
def test_rough_field_the_cell_choice_matters(be, mode, size):
    K.case_against_float64(be, mode, size, 'rough', 0.01)


@pytest.mark.parametrize("size", [K.ONE_PIXEL[0], K.FOUR_PIXEL[0]], ids=str)
@pytest.mark.parametrize("mode", MODES, ids=mode_id)
def test_leaving_the_image(be, mode, size):
    K.case_leaving(be, mode, size)


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("size", K.EDGES, ids=str)
@pytest.mark.parametrize("mode", MODES, ids=mode_id)
def test_edges(be, mode, size, N):
    K.case_against_float64(be, mode, size, 'smooth', 0.01, N=N)


@pytest.mark.parametrize("eps", [0.01, 0.5])
@pytest.mark.parametrize("size", [(16, 32), (64, 64)], ids=str)
def test_zero_residual_is_eps_with_a_zero_gradient(be, size, eps):
    K.case_zero_residual(be, size, eps)


@pytest.mark.parametrize("size", [(16, 32), (64, 64)], ids=str)
def test_constant_translation_in_closed_form(be, size):
    K.case_translation(be, size)


@pytest.mark.parametrize("mode,size", K.DESCENT, ids=lambda v: mode_id(v) if isinstance(v, int) else str(v))
def test_descent_on_the_prediction_through_ops(hip_lib, mode, size):
    from nemar_amd import ops

    def loss_and_grad(p, g, eps=0.01):
        d = torch.from_numpy(p).cuda().requires_grad_(True)
        loss = ops.epe_loss(d, mode, torch.from_numpy(g).cuda(), eps)
        loss.backward()
        return float(loss.detach()), d.grad.cpu().numpy()
    K.case_descent(mode, size, loss_and_grad)


@pytest.mark.parametrize("size", [K.ONE_PIXEL[0], K.FOUR_PIXEL[0], (9, 13)], ids=str)
@pytest.mark.parametrize("mode", MODES, ids=mode_id)
def test_repeatable_overwritten_unaligned_accumulated(be, mode, size):
    K.case_repeatable_unaligned_accumulate(be, mode, size)


@pytest.mark.parametrize("shape", K.GRID_STRIDE, ids=str)
def test_grid_stride_loop_runs_more_than_once(be, shape):
    K.case_grid_stride(be, *shape)


def test_refusals(be):
    K.case_refusals(be)


@pytest.mark.parametrize("size", [K.ONE_PIXEL[1], K.FOUR_PIXEL[0]], ids=str)
@pytest.mark.parametrize("mode", MODES, ids=mode_id)
def test_non_finite_input(be, mode, size):
    K.case_non_finite(be, mode, size)
