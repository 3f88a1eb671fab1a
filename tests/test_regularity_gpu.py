"""`-m gpu`: nemar_jacobian_stats (csrc/regularity.hip) on the gfx950 library — the bodies of tests/regularity_cases.py that
tests/test_regularity_emu.py runs on the emulator, and the network's own size (256 x 256: 64 tiles per sample, one merge step per lane)
— and ops.jacobian_stats on top of it."""
import numpy as np
import pytest
import torch

import regularity_cases as K
from backends import HipBackend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(hip_lib):
    return HipBackend(hip_lib)


@pytest.mark.parametrize("amp", [0.15, 1.0])
@pytest.mark.parametrize("mode", [K.U, K.A])
@pytest.mark.parametrize("size", K.SIZES + [K.NETWORK], ids=str)
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
@pytest.mark.parametrize("size", K.FOLDING + [K.NETWORK], ids=str)
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
@pytest.mark.parametrize("size", [K.RAGGED, ((9, 13), (9, 13)), K.DOWN, K.NETWORK], ids=str)
def test_repeatable_overwritten_unaligned_optional_map(be, size, mode):
    K.case_repeatable_unaligned(be, size, mode, N=8 if size is K.NETWORK else 2)


def test_refusals(be):
    K.case_refusals(be)


@pytest.mark.parametrize("mode", [K.U, K.A])
def test_ops_jacobian_stats(be, mode):
    """the Python layer hands the kernel what the test bodies hand it: the same bits, with and without the map; shapes are checked"""
    from nemar_amd import ops
    N, size = 2, K.RAGGED
    (hf, wf), (Ho, Wo) = size
    _, pred = K.draw(6, mode, N, 1, hf, wf, 1, 1, 1.0)
    det, counts, stats = K.run_jac(be, be.dev(pred), mode, size, N)
    t_pred = torch.from_numpy(pred).cuda()
    c1, s1, none = ops.jacobian_stats(t_pred, mode, (Ho, Wo))
    c2, s2, d2 = ops.jacobian_stats(t_pred, mode, (Ho, Wo), det_map=True)
    assert none is None and c1.dtype == torch.int64 and c1.shape == (N, 2) and s1.dtype == torch.float32 and s1.shape == (N, 5)
    assert c1.is_cuda and s1.is_cuda and d2.is_cuda and d2.shape == (N, Ho, Wo) and d2.dtype == torch.float32
    assert torch.equal(c1, c2) and np.array_equal(s1.cpu().numpy().view(np.uint32), s2.cpu().numpy().view(np.uint32))
    assert np.array_equal(c1.cpu().numpy(), counts.astype(np.int64))
    assert np.array_equal(s1.cpu().numpy().view(np.uint32), stats.view(np.uint32))
    assert np.array_equal(d2.cpu().numpy().view(np.uint32), det.view(np.uint32))
    summary = ops.regularity_summary(c1, s1)
    assert summary['interior'] == N * (Ho - 1) * (Wo - 1) and summary['folds'] == int(counts[:, 1].sum())
    with pytest.raises(ValueError, match="jacobian_stats"):
        ops.jacobian_stats(t_pred, K.GRID_EXPLICIT, (Ho, Wo))
    with pytest.raises(ValueError, match="jacobian_stats"):
        ops.jacobian_stats(t_pred[:, :1] if mode == K.U else t_pred[:, :5], mode, (Ho, Wo))
