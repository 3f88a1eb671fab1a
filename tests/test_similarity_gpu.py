"""`-m gpu`: nemar_joint_histogram (csrc/similarity.hip) on the gfx950 library — the bodies of tests/similarity_cases.py that
tests/test_similarity_emu.py runs on the emulator, the one size at which a workgroup walks two tiles — and ops.joint_histogram on top."""
import numpy as np
import pytest
import torch

import similarity_cases as K
from backends import HipBackend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(hip_lib):
    return HipBackend(hip_lib)


@pytest.mark.parametrize("mode", [K.U, K.A])
@pytest.mark.parametrize("size", K.SIZES, ids=str)
def test_counts_and_moments_against_float64(be, size, mode):
    K.case_float64(be, size, mode, fade=True)


@pytest.mark.parametrize("bins", K.BINS)
@pytest.mark.parametrize("channels", K.CHANNELS, ids=str)
def test_channels_and_bins(be, channels, bins):
    K.case_float64(be, K.RAGGED, K.U, channels=channels, bins=bins, seed=6)


@pytest.mark.parametrize("mode", [K.U, K.A])
@pytest.mark.parametrize("size", K.THIN + [K.ONE_TEXEL_FIELD] + K.EDGES, ids=str)
def test_thin_outputs_one_texel_field_tile_edges(be, size, mode):
    K.case_float64(be, size, mode, seed=K.THIN_SEED[mode] if size in K.THIN else 4)


@pytest.mark.parametrize("mode", [K.U, K.A])
def test_field_leaves_the_source(be, mode):
    K.case_leaves_source(be, mode)


def test_two_tiles_per_workgroup(be):
    K.case_two_trips(be)


@pytest.mark.parametrize("mode,bins", [(K.U, 32), (K.A, 64)])
@pytest.mark.parametrize("size", [K.RAGGED, K.SIZES[5], K.SIZES[6]], ids=str)
def test_repeatable_optional_moments_unaligned_variants(be, size, mode, bins):
    K.case_bitwise(be, size, mode, bins=bins)


@pytest.mark.parametrize("bins", K.BINS)
def test_identity_gives_the_plain_histogram(be, bins):
    K.case_identity(be, bins=bins)


@pytest.mark.parametrize("mode", [K.U, K.A])
def test_mutual_information_ranks_the_prediction_above_the_identity(be, mode):
    K.case_ranking(be, mode=mode)


def test_refusals(be):
    K.case_refusals(be)


@pytest.mark.parametrize("mode", [K.U, K.A])
def test_ops_joint_histogram(be, mode):
    """the Python layer hands the kernel what the test bodies hand it: the same bits, with and without the moments; arguments are checked"""
    from nemar_amd import ops
    N, bins, size = 2, 16, K.RAGGED
    shape = K._shape(size, N, 3, 1)
    moving, fixed, pred = K.draw_pair(6, mode, shape)
    counts, mom = K.run_hist(be, be.dev(moving), be.dev(fixed), be.dev(pred), mode, shape, bins, (0.0, 1.0), (0.25, 0.75))
    t_m, t_f, t_pred = (torch.from_numpy(a).cuda() for a in (moving, fixed, pred))
    c1, m1 = ops.joint_histogram(t_pred, mode, t_m, t_f, bins, (0.0, 1.0), (0.25, 0.75))
    c2, none = ops.joint_histogram(t_pred, mode, t_m, t_f, bins, (0.0, 1.0), (0.25, 0.75), moments=False)
    assert none is None and c1.dtype == torch.int64 and c1.shape == (N, bins, bins) and m1.dtype == torch.float32 and m1.shape == (N, 6)
    assert c1.is_cuda and m1.is_cuda and torch.equal(c1, c2)
    assert np.array_equal(c1.cpu().numpy(), counts) and np.array_equal(m1.cpu().numpy().view(np.uint32), mom.view(np.uint32))
    c3, _ = ops.joint_histogram(t_pred, mode, t_m, t_f)                       # the defaults: 32 bins over [-1, 1]
    assert c3.shape == (N, 32, 32) and int(c3[:, :16].sum()) == 0 and int(c3.sum()) == int(c1.sum())
    summary = ops.similarity_summary(c1, m1)
    assert summary['valid'] == int(counts.sum()) and summary['mi'] >= 0 and -1 <= summary['ncc'] <= 1
    for bad in (dict(bins=1), dict(bins=65), dict(range_moving=(1.0, 1.0)), dict(range_fixed=(2.0, 1.0))):
        with pytest.raises(ValueError, match="joint_histogram"):
            ops.joint_histogram(t_pred, mode, t_m, t_f, **bad)
    with pytest.raises(ValueError, match="joint_histogram"):
        ops.joint_histogram(t_pred, K.GRID_EXPLICIT, t_m, t_f)
    with pytest.raises(ValueError, match="joint_histogram"):
        ops.joint_histogram(t_pred, mode, t_m[0], t_f)
    with pytest.raises(ValueError, match="joint_histogram"):
        ops.joint_histogram(t_pred, mode, t_m, t_f[:1])
