"""CPU tier: nemar_label_overlap and nemar_map_points (csrc/score.hip) compiled for the host SIMT emulator (tests/emu), against the
library's own nearest warp integer for integer and against float64 (tests/score_cases.py); tests/test_score_gpu.py runs the same bodies
on the gfx950 library."""
import pytest

import score_cases as S
from backends import EmuBackend

MODES = [S.GRID_UNET, S.GRID_AFFINE]


@pytest.fixture(scope="module")
def be(emu_lib):
    return EmuBackend(emu_lib)


def _n(size):
    return 1 if size[1][0] > 200 else 2


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", S.ALL_SIZES + S.THIN + [S.ONE_TEXEL_FIELD], ids=str)
def test_exact_against_the_librarys_warp(be, size, mode):
    S.case_exact(be, size, mode, N=_n(size))


@pytest.mark.parametrize("mode", MODES)
def test_exact_where_the_field_leaves_the_source(be, mode):
    S.case_exact(be, S.LEAVES_SOURCE, mode, amp=1.5)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", S.ALL_SIZES, ids=str)
def test_against_float64(be, size, mode):
    S.case_float64(be, size, mode, N=_n(size))


@pytest.mark.parametrize("K", [1, 5, 64, 1024])
@pytest.mark.parametrize("kind", S.KINDS)
def test_label_content(be, kind, K):
    S.case_content(be, kind, K)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind,K", [("random", 5), ("blocky", 64), ("single", 1024)])
def test_values_of_no_class_are_ignored(be, kind, K, mode):
    S.case_content(be, kind, K, mode, junk=True)


def test_identity(be):
    S.case_identity(be)
    S.case_identity(be, hw=(16, 64), K=1, N=1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size,N", [(S.UPSAMPLING[0], 1), (S.UPSAMPLING[3], 3), (S.EQUAL, 3), (S.DOWN, 1)], ids=str)
def test_repeatable_overwritten_unaligned(be, size, N, mode):
    S.case_repeatable_unaligned(be, size, mode, N=N)


def test_refusals(be):
    S.case_refusals(be)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", [S.UPSAMPLING[0], S.UPSAMPLING[4], S.EQUAL, S.DOWN, S.ONE_TEXEL_FIELD, S.THIN[0], S.THIN[1]], ids=str)
def test_points_agree_with_the_grid(be, size, mode):
    S.case_points(be, size, mode)


@pytest.mark.parametrize("mode", MODES)
def test_points_missing_annotations_and_counts(be, mode):
    S.case_points_edges(be, mode)
