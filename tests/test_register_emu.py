"""CPU tier: nemar_warp_resampled_fwd (csrc/register.hip) compiled for the host SIMT emulator (tests/emu), against the composed
nemar_bilinear_fwd + nemar_grid_sample_fwd path bit for bit and against torch's float64 on the CPU (tests/register_cases.py);
tests/test_register_gpu.py runs the same bodies on the gfx950 library."""
import pytest

import register_cases as R
from backends import EmuBackend


@pytest.fixture(scope="module")
def be(emu_lib):
    return EmuBackend(emu_lib)


@pytest.mark.parametrize("size", R.ALL_SIZES, ids=str)
def test_bitwise_against_composed_unet(be, size):
    R.case_bitwise(be, size, R.GRID_UNET, N=1 if size[1][0] > 200 else 2)


@pytest.mark.parametrize("size", R.ALL_SIZES, ids=str)
def test_bitwise_against_composed_affine(be, size):
    R.case_bitwise(be, size, R.GRID_AFFINE, N=1 if size[1][0] > 200 else 2)


@pytest.mark.parametrize("mode", [R.GRID_UNET, R.GRID_AFFINE])
@pytest.mark.parametrize("size", R.ALL_SIZES, ids=str)
def test_bilinear_against_float64(be, size, mode):
    R.case_bilinear(be, size, mode, N=1 if size[1][0] > 200 else 2)


@pytest.mark.parametrize("mode", [R.GRID_UNET, R.GRID_AFFINE])
@pytest.mark.parametrize("size", R.ALL_SIZES, ids=str)
def test_nearest_against_float64(be, size, mode):
    R.case_nearest(be, size, mode, N=1 if size[1][0] > 200 else 2)


def test_nearest_keeps_labels(be):
    R.case_nearest(be, R.UPSAMPLING[0], R.GRID_UNET, labels=True)
    R.case_nearest(be, R.UPSAMPLING[3], R.GRID_AFFINE, labels=True)


@pytest.mark.parametrize("size", [R.UPSAMPLING[0], R.UPSAMPLING[3], R.EQUAL, R.DOWN, ((12, 16), (48, 64), None, 3)], ids=str)
def test_unaligned_views_and_odd_widths(be, size):
    R.case_unaligned(be, size)


@pytest.mark.parametrize("size,amp", [(((8, 12), (1, 77), (9, 13), 2), 0.15), (((8, 12), (50, 1), (9, 13), 2), 0.15),
                                      (((1, 1), (20, 36), None, 1), 0.15), (((16, 24), (67, 45), (30, 41), 3), 1.5),
                                      (((24, 24), (96, 96), None, 3), 1.5), (((64, 64), (24, 40), (50, 70), 3), 1.5)], ids=str)
def test_edges_and_zero_padding(be, size, amp):
    R.case_edges(be, size, R.GRID_UNET, amp=amp)


def test_edges_affine(be):
    R.case_edges(be, ((1, 1), (1, 45), (9, 13), 2), R.GRID_AFFINE)
    R.case_edges(be, ((1, 1), (67, 45), (30, 41), 3), R.GRID_AFFINE, amp=1.5)


@pytest.mark.parametrize("mode", [R.GRID_UNET, R.GRID_AFFINE])
@pytest.mark.parametrize("size", [R.UPSAMPLING[1], R.UPSAMPLING[3], R.EQUAL, R.DOWN, ((12, 16), (50, 68), (31, 47), 2)], ids=str)
def test_vector_route_of_the_measurement_build(be, size, mode):
    R.case_vector_route(be, size, mode)


def test_repeatable(be):
    R.case_repeatable(be)


def test_refusals(be):
    R.case_refusals(be)
