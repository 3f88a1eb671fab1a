"""CPU tier: nemar_surface_distance (csrc/surface.hip) compiled for the host SIMT emulator (tests/emu), integer for integer against the
numpy truth of tests/surface_cases.py over the library's own nearest warp; that truth itself against scipy.ndimage.
tests/test_surface_gpu.py runs the same bodies on the gfx950 library."""
import pytest

import surface_cases as S
from backends import EmuBackend

MODES = [S.GRID_UNET, S.GRID_AFFINE]
# per-pixel random maps are nearly all boundary: a smaller plane (67 x 45: five tile rows, a ragged tile column) keeps the brute-force truth quick
SIZE_OF = {"blocky": S.CONTENT_SIZE, "single": S.CONTENT_SIZE, "random": S.UPSAMPLING[3]}


@pytest.fixture(scope="module")
def be(emu_lib):
    return EmuBackend(emu_lib)


def test_the_truth_agrees_with_scipy():
    S.check_truth_against_scipy()


@pytest.mark.parametrize("route", S.ROUTES, ids=lambda r: r[0])
@pytest.mark.parametrize("hw", S.TILE_EDGES, ids=str)
def test_exact_where_the_tiles_end(be, hw, route):
    _, mode, field = route
    S.case_route(be, S.edge_size(hw, field), mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", [S.UPSAMPLING[0], S.EQUAL, S.DOWN, S.ONE_TEXEL_FIELD], ids=str)
def test_exact_on_every_route(be, size, mode):
    S.case_route(be, size, mode)


@pytest.mark.parametrize("mode", MODES)
def test_exact_where_the_field_leaves_the_source(be, mode):
    S.case_route(be, S.LEAVES_SOURCE, mode, amp=1.5)


@pytest.mark.parametrize("kind,K", [("blocky", 5), ("blocky", 64), ("random", 5), ("single", 1), ("single", 1024)])
def test_label_content(be, kind, K):
    S.case_content(be, kind, K, size=SIZE_OF[kind])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind,K", [("random", 5), ("blocky", 64)])
def test_values_of_no_class_are_never_boundary(be, kind, K, mode):
    S.case_content(be, kind, K, mode, size=SIZE_OF[kind], junk=True)


def test_special_classes(be):
    S.case_special(be)


def test_analytic_rectangles_and_a_map_against_itself(be):
    S.case_analytic(be)


def test_far_tail(be):
    S.case_far(be)


@pytest.mark.parametrize("mode", MODES)
def test_samples_do_not_leak(be, mode):
    S.case_samples(be, mode)


def test_classes_in_several_chunks(be):
    S.case_chunks(be)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size,N", [(S.UPSAMPLING[3], 3), (S.EQUAL, 1), (S.DOWN, 2)], ids=str)
def test_repeatable_overwritten_unaligned(be, size, N, mode):
    S.case_repeatable_unaligned(be, size, mode, N=N)


def test_refusals(be):
    S.case_refusals(be)
