"""CPU tier of tests/warp_limit_cases.py: nemar_grid_sample_bwd with a workspace — the tight bound of its contract, power-of-two
equivariance, heterogeneous magnitudes, collapse and large linear maps, fields with jumps, non-finite data — on the host SIMT emulator,
every buffer guard-banded (tests/backends.py).  tests/test_warp_limits_gpu.py runs the same on the gfx950 library."""
import pytest

import warp_limit_cases as WL
from backends import EmuBackend


@pytest.fixture(scope="module")
def be(emu_lib):
    return EmuBackend(emu_lib)


@pytest.mark.parametrize("H,W", WL.HW)
@pytest.mark.parametrize("field", ["noise", "smooth"])
@pytest.mark.parametrize("mode", WL.MODES)
def test_bound_and_power_of_two_equivariance(be, mode, field, H, W):
    WL.case_equivariance(be, mode, field, H, W)


@pytest.mark.parametrize("H,W", WL.HW_3COL)
@pytest.mark.parametrize("which", WL.HETEROGENEOUS)
def test_heterogeneous_magnitudes(be, which, H, W):
    for mode in (WL.GRID_UNET, WL.GRID_EXPLICIT):
        WL.case_heterogeneous(be, which, mode, H, W)


@pytest.mark.parametrize("H,W", WL.HW)
@pytest.mark.parametrize("which", ["collapse", "collapse_unet", "rot180", "zoom2", "zoom05", "shear"])
def test_collapse_and_linear_maps(be, which, H, W):
    WL.case_linear(be, which, H, W)


def test_quarter_turn_on_a_square_plane(be):
    WL.case_linear(be, "rot90", 48, 48)


@pytest.mark.parametrize("H,W", WL.HW)
@pytest.mark.parametrize("where", WL.JUMPS)
def test_fields_with_jumps(be, where, H, W):
    for mode in (WL.GRID_UNET, WL.GRID_EXPLICIT):
        WL.case_jumps(be, where, mode, H, W)


@pytest.mark.parametrize("mode", [WL.GRID_UNET, WL.GRID_EXPLICIT])
@pytest.mark.parametrize("inf_is_far", [False, True])
def test_nonfinite_gout_leaves_the_workspace_clean(be, inf_is_far, mode):
    WL.case_nonfinite_gout(be, inf_is_far, mode)


def test_nonfinite_offsets_leave_the_workspace_clean(be):
    WL.case_nonfinite_offsets(be)
