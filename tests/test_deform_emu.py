"""CPU tier: the known-misalignment kernels (csrc/deform.hip) compiled for the host SIMT emulator (tests/emu), against the float64 numpy
restatements of tests/deform_cases.py; tests/test_deform_gpu.py runs the same bodies on the gfx950 library."""
import pytest

import deform_cases as D
from backends import EmuBackend


@pytest.fixture(scope="module")
def be(emu_lib):
    return EmuBackend(emu_lib)


@pytest.mark.parametrize("shape", [(5, 7), (31, 47), (64, 64)])
@pytest.mark.parametrize("parts", ["affine", "lattice", "both"])
def test_field(be, shape, parts):
    g = 0 if parts == "affine" else 6
    D.case_field(be, *shape, g, g, affine=parts != "lattice", lattice=parts != "affine")


def test_field_rectangular_lattice_and_identities(be):
    D.case_field(be, 12, 20, 4, 7)
    for shape in ((5, 7), (16, 24)):
        D.case_field_identities(be, *shape, 0, 0)
        D.case_field_identities(be, *shape, 5, 4)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("geom", [(20, 28, 16, 24, 0.3), (20, 28, 16, 24, 1.5), (9, 11, 5, 7, 0.5), (16, 16, 16, 16, 1.5)])
def test_sample(be, C, geom):
    D.case_sample(be, C, *geom)


def test_sample_unaligned_field_takes_the_scalar_route(be):
    D.case_sample(be, 3, 20, 28, 16, 24, 0.4, unaligned=True)


@pytest.mark.parametrize("mode", [D.GRID_UNET, D.GRID_AFFINE])
@pytest.mark.parametrize("shape,kind", [((31, 47), "smooth"), ((32, 48), "smooth"), ((12, 16), "fold"), ((9, 7), "fold")])
def test_meter(be, mode, shape, kind):
    D.case_meter(be, mode, 2, *shape, kind=kind)


def test_meter_closed_forms(be):
    D.case_meter_identity(be, 16, 32)
    D.case_meter_inverse_translation(be, 24, 40)
    D.case_meter_inverse_translation(be, 17, 23, shift=(-1.5, 4.5))


def test_repeatable(be):
    D.case_repeatable(be)


def test_refusals(be):
    D.case_refusals(be)
