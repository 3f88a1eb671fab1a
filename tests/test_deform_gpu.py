"""`-m gpu`: the known-misalignment kernels (csrc/deform.hip) on the gfx950 library — the bodies of tests/deform_cases.py that
tests/test_deform_emu.py runs on the emulator, at larger shapes too."""
import pytest

import deform_cases as D
from backends import HipBackend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(hip_lib):
    return HipBackend(hip_lib)


@pytest.mark.parametrize("shape", [(5, 7), (31, 47), (64, 64), (256, 256)])
@pytest.mark.parametrize("parts", ["affine", "lattice", "both"])
def test_field(be, shape, parts):
    g = 0 if parts == "affine" else 6
    D.case_field(be, *shape, g, g, affine=parts != "lattice", lattice=parts != "affine", B=4)


def test_field_rectangular_lattice_and_identities(be):
    D.case_field(be, 12, 20, 4, 7)
    D.case_field(be, 96, 160, 9, 5)
    for shape in ((5, 7), (16, 24), (256, 256)):
        D.case_field_identities(be, *shape, 0, 0)
        D.case_field_identities(be, *shape, 5, 4)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("geom", [(20, 28, 16, 24, 0.3), (20, 28, 16, 24, 1.5), (9, 11, 5, 7, 0.5), (16, 16, 16, 16, 1.5),
                                  (140, 150, 128, 128, 0.1), (286, 286, 256, 256, 1.5)])
def test_sample(be, C, geom):
    D.case_sample(be, C, *geom)


def test_sample_unaligned_field_takes_the_scalar_route(be):
    D.case_sample(be, 3, 20, 28, 16, 24, 0.4, unaligned=True)
    D.case_sample(be, 3, 140, 150, 128, 128, 0.2, unaligned=True)


@pytest.mark.parametrize("mode", [D.GRID_UNET, D.GRID_AFFINE])
@pytest.mark.parametrize("shape,kind", [((31, 47), "smooth"), ((32, 48), "smooth"), ((96, 128), "smooth"), ((12, 16), "fold"), ((9, 7), "fold")])
def test_meter(be, mode, shape, kind):
    # (one sample at the large shape: with more boundary pixels fewer draws keep every position off the validity boundary by the margin)
    D.case_meter(be, mode, 1 if shape[0] > 64 else 3, *shape, kind=kind)


def test_meter_closed_forms(be):
    D.case_meter_identity(be, 16, 32)
    D.case_meter_identity(be, 128, 128)
    D.case_meter_inverse_translation(be, 24, 40)
    D.case_meter_inverse_translation(be, 17, 23, shift=(-1.5, 4.5))
    D.case_meter_inverse_translation(be, 128, 128)


def test_repeatable(be):
    D.case_repeatable(be)
    D.case_repeatable(be, H=64, W=96, seed=9)


def test_refusals(be):
    D.case_refusals(be)
