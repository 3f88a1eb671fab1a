"""CPU tier: the normalisation kernels (csrc/norm.hip, csrc/norm_planes.hip, csrc/batchnorm.hip) compiled for the host SIMT emulator
(tests/emu) on ill-conditioned planes, against float64 and the reference layer's own fp32 error (tests/norm_cases.py, tests/bn_cases.py);
tests/test_norm_conditioning_gpu.py runs the same bodies, and more planes, on the gfx950 library.

Every row of norm_cases.ROUTES up to HW = 65536 runs here, and the 110592 row once per family group; what the emulator's speed costs is
plane COUNT, not rows: above HW = 16384 a call has 2 planes instead of 6 (1 at 110592), and the per-family calls above 4100 take the
families a statistics formula can get wrong (HARD below) rather than all nine — the "cycle" call of every row still mixes all nine
over the rows.  NEMAR_NORM_REPORT=<file> writes every measured figure there."""
import os

import pytest

import bn_cases as B
import norm_cases as NC
from backends import EmuBackend

HARD = ("first_outlier", "first_outlier_far", "offset", "spike")
ROWS = [(HW, mis) for HW, _, _, vec in NC.ROUTES if HW <= 110592 for mis in ((False, True) if vec else (False,))]


@pytest.fixture(scope="module")
def be(emu_lib):
    yield EmuBackend(emu_lib)
    if os.environ.get("NEMAR_NORM_REPORT"):
        NC.dump_record(os.environ["NEMAR_NORM_REPORT"])


def _planes(HW):
    return 6 if HW <= 16384 else (2 if HW <= 65536 else 1)


@pytest.mark.parametrize("HW,misalign", ROWS)
def test_instnorm_rows_families_cycling(be, HW, misalign):
    """one call whose planes cycle through the families (rotated by the row, so the rows together put every family on every kind of
    instance), with an activation and — on every other row — the residual"""
    i = [r[0] for r in NC.ROUTES].index(HW)
    NC.case_instnorm_conditioned(be, _planes(HW), HW, "cycle", (NC.ACT_RELU, NC.ACT_LRELU, NC.ACT_NONE)[i % 3], i % 2 == 0, misalign, seed=i)


@pytest.mark.parametrize("family", NC.FAMILY_NAMES)
@pytest.mark.parametrize("HW,misalign", [r for r in ROWS if r[0] <= 4100])
def test_instnorm_small_rows_every_family(be, HW, misalign, family):
    NC.case_instnorm_conditioned(be, 6, HW, family, NC.ACT_LRELU, family == "mixed", misalign, seed=11)


@pytest.mark.parametrize("family", HARD)
@pytest.mark.parametrize("HW,misalign", [r for r in ROWS if r[0] > 4100])
def test_instnorm_large_rows_hard_families(be, HW, misalign, family):
    NC.case_instnorm_conditioned(be, _planes(HW), HW, family, NC.ACT_RELU, False, misalign, seed=12)


@pytest.mark.parametrize("pps", [1, 8, 64])
def test_instnorm_max_words_planes_per_sample(be, pps):
    NC.case_instnorm_conditioned(be, 64, 448, "cycle", NC.ACT_LRELU, True, False, pps=pps, seed=3)
    NC.case_instnorm_conditioned(be, 64, 1024, "cycle", NC.ACT_NONE, False, False, pps=pps, seed=4)


@pytest.mark.parametrize("family", NC.PRODUCER_FAMILIES)
@pytest.mark.parametrize("H,W", [(8, 32), (16, 16), (64, 64)])
def test_plane_producers(be, H, W, family):
    NC.case_producers_conditioned(be, H, W, family)
    NC.case_producers_conditioned(be, H, W, family, res_max={"spike": 0.0, "constant": 1.0, "offset": 1e3, "first_outlier": 1.0}[family])


def test_plane_producers_residual_words_and_dropout(be):
    for rm in (0.0, 1.0, 1e3):
        NC.case_producers_conditioned(be, 16, 16, "spike", res_max=rm)
    NC.case_producers_conditioned(be, 16, 16, "spike", drop_p=0.5)
    NC.case_producers_conditioned(be, 8, 32, "first_outlier", res_max=1.0, drop_p=0.5)


@pytest.mark.parametrize("family", B.BN_FAMILIES)
@pytest.mark.parametrize("N,HW,S", [(2, 35, 1), (8, 35, 2), (2, 4096, 2), (8, 4096, 1), (2, 65536, 1)])
def test_batchnorm_families(be, family, N, HW, S):
    H, W = {35: (5, 7), 4096: (64, 64), 65536: (256, 256)}[HW]
    B.case_batchnorm_conditioned(be, N, 3 if HW < 65536 else 2, H, W, S, family)
