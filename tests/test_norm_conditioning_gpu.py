"""`-m gpu`: the normalisation kernels of the gfx950 library on ill-conditioned planes — every row of norm_cases.ROUTES with every
family, aligned and 4 bytes off, plane counts above the number of CUs, the plane producers, BatchNorm, and the product library in a child
process (tests/norm_cases.py, tests/bn_cases.py; tests/test_norm_conditioning_emu.py is the CPU tier of the same bodies).
NEMAR_NORM_REPORT=<file> writes every measured figure there."""
import os
import subprocess
import sys

import pytest

import bn_cases as B
import norm_cases as NC
from backends import HipBackend

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu

ROWS = [(HW, mis) for HW, _, _, vec in NC.ROUTES for mis in ((False, True) if vec else (False,))]


@pytest.fixture(scope="module")
def be(hip_lib):
    yield HipBackend(hip_lib)
    if os.environ.get("NEMAR_NORM_REPORT"):
        NC.dump_record(os.environ["NEMAR_NORM_REPORT"])


@pytest.mark.parametrize("HW,misalign", ROWS)
def test_instnorm_rows_families_cycling(be, HW, misalign):
    i = [r[0] for r in NC.ROUTES].index(HW)
    for k in range(3):                             # three rotations: every family on every row
        NC.case_instnorm_conditioned(be, 6, HW, "cycle", (NC.ACT_RELU, NC.ACT_LRELU, NC.ACT_NONE)[(i + k) % 3], (i + k) % 2 == 0, misalign,
                                     seed=i + 3 * k)


@pytest.mark.parametrize("family", NC.FAMILY_NAMES)
@pytest.mark.parametrize("HW,misalign", ROWS)
def test_instnorm_rows_every_family(be, HW, misalign, family):
    NC.case_instnorm_conditioned(be, 6, HW, family, NC.ACT_LRELU, family == "mixed", misalign, seed=11)


@pytest.mark.parametrize("pps", [1, 8, 64])
@pytest.mark.parametrize("planes,HW", [(512, 4096), (768, 1024)])
def test_instnorm_more_planes_than_cus(be, planes, HW, pps):
    NC.case_instnorm_conditioned(be, planes, HW, "cycle", NC.ACT_LRELU, True, False, pps=pps, seed=5)
    NC.case_instnorm_conditioned(be, planes, HW, "first_outlier", NC.ACT_RELU, False, True, pps=pps, seed=6)


@pytest.mark.parametrize("pps", [1, 8, 64])
def test_instnorm_max_words_planes_per_sample(be, pps):
    NC.case_instnorm_conditioned(be, 64, 448, "cycle", NC.ACT_LRELU, True, False, pps=pps, seed=3)
    NC.case_instnorm_conditioned(be, 64, 110592, "cycle", NC.ACT_NONE, False, False, pps=pps, seed=4)


@pytest.mark.parametrize("family", NC.PRODUCER_FAMILIES)
@pytest.mark.parametrize("H,W", [(8, 32), (16, 16), (64, 64)])
def test_plane_producers(be, H, W, family):
    NC.case_producers_conditioned(be, H, W, family)
    for rm in (0.0, 1.0, 1e3):
        NC.case_producers_conditioned(be, H, W, family, res_max=rm)
    NC.case_producers_conditioned(be, H, W, family, res_max=1.0, drop_p=0.5)
    NC.case_producers_conditioned(be, H, W, family, N=3, C=128, drop_p=0.5)


@pytest.mark.parametrize("family", B.BN_FAMILIES)
@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("HW", [35, 4096, 65536])
@pytest.mark.parametrize("N", [2, 8])
def test_batchnorm_families(be, family, N, HW, S):
    H, W = {35: (5, 7), 4096: (64, 64), 65536: (256, 256)}[HW]
    B.case_batchnorm_conditioned(be, N, 5, H, W, S, family)


def _child(ab):
    env = dict(os.environ, NEMAR_AB_LIBRARY="1" if ab else "0")
    env.pop("NEMAR_TUNE", None)
    env.pop("NEMAR_NORM_REPORT", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "norm_product_child.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(lines) == 1, r.stdout[-2000:]
    return lines[0].split()[1:]


def test_product_library_same_bits_on_ill_conditioned_planes():
    """the product library (a fresh process: a process binds one library for good) passes the first_outlier and spike cases at
    HW 4096, 65536 and 110592 and writes the same output bytes as the measurement build"""
    p, a = _child(False), _child(True)
    assert p[0] == "libnemar_hip.so" and a[0] == "libnemar_hip_ab.so"
    assert p[1:] == a[1:] and len(p) == 2
