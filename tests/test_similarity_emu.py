"""CPU tier: nemar_joint_histogram (csrc/similarity.hip) compiled for the host SIMT emulator (tests/emu), against the numpy statement of
its definition (tests/similarity_cases.py): counts within the ambiguity the float64 reference allows, moments within the stated
addition depth, bitwise repeatability, properties and refusals; tests/test_similarity_gpu.py runs the same bodies on the gfx950 library."""
import pytest

import similarity_cases as K
from backends import EmuBackend


@pytest.fixture(scope="module")
def be(emu_lib):
    return EmuBackend(emu_lib)


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
