"""CPU tier: the convolution size queries and the route every operator takes, against the recorded table (tests/route_cases.py), on
the host emulator library — and the queries of the gfx950 measurement library, which are host functions, against the same table."""
import pytest

import route_cases as RC
from backends import EmuBackend


def test_queries_match_the_table(emu_lib):
    RC.case_queries(emu_lib)


def test_shape_lists_are_the_timed_ones():
    RC.case_shape_lists()


def test_gfx950_library_answers_the_same():
    from nemar_amd import _lib
    lib = _lib.Library(_lib.AB_PATH)
    assert lib.has_switches
    RC.case_queries(lib)


def test_small_shapes_take_the_recorded_routes(emu_lib):
    """CONV_CASES, WGRAD_WIDE_CASES and the guard_cases lists with the work thresholds lifted: the three operators once each on
    zero-filled buffers, without and with an arena"""
    RC.case_routes(EmuBackend(emu_lib), RC.SMALL_SHAPES, True, "routes_emu")
