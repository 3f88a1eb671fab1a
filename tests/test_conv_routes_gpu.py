"""`-m gpu`: the convolution size queries and the routes of the timed shapes, against the recorded table (tests/route_cases.py), on
the gfx950 library.  No oracle comparison: tests/test_conv_real_shapes_gpu.py checks the values these calls compute."""
import pytest

import route_cases as RC
from backends import HipBackend

pytestmark = pytest.mark.gpu


def test_queries_match_the_table(hip_lib):
    RC.case_queries(hip_lib)


def test_shape_lists_are_the_timed_ones():
    RC.case_shape_lists()


def test_timed_shapes_take_the_recorded_routes(hip_lib):
    """SHAPES and SPLIT16_SHAPES at the default thresholds: the three operators once each on zero-filled buffers, without and with an arena"""
    RC.case_routes(HipBackend(hip_lib), RC.GPU_SHAPES, False, "routes_gpu")
