"""Which route every convolution call takes and what the host-side size queries answer, pinned to a recorded table
(tests/golden/conv_routes.json, written by tests/golden/make_conv_routes.py).  The table is the contract of the route planner
(nemar_amd/csrc/conv_route.h): a change of the planning code must leave every value here exactly as it was, or re-record on purpose.

Shared by tests/test_conv_routes_emu.py (host emulator library) and tests/test_conv_routes_gpu.py (gfx950 library)."""
import ctypes
import json
import os

import guard_cases as G
import kernel_cases as K
from nemar_amd._lib import ConvExtras

PAD_ZERO, PAD_REFLECT = 0, 1
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_routes.json")

# the timed shapes (tests/test_conv_real_shapes_gpu.py SHAPES, SPLIT16_SHAPES — that module imports torch, so the lists are restated; the
# tests check that they are still the same):  N, C0, C1, H, W, K, R, stride, pad, pad_mode
REAL_SHAPES = [
    (8, 256, 0, 64, 64, 256, 3, 1, 1, PAD_REFLECT), (8, 256, 0, 32, 32, 512, 4, 1, 1, PAD_ZERO), (8, 64, 32, 256, 256, 32, 3, 1, 1, PAD_ZERO),
    (8, 64, 0, 256, 256, 128, 3, 2, 1, PAD_ZERO), (8, 128, 0, 128, 128, 256, 3, 2, 1, PAD_ZERO), (8, 64, 0, 128, 128, 128, 4, 2, 1, PAD_ZERO),
    (8, 128, 0, 64, 64, 256, 4, 2, 1, PAD_ZERO), (8, 3, 3, 256, 256, 64, 4, 2, 1, PAD_ZERO), (8, 512, 0, 31, 31, 1, 4, 1, 1, PAD_ZERO),
    (8, 3, 0, 256, 256, 64, 7, 1, 3, PAD_REFLECT), (8, 64, 0, 256, 256, 3, 7, 1, 3, PAD_REFLECT), (8, 32, 0, 256, 256, 32, 3, 1, 1, PAD_REFLECT),
    (8, 64, 0, 128, 128, 64, 3, 1, 1, PAD_REFLECT), (8, 3, 3, 256, 256, 32, 3, 1, 1, PAD_ZERO), (8, 128, 0, 2, 2, 128, 3, 1, 1, PAD_REFLECT),
    (8, 32, 0, 256, 256, 2, 3, 1, 1, PAD_ZERO),
]
REAL_SPLIT16_SHAPES = [
    (8, 256, 0, 64, 64, 256, 3, 1, 1, PAD_REFLECT), (2, 256, 0, 128, 128, 256, 3, 1, 1, PAD_REFLECT), (8, 128, 0, 32, 32, 128, 3, 1, 1, PAD_ZERO),
    (8, 256, 0, 32, 32, 512, 4, 1, 1, PAD_ZERO),
]
# tests/test_kernels_emu.py CONV_CASES (C0, C1, K, R, stride, pad, pad_mode), which run at batch 2 on 9 x 10 images
CONV_CASES = [
    (3, 0, 8, 7, 1, 3, PAD_REFLECT), (16, 0, 40, 3, 1, 1, PAD_REFLECT), (32, 0, 70, 3, 2, 1, PAD_ZERO), (16, 16, 24, 3, 1, 1, PAD_ZERO),
    (3, 3, 12, 4, 2, 1, PAD_ZERO), (5, 0, 33, 4, 1, 1, PAD_ZERO), (20, 0, 2, 3, 1, 1, PAD_ZERO), (16, 0, 130, 1, 1, 0, PAD_ZERO),
    (18, 0, 3, 7, 1, 3, PAD_REFLECT), (24, 0, 1, 4, 1, 1, PAD_ZERO), (5, 0, 4, 3, 1, 1, PAD_REFLECT),
]
# one shape on each side of every threshold of the plan
THRESHOLD_SHAPES = [
    (1, 8, 0, 34, 34, 8, 3, 1, 1, PAD_REFLECT), (1, 8, 0, 35, 35, 8, 3, 1, 1, PAD_REFLECT),         # padded domain of 1296 texels / the next size up
    (1, 32, 0, 34, 34, 32, 3, 1, 1, PAD_REFLECT), (1, 32, 0, 35, 35, 32, 3, 1, 1, PAD_REFLECT),
    (2, 4, 0, 9, 10, 16, 3, 1, 1, PAD_REFLECT), (2, 5, 0, 9, 10, 16, 3, 1, 1, PAD_REFLECT),         # 4 / 5 input channels
    (2, 4, 0, 9, 10, 16, 3, 1, 1, PAD_ZERO), (2, 5, 0, 9, 10, 16, 3, 1, 1, PAD_ZERO),
    (2, 16, 0, 9, 10, 4, 3, 1, 1, PAD_ZERO), (2, 16, 0, 9, 10, 5, 3, 1, 1, PAD_ZERO),               # 4 / 5 output channels
    (1, 32, 0, 64, 64, 32, 3, 1, 1, PAD_REFLECT), (1, 32, 0, 64, 64, 32, 7, 1, 3, PAD_REFLECT),     # 9 / 49 taps, stride-1 reflect
    (1, 32, 0, 56, 56, 32, 3, 1, 1, PAD_ZERO), (1, 32, 0, 60, 60, 32, 3, 1, 1, PAD_ZERO),           # 28.9 / 33.2 million multiply-adds
    (1, 32, 0, 56, 56, 32, 3, 1, 1, PAD_REFLECT), (1, 32, 0, 60, 60, 32, 3, 1, 1, PAD_REFLECT),
    (1, 256, 0, 52, 64, 256, 3, 1, 1, PAD_REFLECT), (1, 256, 0, 56, 64, 256, 3, 1, 1, PAD_REFLECT),  # 1963 / 2114 million multiply-adds
    (1, 256, 0, 52, 64, 256, 3, 1, 1, PAD_ZERO), (1, 256, 0, 56, 64, 256, 3, 1, 1, PAD_ZERO),
    (1, 64, 0, 31, 31, 8, 3, 1, 1, PAD_ZERO), (1, 64, 0, 15, 15, 128, 4, 2, 1, PAD_ZERO),           # output planes that are no multiple of 4 floats
    (1, 64, 0, 32, 32, 128, 4, 1, 1, PAD_ZERO), (2, 64, 0, 32, 32, 128, 3, 1, 1, PAD_REFLECT),
    (1, 256, 0, 64, 64, 256, 3, 1, 1, PAD_REFLECT), (2, 256, 0, 64, 64, 256, 3, 1, 1, PAD_REFLECT),  # batch 1, 2, 8, 16: the wide route's reduction split
    (8, 256, 0, 64, 64, 256, 3, 1, 1, PAD_REFLECT), (16, 256, 0, 64, 64, 256, 3, 1, 1, PAD_REFLECT),
    (1, 256, 0, 64, 64, 256, 3, 1, 1, PAD_ZERO), (16, 256, 0, 64, 64, 256, 3, 1, 1, PAD_ZERO),
    (1, 16, 0, 9, 8, 5, 3, 2, 1, PAD_REFLECT),                                                       # strided reflect: padded domain + fold
]


def _k7(s):
    N, C, H, W, Kc, pm = s
    return (N, C, 0, H, W, Kc, 7, 1, 3, pm)


def _wide(s):
    N, C, H, W, Kc, pm = s
    return (N, C, 0, H, W, Kc, 3, 1, 1, pm)


def _transpose(s):              # ConvTranspose2d(Ci -> Co) = the data gradient of a stride-2 convolution Co -> Ci
    N, Ci, Co, H, W, R, op = s
    return (N, Co, 0, (H - 1) * 2 - 2 + R + op, (W - 1) * 2 - 2 + R + op, Ci, R, 2, 1, PAD_ZERO)


def _unique(shapes):
    return list(dict.fromkeys(tuple(int(v) for v in s) for s in shapes))


# the small lists: every one of them also runs the three operators on the emulator
SMALL_SHAPES = _unique(
    [(2, c0, c1, 9, 10, k, r, st, p, pm) for c0, c1, k, r, st, p, pm in CONV_CASES] + list(K.WGRAD_WIDE_CASES) +
    list(G.CONV_EXACT) + list(G.CONV_NARROW) + list(G.CONV_S16G) + list(G.CONV_S16G_WGRAD) + [s + (PAD_ZERO,) for s in G.CONV_S16G_DGRAD] +
    [_k7(s) for s in G.CONV_K7_FWD + G.CONV_K7_DGRAD + G.CONV_K7_WGRAD] +
    [_wide(s) for s in G.CONV_SPLIT16 + G.CONV_SPLIT16_DGRAD + G.CONV_SPLIT16_WGRAD] + [_transpose(s) for s in G.CONV_TRANSPOSE])
GPU_SHAPES = _unique(REAL_SHAPES + REAL_SPLIT16_SHAPES)
QUERY_SHAPES = _unique(REAL_SHAPES + REAL_SPLIT16_SHAPES + SMALL_SHAPES + THRESHOLD_SHAPES)

# nemar_tune settings the queries are recorded under, one at a time, and the value that restores each switch
TUNES = [None, (20, 0), (24, 0), (12, 0), (43, 0), (30, 0), (35, 0), (33, 0), (29, 0), (26, 1), (21, 3)]
TUNE_DEFAULTS = {20: 1, 24: 1, 12: 1, 43: 1, 30: 1, 35: 1, 33: 1, 29: 1, 26: 0, 21: 4, 23: 2000, 25: 30}
QUERY_NAMES = ["fwd_workspace", "bwd_data_workspace", "bwd_weight_workspace", "scratch", "gy_planes_bytes", "fusable", "addend_ok"]


def key(shape, tune=None):
    return ("default" if tune is None else "tune(%d,%d)" % tune) + " " + ",".join(str(int(v)) for v in shape)


def queries(lib, shape):
    """the seven host-side answers for one layer, in the order of QUERY_NAMES"""
    N, C0, C1, H, W, Kc, R, stride, pad, pm = shape
    C = C0 + C1
    OH, OW = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    return [int(lib.conv2d_fwd_workspace(N, H, W, Kc, C, R, R, stride, pad)),
            int(lib.conv2d_bwd_data_workspace(N, C, H, W, Kc, R, R, stride, pad, pm)),
            int(lib.conv2d_bwd_weight_workspace(N, C, H, W, Kc, OH, OW, R, R, stride, pad)),
            int(lib.conv2d_scratch(N, H, W, Kc, C, R, R, stride, pad)),
            int(lib.conv2d_gy_planes_bytes(N, C, H, W, Kc, R, R, stride, pad, pm)),
            int(lib.conv2d_bwd_data_fusable(N, C, H, W, Kc, R, R, stride, pad, pm)),
            int(lib.conv2d_bwd_data_addend_ok(N, C, H, W, Kc, R, R, stride, pad, pm))]


def query_table(lib):
    out = {}
    for t in TUNES:
        if t is not None:
            lib.tune(*t)
        try:
            for s in QUERY_SHAPES:
                out[key(s, t)] = queries(lib, s)
        finally:
            if t is not None:
                lib.tune(t[0], TUNE_DEFAULTS[t[0]])
    return out


def run_ops(be, shape, arena):
    """The three operators once each on zero-filled buffers -> [forward route, data-gradient route, nemar_last_gy_planes of the data gradient,
    weight-gradient route] (None where the operator does not take the layer: a reflect data gradient has one destination).  With `arena` the
    calls bring a scratch arena of nemar_conv2d_scratch bytes and the data gradient offers a gy_planes_out buffer; a layer that wants no
    arena gives None."""
    N, C0, C1, H, W, Kc, R, stride, pad, pm = shape
    C = C0 + C1
    OH, OW = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    lib, P = be.lib, be.ptr
    e = ConvExtras()
    hold = []
    if arena:
        sb = lib.conv2d_scratch(N, H, W, Kc, C, R, R, stride, pad)
        if sb == 0:
            return None
        hold.append(be.bytes_buf(sb))
        e.scratch, e.scratch_bytes = P(hold[-1]).value, sb
    x0, x1 = be.zeros(N, C0, H, W), (be.zeros(N, C1, H, W) if C1 else None)
    w, b, gy = be.zeros(Kc, C, R, R), be.zeros(Kc), be.zeros(N, Kc, OH, OW)

    def ws(nbytes):
        hold.append(be.bytes_buf(max(int(nbytes), 16)))
        return P(hold[-1]), int(nbytes)

    y = be.zeros(N, Kc, OH, OW)
    lib.conv2d_fwd_ex(P(x0), C0, P(x1) if C1 else None, C1, P(w), P(b), P(y), N, H, W, Kc, R, R, stride, pad, pm, 0, 0.0,
                      *ws(lib.conv2d_fwd_workspace(N, H, W, Kc, C, R, R, stride, pad)), 0, be.stream, ctypes.byref(e))
    out = [int(lib.last_route()), None, None, None]
    if not (pm == PAD_REFLECT and C1):
        g0, g1 = be.zeros(N, C0, H, W), (be.zeros(N, C1, H, W) if C1 else None)
        ed = ConvExtras()
        ed.scratch, ed.scratch_bytes = e.scratch, e.scratch_bytes
        gb = lib.conv2d_gy_planes_bytes(N, C, H, W, Kc, R, R, stride, pad, pm) if arena else 0
        if gb:
            hold.append(be.bytes_buf(gb))
            ed.gy_planes_out, ed.gy_planes_bytes = P(hold[-1]).value, gb
        lib.conv2d_bwd_data_ex(P(gy), P(w), None, 0, 0.0, P(g0), C0, P(g1) if C1 else None, C1, N, H, W, Kc, OH, OW, R, R, stride, pad, pm,
                               *ws(lib.conv2d_bwd_data_workspace(N, C, H, W, Kc, R, R, stride, pad, pm)), 0, be.stream, ctypes.byref(ed))
        out[1], out[2] = int(lib.last_route()), int(lib.last_gy_planes())
    gw, gbias = be.zeros(Kc, C, R, R), be.zeros(Kc)
    lib.conv2d_bwd_weight_ex(P(x0), C0, P(x1) if C1 else None, C1, P(gy), P(gw), P(gbias), N, H, W, Kc, OH, OW, R, R, stride, pad, pm,
                             *ws(lib.conv2d_bwd_weight_workspace(N, C, H, W, Kc, OH, OW, R, R, stride, pad)), be.stream, ctypes.byref(e))
    out[3] = int(lib.last_route())
    be.sync()
    return out


def route_table(be, shapes, lift):
    """run_ops for every shape without and with an arena; `lift`: with the work thresholds of the 16-bit-pipe routes at zero (the small lists)"""
    if lift:
        be.lib.tune(23, 0)
        be.lib.tune(25, 0)
    try:
        return {key(s): [run_ops(be, s, False), run_ops(be, s, True)] for s in shapes}
    finally:
        if lift:
            be.lib.tune(23, TUNE_DEFAULTS[23])
            be.lib.tune(25, TUNE_DEFAULTS[25])


def case_shape_lists():
    """REAL_SHAPES / REAL_SPLIT16_SHAPES are still the lists of tests/test_conv_real_shapes_gpu.py"""
    import test_conv_real_shapes_gpu as T
    assert [tuple(s[1:]) for s in T.SHAPES] == REAL_SHAPES and [tuple(s[1:]) for s in T.SPLIT16_SHAPES] == REAL_SPLIT16_SHAPES


def load_table():
    with open(TABLE) as f:
        return json.load(f)


def _differences(got, want):
    return ["%s: %s, recorded %s" % (k, got.get(k), want.get(k)) for k in sorted(set(got) | set(want)) if got.get(k) != want.get(k)]


def case_queries(lib):
    """every query value of every shape under every switch setting equals the recorded one"""
    bad = _differences(query_table(lib), load_table()["queries"])
    assert not bad, "%d query values (%s) moved:\n%s" % (len(bad), ", ".join(QUERY_NAMES), "\n".join(bad[:20]))


def case_routes(be, shapes, lift, section):
    bad = _differences(route_table(be, shapes, lift), load_table()[section])
    assert not bad, "%d layers changed route ([fwd, dgrad, gy planes, wgrad] without / with an arena):\n%s" % (len(bad), "\n".join(bad[:20]))
