"""Cases that aim at the BOUNDS of the kernels (tests/backends.py guards every buffer with 64 KiB of poison on either side and checks
the guards after every library call): the bodies are those of kernel_cases / deform_cases / bn_cases — every float64 comparison still
runs — at shapes that put the last valid element where each kernel's vector, chunk or tile logic ends.  Driven by
tests/test_guards_emu.py and tests/test_guards_gpu.py.

How the shapes were chosen (csrc/ file: what ends where):
  flat kernels (pointwise.hip, loss.hip, core.hip, reduce.hip): 256 threads x float4 = 1024 elements per workgroup, scalar tail of n % 4,
      grid capped at 2048 workgroups (common.h nemar_stream_grid) -> the grid-stride loop takes its second trip from
      n = 4 * 256 * 2048 = 2097152 elements: FLAT_N_LONG sits on that boundary + {0, 1, 3}.
  plane kernels: rows are walked in chunks of 4 (float4) up to 64 columns -> every width 4k - 1 .. 4k + 2 around 4, 8, 16, 32 and 64,
      heights of 1, 2 and 3 where the entry point admits them.
  grid sample (warp.hip): 64 x 16 destination tiles, 70 x 22 staged window.
  convolutions: see CONV_* below, one list per route, each asserting nemar_last_route()."""
import numpy as np

import kernel_cases as K
from backends import both_poisons
from kernel_cases import _assert_close, PAD_ZERO, PAD_REFLECT
from oracle import ops_np as O

# ---- flat kernels ----------------------------------------------------------------------------------------------------------------------
FLAT_N = (1, 3, 4, 5, 12, 255, 256, 257, 1020, 1023, 1024, 1025, 1032)
_TRIP = 4 * 256 * 2048                              # elements one trip of a capped float4 grid covers
FLAT_N_LONG = (_TRIP, _TRIP + 1, _TRIP + 3, _TRIP + 12)


def case_flat_act_add(be, n):
    """nemar_act_fwd / act_bwd (every activation) and nemar_add2 (out of place and in place) on n elements"""
    K.case_pointwise(be, seed=n, flat_n=(n,), pool=(), bilinear=())
    K.case_concat_and_add(be, seed=n, concat=(), add_sizes=(n,))


@both_poisons
def case_flat_dropout(be, n, p=0.5):
    """nemar_dropout / nemar_dropout_max on n elements: every output is 0 or x / (1 - p) exactly, the two entry points agree bit for bit,
    the max word is numpy's maximum; one sample, and three where n % 12 == 0"""
    rng = np.random.default_rng(n)
    x = (rng.uniform(1, 2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    d_x = be.dev(x)
    y0 = be.full((n,), np.nan)
    be.lib.dropout(be.ptr(d_x), be.ptr(y0), n, p, 1234567, 7, be.stream)
    y = np.asarray(be.np(y0), dtype=np.float32)
    kept = (x / np.float32(1 - p)).astype(np.float32)
    assert np.all((y == 0) | (y == kept)), "dropout: an output is neither 0 nor x / (1 - p)"
    for N in [N for N in (1, 3) if n % (4 * N) == 0]:          # (nemar_dropout_max takes samples of a multiple of 4 elements)
        y1, w = be.full((n,), np.nan), be.bytes_buf(4 * N * 2049)           # NEMAR_MAX_WORDS(N)
        be.lib.dropout_max(be.ptr(d_x), be.ptr(y1), N, n // N, p, 1234567, 7, be.ptr(w), be.stream)
        assert np.array_equal(be.raw(y1), be.raw(y0)), "dropout_max != dropout"
        want = np.abs(y.reshape(N, -1)).max(axis=1).astype(np.float32).view(np.uint32)
        assert np.array_equal(be.raw(w)[:4 * N].view(np.uint32), want), "dropout_max words"


def case_flat_losses_adam(be, n):
    """nemar_l1_loss_*, nemar_gan_loss_* (every mode), nemar_adam_step and nemar_adam_step_dev on n elements"""
    # vanilla GAN gradient = (sigmoid(x) - target) * 0.25 / n: the fp32 difference is good to half an ulp of 1 (2^-24), which the case's
    # absolute 1e-9 covers from n ~ 15 up; below that the floor is stated in n
    K.case_losses(be, seed=n, sizes=(n,), gan_bwd_atol=1e-9 + 2.0 ** -24 * 0.25 / n)
    K.case_adam(be, n=n, steps=2, seed=n)
    K.case_step_params_in_device_memory(be, seed=n, n=n)


@both_poisons
def case_flat_absmax(be, n):
    """nemar_absmax on n elements (aligned and from a 4-byte-misaligned view) and nemar_absmax_samples on 3 samples of n"""
    K.case_absmax_and_hint.__wrapped__(be, seed=n, sizes=((n, 0), (n, 1)), with_hint=False, samples=(3, n))


def case_flat_concat(be, n):
    """nemar_concat_pieces: pieces of n elements around a NULL piece, a 3-element piece in front (the following pieces start off the
    16-byte grid), and one piece alone"""
    K.case_concat_and_add(be, seed=n, concat=(((n,), None), ((n, n, n), 1), ((3, n, 1), None), ((n, 5), 0)), add_sizes=())


def case_bias_grad(be, N, Kc, HW, seed=0):
    """nemar_bias_grad: gb[k] += sum over samples and pixels"""
    rng = np.random.default_rng(seed)
    gy = rng.standard_normal((N, Kc, HW)).astype(np.float32)
    d_gy, d_gb = be.dev(gy), be.full((Kc,), -0.25)
    wsb = be.lib.bias_grad_workspace(N, Kc, HW)
    ws = be.bytes_buf(wsb)
    be.lib.bias_grad(be.ptr(d_gy), be.ptr(d_gb), N, Kc, HW, be.ptr(ws), wsb, be.stream)
    want = gy.astype(np.float64).sum(axis=(0, 2))
    _assert_close(be.np(d_gb), want - 0.25, atol=2e-5 * np.sqrt(N * HW), rtol=2e-5, what="bias_grad")


BIAS_GRAD = [(1, 1, 1), (2, 3, 5), (1, 5, 255), (3, 2, 256), (2, 1, 257), (1, 64, 1023), (2, 65, 1025), (1, 130, 4)]

# ---- plane kernels ----------------------------------------------------------------------------------------------------------------------
PLANE_W = (3, 4, 5, 6, 7, 8, 9, 10, 15, 16, 17, 18, 31, 32, 33, 34, 63, 64, 65, 66)
PLANE_H = (1, 2, 3)


@both_poisons
def case_pool_bilinear(be, W):
    """2 x 2 max pool (the NaN-skipping maximum: both poisons) and bilinear resize, forward and backward, at width W and heights 2 .. 5"""
    pool = tuple((H, W) for H in (2, 3, 5) if W >= 2)
    bil = ((1, W, 2, 2 * W), (2, W, 4, 2 * W), (3, W, 6, 2 * W), (4, 2 * W, 2, W), (2, 2 * W, 1, W), (4, 4 * W, 1, W))
    if W <= 8:          # arbitrary ratios: the fp32 source coordinate costs ~W * 6e-8 px, beyond the case's 2e-6 on wide planes
        bil += ((2, W, 3, W + 1), (3, W, 5, max(1, W - 1)), (3, W, 1, max(1, W // 2)))
    K.case_pointwise.__wrapped__(be, seed=W, flat_n=(), pool=pool, bilinear=bil)


def case_smoothness(be, W):
    for H in (2, 3):
        K.case_smoothness(be, N=2, H=H, W=W, Ci=3, alpha=1.3, seed=W)
    K.case_smoothness(be, N=1, H=5, W=W, Ci=0, alpha=0.0, factor=0.5, accumulate=True, seed=W)


def case_crops(be, W):
    """nemar_crop_flip_normalize with crops flush against the right and the bottom edge of the pool, flipped and not, crop widths W and
    W - 1 out of a pool W + 1 wide, crop heights 1, 2 and the whole pool"""
    for Hc, H in ((1, 3), (2, 3), (3, 3)):
        for Wc in {W, max(1, W - 1)}:
            Wp = W + 1
            params = ((1, H - Hc, Wp - Wc, 0), (1, H - Hc, Wp - Wc, 1), (0, 0, 0, 1), (1, H - Hc, 0, 0), (0, 0, Wp - Wc, 1))
            K.case_crop_flip_normalize(be, seed=W, M=2, C=2, H=H, W=Wp, Hc=Hc, Wc=Wc, params=params)


def case_instnorm(be, W):
    """nemar_instnorm_fwd / _bwd on planes of H x W, H in 2, 3 (HW = 4k - 1 .. 4k + 2 over the widths), 1 and 3 planes"""
    for H in (2, 3):
        K.case_instnorm(be, 1, 1, H, W, K.O.ACT_LRELU, residual=False, seed=W)
        K.case_instnorm(be, 1, 3, H, W, K.O.ACT_NONE, residual=True, seed=W)


# ---- grid sample ----------------------------------------------------------------------------------------------------------------------
GRID_W = (63, 64, 65, 127, 129)
GRID_H = (15, 16, 17)


def case_grid_edges(be, mode, H, W, workspace=True):
    """a ragged 64 x 16 tile with ~1 px of noise (near path) and with scale 0.5 (far path: fixed-point atomics, many samples outside)"""
    K.case_grid_sample(be, mode, N=1, C=3, H=H, W=W, Ho=H, Wo=W, scale=0.02, seed=H * W, workspace=workspace, atomic=not workspace)
    K.case_grid_sample(be, mode, N=2, C=2, H=H, W=W, Ho=H, Wo=W, scale=0.5, seed=H * W + 1, workspace=workspace, atomic=not workspace)


def case_grid_borders(be, H, W, workspace=True):
    """smooth whole-pixel translations that send the samples of the border rows / columns to x = -1, W - 1, W and y = -1, H - 1, H exactly
    or within the coordinate rounding of them (both columns / rows of the 2 x 2 patch straddle the border), a half-pixel one, and
    Ho x Wo != H x W"""
    for sx, sy in ((1.0, 1.0), (-1.0, -1.0), (0.5, -0.5), (float(W - 1), 0.0), (0.0, float(-(H - 1)))):
        K.case_grid_sample(be, K.GRID_UNET, N=1, C=2, H=H, W=W, Ho=H, Wo=W, scale=0.0, smooth_px=(sx, sy, 0.0), seed=3, workspace=workspace,
                           atomic=not workspace)
        K.case_grid_sample(be, K.GRID_EXPLICIT, N=1, C=3, H=H, W=W, Ho=H, Wo=W, scale=0.0, smooth_px=(sx, sy, 0.0), seed=4, workspace=workspace,
                           atomic=not workspace)
    K.case_grid_sample(be, K.GRID_AFFINE, N=2, C=3, H=H, W=W, Ho=H - 2, Wo=W + 3, scale=0.1, seed=5, workspace=workspace, atomic=True)
    K.case_grid_sample(be, K.GRID_UNET, N=1, C=2, H=H, W=W, Ho=H + 1, Wo=W - 1, scale=0.05, seed=6, workspace=workspace, atomic=True)


# ---- convolutions ------------------------------------------------------------------------------------------------------------------------
# exact-fp32 implicit GEMM (conv_exact.hip, conv_wgrad.hip; route 0): pixel tiles of 64 / 128 flat output pixels, channel tiles of 64 / 128, 16-channel
# reduction chunks (FAST loader when C % 16 == 0), 16-byte loads when OW % 4 == 0.
#   N, C0, C1, H,  W,  K,  R, stride, pad, pad_mode
CONV_EXACT = [
    (1, 16, 0, 8, 16, 64, 3, 1, 1, PAD_REFLECT),        # P = 128: exactly one pixel tile, OW % 4 == 0, one channel tile
    (1, 15, 0, 3, 43, 63, 3, 1, 1, PAD_ZERO),           # P = 129, one channel short of the chunk and of the tile
    (1, 17, 0, 1, 127, 65, 3, 1, 1, PAD_ZERO),          # P = 127 in ONE row (H = 1), one channel past chunk and tile
    (2, 6, 7, 5, 13, 33, 3, 1, 1, PAD_ZERO),            # two sources, the second starts off the 4-channel grid; P = 130
    (1, 5, 11, 9, 7, 129, 4, 2, 1, PAD_ZERO),           # k4 s2, K one past the 128-row tile; OW = 3
    (2, 32, 0, 4, 17, 127, 1, 1, 0, PAD_ZERO),          # 1x1, OW = 4k + 1, P = 136
    (1, 16, 16, 7, 9, 64, 3, 2, 1, PAD_ZERO),           # stride 2 on odd extents -> 4 x 5 outputs
    (1, 3, 0, 4, 5, 8, 7, 1, 3, PAD_REFLECT),           # pad 3 on a 4 x 5 image
]
# narrow VALU kernels (conv_narrow.hip; route 1): <= 4 output channels; the register-tiled form (4 pixels per lane) from OW >= 64
CONV_NARROW = [
    (1, 18, 0, 4, 63, 3, 7, 1, 3, PAD_REFLECT),         # one short of the 4-pixels-per-lane form
    (1, 18, 0, 4, 64, 3, 7, 1, 3, PAD_REFLECT),
    (1, 9, 0, 2, 65, 2, 3, 1, 1, PAD_ZERO),
    (2, 5, 0, 5, 67, 4, 3, 1, 1, PAD_REFLECT),          # OW = 4k + 3
    (1, 24, 0, 2, 66, 1, 4, 1, 1, PAD_ZERO),            # k4: OW = 65, OH = 1
    (1, 7, 0, 1, 129, 1, 3, 1, 1, PAD_ZERO),            # one row, two tiles in x + 1
    (1, 8, 0, 6, 9, 2, 3, 1, 1, PAD_ZERO),              # the one-pixel-per-lane kernel
]
# general 16-bit-pipe kernels (conv_s16g.hip, conv_s16g_wgrad.hip; route 3): 256-pixel tiles of 32-column row pieces, 16-byte source loads at
# 4-column groups (the source width must be a multiple of 4), 16-channel chunks ("beyond the last channel: any valid address"), 64-row
# channel blocks
CONV_S16G = [
    (1, 16, 0, 8, 32, 64, 3, 1, 1, PAD_ZERO),           # exactly one tile, one chunk, one block
    (1, 15, 0, 7, 28, 63, 3, 1, 1, PAD_REFLECT),        # everything one short (W by one 4-column group)
    (1, 17, 0, 9, 36, 65, 3, 1, 1, PAD_ZERO),           # everything one past
    (2, 6, 11, 3, 44, 40, 3, 1, 1, PAD_ZERO),           # two sources, the second starts off the 4-channel grid; ragged chunk
    (1, 13, 0, 5, 68, 33, 4, 2, 1, PAD_ZERO),           # 4x4 stride 2, OW = 34
    (1, 31, 0, 2, 64, 129, 3, 2, 1, PAD_ZERO),          # stride 2, OH = 1, K one past two blocks
    (1, 33, 0, 1, 36, 31, 1, 1, 0, PAD_ZERO),           # 1x1 on one row
]
# weight gradient (conv_s16g_wgrad.hip): 32 / 64-row tiles of both channel counts, steps of 32 / 64 positions per row
CONV_S16G_WGRAD = [
    (1, 64, 0, 5, 32, 64, 3, 1, 1, PAD_ZERO),           # odd row count
    (1, 32, 0, 4, 64, 32, 3, 1, 1, PAD_REFLECT),        # H = 4: the fewest rows the route takes
    (2, 64, 32, 7, 64, 32, 3, 1, 1, PAD_ZERO),          # two sources
    (1, 64, 0, 6, 64, 64, 3, 2, 1, PAD_ZERO),           # stride 2: 3 x 32 outputs
    (1, 32, 0, 5, 128, 64, 1, 1, 0, PAD_ZERO),          # 1x1, two steps per row
]
#   N, C0, C1, H,  W,  K,  R, stride, pad            (data gradient: C0 + C1 are the output rows)
CONV_S16G_DGRAD = [
    (1, 33, 0, 7, 28, 15, 3, 1, 1),
    (1, 31, 0, 9, 36, 17, 3, 1, 1),
    (2, 6, 11, 3, 44, 24, 3, 1, 1),                     # two destinations, the second off the 4-channel grid
    (1, 48, 0, 6, 72, 16, 3, 2, 1),                     # stride 2: parity classes, 3 x 36 class pixels
    (1, 31, 0, 5, 33, 16, 4, 1, 1),                     # 4x4 stride 1: gy is 4 x 32
]
# 7x7 stem / head (conv_k7.hip; route 4): strips of 32 / 64 columns, row tiles of 4
#   N, C,  H,  W,  K, pad_mode
CONV_K7_FWD = [(1, 3, 4, 31, 32, PAD_REFLECT), (1, 3, 3, 32, 64, PAD_ZERO), (1, 2, 5, 33, 32, PAD_REFLECT), (1, 4, 1, 65, 32, PAD_ZERO),
               (1, 1, 7, 63, 96, PAD_REFLECT)]
CONV_K7_DGRAD = [(1, 32, 4, 31, 3, PAD_REFLECT), (1, 32, 4, 32, 1, PAD_ZERO), (1, 64, 5, 33, 2, PAD_REFLECT), (1, 32, 4, 65, 4, PAD_REFLECT),
                 (1, 32, 9, 63, 3, PAD_ZERO)]
CONV_K7_WGRAD = [(1, 3, 4, 31, 32, PAD_REFLECT), (1, 3, 5, 33, 64, PAD_ZERO), (2, 64, 4, 32, 3, PAD_REFLECT), (1, 32, 7, 36, 4, PAD_ZERO),
                 (1, 4, 9, 65, 32, PAD_REFLECT)]
# split-16 kernels of the wide layers (conv_split16*.hip; route 2, scratch arena of exactly nemar_conv2d_scratch bytes): rows of 32, 64, 128,
# 256 pixels, 16-channel chunks, 128-channel halves, plane rows rounded up to 4
#   N, C,  H,  W,  K, pad_mode
# (nemar_split16_eligible: H a multiple of 256 / W and >= 4 -> the smallest and an odd multiple of every row width)
CONV_SPLIT16 = [(1, 16, 8, 32, 128, PAD_REFLECT), (1, 32, 4, 64, 128, PAD_ZERO), (2, 48, 12, 64, 256, PAD_REFLECT), (1, 16, 6, 128, 128, PAD_ZERO),
                (1, 16, 5, 256, 128, PAD_REFLECT), (1, 16, 24, 32, 128, PAD_ZERO)]
CONV_SPLIT16_DGRAD = [(1, 128, 8, 32, 16, PAD_REFLECT), (1, 128, 4, 64, 32, PAD_ZERO), (2, 256, 12, 64, 16, PAD_REFLECT), (1, 128, 6, 128, 16, PAD_REFLECT),
                      (1, 128, 5, 256, 16, PAD_ZERO), (1, 128, 24, 32, 48, PAD_ZERO)]
CONV_SPLIT16_WGRAD = [(1, 128, 4, 8, 128, PAD_REFLECT), (1, 128, 5, 16, 128, PAD_ZERO), (1, 192, 7, 24, 128, PAD_REFLECT), (2, 128, 6, 32, 192, PAD_ZERO),
                      (1, 128, 9, 16, 128, PAD_REFLECT)]
# transposed convolutions (the data-gradient entry point, stride 2):  N, Ci, Co, H, W, R, output padding
CONV_TRANSPOSE = [(1, 16, 15, 3, 7, 3, 1), (1, 17, 65, 4, 8, 3, 1), (2, 15, 33, 5, 9, 4, 0), (1, 32, 129, 2, 16, 4, 0), (1, 16, 3, 1, 17, 3, 1)]


def case_conv_exact(be, shape):
    N, C0, C1, H, W, Kc, R, stride, pad, pm = shape
    with K.s16g_route(be, on=False):
        K.case_conv_fwd(be, N, C0, C1, H, W, Kc, R, stride, pad, pm, act=O.ACT_LRELU, seed=1)
        assert be.lib.last_route() == 0, "forward took route %d" % be.lib.last_route()
        if not (pm == PAD_REFLECT and C1):
            K.case_conv_bwd_data(be, N, C0, C1, H, W, Kc, R, stride, pad, pm, seed=2)
            assert be.lib.last_route() in (0, 1), "data gradient took route %d" % be.lib.last_route()
        K.case_conv_bwd_weight(be, N, C0, C1, H, W, Kc, R, stride, pad, pm, seed=3)


def case_conv_narrow(be, shape):
    N, C0, C1, H, W, Kc, R, stride, pad, pm = shape
    K.case_conv_fwd(be, N, C0, C1, H, W, Kc, R, stride, pad, pm, act=O.ACT_TANH, seed=1)
    assert be.lib.last_route() == 1, "forward took route %d" % be.lib.last_route()
    K.case_conv_bwd_weight(be, N, C0, C1, H, W, Kc, R, stride, pad, pm, seed=3)
    if not C1:          # the data gradient of a layer with Kc <= 4 INPUT channels runs on the narrow forward: swap the roles
        K.case_conv_bwd_data(be, N, Kc, 0, H, W, C0, R, stride, pad, pm, seed=2)
        # (nemar_last_route says 0 here: the narrow kernel is a branch inside the exact data-gradient path)


def case_conv_s16g(be, shape):
    K.case_conv_s16g_fwd(be, *shape, act=2, seed=1)


def case_conv_s16g_dgrad(be, shape):
    K.case_conv_s16g_bwd_data(be, *shape, seed=2)
    if shape[2] == 0 and shape[7] == 1 and shape[6] == 3:
        K.case_conv_s16g_bwd_data(be, *shape, seed=2, pad_mode=PAD_REFLECT)


def case_conv_split16(be, shape, what):
    N, C, H, W, Kc, pm = shape
    if what == "wgrad":
        K.case_conv_split16_wgrad(be, N, C, H, W, Kc, pm, seed=3)
    else:
        K.case_conv_split16(be, N, C, H, W, Kc, pm, dgrad=(what == "dgrad"), seed=1)
    assert be.lib.last_route() == 2 or what == "wgrad", "took route %d" % be.lib.last_route()
