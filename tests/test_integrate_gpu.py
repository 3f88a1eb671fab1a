"""`-m gpu`: nemar_svf_step_fwd / _bwd (csrc/integrate.hip) on the gfx950 library — the bodies of tests/integrate_cases.py that
tests/test_integrate_emu.py runs on the emulator, the network's own size (256 x 256: 64 tiles per sample), and ops.integrate_velocity:
its forward against the float64 chain, its backward against K manual step calls bit for bit."""
import numpy as np
import pytest
import torch

import integrate_cases as K
from backends import HipBackend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(hip_lib):
    return HipBackend(hip_lib)


@pytest.mark.parametrize("amp", K.AMPS)
@pytest.mark.parametrize("size", K.SIZES + K.EDGES + K.THIN, ids=str)
def test_step_forward_against_float64(be, size, amp):
    K.case_step_fwd(be, size, amp)


@pytest.mark.parametrize("amp", K.AMPS)
@pytest.mark.parametrize("size", K.SIZES, ids=str)
def test_step_backward_against_float64(be, size, amp):
    K.case_step_bwd(be, size, amp)


@pytest.mark.parametrize("size", K.EDGES + K.THIN, ids=str)
def test_step_backward_at_the_edges(be, size):
    K.case_step_bwd(be, size, 1.0)


def test_step_at_the_networks_size(be):
    K.case_step_fwd(be, K.NETWORK, 0.3)
    K.case_step_bwd(be, K.NETWORK, 0.3)


@pytest.mark.parametrize("size", [K.SIZES[0], (9, 13), (17, 65), K.NETWORK], ids=str)
def test_bits(be, size):
    K.case_bits(be, size)


def test_bounds(be):
    K.case_bounds(be)


def test_refusals(be):
    K.case_refusals(be)


@pytest.mark.parametrize("seed", [1, 3])
@pytest.mark.parametrize("size", [K.SIZES[2], K.NETWORK], ids=str)
def test_the_integrated_field_has_no_folds(be, size, seed):
    """the chain through ops.integrate_velocity, the folds through ops.jacobian_stats — after the float64 reference has shown that the
    case means something"""
    from nemar_amd import ops
    H, W = size
    what = "%s seed %d" % (size, seed)
    v = K.smooth_field(seed, 2, H, W, 1.0)
    K.reference_says_it_matters(v, 6, what)
    d_v = torch.from_numpy(v).cuda()
    raw = ops.jacobian_stats(d_v, ops.GRID_UNET, (H, W))[0].cpu().numpy()
    done = ops.jacobian_stats(ops.integrate_velocity(d_v, 6), ops.GRID_UNET, (H, W))[0].cpu().numpy()
    print("svf folds %s: ops.jacobian_stats raw %s, integrated %s of %s" % (what, raw[:, 1], done[:, 1], raw[:, 0]))
    assert raw[:, 1].sum() >= K.MIN_RAW_FOLDS * raw[:, 0].sum()
    assert done[:, 1].sum() == 0, (what, done)


@pytest.mark.parametrize("size", [K.SIZES[2], K.NETWORK], ids=str)
def test_inverse(be, size):
    K.case_inverse(be, size)


@pytest.mark.parametrize("steps", [0, 1, 4, 6])
@pytest.mark.parametrize("size", [K.SIZES[0], K.NETWORK], ids=str)
def test_ops_integrate_velocity(be, size, steps):
    """forward: the float64 chain by the MARGIN rule, and the bits of `steps` manual step calls; backward: the bits of `steps` manual
    nemar_svf_step_bwd calls on the saved step inputs in reverse order.  With the per-step float64 comparison that proves the chain's
    gradient"""
    from nemar_amd import ops
    H, W = size
    N = 2
    shape = (N, 2, H, W)
    bits = lambda a: np.asarray(a).view(np.uint32)
    for sign in (1.0, -1.0):
        v = K.smooth_field(2, N, H, W, 0.3)
        gout = K.gaussian(2, shape)
        d_v = torch.from_numpy(v).cuda().requires_grad_(True)
        out = ops.integrate_velocity(d_v, steps, sign)
        got = out.detach().cpu().numpy()
        K.check_chain_fwd(got, v, steps, sign, "ops %s K %d sign %+g" % (size, steps, sign))
        manual, inputs, scales = K.run_chain(be, v, steps, sign)
        assert np.array_equal(bits(got), bits(manual)), "ops.integrate_velocity is not the chain of step calls"
        out.backward(torch.from_numpy(gout).cuda())
        g = gout
        for d_u, s in zip(reversed(inputs), reversed(scales)):
            g = K.run_bwd(be, d_u, s, be.dev(g), shape)
        if steps == 0:
            g = np.float32(sign) * gout
        assert np.array_equal(bits(d_v.grad.cpu().numpy()), bits(g)), "the backward is not the step calls in reverse order"
    if steps == 0:
        assert ops.integrate_velocity(d_v.detach(), 0) is not None and ops.integrate_velocity(d_v.detach(), 0).data_ptr() == d_v.data_ptr()
    with pytest.raises(ValueError, match="integrate_velocity"):
        ops.integrate_velocity(d_v[:, :1], 2)
    with pytest.raises(ValueError, match="integrate_velocity"):
        ops.integrate_velocity(d_v, -1)
