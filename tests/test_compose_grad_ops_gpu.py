"""`-m gpu`: ops.compose_predictions(grad=True) above nemar_compose_pred_bwd — the forward's bits unchanged, the backward the kernel's
bits for the operands that ask for a gradient, the two-consumer chain of a cascade pass (fork -> warp_unet + compose) against torch-CPU
float64, and the refusals of the Python layer."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import compose_grad_cases as K
import register_grad_cases as R
from backends import HipBackend
from compose_cases import A, MODE_PAIRS, U
from register_cases import MARGIN

pytestmark = pytest.mark.gpu

bits = lambda t: t.detach().cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def be(hip_lib):
    return HipBackend(hip_lib)


@pytest.mark.parametrize("pair", MODE_PAIRS, ids=K.pair_id)
def test_same_forward_bits_and_the_kernels_gradient(be, pair):
    from nemar_amd import ops
    m1, m2 = pair
    hw = H, W = (35, 131)
    first, second, gout, _ = K.draw_case(7, m1, m2, hw)
    N = first.shape[0]
    want = [h.cpu() for h in K.run_bwd(be, be.dev(first), m1, be.dev(second), m2, be.dev(gout), N, H, W)]
    only_first = K.run_bwd(be, be.dev(first), m1, be.dev(second), m2, be.dev(gout), N, H, W, ("first",))[0].cpu()
    t_first, t_second, t_gout = (torch.from_numpy(a).cuda() for a in (first, second, gout))
    plain = ops.compose_predictions(t_first, m1, t_second, m2, hw)
    assert not plain.requires_grad
    f, s = t_first.clone().requires_grad_(True), t_second.clone().requires_grad_(True)
    field = ops.compose_predictions(f, m1, s, m2, hw, grad=True)
    assert field.requires_grad and torch.equal(field, plain), "grad=True changed the forward"
    field.backward(t_gout)
    assert np.array_equal(bits(f.grad), bits(want[0])) and np.array_equal(bits(s.grad), bits(want[1]))
    assert float(f.grad.abs().max()) > 0 and float(s.grad.abs().max()) > 0
    # only the operand that asks receives one (and the kernel is given that pointer alone: the same bits either way)
    f2 = t_first.clone().requires_grad_(True)
    ops.compose_predictions(f2, m1, t_second, m2, hw, grad=True).backward(t_gout)
    assert np.array_equal(bits(f2.grad), bits(only_first)) and np.array_equal(bits(f2.grad), bits(want[0]))
    # twice: the zeroed workspace came back zero
    f3, s3 = t_first.clone().requires_grad_(True), t_second.clone().requires_grad_(True)
    ops.compose_predictions(f3, m1, s3, m2, hw, grad=True).backward(t_gout)
    assert torch.equal(f3.grad, f.grad) and torch.equal(s3.grad, s.grad)


def test_refusals_of_the_python_layer():
    from nemar_amd import ops
    N, H, W = 2, 24, 40
    field, half, th, img = (torch.zeros(s, device='cuda') for s in ((N, 2, H, W), (N, 2, H // 2, W // 2), (N, 6), (N, 3, H, W)))
    with pytest.raises(ValueError, match="compose_predictions: grad=True with image"):
        ops.compose_predictions(field, U, field, U, (H, W), image=img, grad=True)
    for first, second in ((half, field), (field, half)):
        with pytest.raises(ValueError, match="compose_predictions: grad=True.*resampled"):
            ops.compose_predictions(first, U, second, U, (H, W), grad=True)
        assert ops.compose_predictions(first, U, second, U, (H, W)).shape == (N, 2, H, W)      # the forward keeps taking it
    with pytest.raises(ValueError, match="compose_predictions"):
        ops.compose_predictions(field, U, th[:1], A, (H, W), grad=True)
    with pytest.raises(ValueError, match="compose_predictions"):
        ops.compose_predictions(field, 0, th, A, (H, W), grad=True)
    assert ops.compose_predictions(th, A, field, U, (H, W), grad=True).shape == (N, 2, H, W)


def test_a_cascade_pass_fork_warp_and_compose_against_float64():
    """first -> (warp_unet(first, img), compose(first, second)): first.grad is the sum of both paths (ops.fork adds them).  Against
    torch-CPU float64 (F.grid_sample + compose_grad_cases.t_compose) by the float64 rule of compose_grad_cases with the warp's own
    yardstick, S and CHAIN (register_grad_cases, equal sizes) added, + 1 for the addition of the two paths."""
    from nemar_amd import ops
    hw = H, W = (40, 56)
    N, C = 2, 3
    first, second, gc, checked = K.draw_case(8, U, U, hw)
    assert checked
    img = np.random.default_rng(8).random((N, C, H, W)).astype(np.float32)
    gw = np.random.default_rng(9).standard_normal((N, C, H, W)).astype(np.float32)
    kink = R.kink_mask(first, U, H, W, H, W)
    assert kink.mean() <= R.KINK_SHARE
    gw[np.broadcast_to(kink[:, None], gw.shape)] = 0.0

    def torch_cpu(dtype):
        f = torch.tensor(first, dtype=dtype, requires_grad=True)
        s = torch.tensor(second, dtype=dtype, requires_grad=True)
        grid = R._grid(f, U, H, W)
        warped = F.grid_sample(torch.as_tensor(img, dtype=dtype), grid, mode='bilinear', padding_mode='zeros', align_corners=False)
        comp, _, _ = K.t_compose(f, U, s, U, H, W)
        ((warped * torch.as_tensor(gw, dtype=dtype)).sum() + (comp * torch.as_tensor(gc, dtype=dtype)).sum()).backward()
        return warped.detach().numpy(), comp.detach().numpy(), f.grad.numpy().astype(np.float64), s.grad.numpy().astype(np.float64)

    _, _, w_first, w_second = torch_cpu(torch.float64)
    _, _, y_first, y_second = torch_cpu(torch.float32)
    t_first, t_second = (torch.from_numpy(a).cuda().requires_grad_(True) for a in (first, second))
    f_warp, f_comp = ops.fork(t_first, 2)
    warped = ops.warp_unet(f_warp, [torch.from_numpy(img).cuda()])[0]
    comp = ops.compose_predictions(f_comp, U, t_second, U, hw, grad=True)
    torch.autograd.backward([warped, comp], [torch.from_numpy(gw).cuda(), torch.from_numpy(gc).cuda()])
    # each path alone, from the same inputs: the chain's gradient is their sum, rounded once
    a = t_first.detach().clone().requires_grad_(True)
    ops.warp_unet(a, [torch.from_numpy(img).cuda()])[0].backward(torch.from_numpy(gw).cuda())
    b = t_first.detach().clone().requires_grad_(True)
    ops.compose_predictions(b, U, t_second.detach(), U, hw, grad=True).backward(torch.from_numpy(gc).cuda())
    assert float(a.grad.abs().max()) > 0 and float(b.grad.abs().max()) > 0
    assert torch.equal(t_first.grad, a.grad + b.grad), "first.grad is not the sum of the warp's and the compose's gradients"

    S1, S2, count = K.abs_sums(first, U, second, U, H, W, gc)
    _, ggrid = R.ref_grad(img, first, U, H, W, gw)
    S_warp = R.abs_sum(first, U, H, W, ggrid)
    c1, c2 = K.chains(U, U, H, W)
    c_warp = R.chain(U, ((H, W), (H, W), None, C))
    Q = count.repeat(2, axis=1) * K.fixed_point_step(gc, H, W)
    bound1 = MARGIN * np.abs(y_first - w_first).max() + K.EPS24 * (c1 * S1 + c_warp * S_warp + (S1 + S_warp)) + Q
    bound2 = MARGIN * np.abs(y_second - w_second).max() + K.EPS24 * c2 * S2
    for name, got, want, bound in (("first", t_first.grad, w_first, bound1), ("second", t_second.grad, w_second, bound2)):
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        print("cascade pass g%-6s kernel %.3e  worst err/bound %.3f  max |g| %.3e" % (name, err.max(), (err / bound).max(), np.abs(want).max()))
        assert np.all(err <= bound), (name, float(err.max()), float((err / bound).max()))
