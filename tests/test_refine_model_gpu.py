"""`-m gpu`: refinement on the pair above the kernel — ops.warp_resampled(grad=True) (the autograd node over nemar_warp_resampled_bwd),
NEMARModel.refine() for the affine STN, the UNet STN and the UNet STN with --stn_integrate, and `python -m nemar_amd.register --refine`.
The smallest configurations of the model tests: the affine STN at 64 x 64 with 96 x 136 pairs; the UNet STN at 256 x 256, which its
seven poolings need, with 272 x 328 pairs.  A pair is one smooth texture and a copy warped by a known smooth field
(register_cases.smooth_field, amp 0.05); for term 'l1' the identity stands in for netT (one "modality").  Random or zero-initialised
weights: nothing is trained, no number has to be good — the objective has to fall, the run has to repeat, the networks have to stay
untouched."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from register_cases import smooth_field

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = {'affine': (64, (96, 136), []), 'unet': (256, (272, 328), []), 'svf': (256, (272, 328), ['--stn_integrate', '4'])}


def _argv(tmp, kind):
    size, _, extra = CONFIG[kind]
    return ['--model', 'nemar', '--stn_type', 'affine' if kind == 'affine' else 'unet', '--netG', 'resnet_3blocks', '--ngf', '8', '--ndf', '8',
            '--dataset_mode', 'gpupairs', '--dataroot', 'synthetic', '--img_height', str(size), '--img_width', str(size), '--crop_size', str(size),
            '--load_size', str(size + 12), '--batch_size', '2', '--pool_size_pairs', '6', '--checkpoints_dir', str(tmp), '--name', 'refine',
            '--no_dropout', '--gpu_ids', '0', '--lambda_smooth', '1.0', *extra]


def _model(tmp, kind, seed=11):
    from nemar_amd import ops
    from nemar_amd.models import create_model
    from nemar_amd.train import _Options
    opt = _Options().parse(_argv(tmp, kind), quiet=True)
    torch.manual_seed(seed)
    model = create_model(opt)
    model.setup(opt)
    ops.invalidate_packed_weights()
    return model, opt


def _pair(hw, seed=3):
    """(A, B) [2,3,H,W] in [0, 1] on the device: one smooth texture, and the copy a known smooth field makes of it"""
    from nemar_amd import ops
    g = torch.Generator().manual_seed(seed)
    tex = torch.nn.functional.interpolate(torch.rand(2, 3, 12, 17, generator=g), size=hw, mode='bicubic', align_corners=False).clamp_(0, 1)
    A = tex.cuda().contiguous()
    field = torch.from_numpy(smooth_field(seed, 2, hw[0], hw[1], 0.05)).cuda()
    return A, ops.warp_resampled(field, ops.GRID_UNET, [A], None)[0]


def _look(model, opt, A, B):
    from nemar_amd.register import network_batch
    model.set_input(network_batch(A, B, [0, 1], opt))
    model.test()


# ---- the op ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["unet", "affine"])
def test_warp_resampled_grad(hip_lib, mode):
    from nemar_amd import ops
    from nemar_amd.ops import L, Q, _p, _stream
    g = torch.Generator().manual_seed(1)
    N, (hf, wf), (Ho, Wo) = 2, (24, 34), (96, 136)
    gm = ops.GRID_UNET if mode == 'unet' else ops.GRID_AFFINE
    pred = (torch.from_numpy(smooth_field(1, N, hf, wf, 0.1)) if mode == 'unet' else (torch.rand(N, 6, generator=g) - 0.5) * 0.2).cuda()
    imgs = [torch.rand(N, 3, Ho, Wo, generator=g).cuda(), torch.rand(N, 1, 50, 70, generator=g).cuda()]
    gouts = [torch.randn(N, 3, Ho, Wo, generator=g).cuda(), torch.randn(N, 1, Ho, Wo, generator=g).cuda()]
    plain = ops.warp_resampled(pred, gm, imgs, (Ho, Wo))
    assert not any(t.requires_grad for t in plain)

    def direct(img, gout):
        gp = torch.full_like(pred, float('nan'))
        wsb = Q.warp_resampled_bwd_workspace(gm, N, hf, wf, Ho, Wo)
        ws = torch.empty(max(wsb // 4, 1), dtype=torch.float32, device='cuda')
        L.warp_resampled_bwd(_p(img), _p(pred), gm, _p(gout), _p(gp), 0, N, img.shape[1], img.shape[2], img.shape[3],
                             hf if mode == 'unet' else 0, wf if mode == 'unet' else 0, Ho, Wo, _p(ws), wsb, _stream())
        return gp

    singles = [direct(i, g_) for i, g_ in zip(imgs, gouts)]
    # one image: the values are the read-out's, the gradient is the entry point's, bit for bit
    p = pred.clone().requires_grad_(True)
    out = ops.warp_resampled(p, gm, imgs[:1], (Ho, Wo), grad=True)
    assert torch.equal(out[0], plain[0]) and out[0].requires_grad
    (out[0] * gouts[0]).sum().backward()
    assert torch.equal(p.grad, singles[0])
    # two images share one gradient: the sum of the single calls within one rounding
    p = pred.clone().requires_grad_(True)
    out = ops.warp_resampled(p, gm, imgs, (Ho, Wo), grad=True)
    assert all(torch.equal(a, b) for a, b in zip(out, plain))
    assert out[0].grad_fn is out[1].grad_fn, "one autograd node for all images"
    ((out[0] * gouts[0]).sum() + (out[1] * gouts[1]).sum()).backward()
    want = singles[0].double() + singles[1].double()
    assert bool(((p.grad.double() - want).abs() <= 2.0 ** -24 * want.abs() * (1 + 1e-9)).all())
    # refusals, before any launch
    with pytest.raises(ValueError, match="bilinear"):
        ops.warp_resampled(p, gm, imgs, (Ho, Wo), 'nearest', grad=True)
    if mode == 'unet':
        with pytest.raises(ValueError, match="down-sampled"):
            ops.warp_resampled(p, gm, imgs, (hf - 1, Wo), grad=True)


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(tmp_path_factory):
    made = {}

    def get(kind):
        if kind not in made:
            model, opt = _model(tmp_path_factory.mktemp(kind), kind)
            made[kind] = (model, opt, _pair(CONFIG[kind][1]))
        return made[kind]
    return get


@pytest.mark.parametrize("term", ["l1", "mind"])
@pytest.mark.parametrize("kind", ["affine", "unet", "svf"])
def test_refine_lowers_the_objective_repeats_and_leaves_the_networks_alone(models, kind, term):
    from nemar_amd import ops
    model, opt, (A, B) = models(kind)
    netT = model.netT
    if term == 'l1':
        model.netT = torch.nn.Identity()            # one "modality": the texture is its own translation
    try:
        params = [p for net in 'TR' for p in getattr(model, 'net' + net).parameters()] + list(netT.parameters())
        snap = [p.detach().clone() for p in params]
        grads = [None if p.grad is None else p.grad.clone() for p in params]
        runs = []
        for _ in range(2):
            _look(model, opt, A, B)
            start = model.netR.last_prediction()[0].clone()
            told = model.refine(A, B, 30, term=term)
            runs.append(told)
            assert told['objective'].shape == (31,) and told['objective'].is_cuda and not told['offsets'].requires_grad
            assert torch.equal(model.netR.last_prediction()[0], told['offsets']) and not torch.equal(told['offsets'], start)
        obj = runs[0]['objective'].tolist()
        print("refine %s %s: objective %.6f -> %.6f" % (kind, term, obj[0], obj[-1]))
        assert all(np.isfinite(obj)) and obj[-1] < obj[0], obj
        assert torch.equal(runs[0]['offsets'], runs[1]['offsets']) and torch.equal(runs[0]['objective'], runs[1]['objective'])
        assert all(torch.equal(p.detach(), s) for p, s in zip(params, snap)), "a network parameter changed"
        assert all((p.grad is None) if g is None else torch.equal(p.grad, g) for p, g in zip(params, grads)), "a p.grad was touched"
        # register() now warps with the refined prediction
        out = model.register(A, B, translate=False)
        assert torch.equal(out['offsets'], runs[1]['offsets'])
        assert torch.equal(out['registered_A'], model.netR.apply(runs[1]['offsets'], [A])[0])
        if kind == 'svf':
            v = model.netR.last_velocity
            assert torch.equal(runs[1]['offsets'], ops.integrate_velocity(v, 4))
            inv, _ = model.netR.inverse_prediction()
            assert torch.equal(inv, ops.integrate_velocity(v, 4, -1.0)) and float(inv.abs().max()) > 0
    finally:
        model.netT = netT


def test_refine_refusals(models):
    model, opt, (A, B) = models('affine')
    _look(model, opt, A, B)
    with pytest.raises(ValueError, match="term"):
        model.refine(A, B, 2, term='mi')
    with pytest.raises(ValueError, match="netT"):
        model.refine(A[:, :, :95], B[:, :, :95], 2, term='l1')          # 95 rows: the generator's two strided levels do not divide it


def test_register_is_untouched_by_a_refine_elsewhere(models, tmp_path):
    """two register() runs of one model, the second after a refine() on ANOTHER instance: the same bits — no shared state"""
    model, opt, (A, B) = models('affine')
    other, other_opt = _model(tmp_path, 'affine', seed=12)
    _look(model, opt, A, B)
    first = model.register(A, B, translate=False)
    first = {k: v.clone() for k, v in first.items()}
    _look(other, other_opt, A, B)
    other.refine(A, B, 3)
    _look(model, opt, A, B)
    second = model.register(A, B, translate=False)
    assert sorted(first) == sorted(second) and all(torch.equal(first[k], second[k]) for k in first)


def test_command_line(models, tmp_path):
    """without --refine: the files a run of the same checkpoint in this process gives, bit for bit; with --refine 3: refine.json,
    offsets_before_refine.npy (those same offsets) and other offsets.npy"""
    model, opt, (A, B) = models('affine')
    _look(model, opt, A, B)
    want = model.register(A, B, translate=False)
    want = {k: v.cpu().numpy() for k, v in want.items()}
    model.save_networks('latest')
    ckpt = os.path.dirname(model.save_dir)
    root, res = tmp_path / 'pairs', tmp_path / 'res'
    os.makedirs(root)
    np.save(root / 'A.npy', A.cpu().numpy())
    np.save(root / 'B.npy', B.cpu().numpy())
    argv = ['--model', 'nemar', '--stn_type', 'affine', '--netG', 'resnet_3blocks', '--ngf', '8', '--img_height', '64', '--img_width', '64',
            '--batch_size', '2', '--checkpoints_dir', str(ckpt), '--name', 'refine', '--no_dropout', '--gpu_ids', '0']
    run = lambda out, *more: subprocess.run(['timeout', '-k', '10', '300', sys.executable, '-m', 'nemar_amd.register', *argv, '--dataroot', str(root),
                                             '--results_dir', str(out), '--epoch', 'latest', *more], cwd=ROOT, capture_output=True, text=True,
                                            timeout=320)
    r = run(res / 'plain')
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'refined' not in r.stdout
    assert sorted(os.listdir(res / 'plain' / 'refine')) == ['offsets.npy', 'registered_A.npy']
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert np.array_equal(bits(np.load(res / 'plain' / 'refine' / 'offsets.npy')), bits(want['offsets']))
    assert np.array_equal(bits(np.load(res / 'plain' / 'refine' / 'registered_A.npy')), bits(want['registered_A']))
    r = run(res / 'fine', '--refine', '3')
    assert r.returncode == 0, r.stderr[-3000:]
    assert ', refined 3 steps: objective ' in r.stdout, r.stdout
    assert sorted(os.listdir(res / 'fine' / 'refine')) == ['offsets.npy', 'offsets_before_refine.npy', 'refine.json', 'registered_A.npy']
    before, after = np.load(res / 'fine' / 'refine' / 'offsets_before_refine.npy'), np.load(res / 'fine' / 'refine' / 'offsets.npy')
    assert np.array_equal(bits(before), bits(want['offsets'])) and not np.array_equal(before, after)
    with open(res / 'fine' / 'refine' / 'refine.json') as f:
        told = json.load(f)
    assert told['steps'] == 3 and told['term'] == 'mind' and np.isfinite(told['objective_before']) and np.isfinite(told['objective_after'])
