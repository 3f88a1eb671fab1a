"""`-m gpu`: cascaded registration through the model and the command line — NEMARModel.cascade(passes) against predictions composed by
hand (test(), the registered image fed back through set_input, test() again, netR.compose), register() on the composite, and
`python -m nemar_amd.register --passes K` in a fresh process against the model path bit for bit.  Same small nets as
tests/test_register_gpu.py::test_model_register_and_command_line.  Random weights: nothing is trained, no score has to improve."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = (131, 203)


def _argv(tmp, stn, size):
    return ['--model', 'nemar', '--stn_type', stn, '--netG', 'resnet_3blocks', '--ngf', '8', '--img_height', str(size), '--img_width', str(size),
            '--batch_size', '2', '--checkpoints_dir', str(tmp), '--name', 'reg', '--no_dropout', '--gpu_ids', '0']


def _pairs(seed):
    """two seeded float pairs at FULL: smooth textures (something a registration network can read)"""
    g = torch.Generator().manual_seed(seed)
    up = lambda t: torch.nn.functional.interpolate(t, size=FULL, mode='bicubic', align_corners=False)
    A = up(torch.rand(2, 3, 16, 20, generator=g)).clamp_(0, 1).numpy().astype(np.float32)
    B = up(torch.rand(2, 3, 16, 20, generator=g)).clamp_(0, 1).numpy().astype(np.float32)
    return A, B


def _run(tmp, stn, size, root, res, *more):
    r = subprocess.run(['timeout', '-k', '10', '400', sys.executable, '-m', 'nemar_amd.register', *_argv(tmp, stn, size), '--dataroot', str(root),
                        '--results_dir', str(res), '--epoch', 'latest', *more], cwd=ROOT, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'registered 2 pairs' in r.stdout
    return r.stdout, {n: open(res / 'reg' / n, 'rb').read() for n in ('registered_A.npy', 'offsets.npy')}


@pytest.mark.parametrize("stn,size", [("affine", 64), ("unet", 256)])       # (the UNet STN's seven poolings need 256 x 256: 64 x 64 has no such net)
def test_model_cascade_and_command_line(tmp_path, stn, size):
    from nemar_amd import ops
    from nemar_amd.models import create_model
    from nemar_amd.register import network_batch
    from nemar_amd.train import _Options
    torch.manual_seed(11)
    opt = _Options().parse(_argv(tmp_path, stn, size) + ['--ndf', '8'], quiet=True)
    model = create_model(opt)
    model.setup(opt)
    # the layer that predicts the transformation starts at (near) zero: give it weights that move pixels
    g = torch.Generator(device='cuda').manual_seed(5)
    with torch.no_grad():
        if stn == 'unet':
            w = model.netR.offset_map.output.conv2d.weight
            w.copy_(torch.randn(w.shape, generator=g, device='cuda') * 0.02)
        else:
            b = model.netR.net.local.at(2).bias
            b.copy_((torch.rand(b.shape, generator=g, device='cuda') - 0.5) * 0.2)
    ops.invalidate_packed_weights()
    A, B = _pairs(3)
    d_A, d_B = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    batch = network_batch(d_A, d_B, [0, 1], opt)
    with pytest.raises(ValueError, match='cascade'):
        model.cascade(0)

    # one pass by hand, then the registered image fed back as modality A: the second prediction
    model.set_input(batch)
    model.test()
    P1, mode = model.netR.last_prediction()
    P1, reg1, fake_B1, fake_TR1, fake_RT1 = P1.clone(), model.registered_real_A.clone(), model.fake_B.clone(), model.fake_TR_B.clone(), model.fake_RT_B.clone()
    assert float(P1.abs().max()) > 1e-3, "the prediction does not move anything: the test would show nothing"
    model.set_input(dict(batch, A=reg1))
    model.test()
    P2 = model.netR.last_prediction()[0].clone()
    assert float(P2.abs().max()) > 1e-3 and not torch.equal(P1, P2)
    if stn == 'unet':
        want, want_reg = model.netR.compose((P1, mode), (P2, mode), batch['A'].cuda())
        assert mode == ops.GRID_UNET and want.shape == P1.shape
    else:
        want = model.netR.compose(P1, P2)
        want_reg = model.netR.apply(want, [batch['A'].cuda()])[0]
        assert mode == ops.GRID_AFFINE and want.shape == (2, 6)

    # cascade(1) is test(), bit for bit
    model.set_input(batch)
    model.cascade(1)
    assert torch.equal(model.netR.last_prediction()[0], P1) and model.netR.last_prediction()[1] == mode
    for name, t in (('registered_real_A', reg1), ('fake_B', fake_B1), ('fake_TR_B', fake_TR1), ('fake_RT_B', fake_RT1)):
        assert torch.equal(getattr(model, name), t), name

    # cascade(2): the composite of the two predictions made by hand; everything downstream reads it
    model.set_input(batch)
    model.cascade(2)
    got, got_mode = model.netR.last_prediction()
    assert got_mode == mode and torch.equal(got, want), float((got - want).abs().max())
    assert not torch.equal(got, P1)
    assert torch.equal(model.registered_real_A, want_reg)
    assert torch.equal(model.registered_real_A, model.netR.apply((got, mode), [model.real_A])[0])           # the ORIGINAL image, warped once
    assert torch.equal(model.fake_RT_B, model.netR.apply((got, mode), [model.fake_B])[0]) and torch.equal(model.fake_B, fake_B1)
    assert model.fake_TR_B.shape == fake_TR1.shape and not torch.equal(model.fake_TR_B, fake_TR1)
    out = model.register(d_A, d_B, translate=False)
    assert out['offsets'] is got and out['registered_A'].shape == (2, 3, *FULL)
    assert torch.equal(out['registered_A'], model.netR.apply((got, mode), [d_A])[0])
    model.set_input(batch)
    model.cascade(3)
    cascade3 = model.netR.last_prediction()[0]
    assert cascade3.shape == got.shape and not torch.equal(cascade3, got) and bool(torch.isfinite(cascade3).all())

    # the command line, in a fresh process, on the same two pairs
    model.save_networks('latest')
    root = tmp_path / 'data'
    os.makedirs(root)
    np.save(root / 'A.npy', A)
    np.save(root / 'B.npy', B)
    said0, plain = _run(tmp_path, stn, size, root, tmp_path / 'r0')
    said1, one = _run(tmp_path, stn, size, root, tmp_path / 'r1', '--passes', '1')
    said2, two = _run(tmp_path, stn, size, root, tmp_path / 'r2', '--passes', '2')
    assert one == plain, "--passes 1 does not write what no flag writes"
    assert ' passes' not in said0 and ' passes' not in said1 and ' in 2 passes' in said2
    assert np.array_equal(np.load(tmp_path / 'r0' / 'reg' / 'offsets.npy'), P1.cpu().numpy())
    assert np.array_equal(np.load(tmp_path / 'r2' / 'reg' / 'offsets.npy'), got.cpu().numpy())
    assert np.array_equal(np.load(tmp_path / 'r2' / 'reg' / 'registered_A.npy'), out['registered_A'].cpu().numpy())
