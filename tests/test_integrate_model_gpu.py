"""`-m gpu`: scaling and squaring above the kernels — UnetSTN(integrate=K) in the training step (--stn_integrate): off by default with
nothing changed bit for bit, on as a velocity field whose exponential the warp reads, eagerly and under the captured step graph, with
--lambda_fold as well; the inverse prediction through NEMARModel.register(inverse=True) and `python -m nemar_amd.register --inverse`.  The
smallest UNet-STN configuration of the model tests (tests/test_fold_model_gpu.py); random weights: nothing is trained, no number has to
be good."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 256                  # (the UNet STN's seven poolings need 256 x 256)
FULL = (131, 203)


def _argv(tmp, stn='unet', size=SIZE, extra=()):
    return ['--model', 'nemar', '--stn_type', stn, '--netG', 'resnet_3blocks', '--ngf', '8', '--ndf', '8', '--dataset_mode', 'gpupairs',
            '--dataroot', 'synthetic', '--img_height', str(size), '--img_width', str(size), '--crop_size', str(size), '--load_size',
            str(size + 12), '--batch_size', '2', '--pool_size_pairs', '6', '--checkpoints_dir', str(tmp), '--name', 'svf', '--no_dropout',
            '--gpu_ids', '0', '--lambda_smooth', '1.0', *extra]


def _opt(tmp, **kw):
    from nemar_amd.train import _Options
    return _Options().parse(_argv(tmp, **kw), quiet=True)


def _two_steps(opt, data):
    """two seeded optimize_parameters() from identical state -> (the model, its losses per step, its parameters afterwards)"""
    from nemar_amd import ops
    from nemar_amd.models import create_model
    torch.manual_seed(11)
    model = create_model(opt)
    model.setup(opt)
    ops.invalidate_packed_weights()
    losses = []
    for _ in range(2):
        model.set_input(data)
        model.optimize_parameters()
        losses.append(model.get_current_losses())
    torch.cuda.synchronize()
    return model, losses, [p.detach().clone() for net in 'TRD' for p in getattr(model, 'net' + net).parameters()]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from nemar_amd.data import create_dataset
    torch.manual_seed(7)
    return next(iter(create_dataset(_opt(tmp_path_factory.mktemp('data')))))


def test_off_by_default_nothing_changes(tmp_path, data):
    opt = _opt(tmp_path)
    assert not hasattr(opt, 'stn_integrate'), "the default option set carries the flag: the frozen option sets would change"
    m0, l0, p0 = _two_steps(opt, data)
    m1, l1, p1 = _two_steps(_opt(tmp_path, extra=['--stn_integrate', '0']), data)
    assert m0.netR.integrate == 0 and m1.netR.integrate == 0 and not hasattr(m0.netR, 'last_velocity')
    assert l0 == l1 and len(p0) == len(p1) and all(torch.equal(a, b) for a, b in zip(p0, p1))
    with pytest.raises(RuntimeError, match="inverse_prediction.*stn_integrate"):
        m0.netR.inverse_prediction()


def test_on_the_warp_reads_the_integrated_field(tmp_path, data):
    from nemar_amd import ops
    model, losses, params = _two_steps(_opt(tmp_path, extra=['--stn_integrate', '4', '--stn_no_identity_init']), data)
    assert model.netR.integrate == 4
    assert all(math.isfinite(v) for step in losses for v in step.values()), losses
    assert all(bool(torch.isfinite(p).all()) for p in params)
    pred, mode = model.netR.last_prediction()
    v = model.netR.last_velocity
    assert mode == ops.GRID_UNET and pred.shape == v.shape == (2, 2, SIZE, SIZE) and not v.requires_grad
    assert float(v.abs().max()) > 0 and not torch.equal(pred, v), "the prediction is the velocity itself"
    assert torch.equal(pred, ops.integrate_velocity(v, 4)), "the prediction is not exp(v) of the velocity kept beside it"
    inv, inv_mode = model.netR.inverse_prediction()
    assert inv_mode == ops.GRID_UNET and torch.equal(inv, ops.integrate_velocity(v, 4, -1.0))


def test_affine_stn_has_no_velocity(tmp_path):
    from nemar_amd.models import create_model
    with pytest.raises(ValueError, match="stn_integrate.*unet"):
        create_model(_opt(tmp_path, stn='affine', size=64, extra=['--stn_integrate', '4']))
    create_model(_opt(tmp_path, stn='affine', size=64, extra=['--stn_integrate', '0']))      # off: any STN


@pytest.mark.parametrize("fold", [False, True], ids=["plain", "lambda_fold"])
def test_step_graph_replay_equals_eager(tmp_path, data, fold):
    """the integration makes no host sync and no allocation outside the caching allocator: three replays of the captured step
    (NEMARModel.enable_step_graph) are three eager steps with the step parameters in device memory, bit for bit"""
    from nemar_amd import ops
    from nemar_amd.models import create_model
    opt = _opt(tmp_path, extra=['--stn_integrate', '4', '--stn_no_identity_init'] + (['--lambda_fold', '5', '--fold_margin', '2'] if fold else []))
    snaps = []
    try:
        ops.step_params(True, torch.device('cuda:0'))
        for graph in (False, True):
            ops._step_params["step"] = 0
            torch.manual_seed(11)
            m = create_model(opt)
            m.setup(opt)
            ops.invalidate_packed_weights()
            m.set_input(data)
            if graph:
                m.enable_step_graph(warmup=2)
            losses = []
            for _ in range(3):
                m.set_input(data)
                m.optimize_parameters()
                losses.append(m.get_current_losses())
            torch.cuda.synchronize()
            snaps.append(([p.detach().clone() for o in m.optimizers for p in (o.flat_p, o.m, o.v)], losses))
    finally:
        ops.step_params(False)
        ops.pin_workspaces(False)
    (p_eager, l_eager), (p_graph, l_graph) = snaps
    assert l_eager[0] != l_eager[-1]                                                  # (the steps do move the losses)
    assert ('fold' in l_eager[0]) == fold
    assert l_eager == l_graph, (l_eager, l_graph)
    assert all(torch.equal(a, b) for a, b in zip(p_eager, p_graph))


def test_register_inverse_and_command_line(tmp_path):
    from nemar_amd import ops
    from nemar_amd.models import create_model
    from nemar_amd.register import network_batch
    flags = ['--stn_integrate', '4']
    g = torch.Generator().manual_seed(3)
    up = lambda t: torch.nn.functional.interpolate(t, size=FULL, mode='bicubic', align_corners=False)
    A = up(torch.rand(2, 3, 16, 20, generator=g)).clamp_(0, 1).numpy().astype(np.float32)
    B = up(torch.rand(2, 3, 16, 20, generator=g)).clamp_(0, 1).numpy().astype(np.float32)
    d_A, d_B = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    models = {}
    for name, extra in (('plain', []), ('svf', flags)):
        torch.manual_seed(11)
        opt = _opt(tmp_path, extra=extra)
        model = create_model(opt)
        model.setup(opt)
        gw = torch.Generator(device='cuda').manual_seed(5)
        with torch.no_grad():      # the layer that predicts the field starts at zero: give it weights that move pixels
            w = model.netR.offset_map.output.conv2d.weight
            w.copy_(torch.randn(w.shape, generator=gw, device='cuda') * 0.02)
        ops.invalidate_packed_weights()
        model.set_input(network_batch(d_A, d_B, [0, 1], opt))
        model.test()
        models[name] = model
    with pytest.raises(ValueError, match="inverse.*stn_integrate"):
        models['plain'].register(d_A, d_B, translate=False, inverse=True)
    model = models['svf']
    with pytest.raises(ValueError, match="inverse.*full_B"):
        model.register(d_A, None, translate=False, inverse=True)
    plain = model.register(d_A, d_B, translate=False)
    out = model.register(d_A, d_B, translate=False, inverse=True)
    assert sorted(plain) == ['offsets', 'registered_A'] and sorted(out) == ['inverse_offsets', 'offsets', 'registered_A', 'registered_B']
    assert all(torch.equal(plain[k], out[k]) for k in plain)
    assert out['registered_B'].shape == d_B.shape and out['inverse_offsets'].shape == (2, 2, SIZE, SIZE)
    assert float(out['inverse_offsets'].abs().max()) > 1e-3 and bool(torch.isfinite(out['registered_B']).all())
    assert torch.equal(out['registered_B'], ops.warp_resampled(out['inverse_offsets'], ops.GRID_UNET, [d_B], None, 'bilinear')[0])

    # the command line, in a fresh process, on the same two pairs
    model.save_networks('latest')
    root, res = tmp_path / 'pairs', tmp_path / 'res'
    os.makedirs(root)
    np.save(root / 'A.npy', A)
    np.save(root / 'B.npy', B)
    argv = ['--model', 'nemar', '--stn_type', 'unet', '--netG', 'resnet_3blocks', '--ngf', '8', '--img_height', str(SIZE), '--img_width', str(SIZE),
            '--batch_size', '2', '--checkpoints_dir', str(tmp_path), '--name', 'svf', '--no_dropout', '--gpu_ids', '0', *flags]
    run = lambda *more: subprocess.run(['timeout', '-k', '10', '400', sys.executable, '-m', 'nemar_amd.register', *argv, '--dataroot', str(root),
                                        '--results_dir', str(res), '--epoch', 'latest', *more], cwd=ROOT, capture_output=True, text=True, timeout=420)
    r = run('--inverse', '--regularity')
    assert r.returncode == 0, r.stderr[-3000:]
    assert sorted(os.listdir(res / 'svf')) == ['inverse_offsets.npy', 'offsets.npy', 'registered_A.npy', 'registered_B.npy', 'regularity.json']
    reg_B, inv = np.load(res / 'svf' / 'registered_B.npy'), np.load(res / 'svf' / 'inverse_offsets.npy')
    assert reg_B.shape == B.shape and reg_B.dtype == B.dtype and inv.shape == (2, 2, SIZE, SIZE) and inv.dtype == np.float32
    assert np.array_equal(inv.view(np.uint32), out['inverse_offsets'].cpu().numpy().view(np.uint32))
    assert np.array_equal(reg_B.view(np.uint32), out['registered_B'].cpu().numpy().view(np.uint32))
