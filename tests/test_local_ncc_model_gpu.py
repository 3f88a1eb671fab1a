"""`-m gpu`: local NCC above the kernels — ops.local_ncc's autograd node against the entry points bit for bit, and the terms in the
training step (--lambda_lncc, --lncc_win): off by default with nothing changed, on as two more losses (LNCC_TR, LNCC_RT against real_B),
two more roots of the translation + registration step and two more scalars of the training monitor.  The configuration of
tests/test_fold_model_gpu.py; random weights, one step: nothing is trained, no number has to be good."""
import json
import math
import os

import numpy as np
import pytest
import torch

import local_ncc_cases as K
from backends import HipBackend

pytestmark = pytest.mark.gpu

SIZE = 256                  # (the UNet STN's seven poolings need 256 x 256)
TODAY = ['L1_TR', 'GAN_TR', 'L1_RT', 'GAN_RT', 'smoothness', 'D_fake_TR', 'D_fake_RT', 'D']
ON = ['--lambda_lncc', '10', '--lncc_win', '9']


def _argv(tmp, stn='unet', size=SIZE, extra=()):
    return ['--model', 'nemar', '--stn_type', stn, '--netG', 'resnet_3blocks', '--ngf', '8', '--ndf', '8', '--dataset_mode', 'gpupairs',
            '--dataroot', 'synthetic', '--img_height', str(size), '--img_width', str(size), '--crop_size', str(size), '--load_size',
            str(size + 12), '--batch_size', '2', '--pool_size_pairs', '6', '--checkpoints_dir', str(tmp), '--name', 'lncc', '--no_dropout',
            '--gpu_ids', '0', '--lambda_smooth', '1.0', '--enable_tbvis', '--tbvis_iteration_update_rate', '1', '--tbvis_disable_report_weights',
            *extra]


def _opt(tmp, **kw):
    from nemar_amd.train import _Options
    return _Options().parse(_argv(tmp, **kw), quiet=True)


def test_ops_local_ncc_is_the_kernels_loss_and_gradients(hip_lib):
    from nemar_amd import ops
    be = HipBackend(hip_lib)
    shape = (2, 3, 35, 131)
    xs, ys = K.images(shape[2:], 5, False, 2, 3)
    d_x, d_y = be.dev(xs), be.dev(ys)
    want_loss, want_cc = K.run_fwd(be, d_x, d_y, shape, 9, 1e-5, 0.25)
    want_gx, want_gy = K.run_bwd(be, d_x, d_y, shape, 9, 1e-5, 0.25, 3.0)
    only_gx, _ = K.run_bwd(be, d_x, d_y, shape, 9, 1e-5, 0.25, 3.0, want_gy=False)
    bits = lambda a: np.asarray(a).view(np.uint32)
    x = torch.from_numpy(xs.copy()).cuda().requires_grad_(True)
    y = torch.from_numpy(ys.copy()).cuda().requires_grad_(True)
    loss, cc = ops.local_ncc(x, y, win=9, factor=0.25, return_map=True)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda and loss.requires_grad
    assert cc.shape == x.shape and not cc.requires_grad
    loss.backward(torch.full((), 3.0, device='cuda'))
    assert bits(loss.detach().cpu().numpy()) == bits(want_loss)
    assert np.array_equal(bits(cc.cpu().numpy()), bits(want_cc))
    assert np.array_equal(bits(x.grad.cpu().numpy()), bits(want_gx)) and float(x.grad.abs().max()) > 0
    assert np.array_equal(bits(y.grad.cpu().numpy()), bits(want_gy)) and float(y.grad.abs().max()) > 0
    # y as a constant (the step's real_B): the scalar alone, a gradient towards x only
    x2 = x.detach().clone().requires_grad_(True)
    alone = ops.local_ncc(x2, y.detach(), factor=0.25)
    assert torch.is_tensor(alone) and torch.equal(alone, loss.detach())
    alone.backward(torch.full((), 3.0, device='cuda'))
    assert np.array_equal(bits(x2.grad.cpu().numpy()), bits(only_gx))
    with pytest.raises(ValueError, match="local_ncc"):
        ops.local_ncc(x, y[:, :1])
    with pytest.raises(ValueError, match="local_ncc"):
        ops.local_ncc(x[0], y[0])


@pytest.fixture(scope="module")
def steps(tmp_path_factory):
    """one seeded optimize_parameters() from identical state, with the terms off and on: what each run left behind"""
    from nemar_amd import ops
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    out = {}
    data = None
    for name, extra in (('off', ['--lambda_lncc', '0']), ('on', ON)):
        tmp = tmp_path_factory.mktemp(name)
        opt = _opt(tmp, extra=extra)
        if data is None:
            torch.manual_seed(7)
            data = next(iter(create_dataset(opt)))
        torch.manual_seed(11)                                 # identical initial weights in both runs
        model = create_model(opt)
        model.setup(opt)
        ops.invalidate_packed_weights()
        calls = []
        real = ops.local_ncc

        def counting(*a, **k):
            calls.append(1)
            return real(*a, **k)
        ops.local_ncc = counting
        try:
            model.set_input(data)
            model.optimize_parameters()
        finally:
            ops.local_ncc = real
        torch.cuda.synchronize()
        run = {'loss_names': list(model.loss_names), 'calls': len(calls), 'losses': model.get_current_losses(),
               'params': {net: [p.detach().clone() for p in getattr(model, 'net' + net).parameters()] for net in 'TRD'},
               'scalars': [json.loads(l) for l in open(os.path.join(str(tmp), 'lncc', 'lncc_tensorboard_logs', 'scalars.jsonl'))]}
        if name == 'on':
            run['loss_LNCC_TR'] = model.loss_LNCC_TR.clone()
            run['loss_LNCC_RT'] = model.loss_LNCC_RT.clone()
            run['recomputed'] = 10 * ops.local_ncc(model.fake_TR_B.detach(), model.real_B)
            run['as_factor'] = ops.local_ncc(model.fake_TR_B.detach(), model.real_B, 9, factor=10.0)
        else:
            run['has_loss'] = hasattr(model, 'loss_LNCC_TR') or hasattr(model, 'loss_LNCC_RT')
        out[name] = run
        if model.tb_visualizer is not None:
            model.tb_visualizer.end()
        del model
    return out


def test_off_by_default_nothing_changes(steps):
    off = steps['off']
    assert off['loss_names'] == TODAY and list(off['losses']) == TODAY
    assert off['calls'] == 0, "ops.local_ncc ran with --lambda_lncc 0"
    assert not off['has_loss']
    assert not [r for r in off['scalars'] if 'LNCC' in r['tag']]


def test_on_they_are_losses_of_the_step(steps):
    on = steps['on']
    assert on['loss_names'] == TODAY[:4] + ['LNCC_TR', 'LNCC_RT'] + TODAY[4:]
    assert on['calls'] == 2                                                   # (the recomputations came after the count was taken)
    by = {r['tag']: r['value'] for r in on['scalars']}
    for name in ('LNCC_TR', 'LNCC_RT'):
        v = float(on['loss_' + name])
        assert math.isfinite(v) and 0 < v <= 10, (name, v)
        assert on['losses'][name] == v and by['loss/' + name] == v
    # 10 * local_ncc(factor 1) on the image the step left behind, bit for bit (the kernel's factor is one float product on the rounded
    # 1 - mean cc), and the same call with the factor inside
    assert torch.equal(on['loss_LNCC_TR'], on['recomputed']), (on['loss_LNCC_TR'], on['recomputed'])
    assert torch.equal(on['loss_LNCC_TR'], on['as_factor']), (on['loss_LNCC_TR'], on['as_factor'])


def test_the_terms_reach_netT_and_netR_but_not_netD(steps):
    off, on = steps['off']['params'], steps['on']['params']
    assert len(off['D']) == len(on['D']) > 0
    # netD's step reads detached images of the same forward pass
    assert all(torch.equal(a, b) for a, b in zip(off['D'], on['D'])), "netD differs: the terms reached it, or the step is not repeatable"
    for net in 'TR':
        assert any(not torch.equal(a, b) for a, b in zip(off[net], on[net])), "net%s is the same with and without the local NCC terms" % net
        assert all(bool(torch.isfinite(p).all()) for p in on[net])


def test_affine_stn_trains_a_step_with_the_terms_on(tmp_path):
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    opt = _opt(tmp_path, stn='affine', size=64, extra=ON)
    torch.manual_seed(7)
    data = next(iter(create_dataset(opt)))
    torch.manual_seed(11)
    model = create_model(opt)
    model.setup(opt)
    model.set_input(data)
    model.optimize_parameters()
    torch.cuda.synchronize()
    losses = model.get_current_losses()
    assert 0 < losses['LNCC_TR'] <= 10 and 0 < losses['LNCC_RT'] <= 10
    assert all(bool(torch.isfinite(p).all()) for net in 'TR' for p in getattr(model, 'net' + net).parameters())
    if model.tb_visualizer is not None:
        model.tb_visualizer.end()
    with pytest.raises(ValueError, match="lncc_win"):
        create_model(_opt(tmp_path, stn='affine', size=64, extra=['--lambda_lncc', '1', '--lncc_win', '8']))


def test_step_graph_replay_equals_eager_with_the_terms_on(tmp_path):
    """the terms make no host sync and no allocation outside the caching allocator: three replays of the captured step
    (NEMARModel.enable_step_graph) are three eager steps with the step parameters in device memory, bit for bit"""
    from nemar_amd import ops
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    argv = [a for a in _argv(tmp_path, extra=ON) if a not in ('--enable_tbvis', '--tbvis_disable_report_weights')]
    del argv[argv.index('--tbvis_iteration_update_rate'):argv.index('--tbvis_iteration_update_rate') + 2]      # (the monitor reads tensors between launches)
    from nemar_amd.train import _Options
    opt = _Options().parse(argv, quiet=True)
    torch.manual_seed(7)
    data = next(iter(create_dataset(opt)))
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
    assert l_eager[0]['LNCC_TR'] > 0 and l_eager[0] != l_eager[-1]                    # (the steps do move the losses)
    assert l_eager == l_graph, (l_eager, l_graph)
    assert all(torch.equal(a, b) for a, b in zip(p_eager, p_graph))
