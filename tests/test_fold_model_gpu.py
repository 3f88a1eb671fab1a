"""`-m gpu`: the fold penalty above the kernels — ops.fold_penalty's autograd node against the entry points bit for bit, and the term in
the training step (--lambda_fold, --fold_margin): off by default with nothing changed, on as one more loss, one more root of the
translation + registration step that reaches netR only, and one more scalar of the training monitor.  The smallest UNet-STN
configuration of the model tests (tests/test_misalign_gpu.py); random weights, one step: nothing is trained, no number has to be good."""
import json
import math
import os

import numpy as np
import pytest
import torch

import fold_cases as K
from backends import HipBackend

pytestmark = pytest.mark.gpu

SIZE = 256                  # (the UNet STN's seven poolings need 256 x 256)
TODAY = ['L1_TR', 'GAN_TR', 'L1_RT', 'GAN_RT', 'smoothness', 'D_fake_TR', 'D_fake_RT', 'D']


def _argv(tmp, stn='unet', size=SIZE, extra=()):
    return ['--model', 'nemar', '--stn_type', stn, '--netG', 'resnet_3blocks', '--ngf', '8', '--ndf', '8', '--dataset_mode', 'gpupairs',
            '--dataroot', 'synthetic', '--img_height', str(size), '--img_width', str(size), '--crop_size', str(size), '--load_size',
            str(size + 12), '--batch_size', '2', '--pool_size_pairs', '6', '--checkpoints_dir', str(tmp), '--name', 'fold', '--no_dropout',
            '--gpu_ids', '0', '--lambda_smooth', '1.0', '--enable_tbvis', '--tbvis_iteration_update_rate', '1', '--tbvis_disable_report_weights',
            *extra]


def _opt(tmp, **kw):
    from nemar_amd.train import _Options
    return _Options().parse(_argv(tmp, **kw), quiet=True)


def test_ops_fold_penalty_is_the_kernels_loss_and_gradient(hip_lib):
    from nemar_amd import ops
    be = HipBackend(hip_lib)
    N, H, W = 2, 35, 131
    shape = (N, 2, H, W)
    pred = K.smooth_field(5, N, H, W, 1.0)
    d_pred = be.dev(pred)
    want_loss, want_active = K.run_fwd(be, d_pred, shape, 0.5, 0.25)
    want_gd = K.run_bwd(be, d_pred, shape, 0.5, 0.25, 3.0)
    d = torch.from_numpy(pred).cuda().requires_grad_(True)
    loss, active = ops.fold_penalty(d, margin=0.5, factor=0.25, return_active=True)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda and loss.requires_grad
    assert active.shape == (N,) and active.dtype == torch.int32 and active.is_cuda and not active.requires_grad
    loss.backward(torch.full((), 3.0, device='cuda'))
    bits = lambda a: np.asarray(a).view(np.uint32)
    assert bits(loss.detach().cpu().numpy()) == bits(want_loss)
    assert np.array_equal(active.cpu().numpy().view(np.uint32), want_active) and want_active.sum() > 0
    assert np.array_equal(bits(d.grad.cpu().numpy()), bits(want_gd)) and float(d.grad.abs().max()) > 0
    alone = ops.fold_penalty(d.detach(), margin=0.5, factor=0.25)                    # without the count: the scalar alone
    assert torch.is_tensor(alone) and torch.equal(alone, loss.detach())
    with pytest.raises(ValueError, match="fold_penalty"):
        ops.fold_penalty(d[:, :1])


@pytest.fixture(scope="module")
def steps(tmp_path_factory):
    """one seeded optimize_parameters() from identical state, with the term off and on: what each run left behind"""
    from nemar_amd import ops
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    out = {}
    data = None
    for name, extra in (('off', ['--lambda_fold', '0']), ('on', ['--lambda_fold', '5', '--fold_margin', '2'])):
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
        real = ops.fold_penalty

        def counting(*a, **k):
            calls.append(1)
            return real(*a, **k)
        ops.fold_penalty = counting
        try:
            model.set_input(data)
            model.optimize_parameters()
        finally:
            ops.fold_penalty = real
        torch.cuda.synchronize()
        pred = model.netR.last_prediction()[0]
        run = {'loss_names': list(model.loss_names), 'calls': len(calls), 'losses': model.get_current_losses(),
               'params': {net: [p.detach().clone() for p in getattr(model, 'net' + net).parameters()] for net in 'TRD'},
               'scalars': [json.loads(l) for l in open(os.path.join(str(tmp), 'fold', 'fold_tensorboard_logs', 'scalars.jsonl'))]}
        if name == 'on':
            run['loss_fold'] = model.loss_fold.clone()
            run['recomputed'] = 5 * ops.fold_penalty(pred, margin=2)
            run['det_range'] = [float(v) for v in ops.jacobian_stats(pred, ops.GRID_UNET, (SIZE, SIZE))[1][:, :2].cpu().numpy().ravel()]
        else:
            run['has_loss_fold'] = hasattr(model, 'loss_fold')
        out[name] = run
        if model.tb_visualizer is not None:
            model.tb_visualizer.end()
        del model
    return out


def test_off_by_default_nothing_changes(steps):
    off = steps['off']
    assert off['loss_names'] == TODAY and list(off['losses']) == TODAY
    assert off['calls'] == 0, "ops.fold_penalty ran with --lambda_fold 0"
    assert not off['has_loss_fold']
    assert not [r for r in off['scalars'] if r['tag'].startswith('fold/') or r['tag'] == 'loss/fold']


def test_on_it_is_a_loss_of_the_step(steps):
    on = steps['on']
    assert on['loss_names'] == TODAY[:5] + ['fold'] + TODAY[5:]
    assert on['calls'] == 1                                                   # (the recomputation below came after the count was taken)
    lo, hi = min(on['det_range'][0::2]), max(on['det_range'][1::2])
    assert 0 < lo and hi < 2, "the near-identity prediction's determinant is not below the margin everywhere: %r" % (on['det_range'],)
    v = float(on['loss_fold'])
    assert math.isfinite(v) and v > 0
    assert torch.equal(on['loss_fold'], on['recomputed']), (on['loss_fold'], on['recomputed'])
    assert on['losses']['fold'] == v
    # every pixel is below the margin: 5 * mean(2 - det), det within [lo, hi]
    assert 5 * (2 - hi) * (1 - 1e-5) <= v <= 5 * (2 - lo) * (1 + 1e-5)
    by = {r['tag']: r['value'] for r in on['scalars']}
    assert by['fold/active_frac'] == 1.0 and by['loss/fold'] == v


def test_the_term_reaches_netR_only(steps):
    off, on = steps['off']['params'], steps['on']['params']
    for net in 'TD':
        assert len(off[net]) == len(on[net]) > 0
        assert all(torch.equal(a, b) for a, b in zip(off[net], on[net])), "net%s differs: the fold term reached it, or the step is not repeatable" % net
    assert any(not torch.equal(a, b) for a, b in zip(off['R'], on['R'])), "netR is the same with and without the fold term"
    assert all(bool(torch.isfinite(p).all()) for p in on['R'])


def test_affine_stn_has_no_fold_term(tmp_path):
    from nemar_amd.models import create_model
    with pytest.raises(ValueError, match="lambda_fold.*unet"):
        create_model(_opt(tmp_path, stn='affine', size=64, extra=['--lambda_fold', '1']))
    create_model(_opt(tmp_path, stn='affine', size=64, extra=['--lambda_fold', '0', '--fold_margin', '0.5']))      # off: any STN


def test_step_graph_replay_equals_eager_with_the_term_on(tmp_path):
    """the term makes no host sync and no allocation outside the caching allocator: three replays of the captured step
    (NEMARModel.enable_step_graph) are three eager steps with the step parameters in device memory, bit for bit"""
    from nemar_amd import ops
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    argv = [a for a in _argv(tmp_path, extra=['--lambda_fold', '5', '--fold_margin', '2']) if a not in ('--enable_tbvis', '--tbvis_disable_report_weights')]
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
    assert l_eager[0]['fold'] > 0 and l_eager[0] != l_eager[-1]                       # (the steps do move the losses)
    assert l_eager == l_graph, (l_eager, l_graph)
    assert all(torch.equal(a, b) for a, b in zip(p_eager, p_graph))
