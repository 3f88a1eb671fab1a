"""`-m gpu`: the EPE loss above the kernels — ops.epe_loss's autograd node against the entry points bit for bit, and the term in the
training step (--lambda_epe, --epe_eps) on known-misalignment batches (--misalign both --synthetic_pairs mapped): off by default with
nothing changed, on as one more loss, one more root of the translation + registration step that reaches netR only, and one more scalar of
the training monitor; with the UNet STN, with --stn_integrate, and with the affine STN.  The smallest configurations of the model tests
(tests/test_fold_model_gpu.py); random weights, one step: nothing is trained, no number has to be good."""
import json
import math
import os

import numpy as np
import pytest
import torch

import deform_cases as D
import epe_cases as K
from backends import HipBackend
from register_cases import GRID_AFFINE, GRID_UNET

pytestmark = pytest.mark.gpu

TODAY = ['L1_TR', 'GAN_TR', 'L1_RT', 'GAN_RT', 'smoothness', 'D_fake_TR', 'D_fake_RT', 'D']
MISALIGN = ['--misalign', 'both', '--synthetic_pairs', 'mapped']
LAMBDA, EPS = 5.0, 0.05
#          name        stn      size  further flags                (the UNet STN's seven poolings need 256 x 256)
CONFIGS = [('unet', 'unet', 256, []), ('affine', 'affine', 64, []), ('integrate', 'unet', 256, ['--stn_integrate', '4'])]


def _argv(tmp, stn='unet', size=256, extra=(), monitor=True):
    tb = ['--enable_tbvis', '--tbvis_iteration_update_rate', '1', '--tbvis_disable_report_weights'] if monitor else []
    return ['--model', 'nemar', '--stn_type', stn, '--netG', 'resnet_3blocks', '--ngf', '8', '--ndf', '8', '--dataset_mode', 'gpupairs',
            '--dataroot', 'synthetic', '--img_height', str(size), '--img_width', str(size), '--crop_size', str(size), '--load_size',
            str(size + 12), '--batch_size', '2', '--pool_size_pairs', '6', '--checkpoints_dir', str(tmp), '--name', 'epe', '--no_dropout',
            '--gpu_ids', '0', '--lambda_smooth', '1.0', *tb, *extra]


def _opt(tmp, **kw):
    from nemar_amd.train import _Options
    return _Options().parse(_argv(tmp, **kw), quiet=True)


@pytest.mark.parametrize("mode,size", [(GRID_UNET, (35, 131)), (GRID_UNET, (40, 56)), (GRID_AFFINE, (35, 131))],
                         ids=lambda v: str(v))
def test_ops_epe_loss_is_the_kernels_loss_and_gradient(hip_lib, mode, size):
    from nemar_amd import ops
    be = HipBackend(hip_lib)
    N, (H, W) = 2, size
    pred, g = D._draw_meter_inputs(np.random.default_rng(5), mode, N, H, W, 'smooth')
    d_pred, d_g = be.dev(pred), be.dev(g)
    want_loss = K.run_fwd(be, d_pred, mode, d_g, (N, H, W), 0.05, 0.25)
    want_grad = K.run_bwd(be, d_pred, mode, d_g, (N, H, W), 0.05, 0.25, 3.0)
    p, gt = torch.from_numpy(pred).cuda().requires_grad_(True), torch.from_numpy(g).cuda().requires_grad_(True)
    loss = ops.epe_loss(p, mode, gt, eps=0.05, factor=0.25)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda and loss.requires_grad
    loss.backward(torch.full((), 3.0, device='cuda'))
    bits = lambda a: np.asarray(a).view(np.uint32)
    assert bits(loss.detach().cpu().numpy()) == bits(want_loss)
    assert np.array_equal(bits(p.grad.cpu().numpy()), bits(want_grad)) and float(p.grad.abs().max()) > 0
    assert gt.grad is None, "the ground-truth field carries no gradient"
    for bad in (lambda: ops.epe_loss(p[:1], mode, gt), lambda: ops.epe_loss(p, mode, gt[:, :1]), lambda: ops.epe_loss(p, mode, gt, eps=0.0),
                lambda: ops.epe_loss(p, mode, gt, eps=-1.0), lambda: ops.epe_loss(p, GRID_AFFINE if mode == GRID_UNET else GRID_UNET, gt)):
        with pytest.raises(ValueError, match="epe_loss"):
            bad()


@pytest.fixture(scope="module", params=CONFIGS, ids=lambda c: c[0])
def steps(request, tmp_path_factory):
    """one seeded optimize_parameters() from identical state, with the term off and on: what each run left behind"""
    from nemar_amd import ops
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    name, stn, size, flags = request.param
    out = {'size': size}
    data = None
    for run_name, extra in (('off', ['--lambda_epe', '0']), ('on', ['--lambda_epe', str(LAMBDA), '--epe_eps', str(EPS)])):
        tmp = tmp_path_factory.mktemp(name + '_' + run_name)
        opt = _opt(tmp, stn=stn, size=size, extra=MISALIGN + flags + extra)
        if data is None:
            torch.manual_seed(7)
            data = next(iter(create_dataset(opt)))
            assert data.get('gt_field') is not None
        torch.manual_seed(11)                                 # identical initial weights in both runs
        model = create_model(opt)
        model.setup(opt)
        ops.invalidate_packed_weights()
        calls = []
        real = ops.epe_loss

        def counting(*a, **k):
            calls.append(1)
            return real(*a, **k)
        ops.epe_loss = counting
        try:
            model.set_input(data)
            model.optimize_parameters()
        finally:
            ops.epe_loss = real
        torch.cuda.synchronize()
        pred, mode = model.netR.last_prediction()
        run = {'loss_names': list(model.loss_names), 'calls': len(calls), 'losses': model.get_current_losses(),
               'params': {net: [p.detach().clone() for p in getattr(model, 'net' + net).parameters()] for net in 'TRD'},
               'scalars': [json.loads(l) for l in open(os.path.join(str(tmp), 'epe', 'epe_tensorboard_logs', 'scalars.jsonl'))]}
        if run_name == 'on':
            run['loss_EPE'] = model.loss_EPE.clone()
            run['recomputed'] = LAMBDA * ops.epe_loss(pred, mode, model.gt_field, EPS)
        else:
            run['has_loss_EPE'] = hasattr(model, 'loss_EPE')
        out[run_name] = run
        if model.tb_visualizer is not None:
            model.tb_visualizer.end()
        del model
    return out


def test_off_by_default_nothing_changes(steps):
    off = steps['off']
    assert off['loss_names'] == TODAY and list(off['losses']) == TODAY
    assert off['calls'] == 0, "ops.epe_loss ran with --lambda_epe 0"
    assert not off['has_loss_EPE']
    assert not [r for r in off['scalars'] if r['tag'] == 'loss/EPE']


def test_on_it_is_a_loss_of_the_step(steps):
    on = steps['on']
    assert on['loss_names'] == TODAY[:5] + ['EPE'] + TODAY[5:]
    assert on['calls'] == 1                                                   # (the recomputation came after the count was taken)
    v = float(on['loss_EPE'])
    assert math.isfinite(v) and v > LAMBDA * EPS                              # (rho >= eps at every pixel)
    assert torch.equal(on['loss_EPE'], on['recomputed']), (on['loss_EPE'], on['recomputed'])
    assert on['losses']['EPE'] == v
    by = {r['tag']: r['value'] for r in on['scalars']}
    assert by['loss/EPE'] == v
    # the other losses of the step were formed before the term's gradient acted: today's values
    assert {k: x for k, x in on['losses'].items() if k != 'EPE'} == steps['off']['losses']


def test_the_term_reaches_netR_only(steps):
    off, on = steps['off']['params'], steps['on']['params']
    for net in 'TD':
        assert len(off[net]) == len(on[net]) > 0
        assert all(torch.equal(a, b) for a, b in zip(off[net], on[net])), "net%s differs: the EPE term reached it, or the step is not repeatable" % net
    assert any(not torch.equal(a, b) for a, b in zip(off['R'], on['R'])), "netR is the same with and without the EPE term"
    assert all(bool(torch.isfinite(p).all()) for p in on['R'])


def test_fold_and_epe_together_keep_their_places(tmp_path):
    from nemar_amd.models import create_model
    m = create_model(_opt(tmp_path, extra=MISALIGN + ['--lambda_fold', '1', '--lambda_epe', '1', '--lambda_lncc', '1']))
    assert m.loss_names == TODAY[:4] + ['LNCC_TR', 'LNCC_RT', 'smoothness', 'fold', 'EPE'] + TODAY[5:]
    with pytest.raises(ValueError, match="epe_eps"):
        create_model(_opt(tmp_path, extra=MISALIGN + ['--lambda_epe', '1', '--epe_eps', '0']))
    assert not hasattr(_opt(tmp_path, extra=MISALIGN), 'lambda_epe'), "the default option set carries the flag: the frozen option sets would change"


@pytest.mark.parametrize("batched", ['1', '0'])
def test_a_batch_without_or_with_another_gt_field_is_refused(tmp_path, monkeypatch, batched):
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    monkeypatch.setenv('NEMAR_BATCHED_PASSES', batched)
    flags = dict(stn='affine', size=64, monitor=False)
    opt = _opt(tmp_path, extra=['--misalign', 'none', '--lambda_epe', '1'], **flags)
    model = create_model(opt)
    model.setup(opt)
    model.set_input(next(iter(create_dataset(opt))))
    with pytest.raises(RuntimeError, match="--misalign"):
        model.optimize_parameters()
    opt = _opt(tmp_path, extra=MISALIGN + ['--lambda_epe', '1'], **flags)
    data = next(iter(create_dataset(opt)))
    model = create_model(opt)
    model.setup(opt)
    model.set_input(data)
    model.optimize_parameters()                                               # (a batch that carries one trains)
    assert math.isfinite(float(model.loss_EPE)) and float(model.loss_EPE) > 0
    model.set_input(dict(data, gt_field=data['gt_field'][:, :, :32]))
    with pytest.raises(ValueError, match="gt_field"):
        model.optimize_parameters()


def test_step_graph_replay_equals_eager_with_the_term_on(tmp_path):
    """the term makes no host sync and no allocation outside the caching allocator, and its ground-truth field is a static buffer of the
    capture: three replays of the captured step (NEMARModel.enable_step_graph) on three different batches are three eager steps with the
    step parameters in device memory, bit for bit"""
    from nemar_amd import ops
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    opt = _opt(tmp_path, extra=MISALIGN + ['--lambda_epe', str(LAMBDA)], monitor=False)      # (the monitor reads tensors between launches)
    torch.manual_seed(7)
    batches = []
    for data in create_dataset(opt):
        batches.append(data)
        if len(batches) == 3:
            break
    assert not torch.equal(batches[0]['gt_field'], batches[1]['gt_field'])
    snaps = []
    try:
        ops.step_params(True, torch.device('cuda:0'))
        for graph in (False, True):
            ops._step_params["step"] = 0
            torch.manual_seed(11)
            m = create_model(opt)
            m.setup(opt)
            ops.invalidate_packed_weights()
            m.set_input(batches[0])
            if graph:
                m.enable_step_graph(warmup=2)
            losses = []
            for data in batches:
                m.set_input(data)
                m.optimize_parameters()
                losses.append(m.get_current_losses())
            torch.cuda.synchronize()
            snaps.append(([p.detach().clone() for o in m.optimizers for p in (o.flat_p, o.m, o.v)], losses))
    finally:
        ops.step_params(False)
        ops.pin_workspaces(False)
    (p_eager, l_eager), (p_graph, l_graph) = snaps
    assert l_eager[0]['EPE'] > 0 and l_eager[0]['EPE'] != l_eager[1]['EPE']          # (each step saw its own field)
    assert l_eager == l_graph, (l_eager, l_graph)
    assert all(torch.equal(a, b) for a, b in zip(p_eager, p_graph))
