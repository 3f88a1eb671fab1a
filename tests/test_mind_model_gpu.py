"""`-m gpu`: the MIND term above the kernels — ops.mind_loss's autograd node against the entry points bit for bit, and the term in the
training step (--lambda_mind, --mind_patch, --mind_dilation, --mind_eps): off by default with nothing changed, on as one more loss
(MIND_R: registered_real_A against real_B), one more root of the translation + registration step that reaches netR alone, in both
forward orders, with both STNs, with --stn_integrate and as a captured step graph.  The configuration of
tests/test_local_ncc_model_gpu.py; random weights, one step: nothing is trained, no number has to be good."""
import collections
import json
import math
import os

import numpy as np
import pytest
import torch

import mind_cases as K
from backends import HipBackend, _launches

pytestmark = pytest.mark.gpu

SIZE = 256                  # (the UNet STN's seven poolings need 256 x 256)
TODAY = ['L1_TR', 'GAN_TR', 'L1_RT', 'GAN_RT', 'smoothness', 'D_fake_TR', 'D_fake_RT', 'D']
LAMBDA = 10.0
ON = ['--lambda_mind', str(LAMBDA), '--mind_patch', '5', '--mind_dilation', '2']
TB = ['--enable_tbvis', '--tbvis_iteration_update_rate', '1', '--tbvis_disable_report_weights']

bits = lambda a: np.asarray(a).view(np.uint32)


def _argv(tmp, stn='unet', size=SIZE, extra=()):
    return ['--model', 'nemar', '--stn_type', stn, '--netG', 'resnet_3blocks', '--ngf', '8', '--ndf', '8', '--dataset_mode', 'gpupairs',
            '--dataroot', 'synthetic', '--img_height', str(size), '--img_width', str(size), '--crop_size', str(size), '--load_size',
            str(size + 12), '--batch_size', '2', '--pool_size_pairs', '6', '--checkpoints_dir', str(tmp), '--name', 'mind', '--no_dropout',
            '--gpu_ids', '0', '--lambda_smooth', '1.0', *extra]


def _opt(tmp, **kw):
    from nemar_amd.train import _Options
    return _Options().parse(_argv(tmp, **kw), quiet=True)


def test_ops_mind_loss_is_the_kernels_loss_and_gradients(hip_lib):
    from nemar_amd import ops
    be = HipBackend(hip_lib)
    shape = (2, 3, 1, 35, 131)
    xs, ys = K.images(shape[3:], 5)
    d_x, d_y = be.dev(xs), be.dev(ys)
    want_loss, want_dm = K.run_fwd(be, d_x, d_y, shape, 5, 2, 1e-5, 0.25)
    want_gx, want_gy = K.run_bwd(be, d_x, d_y, shape, 5, 2, 1e-5, 0.25, 3.0)
    only_gx, _ = K.run_bwd(be, d_x, d_y, shape, 5, 2, 1e-5, 0.25, 3.0, want_gy=False)
    x = torch.from_numpy(xs.copy()).cuda().requires_grad_(True)
    y = torch.from_numpy(ys.copy()).cuda().requires_grad_(True)
    loss, dm = ops.mind_loss(x, y, patch=5, dilation=2, factor=0.25, return_map=True)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda and loss.requires_grad
    assert tuple(dm.shape) == (2, 1, 35, 131) and not dm.requires_grad
    loss.backward(torch.full((), 3.0, device='cuda'))
    assert bits(loss.detach().cpu().numpy()) == bits(want_loss)
    assert np.array_equal(bits(dm.cpu().numpy()), bits(want_dm))
    assert np.array_equal(bits(x.grad.cpu().numpy()), bits(want_gx)) and float(x.grad.abs().max()) > 0
    assert np.array_equal(bits(y.grad.cpu().numpy()), bits(want_gy)) and float(y.grad.abs().max()) > 0
    # y as a constant (the step's real_B): the scalar alone, a gradient towards x only
    x2 = x.detach().clone().requires_grad_(True)
    alone = ops.mind_loss(x2, y.detach(), 5, 2, factor=0.25)
    assert torch.is_tensor(alone) and torch.equal(alone, loss.detach())
    alone.backward(torch.full((), 3.0, device='cuda'))
    assert np.array_equal(bits(x2.grad.cpu().numpy()), bits(only_gx))
    # the defaults are patch 3, dilation 2
    assert torch.equal(ops.mind_loss(x2, y.detach()), ops.mind_loss(x2, y.detach(), 3, 2, 1e-5, 1.0))
    for bad in ((x, y[:1]), (x, y[:, :, :-1]), (x, y[:, :, :, :-1]), (x[0], y[0])):
        with pytest.raises(ValueError, match="mind_loss"):
            ops.mind_loss(*bad)


class _Counting:
    """ops.L with every launching entry point counted by name"""

    def __init__(self, lib):
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not callable(fn) or not _launches(self._lib, name if name.startswith("nemar_") else "nemar_" + name):
            return fn

        def counted(*a):
            self.calls[name] += 1
            return fn(*a)
        return counted


def _run(tmp, extra, stn='unet', size=SIZE, batched=None, monkeypatch=None, data=None, only_mind=False, profile=False):
    """one seeded optimize_parameters() on one batch from identical initial weights -> what the run left behind"""
    from nemar_amd import ops
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    if batched is not None:
        monkeypatch.setenv('NEMAR_BATCHED_PASSES', batched)
    if only_mind:
        extra = list(extra) + ['--lambda_GAN', '0', '--lambda_recon', '0', '--lambda_smooth', '0']
    opt = _opt(tmp, stn=stn, size=size, extra=extra)
    if data is None:
        torch.manual_seed(7)
        data = next(iter(create_dataset(opt)))
    torch.manual_seed(11)
    model = create_model(opt)
    model.setup(opt)
    ops.invalidate_packed_weights()
    real = ops.L
    ops.L = counting = _Counting(real)
    events = None
    try:
        model.set_input(data)
        if profile:
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
                model.optimize_parameters()
                torch.cuda.synchronize()
            events = collections.Counter(e.name for e in prof.events())
        else:
            model.optimize_parameters()
    finally:
        ops.L = real
    torch.cuda.synchronize()
    grads = {net: getattr(model, 'optimizer_' + net).flat_g.detach().clone() for net in 'TRD'}      # (what the step's backward passes left)
    run = {'loss_names': list(model.loss_names), 'losses': model.get_current_losses(), 'calls': dict(counting.calls), 'data': data,
           'model': model, 'grads': grads, 'events': events,
           'params': {net: [p.detach().clone() for p in getattr(model, 'net' + net).parameters()] for net in 'TRD'}}
    log = os.path.join(str(tmp), 'mind', 'mind_tensorboard_logs', 'scalars.jsonl')
    if model.tb_visualizer is not None:
        model.tb_visualizer.end()
        run['scalars'] = [json.loads(l) for l in open(log)]
    return run


@pytest.fixture(scope="module")
def steps(tmp_path_factory):
    """the step without the options, with --lambda_mind 0, and with the term on: the same batch, the same initial weights"""
    absent = _run(tmp_path_factory.mktemp('absent'), TB)
    zero = _run(tmp_path_factory.mktemp('zero'), TB + ['--lambda_mind', '0', '--mind_patch', '5'], data=absent['data'])
    on = _run(tmp_path_factory.mktemp('on'), TB + ON, data=absent['data'])
    return {'absent': absent, 'zero': zero, 'on': on}


def test_off_by_default_nothing_changes(steps, tmp_path):
    absent, zero = steps['absent'], steps['zero']
    assert not hasattr(_opt(tmp_path), 'lambda_mind'), "the default option set carries the flag: the frozen option sets would change"
    for run in (absent, zero):
        assert run['loss_names'] == TODAY and list(run['losses']) == TODAY
        assert not [k for k in run['calls'] if 'mind' in k], "a MIND entry point ran with the term off"
        assert not hasattr(run['model'], 'loss_MIND_R')
        assert not [r for r in run['scalars'] if 'MIND' in r['tag']]
    # the same launches (entry point by entry point), the same losses, the same parameters after the step, bit for bit
    assert absent['calls'] == zero['calls'] and sum(absent['calls'].values()) > 100
    assert absent['losses'] == zero['losses']
    for net in 'TRD':
        assert all(torch.equal(a, b) for a, b in zip(absent['params'][net], zero['params'][net]))


def test_on_it_is_a_loss_of_the_step(steps):
    from nemar_amd import ops
    off, on = steps['absent'], steps['on']
    assert on['loss_names'] == TODAY[:4] + ['MIND_R'] + TODAY[4:]
    extra = {k: v - off['calls'].get(k, 0) for k, v in on['calls'].items() if v != off['calls'].get(k, 0)}
    print("further calls with the term on:", extra)
    # one forward and one backward launch pair, and ONE more library addition: registered_real_A's two gradients (netT's and the term's)
    assert extra == {'mind_loss_fwd': 1, 'mind_loss_bwd': 1, 'add2': 1}
    v = on['losses']['MIND_R']
    assert math.isfinite(v) and 0 < v <= LAMBDA
    by = {r['tag']: r['value'] for r in on['scalars']}
    assert by['loss/MIND_R'] == v                                     # the log line
    m = on['model']
    # the forward pass ran before the step's updates: the image the step left behind is the one the term read
    again = LAMBDA * ops.mind_loss(m.registered_real_A.detach(), m.real_B, 5, 2)
    inside = ops.mind_loss(m.registered_real_A.detach(), m.real_B, 5, 2, factor=LAMBDA)
    assert float(again) == v and float(inside) == v, (v, float(again), float(inside))
    # the other losses are what they were, and the total contains the term
    assert {k: x for k, x in on['losses'].items() if k != 'MIND_R'} == off['losses']
    # visuals read registered_real_A as before
    vis = m.get_current_visuals()
    assert torch.equal(vis['registered_real_A'], m.registered_real_A) and tuple(m.registered_real_A.shape) == tuple(m.real_A.shape)
    # netD's step reads detached images of the same forward pass
    assert all(torch.equal(a, b) for a, b in zip(off['params']['D'], on['params']['D'])), "netD differs: the term reached it"
    assert any(not torch.equal(a, b) for a, b in zip(off['params']['R'], on['params']['R']))
    assert all(bool(torch.isfinite(p).all()) for net in 'TR' for p in on['params'][net])


def test_the_total_contains_it(tmp_path):
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    totals = []
    data = None
    for extra in ([], ON):
        opt = _opt(tmp_path, stn='affine', size=64, extra=extra)
        if data is None:
            torch.manual_seed(7)
            data = next(iter(create_dataset(opt)))
        torch.manual_seed(11)
        m = create_model(opt)
        m.setup(opt)
        m.set_input(data)
        m.forward()
        m.set_requires_grad([m.netD, *m.netD_multiresolution], False)
        total = m.backward_T_and_R()
        totals.append((float(total), {'MIND_R': float(m.loss_MIND_R)} if extra else None))
    (t_off, _), (t_on, losses) = totals
    print("total without %.9g, with %.9g, MIND_R %.9g" % (t_off, t_on, losses['MIND_R']))
    # (the total is a float32 sum of the terms on the device: one more addition)
    assert abs((t_on - t_off) - losses['MIND_R']) <= 4 * 2.0 ** -24 * abs(t_on) and losses['MIND_R'] > 0


def test_it_reaches_netR_and_neither_netT_nor_netD(tmp_path):
    """every other weight 0: what is left of the translation + registration step's gradients is the term's"""
    on = _run(tmp_path, ON, stn='affine', size=64, only_mind=True)
    g = on['grads']
    assert on['losses']['MIND_R'] > 0
    assert float(g['R'].abs().max()) > 0 and bool(torch.isfinite(g['R']).all()), "netR hears nothing from the term"
    assert float(g['T'].abs().max()) == 0, "netT hears from the term"
    assert float(g['D'].abs().max()) == 0, "netD hears from the term"
    # and without the term nothing is left at all: what netR got is the term's
    off = _run(tmp_path / 'off', [], stn='affine', size=64, only_mind=True, data=on['data'])
    assert all(float(off['grads'][net].abs().max()) == 0 for net in 'TRD')


def test_both_forward_orders_agree(tmp_path, monkeypatch):
    a = _run(tmp_path / 'a', ON, batched='1', monkeypatch=monkeypatch, only_mind=True)
    b = _run(tmp_path / 'b', ON, batched='0', monkeypatch=monkeypatch, data=a['data'], only_mind=True)
    assert a['model']._batched and not b['model']._batched
    assert a['loss_names'] == b['loss_names']
    # registered_real_A is the warp of real_A by netR's prediction for the same pair with the same weights in either order
    assert a['losses']['MIND_R'] == b['losses']['MIND_R'] > 0
    for k in ('mind_loss_fwd', 'mind_loss_bwd'):
        assert a['calls'][k] == b['calls'][k] == 1
    # netR's gradients: what tests/test_step_gpu.py allows between the two orders, 2e-3 of the largest
    ga, gb = a['grads']['R'], b['grads']['R']
    scale = float(gb.abs().max())
    print("netR gradients, batched vs reference order: max difference %.3e of %.3e" % (float((ga - gb).abs().max()), scale))
    assert scale > 0 and float((ga - gb).abs().max()) <= 2e-3 * scale


def test_affine_stn_and_the_integrated_unet_train_a_step(tmp_path):
    from nemar_amd.models import create_model
    for stn, size, extra in (('affine', 64, []), ('unet', SIZE, ['--stn_integrate', '4'])):
        run = _run(tmp_path / stn, ON + extra, stn=stn, size=size)
        assert 0 < run['losses']['MIND_R'] <= LAMBDA
        assert all(bool(torch.isfinite(p).all()) for net in 'TR' for p in run['params'][net])
    for bad, match in ((['--mind_patch', '4'], "mind_patch"), (['--mind_patch', '7'], "mind_patch"), (['--mind_dilation', '3'], "mind_dilation"),
                       (['--mind_dilation', '0'], "mind_dilation"), (['--mind_eps', '0'], "mind_eps")):
        with pytest.raises(ValueError, match=match):
            create_model(_opt(tmp_path, stn='affine', size=64, extra=['--lambda_mind', '1'] + bad))
    # with the other terms: after the local NCC names
    m = create_model(_opt(tmp_path, extra=['--lambda_fold', '1', '--lambda_lncc', '1', '--lambda_mind', '1']))
    assert m.loss_names == TODAY[:4] + ['LNCC_TR', 'LNCC_RT', 'MIND_R', 'smoothness', 'fold'] + TODAY[5:]


def test_no_aten_addition_joins_the_gradients(tmp_path, monkeypatch):
    """registered_real_A has two consumers with the term on; in both forward orders their gradients meet in the library's add kernel
    (ops.fork), not in autograd's accumulation: the step records as many ATen additions with the term as without"""
    for batched in ('1', '0'):
        off = _run(tmp_path / ('off' + batched), [], stn='affine', size=64, batched=batched, monkeypatch=monkeypatch, profile=True)
        on = _run(tmp_path / ('on' + batched), ON, stn='affine', size=64, batched=batched, monkeypatch=monkeypatch, data=off['data'], profile=True)
        adds = lambda ev: {k: v for k, v in ev.items() if k in ('aten::add', 'aten::add_', 'aten::sum', 'aten::cat')}
        print("NEMAR_BATCHED_PASSES=%s ATen additions without / with the term:" % batched, adds(off['events']), adds(on['events']))
        assert len(off['events']) > 20 and any('_MindLoss' in k for k in on['events']), "the profile holds no events: the comparison would show nothing"
        assert adds(off['events']) == adds(on['events'])
        assert on['calls']['add2'] == off['calls'].get('add2', 0) + 1


def test_step_graph_replay_equals_eager_with_the_term_on(tmp_path):
    """the term makes no host sync and no allocation outside the caching allocator, and needs no static buffer beyond the two images':
    three replays of the captured step (NEMARModel.enable_step_graph) are three eager steps with the step parameters in device memory,
    bit for bit"""
    from nemar_amd import ops
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    opt = _opt(tmp_path, extra=ON)
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
    assert l_eager[0]['MIND_R'] > 0 and l_eager[0] != l_eager[-1]                     # (the steps do move the losses)
    assert l_eager == l_graph, (l_eager, l_graph)
    assert all(torch.equal(a, b) for a, b in zip(p_eager, p_graph))
