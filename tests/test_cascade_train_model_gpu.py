"""`-m gpu`: training the cascade — UnetSTN.predict(passes=K) in the training step (--train_passes K): absent by default with nothing
changed bit for bit, on as K looks with shared weights whose composite every term acts on, in both forward orders (each in a fresh child
process), together with --stn_integrate, --lambda_fold and --lambda_epe, and under the captured step graph.  The smallest UNet-STN
configuration of the model tests (tests/test_integrate_model_gpu.py); random weights: nothing is trained, no number has to be good."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 256                  # (the UNet STN's seven poolings need 256 x 256)
MOVING = ['--stn_no_identity_init']      # (the layer that predicts the field starts at zero otherwise: no gradient behind it on step 1)


def _argv(tmp, stn='unet', size=SIZE, extra=()):
    return ['--model', 'nemar', '--stn_type', stn, '--netG', 'resnet_3blocks', '--ngf', '8', '--ndf', '8', '--dataset_mode', 'gpupairs',
            '--dataroot', 'synthetic', '--img_height', str(size), '--img_width', str(size), '--crop_size', str(size), '--load_size',
            str(size + 12), '--batch_size', '2', '--pool_size_pairs', '6', '--checkpoints_dir', str(tmp), '--name', 'cascade', '--no_dropout',
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


@pytest.fixture(scope="module")
def single(tmp_path_factory, data):
    """the single look: what every K > 1 run is compared with"""
    return _two_steps(_opt(tmp_path_factory.mktemp('single'), extra=MOVING), data)


def test_absent_by_default_and_one_pass_changes_nothing(tmp_path, data, single):
    opt = _opt(tmp_path, extra=MOVING)
    assert not hasattr(opt, 'train_passes'), "the default option set carries the flag: the frozen option sets would change"
    m0, l0, p0 = single
    m1, l1, p1 = _two_steps(_opt(tmp_path, extra=MOVING + ['--train_passes', '1']), data)
    assert m0._train_passes == 1 and m1._train_passes == 1 and not hasattr(m1.netR, 'last_pass_predictions')
    assert l0 == l1 and len(p0) == len(p1) and all(torch.equal(a, b) for a, b in zip(p0, p1))


def _recomposed(netR, fields):
    with torch.no_grad():
        acc = fields[0]
        for nxt in fields[1:]:
            acc = netR.compose(acc, nxt)
    return acc


@pytest.mark.parametrize("K", [2, 3])
def test_k_passes_train_the_composite(tmp_path, data, single, K):
    from nemar_amd import ops
    model, losses, params = _two_steps(_opt(tmp_path, extra=MOVING + ['--train_passes', str(K)]), data)
    assert model._train_passes == K
    assert all(math.isfinite(v) for step in losses for v in step.values()), losses
    assert list(losses[0]) == list(single[1][0])                              # (no new loss name: the terms act on the composite)
    assert all(bool(torch.isfinite(p).all()) for p in params)
    fields = model.netR.last_pass_predictions
    assert len(fields) == K and all(f.shape == (2, 2, SIZE, SIZE) and not f.requires_grad for f in fields)
    assert all(float(f.abs().max()) > 0 for f in fields)
    pred, mode = model.netR.last_prediction()
    assert mode == ops.GRID_UNET and not pred.requires_grad and model.netR.last_velocity is None
    assert torch.equal(pred, _recomposed(model.netR, fields)), "the prediction is not the composite of the per-pass fields"
    dead = [name for name, p in model.netR.named_parameters() if p.grad is None or float(p.grad.abs().max()) == 0.0]
    assert not dead, "netR parameters without a gradient: %s" % dead
    assert len(params) == len(single[2]) and any(not torch.equal(a, b) for a, b in zip(params, single[2])), "the same parameters as a single look"
    # the cascade is a matter of the training step: test() and cascade() look as they always did
    model.set_input(data)
    model.cascade(2)
    assert model.netR.last_prediction()[0].shape == (2, 2, SIZE, SIZE) and bool(torch.isfinite(model.registered_real_A).all())


_CHILD = """
import json, math, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import torch
import test_cascade_train_model_gpu as T
from nemar_amd.data import create_dataset
opt = T._opt(%r, extra=%r)
torch.manual_seed(7)
data = next(iter(create_dataset(opt)))
model, losses, params = T._two_steps(opt, data)
fields = model.netR.last_pass_predictions
print(json.dumps({'batched': model._batched, 'passes': len(fields), 'losses': losses, 'names': list(losses[0]),
                  'finite': all(bool(torch.isfinite(p).all()) for p in params),
                  'composite': bool(torch.equal(model.netR.last_prediction()[0], T._recomposed(model.netR, fields))),
                  'dead': [n for n, p in model.netR.named_parameters() if float(p.grad.abs().max()) == 0.0]}))
"""

FURTHER = ['--stn_integrate', '4', '--lambda_fold', '1', '--misalign', 'both', '--synthetic_pairs', 'mapped', '--lambda_epe', '1']


@pytest.mark.parametrize("batched,extra", [('1', []), ('0', []), ('1', FURTHER)], ids=["batched", "reference_order", "integrate_fold_epe"])
def test_both_forward_orders_in_a_fresh_process(tmp_path, batched, extra):
    env = dict(os.environ, NEMAR_BATCHED_PASSES=batched)
    code = _CHILD % (ROOT, os.path.join(ROOT, 'tests'), str(tmp_path), MOVING + ['--train_passes', '2'] + extra)
    r = subprocess.run(['timeout', '-k', '10', '300', sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=320)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out['batched'] == (batched == '1') and out['passes'] == 2 and out['finite'] and out['composite'] and not out['dead'], out
    assert all(math.isfinite(v) for step in out['losses'] for v in step.values()), out
    assert ('fold' in out['names']) == bool(extra) and ('EPE' in out['names']) == bool(extra)


def test_step_graph_replay_equals_eager(tmp_path, data):
    """the compose gradient makes no host sync and no allocation outside the caching allocator, and its accumulator comes back zero:
    three replays of the captured step (NEMARModel.enable_step_graph) are three eager steps with the step parameters in device memory,
    bit for bit, at K = 2"""
    from nemar_amd import ops
    from nemar_amd.models import create_model
    opt = _opt(tmp_path, extra=MOVING + ['--train_passes', '2'])
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
    assert l_eager == l_graph, (l_eager, l_graph)
    assert all(torch.equal(a, b) for a, b in zip(p_eager, p_graph))


def test_what_the_flag_refuses(tmp_path):
    from nemar_amd.models import create_model
    with pytest.raises(ValueError, match="train_passes 2 needs --stn_type unet"):
        create_model(_opt(tmp_path, stn='affine', size=64, extra=['--train_passes', '2']))
    create_model(_opt(tmp_path, stn='affine', size=64, extra=['--train_passes', '1']))      # a single look: any STN
    for k in ('0', '9'):
        with pytest.raises(ValueError, match="train_passes %s.*1 .. 8" % k):
            create_model(_opt(tmp_path, extra=['--train_passes', k]))
    from nemar_amd.models.stn.unet_stn import UnetSTN
    with pytest.raises(ValueError, match="passes 9"):
        UnetSTN.predict(None, None, None, passes=9)
