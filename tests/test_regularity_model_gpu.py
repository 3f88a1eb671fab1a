"""`-m gpu`: the regularity read-out through the model and the command line — netR.regularity, NEMARModel.register(regularity=True),
NEMARModel.cascade(passes, regularity=True) and `python -m nemar_amd.register --regularity --jacobian_map` in a fresh process against the
model path bit for bit.  Same small nets as tests/test_cascade_gpu.py.  Random weights: nothing is trained, no number has to be good."""
import json
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
    return r.stdout, {n: open(res / 'reg' / n, 'rb').read() for n in sorted(os.listdir(res / 'reg'))}


def _same(a, b):
    """two (counts, stats[, det]) read-outs, bit for bit"""
    return all((x is None and y is None) or (x.shape == y.shape and x.dtype == y.dtype and
                                             np.array_equal(x.cpu().numpy().view(np.uint32), y.cpu().numpy().view(np.uint32))) for x, y in zip(a, b))


@pytest.mark.parametrize("stn,size", [("affine", 64), ("unet", 256)])       # (the UNet STN's seven poolings need 256 x 256: 64 x 64 has no such net)
def test_model_regularity_and_command_line(tmp_path, stn, size):
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

    # netR.regularity is ops.jacobian_stats of the same tensor: at the network's size by default, at any other on request
    model.set_input(batch)
    model.test()
    pred = model.netR.last_prediction()
    P1, mode = pred[0].clone(), pred[1]
    assert float(P1.abs().max()) > 1e-3, "the prediction does not move anything: the test would show nothing"
    assert _same(model.netR.regularity(pred), ops.jacobian_stats(P1, mode, (size, size)))
    assert _same(model.netR.regularity(P1, det_map=True), ops.jacobian_stats(P1, mode, (size, size), det_map=True))
    assert _same(model.netR.regularity(pred, out_hw=FULL, det_map=True), ops.jacobian_stats(P1, mode, FULL, det_map=True))
    counts, stats, det = model.netR.regularity(pred, det_map=True)
    assert counts.tolist() == [[(size - 1) ** 2, int((det[n, :-1, :-1] <= 0).sum())] for n in range(2)] and bool(torch.isfinite(stats).all())

    # register(): the defaults return what a call without the new arguments returns; regularity at full_B's size, or full_A's without it
    plain = model.register(d_A, d_B, translate=False)
    again = model.register(d_A, d_B, translate=False, regularity=False, jacobian_map=False)
    assert sorted(plain) == sorted(again) == ['offsets', 'registered_A']
    assert all(torch.equal(plain[k], again[k]) for k in plain)
    out = model.register(d_A, d_B, translate=False, regularity=True)
    assert sorted(out) == ['jac_counts', 'jac_stats', 'offsets', 'registered_A'] and all(torch.equal(plain[k], out[k]) for k in plain)
    assert _same((out['jac_counts'], out['jac_stats']), ops.jacobian_stats(out['offsets'], mode, FULL))
    out = model.register(d_A, d_B[:, :, :90, :120], translate=False, regularity=True, jacobian_map=True)
    assert _same((out['jac_counts'], out['jac_stats'], out['jacobian_det']), ops.jacobian_stats(P1, mode, (90, 120), det_map=True))
    out = model.register(d_A, None, translate=False, jacobian_map=True)                # the map implies the statistics
    assert _same((out['jac_counts'], out['jac_stats'], out['jacobian_det']), ops.jacobian_stats(P1, mode, FULL, det_map=True))

    # cascade(): None as before by default; one (counts, stats) per pass with the flag, of the accumulated transformation at the network's size
    model.set_input(batch)
    assert model.cascade(2) is None
    composite = model.netR.last_prediction()[0].clone()
    model.set_input(batch)
    per_pass = model.cascade(2, regularity=True)
    assert torch.equal(model.netR.last_prediction()[0], composite), "the read-out changed the cascade"
    assert len(per_pass) == 2 and all(len(p) == 2 for p in per_pass)
    assert _same(per_pass[0], ops.jacobian_stats(P1, mode, (size, size))[:2])
    assert _same(per_pass[1], model.netR.regularity(model.netR.last_prediction())[:2])
    assert not _same(per_pass[0], per_pass[1])
    full = model.register(d_A, d_B, translate=False, jacobian_map=True)
    model.set_input(batch)
    assert len(model.cascade(1, regularity=True)) == 1

    # the command line, in a fresh process, on the same two pairs
    model.save_networks('latest')
    root = tmp_path / 'data'
    os.makedirs(root)
    np.save(root / 'A.npy', A)
    np.save(root / 'B.npy', B)
    said0, plain_files = _run(tmp_path, stn, size, root, tmp_path / 'r0', '--passes', '2')
    said1, files = _run(tmp_path, stn, size, root, tmp_path / 'r1', '--passes', '2', '--regularity', '--jacobian_map')
    said2, stats_only = _run(tmp_path, stn, size, root, tmp_path / 'r2', '--jacobian_map')
    assert sorted(plain_files) == ['offsets.npy', 'registered_A.npy']
    assert sorted(files) == ['jacobian_det.npy', 'offsets.npy', 'registered_A.npy', 'regularity.json'] == sorted(stats_only)
    assert all(files[n] == plain_files[n] for n in plain_files), "the flags changed registered_A.npy or offsets.npy"
    assert 'folds' not in said0 and 'SDlogJ' not in said0
    want = ops.regularity_summary(full['jac_counts'], full['jac_stats'])
    assert ', folds %.2f %%, SDlogJ %.3f' % (100 * want['fold_frac'], want['log_det_std']) in said1
    told = json.loads(files['regularity.json'])
    assert told.pop('per_pass') == [ops.regularity_summary(*p) for p in per_pass]
    assert told == want
    assert 'per_pass' not in json.loads(stats_only['regularity.json'])
    det = np.load(tmp_path / 'r1' / 'reg' / 'jacobian_det.npy')
    assert det.shape == (2, *FULL) and det.dtype == np.float32
    assert np.array_equal(det.view(np.uint32), full['jacobian_det'].cpu().numpy().view(np.uint32))
