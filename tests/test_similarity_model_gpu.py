"""`-m gpu`: the intensity-agreement read-out through the model and the command line — netR.similarity,
NEMARModel.register(similarity=True), NEMARModel.cascade(passes, similarity=True) and `python -m nemar_amd.register --similarity` in a
fresh process on a directory that holds A.npy and B.npy only.  Same small nets as tests/test_regularity_model_gpu.py.  Random weights:
nothing is trained, no number has to be good."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = (96, 128)
KEYS = ['entropy_fixed', 'entropy_joint', 'entropy_moving', 'mae', 'mi', 'mse', 'ncc', 'nmi', 'valid']


def _argv(tmp, stn, size):
    return ['--model', 'nemar', '--stn_type', stn, '--netG', 'resnet_3blocks', '--ngf', '8', '--img_height', str(size), '--img_width', str(size),
            '--batch_size', '2', '--checkpoints_dir', str(tmp), '--name', 'sim', '--no_dropout', '--gpu_ids', '0']


def _pairs(seed):
    """two seeded float pairs at FULL in [0, 1]: smooth textures, B a nonlinear function of a shifted A (another "modality")"""
    g = torch.Generator().manual_seed(seed)
    up = lambda t: torch.nn.functional.interpolate(t, size=FULL, mode='bicubic', align_corners=False)
    A = up(torch.rand(2, 3, 8, 10, generator=g)).clamp_(0, 1)
    B = (1.0 - torch.roll(A, (3, -4), (2, 3))) ** 2
    return A.numpy().astype(np.float32), B.numpy().astype(np.float32)


def _same(a, b):
    """two (counts, moments) read-outs, bit for bit"""
    return all(x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.cpu().numpy().view(np.uint32), y.cpu().numpy().view(np.uint32))
               for x, y in zip(a, b))


def _model(tmp_path, stn, size):
    from nemar_amd import ops
    from nemar_amd.models import create_model
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
    return model, opt


@pytest.mark.parametrize("stn,size", [("affine", 64), ("unet", 256)])       # (the UNet STN's seven poolings need 256 x 256: 64 x 64 has no such net)
def test_model_similarity(tmp_path, stn, size):
    from nemar_amd import ops
    from nemar_amd.register import network_batch
    model, opt = _model(tmp_path, stn, size)
    A, B = _pairs(3)
    d_A, d_B = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    batch = network_batch(d_A, d_B, [0, 1], opt)
    model.set_input(batch)
    model.test()
    pred = model.netR.last_prediction()
    P1, mode = pred[0].clone(), pred[1]
    assert float(P1.abs().max()) > 1e-3, "the prediction does not move anything: the test would show nothing"

    # netR.similarity is ops.joint_histogram of the same tensors
    assert _same(model.netR.similarity(pred, d_A, d_B, 16, (0.0, 1.0), (0.0, 1.0)), ops.joint_histogram(P1, mode, d_A, d_B, 16, (0.0, 1.0), (0.0, 1.0)))
    assert _same(model.netR.similarity(P1, model.real_A, model.real_B), ops.joint_histogram(P1, mode, model.real_A, model.real_B))
    counts, none = model.netR.similarity(pred, d_A, d_B, moments=False)
    assert none is None and counts.shape == (2, 32, 32) and int(counts.sum()) > 0

    # register(): the defaults return what a call without the new arguments returns; with the flag, before (the identity) and after
    plain = model.register(d_A, d_B, translate=False)
    again = model.register(d_A, d_B, translate=False, similarity=False)
    assert sorted(plain) == sorted(again) == ['offsets', 'registered_A'] and all(torch.equal(plain[k], again[k]) for k in plain)
    out = model.register(d_A, d_B, translate=False, similarity=True, bins=16, intensity_range=(0.0, 1.0))
    assert sorted(out) == ['offsets', 'registered_A', 'similarity'] and all(torch.equal(plain[k], out[k]) for k in plain)
    assert sorted(out['similarity']) == ['after', 'before']
    assert _same(out['similarity']['after'], ops.joint_histogram(out['offsets'], mode, d_A, d_B, 16, (0.0, 1.0), (0.0, 1.0)))
    zeros = torch.zeros(2, 6, device='cuda')
    assert _same(out['similarity']['before'], ops.joint_histogram(zeros, ops.GRID_AFFINE, d_A, d_B, 16, (0.0, 1.0), (0.0, 1.0)))
    assert int(out['similarity']['before'][0].sum()) == 2 * FULL[0] * FULL[1]            # the identity counts every pixel
    assert not _same(out['similarity']['before'], out['similarity']['after'])
    summary = ops.similarity_summary(*out['similarity']['after'])
    assert sorted(summary) == KEYS and all(summary[k] is not None for k in KEYS)
    with pytest.raises(ValueError, match='full_B'):
        model.register(d_A, None, translate=False, similarity=True)

    # cascade(): None as before by default; one (counts, moments) per pass with the flag, at the network's size
    model.set_input(batch)
    assert model.cascade(2) is None
    composite = model.netR.last_prediction()[0].clone()
    model.set_input(batch)
    per_pass = model.cascade(2, similarity=True)
    assert torch.equal(model.netR.last_prediction()[0], composite), "the read-out changed the cascade"
    assert len(per_pass) == 2 and all(len(p) == 2 for p in per_pass)
    assert _same(per_pass[0], ops.joint_histogram(P1, mode, model.real_A, model.real_B))
    assert _same(per_pass[1], model.netR.similarity(model.netR.last_prediction(), model.real_A, model.real_B))
    assert not _same(per_pass[0], per_pass[1])
    model.set_input(batch)
    both = model.cascade(2, regularity=True, similarity=True, bins=16)
    assert sorted(both) == ['regularity', 'similarity'] and len(both['regularity']) == len(both['similarity']) == 2
    assert both['similarity'][0][0].shape == (2, 16, 16)


def test_command_line_needs_images_only(tmp_path):
    from nemar_amd import ops
    from nemar_amd.register import network_batch
    stn, size = 'affine', 64
    model, opt = _model(tmp_path, stn, size)
    A, B = _pairs(3)
    d_A, d_B = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    batch = network_batch(d_A, d_B, [0, 1], opt)
    model.set_input(batch)
    per_pass = model.cascade(2, similarity=True, bins=16)
    want = model.register(d_A, d_B, translate=False, similarity=True, bins=16, intensity_range=(0.0, 1.0))['similarity']
    want = {k: ops.similarity_summary(*v) for k, v in want.items()}
    model.save_networks('latest')
    root, res = tmp_path / 'data', tmp_path / 'r'
    os.makedirs(root)
    np.save(root / 'A.npy', A)
    np.save(root / 'B.npy', B)
    r = subprocess.run(['timeout', '-k', '10', '400', sys.executable, '-m', 'nemar_amd.register', *_argv(tmp_path, stn, size), '--dataroot', str(root),
                        '--results_dir', str(res), '--epoch', 'latest', '--passes', '2', '--similarity', '--bins', '16'],
                       cwd=ROOT, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'registered 2 pairs' in r.stdout
    assert sorted(os.listdir(res / 'sim')) == ['offsets.npy', 'registered_A.npy', 'similarity.json']
    told = json.load(open(res / 'sim' / 'similarity.json'))
    assert sorted(told) == ['after', 'before', 'per_pass'] and sorted(told['after']) == sorted(told['before']) == KEYS
    assert told.pop('per_pass') == [ops.similarity_summary(*p) for p in per_pass]
    assert told == want
    assert ', MI %.4f -> %.4f' % (want['before']['mi'], want['after']['mi']) in r.stdout
