"""`-m gpu`: the boundary-distance read-out through the model and the command line — netR.surface, NEMARModel.register(surface=True)
and `python -m nemar_amd.register --surface` in a fresh process on a tiny synthetic directory.  Same small nets as
tests/test_similarity_model_gpu.py.  Random weights: nothing is trained, no number has to be good."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import surface_cases as S
from score_cases import label_map

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = (96, 128)
K = 6
D = 24
NAMES = ['asd_fm', 'asd_mf', 'assd', 'hd', 'hd95']


def _argv(tmp, stn, size):
    return ['--model', 'nemar', '--stn_type', stn, '--netG', 'resnet_3blocks', '--ngf', '8', '--img_height', str(size), '--img_width', str(size),
            '--batch_size', '2', '--checkpoints_dir', str(tmp), '--name', 'surf', '--no_dropout', '--gpu_ids', '0']


def _data(seed):
    """two seeded float pairs at FULL in [0, 1] and blocky K-class label maps of both modalities, B's the same anatomy displaced"""
    g = torch.Generator().manual_seed(seed)
    up = lambda t: torch.nn.functional.interpolate(t, size=FULL, mode='bicubic', align_corners=False)
    A = up(torch.rand(2, 3, 8, 10, generator=g)).clamp_(0, 1).numpy().astype(np.float32)
    B = up(torch.rand(2, 3, 8, 10, generator=g)).clamp_(0, 1).numpy().astype(np.float32)
    labels_A = label_map("blocky", seed, 2, *FULL, K).astype(np.int16)
    return A, B, labels_A, np.roll(labels_A, (3, -5), (1, 2))


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


def _same(a, b):
    return len(a) == len(b) and all((x is None and y is None) or (x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y)) for x, y in zip(a, b))


def _device(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a).astype(np.float32)).cuda() for a in arrays]


@pytest.mark.parametrize("stn,size", [("affine", 64), ("unet", 256)])       # (the UNet STN's seven poolings need 256 x 256: 64 x 64 has no such net)
def test_model_surface(tmp_path, stn, size):
    from nemar_amd import ops
    from nemar_amd.register import network_batch
    model, opt = _model(tmp_path, stn, size)
    A, B, labels_A, labels_B = _data(3)
    d_A, d_B, d_la, d_lb = _device(A, B, labels_A[:, None], labels_B[:, None])
    model.set_input(network_batch(d_A, d_B, [0, 1], opt))
    model.test()
    pred = model.netR.last_prediction()
    P1, mode = pred[0].clone(), pred[1]
    assert float(P1.abs().max()) > 1e-3, "the prediction does not move anything: the test would show nothing"

    # netR.surface is ops.surface_distance of the same tensors; the op against the numpy truth over the model's own warped labels
    by_hand = ops.surface_distance(P1, mode, d_la, d_lb, K, D, True)
    assert _same(model.netR.surface(pred, d_la, d_lb, K, D, True), by_hand)
    counts, hist, dist2 = by_hand
    assert counts.dtype == torch.int64 and counts.shape == (2, K, 2, 3) and hist.dtype == torch.int32 and hist.shape == (2, K, 2, D * D)
    assert dist2.dtype == torch.int32 and dist2.shape == (2, 2, *FULL) and len(ops.SURFACE_COUNT_COLUMNS) == 3
    warped = model.netR.apply(pred, [d_la], sample='nearest')[0].cpu().numpy()[:, 0]
    want = S.truth(warped, labels_B.astype(np.float32), K, D)
    for got, w in zip(by_hand, want):
        assert np.array_equal(got.cpu().numpy().astype(np.int64), w)
    none = ops.surface_distance(P1, mode, d_la[:, 0], d_lb[:, 0], K, D)         # [N,H,W] maps, no map asked for
    assert none[2] is None and _same(none[:2], by_hand[:2])
    with pytest.raises(ValueError, match='max_dist'):
        ops.surface_distance(P1, mode, d_la, d_lb, K, 129)

    # register(): without the flag the keys of before; with it, before (the identity) and after equal the op called by hand
    plain = model.register(d_A, d_B, d_la, translate=False, labels_B=d_lb, num_classes=K)
    again = model.register(d_A, d_B, d_la, translate=False, labels_B=d_lb, num_classes=K, surface=False)
    assert sorted(plain) == sorted(again) == ['offsets', 'overlap', 'overlap_before', 'registered_A', 'registered_labels_A']
    assert all(torch.equal(plain[k], again[k]) for k in plain)
    out = model.register(d_A, d_B, d_la, translate=False, labels_B=d_lb, num_classes=K, surface=True, surface_max_dist=D)
    assert sorted(out) == sorted(plain) + ['surface'] and all(torch.equal(plain[k], out[k]) for k in plain)
    assert sorted(out['surface']) == ['after', 'before']
    zeros = torch.zeros(2, 6, device='cuda')
    assert _same(out['surface']['after'], by_hand[:2])
    assert _same(out['surface']['before'], ops.surface_distance(zeros, ops.GRID_AFFINE, d_la, d_lb, K, D)[:2])
    assert not _same(out['surface']['before'], out['surface']['after'])
    mapped = model.register(d_A, d_B, d_la, translate=False, labels_B=d_lb, num_classes=K, surface=True, surface_max_dist=D, surface_map=True)
    assert sorted(mapped) == sorted(out) + ['surface_dist2'] and torch.equal(mapped['surface_dist2'], dist2)
    assert _same(mapped['surface']['after'], out['surface']['after'])
    assert out['surface']['after'][1].shape[-1] == D * D and model.register(
        d_A, d_B, d_la, translate=False, labels_B=d_lb, num_classes=K, surface=True)['surface']['after'][1].shape[-1] == 64 * 64
    summary = ops.surface_summary(*out['surface']['after'])
    assert sorted(summary['mean']) == NAMES and summary['pairs'] > 0 and summary['mean']['hd'] is not None
    for missing in (dict(labels_A=None, labels_B=d_lb, num_classes=K), dict(labels_A=d_la, labels_B=None, num_classes=K),
                    dict(labels_A=d_la, labels_B=d_lb, num_classes=None)):
        with pytest.raises(ValueError, match='surface=True needs'):
            model.register(d_A, d_B, translate=False, surface=True, **missing)


def _run(tmp_path, stn, size, root, res, *flags):
    return subprocess.run(['timeout', '-k', '10', '400', sys.executable, '-m', 'nemar_amd.register', *_argv(tmp_path, stn, size), '--dataroot', str(root),
                           '--results_dir', str(res), '--epoch', 'latest', *flags], cwd=ROOT, capture_output=True, text=True, timeout=420)


def test_command_line(tmp_path):
    """surface.json == surface_summary of register()'s tensors, with two passes (the composite is scored); without --surface the files of
    before, byte for byte"""
    from nemar_amd import ops
    from nemar_amd.register import network_batch
    stn, size = 'affine', 64
    model, opt = _model(tmp_path, stn, size)
    A, B, labels_A, labels_B = _data(3)
    d_A, d_B, d_la, d_lb = _device(A, B, labels_A[:, None], labels_B[:, None])
    model.set_input(network_batch(d_A, d_B, [0, 1], opt))
    model.cascade(2)
    out = model.register(d_A, d_B, d_la, translate=False, labels_B=d_lb, num_classes=K, surface=True, surface_max_dist=D, surface_map=True)
    want = {k: ops.surface_summary(*v) for k, v in out['surface'].items()}
    model.save_networks('latest')
    root = tmp_path / 'data'
    os.makedirs(root)
    for name, a in (('A', A), ('B', B), ('labels_A', labels_A), ('labels_B', labels_B)):
        np.save(root / (name + '.npy'), a)
    r = _run(tmp_path, stn, size, root, tmp_path / 'with', '--passes', '2', '--surface', '--surface_max_dist', str(D), '--surface_map')
    assert r.returncode == 0, r.stderr[-3000:]
    files = ['offsets.npy', 'registered_A.npy', 'registered_labels_A.npy', 'scores.json']
    assert sorted(os.listdir(tmp_path / 'with' / 'surf')) == sorted(files + ['surface.json', 'surface_dist2.npy'])
    told = json.load(open(tmp_path / 'with' / 'surf' / 'surface.json'))
    assert told == json.loads(json.dumps(want)), (told, want)
    assert sorted(told) == ['after', 'before'] and told['after']['classes'] == list(range(K)) and sorted(told['after']['per_class']) == NAMES
    assert told['before']['pairs'] > 0 and told['before']['mean']['hd'] > 0          # (the maps are 3 rows and 5 columns apart)
    assert np.array_equal(np.load(tmp_path / 'with' / 'surf' / 'surface_dist2.npy'), out['surface_dist2'].cpu().numpy())
    assert ', HD95 %.3f -> %.3f px' % (want['before']['mean']['hd95'], want['after']['mean']['hd95']) in r.stdout
    r0 = _run(tmp_path, stn, size, root, tmp_path / 'without', '--passes', '2')
    assert r0.returncode == 0, r0.stderr[-3000:]
    assert sorted(os.listdir(tmp_path / 'without' / 'surf')) == sorted(files) and 'HD95' not in r0.stdout
    for f in files:
        assert open(tmp_path / 'without' / 'surf' / f, 'rb').read() == open(tmp_path / 'with' / 'surf' / f, 'rb').read(), f


def test_command_line_without_label_files(tmp_path):
    A, B, labels_A, _ = _data(3)
    root = tmp_path / 'data'
    os.makedirs(root)
    for name, a in (('A', A), ('B', B), ('labels_A', labels_A)):
        np.save(root / (name + '.npy'), a)
    r = _run(tmp_path, 'affine', 64, root, tmp_path / 'r', '--surface')
    assert r.returncode != 0 and '--surface needs labels_A.npy and labels_B.npy' in r.stderr
    assert not os.path.exists(tmp_path / 'r')
