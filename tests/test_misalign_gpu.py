"""`-m gpu`: known-misalignment training pairs through the dataset, the model's registration-error read-out and the training monitor."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import deform_cases as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _argv(tmp, stn='affine', size=64, extra=()):
    return ['--model', 'nemar', '--stn_type', stn, '--netG', 'resnet_3blocks', '--ngf', '8', '--ndf', '8', '--dataset_mode', 'gpupairs',
            '--dataroot', 'synthetic', '--img_height', str(size), '--img_width', str(size), '--crop_size', str(size), '--load_size',
            str(size + 12), '--batch_size', '2', '--pool_size_pairs', '6', '--checkpoints_dir', str(tmp), '--name', 'mis', '--no_dropout',
            '--print_freq', '2', '--niter', '1', '--niter_decay', '0', '--save_epoch_freq', '100', '--gpu_ids', '0', *extra]


def _opt(tmp, stn='affine', size=64, extra=()):
    from nemar_amd.train import _Options
    return _Options().parse(_argv(tmp, stn, size, extra), quiet=True)


def _batches(opt, n=2):
    from nemar_amd.data import create_dataset
    ds = create_dataset(opt)
    out = []
    for data in ds:
        out.append((data, ds.dataset._last_params.copy()))
        if len(out) == n:
            break
    return out


def test_misalign_none_is_todays_batch(tmp_path):
    plain = _batches(_opt(tmp_path))
    spelled = _batches(_opt(tmp_path, extra=['--misalign', 'none', '--misalign_max_px', '8.0', '--misalign_rot_deg', '5.0', '--misalign_scale',
                                             '0.05', '--misalign_grid', '6', '--synthetic_pairs', 'independent']))
    for (a, pa), (b, pb) in zip(plain, spelled):
        assert set(a) == set(b) == {'A', 'B', 'A_paths', 'B_paths'}
        assert torch.equal(a['A'], b['A']) and torch.equal(a['B'], b['B']) and np.array_equal(pa, pb) and a['A_paths'] == b['A_paths']


@pytest.mark.parametrize("mode", ["affine", "elastic", "both"])
def test_misalign_batches(tmp_path, mode):
    flags = ['--misalign', mode, '--misalign_max_px', '5', '--misalign_rot_deg', '4', '--misalign_scale', '0.08', '--misalign_grid', '5']
    plain = _batches(_opt(tmp_path))
    mis = _batches(_opt(tmp_path, extra=flags))
    again = _batches(_opt(tmp_path, extra=flags))
    opt_r1 = _opt(tmp_path, extra=flags)
    opt_r1.shard_rank, opt_r1.shard_world, opt_r1.batch_size = 1, 2, 4
    rank1 = _batches(opt_r1)
    # max |g| from the flags: |(M - I)(q - c)| <= (|s - 1| + s * 2 sin(rot / 2)) * half-diagonal, + the translation, + the lattice (a
    # convex combination of control points) — the latter two up to max_px per component
    half_diag = math.hypot(63, 63) / 2
    bound = 0.0
    if mode in ('affine', 'both'):
        bound += (0.08 + 1.08 * 2 * math.sin(math.radians(4) / 2)) * half_diag + math.sqrt(2) * 5
    if mode in ('elastic', 'both'):
        bound += math.sqrt(2) * 5
    for (p, pp), (m, pm), (a, _), (r, _) in zip(plain, mis, again, rank1):
        assert np.array_equal(pp, pm) and torch.equal(p['B'], m['B'])          # the crop / flip stream and modality B are untouched
        assert not torch.equal(p['A'], m['A'])
        g = m['gt_field']
        assert g.shape == (2, 2, 64, 64) and g.dtype == torch.float32 and g.is_cuda
        norm = g.double().pow(2).sum(1).sqrt()
        assert 0.0 < float(norm.max()) <= bound * (1 + 1e-6), (float(norm.max()), bound)
        assert float(m['A'].min()) >= -1.0 and float(m['A'].max()) <= 1.0
        assert torch.equal(g, a['gt_field']) and torch.equal(m['A'], a['A'])    # one seed, one batch
        assert not torch.equal(g, r['gt_field'])                                # another shard rank draws other fields
        # A is the plain crop of the same pair read at q + g(q)
        ds_A = (p['A'].double().cpu().numpy() + 1) / 2
        for b in range(2):
            want = (D._bilinear_clamped(ds_A[b], np.arange(64.0)[None, :] + g[b, 0].double().cpu().numpy(),
                                        np.arange(64.0)[:, None] + g[b, 1].double().cpu().numpy()) - 0.5) / 0.5
            assert np.abs(m['A'][b].double().cpu().numpy() - want).max() <= 4e-6 * 76


def test_mapped_synthetic_pairs_share_structure(tmp_path):
    from nemar_amd.data import create_dataset
    ds = create_dataset(_opt(tmp_path, extra=['--synthetic_pairs', 'mapped'])).dataset
    A, B = ds.pool_A, ds.pool_B
    assert A.shape == B.shape == (6, 3, 76, 76) and float(A.min()) >= 0 and float(A.max()) <= 1 and float(B.min()) >= 0 and float(B.max()) <= 1
    assert torch.equal(B, ds._remap(A))                      # B is a function of A, pixel by pixel
    # band-limited: neighbouring pixels differ far less than independent noise would (mean |difference| of U[0,1] noise: 1/3)
    assert float((A[..., 1:] - A[..., :-1]).abs().mean()) < 0.05
    ind = create_dataset(_opt(tmp_path)).dataset
    assert float((ind.pool_A[..., 1:] - ind.pool_A[..., :-1]).abs().mean()) > 0.3


@pytest.mark.parametrize("stn,size", [("affine", 64), ("unet", 256)])       # (the UNet STN's seven poolings need 256 x 256)
def test_model_registration_error(tmp_path, stn, size):
    from nemar_amd import ops
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    opt = _opt(tmp_path, stn, size, extra=['--misalign', 'both', '--synthetic_pairs', 'mapped'])
    data = next(iter(create_dataset(opt)))
    model = create_model(opt)
    model.setup(opt)
    model.set_input(data)
    assert model.gt_field is data['gt_field'] or torch.equal(model.gt_field, data['gt_field'])
    model.test()
    pred, mode = model.netR.last_prediction()
    assert mode == (ops.GRID_AFFINE if stn == 'affine' else ops.GRID_UNET)
    assert all(math.isfinite(v) for v in model.registration_error().values())      # the forward pass's own prediction
    pred.zero_()                                               # a known prediction: zero dtheta / zero offsets
    got = model.registration_error()
    want, _, _ = D.ref_meter(np.zeros(tuple(pred.shape)), mode, data['gt_field'].cpu().numpy())
    px = 2 * size * size
    ref = {'epe_px': want[:, 1].sum() / want[:, 0].sum(), 'epe_before_px': want[:, 3].sum() / px, 'max_px': want[:, 2].max(),
           'fold_frac': want[:, 4].sum() / want[:, 5].sum(), 'valid_frac': want[:, 0].sum() / px}
    assert set(got) == set(ref) and all(isinstance(v, float) for v in got.values())
    for k in ('epe_px', 'epe_before_px', 'max_px'):
        assert abs(got[k] - ref[k]) <= 2e-5 * abs(ref[k]) + 1e-6, (k, got[k], ref[k])
    assert got['fold_frac'] == ref['fold_frac'] == 0.0 and got['valid_frac'] == ref['valid_frac']
    # after a training step as well, and an error without a ground-truth field
    model.optimize_parameters()
    assert math.isfinite(model.registration_error()['epe_px'])
    model.set_input({k: v for k, v in data.items() if k != 'gt_field'})
    with pytest.raises(RuntimeError, match='gt_field'):
        model.registration_error()


def _scalars(tmp):
    rows = [json.loads(l) for l in open(os.path.join(str(tmp), 'mis', 'mis_tensorboard_logs', 'scalars.jsonl'))]
    by = {}
    for r in rows:
        by.setdefault(r['tag'], []).append((r['step'], r['value']))
    return by


@pytest.mark.parametrize("stn,size", [("affine", 64), ("unet", 256)])
def test_train_loop_reports_registration_and_the_meter_only_reads(tmp_path, stn, size):
    """three iterations in a child process; the same run with --tbvis_disable_report_registration gives the same losses bit for bit"""
    extra = ['--misalign', 'both', '--synthetic_pairs', 'mapped', '--enable_tbvis', '--tbvis_iteration_update_rate', '1', '--seed', '7',
             '--tbvis_disable_report_weights']
    runs = {}
    for name, more in (('on', []), ('off', ['--tbvis_disable_report_registration'])):
        tmp = tmp_path / name
        r = subprocess.run([sys.executable, '-m', 'nemar_amd.train', *_argv(tmp, stn, size, extra + more)], cwd=ROOT, capture_output=True,
                           text=True, timeout=420)
        assert r.returncode == 0, r.stderr[-3000:]
        runs[name] = _scalars(tmp)
    on, off = runs['on'], runs['off']
    tags = ['registration/epe_px', 'registration/epe_before_px', 'registration/max_px', 'registration/fold_frac', 'registration/valid_frac']
    assert not [t for t in off if t.startswith('registration/')]
    for t in tags:
        assert len(on[t]) == 3 and all(math.isfinite(v) for _, v in on[t]), (t, on.get(t))
    assert all(v > 0 for _, v in on['registration/epe_before_px'])
    assert all(0.0 <= v <= 1.0 for _, v in on['registration/valid_frac'] + on['registration/fold_frac'])
    losses = [t for t in on if t.startswith('loss/')]
    assert len(losses) == 8 and all(len(on[t]) == 3 for t in losses)
    for t in losses:
        assert on[t] == off[t], (t, on[t], off[t])
