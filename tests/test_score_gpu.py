"""`-m gpu`: nemar_label_overlap and nemar_map_points (csrc/score.hip) on the gfx950 library — the bodies of tests/score_cases.py that
tests/test_score_emu.py runs on the emulator, at larger shapes too — and the layers above them: NEMARModel.register() with labels and
landmarks against numpy over its own outputs, and `python -m nemar_amd.register` in a fresh process against register()."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import score_cases as S
from backends import HipBackend

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [S.GRID_UNET, S.GRID_AFFINE]
LARGE = [((256, 256), (1024, 1024), None, 3), ((128, 160), (515, 770), (400, 600), 3)]      # test_register_gpu.py's


@pytest.fixture(scope="module")
def be(hip_lib):
    return HipBackend(hip_lib)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", S.ALL_SIZES + S.THIN + [S.ONE_TEXEL_FIELD] + LARGE, ids=str)
def test_exact_against_the_librarys_warp(be, size, mode):
    S.case_exact(be, size, mode)


@pytest.mark.parametrize("mode", MODES)
def test_exact_where_the_field_leaves_the_source(be, mode):
    S.case_exact(be, S.LEAVES_SOURCE, mode, amp=1.5)
    S.case_exact(be, ((64, 64), (512, 512), (300, 200), 3), mode, amp=1.5)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", S.ALL_SIZES + LARGE, ids=str)
def test_against_float64(be, size, mode):
    S.case_float64(be, size, mode)


@pytest.mark.parametrize("K", [1, 5, 64, 1024])
@pytest.mark.parametrize("kind", S.KINDS)
def test_label_content(be, kind, K):
    S.case_content(be, kind, K)


@pytest.mark.parametrize("size", LARGE, ids=str)
@pytest.mark.parametrize("kind,K", [("random", 1024), ("blocky", 64), ("single", 5)])
def test_label_content_large(be, kind, K, size):
    S.case_content(be, kind, K, size=size)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind,K", [("random", 5), ("blocky", 64), ("single", 1024)])
def test_values_of_no_class_are_ignored(be, kind, K, mode):
    S.case_content(be, kind, K, mode, junk=True)
    S.case_content(be, kind, K, mode, size=LARGE[1], junk=True)


def test_identity(be):
    S.case_identity(be)
    S.case_identity(be, hw=(16, 64), K=1, N=1)
    S.case_identity(be, hw=(515, 770), K=64, N=3)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size,N", [(S.UPSAMPLING[0], 1), (S.UPSAMPLING[3], 3), (S.EQUAL, 3), (S.DOWN, 1), (LARGE[0], 3)], ids=str)
def test_repeatable_overwritten_unaligned(be, size, N, mode):
    S.case_repeatable_unaligned(be, size, mode, N=N)


def test_refusals(be):
    S.case_refusals(be)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", [S.UPSAMPLING[0], S.UPSAMPLING[4], S.EQUAL, S.DOWN, S.ONE_TEXEL_FIELD, S.THIN[0], S.THIN[1]] + LARGE, ids=str)
def test_points_agree_with_the_grid(be, size, mode):
    S.case_points(be, size, mode)


@pytest.mark.parametrize("mode", MODES)
def test_points_missing_annotations_and_counts(be, mode):
    S.case_points_edges(be, mode)


# ---- through the model and the command line -------------------------------------------------------------------------------------------
FULL = (131, 203)
K = 8
P = 300


def _argv(tmp, stn, size):
    return ['--model', 'nemar', '--stn_type', stn, '--netG', 'resnet_3blocks', '--ngf', '8', '--img_height', str(size), '--img_width', str(size),
            '--batch_size', '2', '--checkpoints_dir', str(tmp), '--name', 'reg', '--no_dropout', '--gpu_ids', '0']


def _data(seed):
    """two seeded pairs at FULL, blocky 8-class label maps of both modalities, P point pairs a few pixels apart (one of them missing)"""
    g = torch.Generator().manual_seed(seed)
    up = lambda t: torch.nn.functional.interpolate(t, size=FULL, mode='bicubic', align_corners=False)
    A = up(torch.rand(2, 3, 16, 20, generator=g)).clamp_(0, 1).numpy().astype(np.float32)
    B = up(torch.rand(2, 3, 16, 20, generator=g)).clamp_(0, 1).numpy().astype(np.float32)
    labels_A = S.label_map("blocky", seed, 2, *FULL, K).astype(np.int16)
    labels_B = np.roll(labels_A, (3, -5), (1, 2))                       # the same anatomy, displaced: a real share of agreement
    rng = np.random.default_rng(seed)
    lm_B = (rng.random((2, P, 2)) * [FULL[1], FULL[0]] - 0.5).astype(np.float32)
    lm_A = (lm_B + rng.normal(0, 4, lm_B.shape)).astype(np.float32)
    lm_A[0, 7], lm_B[1, 11, 0] = np.nan, np.nan
    return A, B, labels_A, labels_B, lm_A, lm_B


def _tre(S_of, lm_A, dtype):
    return np.linalg.norm(S_of.astype(dtype) - lm_A.astype(dtype), axis=-1)


@pytest.mark.parametrize("stn,size", [("affine", 64), ("unet", 256)])       # (the UNet STN's seven poolings need 256 x 256: 64 x 64 has no such net)
def test_model_register_scores_and_command_line(tmp_path, stn, size):
    """register() with labels and landmarks: 'overlap' == numpy counts over its own 'registered_labels_A', 'tre_px' within the point rule of
    the float64 evaluation of its own 'offsets'; nothing changes without the new arguments; scores.json of a fresh process == the
    same numbers from register().  Random weights: nothing is trained, no score has to improve."""
    from nemar_amd import ops
    from nemar_amd.models import create_model
    from nemar_amd.register import network_batch, score_summary
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
    A, B, labels_A, labels_B, lm_A, lm_B = _data(3)
    d_A, d_B = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    d_la, d_lb = (torch.from_numpy(l.astype(np.float32)).cuda()[:, None] for l in (labels_A, labels_B))
    model.set_input(network_batch(d_A, d_B, [0, 1], opt))
    model.test()
    plain = model.register(d_A, d_B, d_la, translate=False)
    assert set(plain) == {'registered_A', 'registered_labels_A', 'offsets'}
    out = model.register(d_A, d_B, d_la, translate=False, labels_B=d_lb, landmarks_A=torch.from_numpy(lm_A), landmarks_B=torch.from_numpy(lm_B))
    assert set(out) == set(plain) | {'overlap', 'overlap_before', 'tre_px', 'tre_before_px'}
    for k in plain:
        assert torch.equal(plain[k], out[k]), k
    assert set(model.register(d_A, d_B, d_la, translate=False, labels_B=d_lb)) == set(plain) | {'overlap', 'overlap_before'}
    assert set(model.register(d_A, d_B, translate=False, labels_B=d_lb, landmarks_A=torch.from_numpy(lm_A))) == {'registered_A', 'offsets'}
    pred, mode = model.netR.last_prediction()
    p = pred.cpu().numpy()
    assert float(pred.abs().max()) > 1e-3, "the prediction does not move anything: the test would show nothing"
    # overlap: numpy over the model's own warped label map; before: the two maps as they are (equal sizes: the identity copies)
    overlap, before = out['overlap'].cpu().numpy(), out['overlap_before'].cpu().numpy()
    assert overlap.dtype == np.int32 and overlap.shape == (2, K, 3)                      # (K found on the device: 1 + the largest id)
    assert np.array_equal(overlap, S.count_np(out['registered_labels_A'].cpu().numpy()[:, 0], labels_B, K))
    assert np.array_equal(before, S.count_np(labels_A, labels_B, K))
    assert np.array_equal(model.register(d_A, d_B, d_la, translate=False, labels_B=d_lb, num_classes=11)['overlap'].cpu().numpy()[:, :K], overlap)
    # landmark distances: float64 of the model's own prediction; the yardstick is numpy's float32 evaluation of the same formula
    missing = np.isnan(lm_A).any(-1) | np.isnan(lm_B).any(-1)
    assert missing.sum() == 2
    for key, (q, m) in (('tre_px', (p, mode)), ('tre_before_px', (np.zeros((2, 6), np.float32), S.GRID_AFFINE))):
        got = out[key].cpu().numpy().astype(np.float64)
        assert got.shape == (2, P) and np.all(np.isnan(got[missing])) and np.all(np.isfinite(got[~missing]))
        clean = np.where(missing[..., None], 0, lm_B).astype(np.float32)
        want = _tre(S.ref_points(clean, q, m, *FULL, *FULL), lm_A, np.float64)
        yard = np.abs(_tre(S.ref_points(clean, q, m, *FULL, *FULL, np.float32), lm_A, np.float32) - want)[~missing].max()
        err = np.abs(got - want)[~missing].max()
        print("register %-14s %-6s kernel %.3e  numpy-fp32 %.3e  ratio %.2f" % (key, stn, err, yard, err / yard if yard else float('inf')))
        assert err <= S.MARGIN * yard, (key, err, yard)
    assert np.abs(out['tre_before_px'].cpu().numpy() - _tre(lm_B, lm_A, np.float64))[~missing].max() < 1e-3       # the identity maps p to p
    # the command line, in a fresh process, on the same two pairs
    model.save_networks('latest')
    root, res = tmp_path / 'data', tmp_path / 'results'
    os.makedirs(root)
    for name, a in (('A', A), ('B', B), ('labels_A', labels_A), ('labels_B', labels_B), ('landmarks_A', lm_A), ('landmarks_B', lm_B)):
        np.save(root / (name + '.npy'), a)
    r = subprocess.run(['timeout', '-k', '10', '400', sys.executable, '-m', 'nemar_amd.register', *_argv(tmp_path, stn, size), '--dataroot', str(root),
                        '--results_dir', str(res), '--epoch', 'latest'], cwd=ROOT, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'registered 2 pairs' in r.stdout and 'mean Dice' in r.stdout and 'mean TRE' in r.stdout and 'over %d points' % (2 * P - 2) in r.stdout
    scores = json.load(open(res / 'reg' / 'scores.json'))
    want = score_summary(before, overlap, out['tre_before_px'].cpu().numpy(), out['tre_px'].cpu().numpy())
    assert scores == json.loads(json.dumps(want)), (scores, want)
    assert scores['dice']['classes'] == list(range(K)) and scores['tre_px']['points'] == 2 * P - 2
    tot = overlap.astype(np.int64).sum(0)
    assert scores['dice']['after'] == [2.0 * int(tot[k, 0]) / int(tot[k, 1] + tot[k, 2]) for k in range(K)]
    assert np.array_equal(np.load(res / 'reg' / 'registered_labels_A.npy'), out['registered_labels_A'].cpu().numpy()[:, 0].astype(np.int16))
