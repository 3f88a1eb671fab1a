"""`-m gpu`: nemar_warp_resampled_fwd (csrc/register.hip) on the gfx950 library — the bodies of tests/register_cases.py that
tests/test_register_emu.py runs on the emulator, at larger shapes too — and the layers above it: NEMARModel.register() against torch's
float64 composition of the model's own prediction, and `python -m nemar_amd.register` in a fresh process against register() bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import register_cases as R
from backends import HipBackend

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LARGE = [((256, 256), (1024, 1024), None, 3), ((128, 160), (515, 770), (400, 600), 3)]


@pytest.fixture(scope="module")
def be(hip_lib):
    return HipBackend(hip_lib)


@pytest.mark.parametrize("mode", [R.GRID_UNET, R.GRID_AFFINE])
@pytest.mark.parametrize("size", R.ALL_SIZES + LARGE, ids=str)
def test_bitwise_against_composed(be, size, mode):
    R.case_bitwise(be, size, mode)


@pytest.mark.parametrize("mode", [R.GRID_UNET, R.GRID_AFFINE])
@pytest.mark.parametrize("size", R.ALL_SIZES + LARGE, ids=str)
def test_bilinear_against_float64(be, size, mode):
    R.case_bilinear(be, size, mode)


@pytest.mark.parametrize("mode", [R.GRID_UNET, R.GRID_AFFINE])
@pytest.mark.parametrize("size", R.ALL_SIZES + LARGE, ids=str)
def test_nearest_against_float64(be, size, mode):
    R.case_nearest(be, size, mode)


def test_nearest_keeps_labels(be):
    R.case_nearest(be, R.UPSAMPLING[0], R.GRID_UNET, labels=True)
    R.case_nearest(be, R.UPSAMPLING[3], R.GRID_AFFINE, labels=True)
    R.case_nearest(be, LARGE[1], R.GRID_UNET, labels=True)


@pytest.mark.parametrize("size", [R.UPSAMPLING[0], R.UPSAMPLING[3], R.EQUAL, R.DOWN, ((12, 16), (48, 64), None, 3), LARGE[0]], ids=str)
def test_unaligned_views_and_odd_widths(be, size):
    R.case_unaligned(be, size)


@pytest.mark.parametrize("size,amp", [(((8, 12), (1, 77), (9, 13), 2), 0.15), (((8, 12), (50, 1), (9, 13), 2), 0.15),
                                      (((1, 1), (20, 36), None, 1), 0.15), (((16, 24), (67, 45), (30, 41), 3), 1.5),
                                      (((24, 24), (96, 96), None, 3), 1.5), (((64, 64), (24, 40), (50, 70), 3), 1.5),
                                      (((64, 64), (512, 512), (300, 200), 3), 1.5)], ids=str)
def test_edges_and_zero_padding(be, size, amp):
    R.case_edges(be, size, R.GRID_UNET, amp=amp)


def test_edges_affine(be):
    R.case_edges(be, ((1, 1), (1, 45), (9, 13), 2), R.GRID_AFFINE)
    R.case_edges(be, ((1, 1), (67, 45), (30, 41), 3), R.GRID_AFFINE, amp=1.5)


@pytest.mark.parametrize("mode", [R.GRID_UNET, R.GRID_AFFINE])
@pytest.mark.parametrize("size", [R.UPSAMPLING[1], R.UPSAMPLING[3], R.EQUAL, R.DOWN, ((12, 16), (50, 68), (31, 47), 2)], ids=str)
def test_vector_route_of_the_measurement_build(be, size, mode):
    R.case_vector_route(be, size, mode)


def test_repeatable(be):
    R.case_repeatable(be)
    R.case_repeatable(be, size=LARGE[0])


def test_refusals(be):
    R.case_refusals(be)


# ---- through the model and the command line -------------------------------------------------------------------------------------------
FULL = (256, 320)


def _argv(tmp, stn, size):
    return ['--model', 'nemar', '--stn_type', stn, '--netG', 'resnet_3blocks', '--ngf', '8', '--img_height', str(size), '--img_width', str(size),
            '--batch_size', '2', '--checkpoints_dir', str(tmp), '--name', 'reg', '--no_dropout', '--gpu_ids', '0']


def _pairs(seed):
    """two seeded float pairs at FULL: smooth textures (something a registration network can read) and an 8-class label map of A"""
    g = torch.Generator().manual_seed(seed)
    up = lambda t: torch.nn.functional.interpolate(t, size=FULL, mode='bicubic', align_corners=False)
    A = up(torch.rand(2, 3, 16, 20, generator=g)).clamp_(0, 1).numpy().astype(np.float32)
    B = up(torch.rand(2, 3, 16, 20, generator=g)).clamp_(0, 1).numpy().astype(np.float32)
    labels = torch.randint(0, 8, (2, FULL[0] // 8, FULL[1] // 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2).numpy().astype(np.int16)
    return A, B, labels


@pytest.mark.parametrize("stn,size", [("affine", 64), ("unet", 256)])       # (the UNet STN's seven poolings need 256 x 256: 64 x 64 has no such net)
def test_model_register_and_command_line(tmp_path, stn, size):
    from nemar_amd import ops
    from nemar_amd.models import create_model
    from nemar_amd.register import network_batch
    from nemar_amd.train import _Options
    torch.manual_seed(11)
    opt = _Options().parse(_argv(tmp_path, stn, size) + ['--ndf', '8'], quiet=True)
    model = create_model(opt)
    model.setup(opt)
    with pytest.raises(RuntimeError, match='no forward pass yet'):
        model.register(torch.zeros(2, 3, *FULL))
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
    A, B, labels = _pairs(3)
    d_A, d_B = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()          # (in [0, 1], as the command line holds them: the warp is linear)
    d_lab = torch.from_numpy(labels.astype(np.float32)).cuda()[:, None]
    model.set_input(network_batch(d_A, d_B, [0, 1], opt))
    model.test()
    out = model.register(d_A, d_B, d_lab)
    assert set(out) == {'registered_A', 'fake_RT_B', 'registered_labels_A', 'offsets'}
    assert out['registered_A'].shape == (2, 3, *FULL) and out['fake_RT_B'].shape == (2, 3, *FULL) and out['registered_labels_A'].shape == (2, 1, *FULL)
    pred, mode = model.netR.last_prediction()
    assert out['offsets'] is pred and float(pred.abs().max()) > 1e-3, "the prediction does not move anything: the test would show nothing"
    p = pred.cpu().numpy()
    R.check_bilinear(out['registered_A'].cpu().numpy().astype(np.float64), A, p, mode, *FULL, "model.register %s" % stn)
    R.check_nearest(out['registered_labels_A'].cpu().numpy().astype(np.float64), labels.astype(np.float32)[:, None], p, mode, *FULL, "model.register labels %s" % stn)
    assert set(np.unique(out['registered_labels_A'].cpu().numpy())) <= set(range(8))
    # an odd size netT cannot take: the key is absent, nothing is resized
    odd = model.register(d_A[:, :, :255, :319])
    assert set(odd) == {'registered_A', 'offsets'} and odd['registered_A'].shape == (2, 3, 255, 319)
    plain = model.register(d_A, translate=False)               # no generator pass asked for
    assert set(plain) == {'registered_A', 'offsets'} and torch.equal(plain['registered_A'], out['registered_A'])
    # the command line, in a fresh process, on the same two pairs
    model.save_networks('latest')
    root, res = tmp_path / 'data', tmp_path / 'results'
    os.makedirs(root)
    np.save(root / 'A.npy', A)
    np.save(root / 'B.npy', B)
    np.save(root / 'labels_A.npy', labels)
    r = subprocess.run(['timeout', '-k', '10', '400', sys.executable, '-m', 'nemar_amd.register', *_argv(tmp_path, stn, size), '--dataroot', str(root),
                        '--results_dir', str(res), '--epoch', 'latest'], cwd=ROOT, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'registered 2 pairs' in r.stdout
    got_A, got_l, got_o = (np.load(res / 'reg' / n) for n in ('registered_A.npy', 'registered_labels_A.npy', 'offsets.npy'))
    assert got_A.dtype == np.float32 and np.array_equal(got_A, out['registered_A'].cpu().numpy())
    assert got_l.dtype == np.int16 and got_l.shape == labels.shape and np.array_equal(got_l, out['registered_labels_A'].cpu().numpy()[:, 0].astype(np.int16))
    assert np.array_equal(got_o, pred.cpu().numpy())
