"""Two records of the EPE loss (csrc/epe.hip, --lambda_epe), no gate on either:

  timing    nemar_epe_loss_fwd / _bwd next to nemar_registration_error — the meter whose residual the loss differentiates — as they stand
            in this tree, at 8 x 256^2 (the training size) and 2 x 1024^2, UNet offsets and affine dtheta.  The prediction is a smooth
            field of a few pixels against a smooth ground truth of the same size, so the gathers land next to the pixel, as they do for
            any registration worth training on.  Compulsory bytes: the loss reads 16 B/px (the prediction and the field; an affine
            prediction: 8), the gradient writes 8 more for UNet offsets; the meter reads 16 B/px too.  One process; the calls ALTERNATE
            inside every round, each timed by device events around `--calls` back-to-back calls; a figure is the MEDIAN over `--rounds`
            rounds (min and max are printed: the spread).
  training  the seeded `--misalign both --synthetic_pairs mapped` UNet run of tools/misalign_record.py, `--steps` steps, once with
            --lambda_epe 0 and once with it on; afterwards registration/epe_px on `--eval_batches` further batches of the same seeded
            stream (new crops and new misalignments, the same ones for both runs), which no step trained on.

    python tools/epe_record.py [--steps 300] [--lambda_epe 10] [--out tools/profiles/epe_loss.txt]"""
import argparse
import ctypes
import math
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = ((8, 256, 256), (2, 1024, 1024))
_record = [None]


def emit(line):
    print(line)
    sys.stdout.flush()
    if _record[0] is not None:
        _record[0].write(line + '\n')
        _record[0].flush()


def _smooth(N, H, W, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    d = F.interpolate(torch.randn(N, 2, 4, 5, device=dev, generator=g), size=(H, W), mode='bicubic')
    return (d / d.abs().max()).contiguous()


def timing(rounds, calls):
    from nemar_amd import _lib, ops
    lib, dev = _lib.load(), torch.device('cuda:0')
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    emit('# timing: rounds %d x %d calls, medians [min .. max]; GB/s over the compulsory bytes' % (rounds, calls))
    for (N, H, W) in SHAPES:
        gt = (_smooth(N, H, W, 1, dev) * 6.0).contiguous()                         # a ground truth of up to 6 px
        offsets = (_smooth(N, H, W, 2, dev) * (8.0 / W)).contiguous()              # offsets of up to 4 px, normalised units
        dtheta = ((torch.rand(N, 6, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) - 0.5) * 0.04).contiguous()
        one = torch.ones(1, device=dev)
        wsb, wsb_m = lib.epe_loss_workspace(N, H, W), lib.registration_error_workspace(N, H, W)
        ws, ws_m = torch.empty(wsb // 4 + 1, dtype=torch.int32, device=dev), torch.empty(wsb_m // 4 + 1, dtype=torch.int32, device=dev)
        for label, pred, mode, bpp_f, bpp_b in (('unet', offsets, ops.GRID_UNET, 16, 24), ('affine', dtheta, ops.GRID_AFFINE, 8, 8)):
            loss, gpred, rows = torch.empty(1, device=dev), torch.empty_like(pred), torch.empty(N, 6, device=dev)
            variants = [
                ('epe_loss_fwd', lambda: lib.epe_loss_fwd(P(pred), mode, P(gt), 0.01, 1.0, P(loss), 0, P(ws), wsb, N, H, W, st()), bpp_f),
                ('epe_loss_bwd', lambda: lib.epe_loss_bwd(P(pred), mode, P(gt), 0.01, P(one), 1.0, P(gpred), 0, P(ws), wsb, N, H, W, st()), bpp_b),
                ('registration_error', lambda: lib.registration_error(P(pred), mode, P(gt), P(rows), P(ws_m), wsb_m, N, H, W, st()),
                 16 if mode == ops.GRID_UNET else 8),
            ]
            for _, fn, _ in variants:                                         # warm-up: code objects, clocks
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {name: [] for name, _, _ in variants}
            for _ in range(rounds):
                for name, fn, _ in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(calls):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1) * 1e3 / calls)      # us per call
            valid, sum_r = rows[:, 0].sum().item(), rows[:, 1].sum().item()
            emit('%d x %d x %d %-6s  (loss %.6f px over all pixels; the meter: epe_px %.6f over the %.4f that stay inside)'
                 % (N, H, W, label, float(loss), sum_r / max(valid, 1.0), valid / (N * H * W)))
            for name, _, bpp in variants:
                t = sorted(times[name])
                med = statistics.median(t)
                emit('  %-20s %9.1f us [%9.1f .. %9.1f]   %7.1f GB/s over %d B/px' % (name, med, t[0], t[-1], N * H * W * bpp / med / 1e3, bpp))


def training(lam, eps, steps, batch, eval_batches, ck):
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    from nemar_amd.train import _Options
    size = 256
    opt = _Options().parse(['--model', 'nemar', '--stn_type', 'unet', '--netG', 'resnet_3blocks', '--ngf', '16', '--ndf', '16', '--dataset_mode',
                            'gpupairs', '--dataroot', 'synthetic', '--synthetic_pairs', 'mapped', '--misalign', 'both', '--img_height', str(size),
                            '--img_width', str(size), '--crop_size', str(size), '--load_size', str(size + 30), '--batch_size', str(batch),
                            '--pool_size_pairs', '64', '--checkpoints_dir', ck, '--name', 'epe_%g' % lam, '--gpu_ids', '0', '--lambda_smooth', '10',
                            '--lambda_epe', str(lam), '--epe_eps', str(eps)], quiet=True)
    torch.manual_seed(7)
    dataset = create_dataset(opt)
    model = create_model(opt)
    model.setup(opt)
    step = 0
    while step < steps:
        for data in dataset:
            model.set_input(data)
            model.optimize_parameters()
            step += 1
            if step >= steps:
                break
    losses = model.get_current_losses()
    rows, seen = [], 0
    for data in dataset:                                                      # further batches of the stream: never trained on
        model.set_input(data)
        model.test()
        rows.append(model.registration_error())
        seen += 1
        if seen >= eval_batches:
            break
    emit('  --lambda_epe %-5g --epe_eps %g: after %d steps losses %s' % (lam, eps, steps, '  '.join('%s %.4f' % kv for kv in losses.items())))
    mean = lambda k: statistics.mean(r[k] for r in rows)
    assert all(math.isfinite(r['epe_px']) for r in rows)
    emit('    held-out: registration/epe_px %8.4f (before %.4f)   max_px %.3f   fold_frac %.5f   valid_frac %.4f'
         % (mean('epe_px'), mean('epe_before_px'), max(r['max_px'] for r in rows), mean('fold_frac'), mean('valid_frac')))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--eval_batches', type=int, default=4)
    ap.add_argument('--lambda_epe', type=float, default=10.0)
    ap.add_argument('--epe_eps', type=float, default=0.01)
    ap.add_argument('--skip_training', action='store_true')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'profiles', 'epe_loss.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('epe_record: no GPU — a timing from anything else would say nothing')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    _record[0] = open(a.out, 'w')
    emit('# %s' % torch.cuda.get_device_name(0))
    timing(a.rounds, a.calls)
    if not a.skip_training:
        emit('# training: UNet STN, 256 x 256, batch %d, ngf = ndf = 16, resnet_3blocks, --misalign both (defaults), mapped synthetic pairs, seed 7, '
             '--lambda_smooth 10; read-out on %d further batches of the stream' % (a.batch, a.eval_batches))
        with tempfile.TemporaryDirectory() as ck:
            for lam in (0.0, a.lambda_epe):
                training(lam, a.epe_eps, a.steps, a.batch, a.eval_batches, ck)
    _record[0].close()
