"""Two records of the fold penalty (csrc/fold.hip, --lambda_fold), no gate on either:

  timing    nemar_fold_penalty_fwd / _bwd next to nemar_smoothness_fwd / _bwd without the bilateral image, as they stand in this tree,
            at 8 x 2 x 256^2 (the training size), 2 x 2 x 1024^2 and 8 x 2 x 1024^2.  The compulsory bytes are the same (forward reads
            8 B/px; backward reads 8 and writes 8), so parity is what to expect.  One process; the four calls ALTERNATE inside every
            round, each timed by device events around `--calls` back-to-back calls; a figure is the MEDIAN over `--rounds` rounds (min
            and max are printed: the spread).
  training  the seeded `--misalign both --synthetic_pairs mapped` UNet run of tools/misalign_record.py, `--steps` steps, once with
            --lambda_fold 0 and once with it on; afterwards, on `--eval_batches` further batches of the same stream:
            registration/epe_px and the fold share (ops.jacobian_stats) of the prediction and of a 3-pass cascade.

    python tools/fold_penalty_record.py [--steps 300] [--lambda_fold 10] [--out tools/profiles/fold_penalty.txt]"""
import argparse
import ctypes
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = ((8, 256, 256), (2, 1024, 1024), (8, 1024, 1024))
_record = [None]


def emit(line):
    print(line)
    sys.stdout.flush()
    if _record[0] is not None:
        _record[0].write(line + '\n')
        _record[0].flush()


def timing(rounds, calls):
    from nemar_amd import _lib
    lib, dev = _lib.load(), torch.device('cuda:0')
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    emit('# timing: rounds %d x %d calls, medians [min .. max]; GB/s over the compulsory bytes (fwd 8 B/px, bwd 16 B/px)' % (rounds, calls))
    for (N, H, W) in SHAPES:
        g = torch.Generator(device=dev).manual_seed(1)
        d = F.interpolate(torch.randn(N, 2, 4, 5, device=dev, generator=g), size=(H, W), mode='bicubic')
        d = (d * (1.0 / d.abs().max())).contiguous()                          # amplitude 1: a fifth of the pixels or more fold
        gd_f, gd_s = torch.empty_like(d), torch.empty_like(d)
        loss_f, loss_s, one = torch.empty(1, device=dev), torch.empty(1, device=dev), torch.ones(1, device=dev)
        active = torch.empty(N, dtype=torch.int32, device=dev)
        wsb_f, wsb_s = lib.fold_penalty_workspace(N, H, W), lib.smoothness_workspace(N, H, W)
        ws_f, ws_s = torch.empty(wsb_f // 4 + 1, dtype=torch.int32, device=dev), torch.empty(wsb_s // 4 + 1, dtype=torch.int32, device=dev)
        variants = [
            ('fold_penalty_fwd', lambda: lib.fold_penalty_fwd(P(d), 0.0, 1.0, P(loss_f), 0, P(active), P(ws_f), wsb_f, N, H, W, st()), 8),
            ('smoothness_fwd (no image)', lambda: lib.smoothness_fwd(P(d), None, 0, 0.0, 1.0, P(loss_s), 0, P(ws_s), wsb_s, N, H, W, st()), 8),
            ('fold_penalty_bwd', lambda: lib.fold_penalty_bwd(P(d), 0.0, P(one), 1.0, P(gd_f), 0, N, H, W, st()), 16),
            ('smoothness_bwd (no image)', lambda: lib.smoothness_bwd(P(d), None, 0, 0.0, P(one), 1.0, P(gd_s), 0, N, H, W, st()), 16),
        ]
        for _, fn, _ in variants:                                             # warm-up: code objects, clocks
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
                times[name].append(e0.elapsed_time(e1) * 1e3 / calls)          # us per call
        emit('%d x 2 x %d x %d   (active %s of %d per sample, loss %.6f)' % (N, H, W, active.tolist(), (H - 1) * (W - 1), float(loss_f)))
        med = {}
        for name, _, bpp in variants:
            t = sorted(times[name])
            med[name] = statistics.median(t)
            emit('  %-28s %9.1f us [%9.1f .. %9.1f]   %7.1f GB/s' % (name, med[name], t[0], t[-1], N * H * W * bpp / med[name] / 1e3))
        emit('  fold fwd / smoothness fwd = %.2f   fold bwd / smoothness bwd = %.2f'
             % (med['fold_penalty_fwd'] / med['smoothness_fwd (no image)'], med['fold_penalty_bwd'] / med['smoothness_bwd (no image)']))


def training(lam, margin, steps, batch, eval_batches, ck):
    from nemar_amd import ops
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    from nemar_amd.train import _Options
    size = 256
    opt = _Options().parse(['--model', 'nemar', '--stn_type', 'unet', '--netG', 'resnet_3blocks', '--ngf', '16', '--ndf', '16', '--dataset_mode',
                            'gpupairs', '--dataroot', 'synthetic', '--synthetic_pairs', 'mapped', '--misalign', 'both', '--img_height', str(size),
                            '--img_width', str(size), '--crop_size', str(size), '--load_size', str(size + 30), '--batch_size', str(batch),
                            '--pool_size_pairs', '64', '--checkpoints_dir', ck, '--name', 'fold_%g' % lam, '--gpu_ids', '0', '--lambda_smooth', '10',
                            '--lambda_fold', str(lam), '--fold_margin', str(margin)], quiet=True)
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
    # read-out on further batches of the same stream: the prediction, then a 3-pass cascade
    rows = {1: [[], [], []], 3: [[], [], []]}                                 # passes -> counts, stats, registration_error dicts
    seen = 0
    for data in dataset:
        for passes in (1, 3):
            model.set_input(data)
            counts, stats = model.cascade(passes, regularity=True)[-1]
            rows[passes][0].append(counts)
            rows[passes][1].append(stats)
            rows[passes][2].append(model.registration_error())
        seen += 1
        if seen >= eval_batches:
            break
    emit('  --lambda_fold %-5g --fold_margin %g: after %d steps losses %s' % (lam, margin, steps, '  '.join('%s %.4f' % kv for kv in losses.items())))
    for passes in (1, 3):
        s = ops.regularity_summary(torch.cat(rows[passes][0]), torch.cat(rows[passes][1]))
        epe = statistics.mean(r['epe_px'] for r in rows[passes][2])
        before = statistics.mean(r['epe_before_px'] for r in rows[passes][2])
        emit('    %-22s registration/epe_px %8.4f (before %.4f)   folds %8d of %d = %.5f %%   det min %.4f   SDlogJ %s'
             % ('the prediction' if passes == 1 else 'a %d-pass cascade' % passes, epe, before, s['folds'], s['interior'], 100 * s['fold_frac'],
                s['det_min'], '%.4f' % s['log_det_std'] if s['log_det_std'] is not None else 'n/a'))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--eval_batches', type=int, default=4)
    ap.add_argument('--lambda_fold', type=float, default=10.0)
    ap.add_argument('--fold_margin', type=float, default=0.0)
    ap.add_argument('--skip_training', action='store_true')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'profiles', 'fold_penalty.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('fold_penalty_record: no GPU — a timing from anything else would say nothing')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    _record[0] = open(a.out, 'w')
    emit('# %s' % torch.cuda.get_device_name(0))
    timing(a.rounds, a.calls)
    if not a.skip_training:
        emit('# training: UNet STN, 256 x 256, batch %d, ngf = ndf = 16, resnet_3blocks, --misalign both (defaults), mapped synthetic pairs, seed 7, '
             '--lambda_smooth 10; read-out on %d further batches' % (a.batch, a.eval_batches))
        with tempfile.TemporaryDirectory() as ck:
            for lam in (0.0, a.lambda_fold):
                training(lam, a.fold_margin, a.steps, a.batch, a.eval_batches, ck)
    _record[0].close()
