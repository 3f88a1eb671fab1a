"""Three records of the MIND loss (csrc/mind.hip, --lambda_mind), no gate on any:

  timing    nemar_mind_loss_fwd / _bwd (gx only: the step's call) at 16 x 3 x 256^2 and 8 x 3 x 1024^2 for (patch, dil) = (3,1), (3,2),
            (5,2), next to ops.local_ncc's two calls at win 9 and ops.l1_loss's two calls (the HBM-bound yardstick of this code base) on
            the same tensors in the same process.  Algorithmic bytes per pixel of a plane: MIND forward a read of x and y (4 (Cx + Cy)
            B), backward that and a write of gx (4 (2 Cx + Cy) B) — Cx = Cy = 3 here: 24 and 36 B per pixel; local NCC and L1 the same
            bytes (8 and 12 B per element).  The calls ALTERNATE inside every round, each timed by device events around `--calls`
            back-to-back calls; a figure is the MEDIAN over `--rounds` rounds (min and max are printed: the spread).
  ratios    the worst kernel / float32-yardstick error ratio of every family that tests/test_mind_gpu.py prints (dm, gx, gy, loss against
            its bound, the symmetry and channel-sum comparisons), from a run of that file.
  training  the seeded `--misalign both --synthetic_pairs mapped` UNet run of tools/epe_record.py, `--steps` steps, once without and once
            with --lambda_mind: registration/epe_px of the training batches as means over blocks of 50 steps (the curve), and afterwards
            on `--eval_batches` further batches of the same seeded stream, which no step trained on.

Every section runs in a child process of its own under its own time limit; a section that fails or runs out of time is recorded as
such and nothing more is started.

    python tools/mind_record.py [--steps 300] [--lambda_mind 10] [--out tools/profiles/mind_loss.txt]"""
import argparse
import contextlib
import ctypes
import io
import math
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((16, 3, 256, 256), (8, 3, 1024, 1024))
CONFIGS = ((3, 1), (3, 2), (5, 2))
WIN = 9


def emit(line):
    print(line)
    sys.stdout.flush()


def timing(shape, rounds, calls):
    import torch
    from nemar_amd import _lib
    lib, dev = _lib.load(), torch.device('cuda:0')
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    N, C, H, W = shape
    g = torch.Generator(device=dev).manual_seed(1)
    low = torch.randn(N, C, H // 16, W // 16, device=dev, generator=g)
    x = (torch.nn.functional.interpolate(low, size=(H, W), mode='bicubic') * 0.3 + 0.05 * torch.randn(N, C, H, W, device=dev, generator=g)).contiguous()
    y = (-0.8 * torch.tanh(2.0 * (0.6 * x + 0.1 * torch.randn(N, C, H, W, device=dev, generator=g)))).contiguous()      # another "modality"
    gx = torch.empty_like(x)
    loss, one = torch.empty(1, device=dev), torch.ones(1, device=dev)
    wsb_m = max(lib.mind_loss_workspace(N, H, W, p, d) for p, d in CONFIGS)
    wsb_n, wsb_1 = lib.local_ncc_workspace(N, C, H, W, WIN), lib.loss_workspace()
    ws = torch.empty(max(wsb_m, wsb_n, wsb_1) // 4 + 1, device=dev)
    n = x.numel()
    variants = []
    for p, d in CONFIGS:
        variants.append(('mind_fwd %d,%d' % (p, d), lambda p=p, d=d: lib.mind_loss_fwd(P(x), C, P(y), C, p, d, 1e-5, 1.0, P(loss), 0, None, P(ws), wsb_m, N, H, W, st()), 8))
        variants.append(('mind_bwd %d,%d' % (p, d), lambda p=p, d=d: lib.mind_loss_bwd(P(x), C, P(y), C, p, d, 1e-5, P(one), 1.0, P(gx), None, 0, N, H, W, st()), 12))
    variants += [
        ('local_ncc_fwd', lambda: lib.local_ncc_fwd(P(x), P(y), WIN, 1e-5, 1.0, P(loss), 0, None, P(ws), wsb_n, N, C, H, W, st()), 8),
        ('local_ncc_bwd', lambda: lib.local_ncc_bwd(P(x), P(y), WIN, 1e-5, P(one), 1.0, P(gx), None, 0, N, C, H, W, st()), 12),
        ('l1_loss_fwd', lambda: lib.l1_loss_fwd(P(x), P(y), n, 1.0, P(loss), 0, P(ws), wsb_1, st()), 8),
        ('l1_loss_bwd', lambda: lib.l1_loss_bwd(P(x), P(y), n, P(one), 1.0, P(gx), 0, st()), 12),
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
    emit('%d x %d x %d x %d' % (N, C, H, W))
    med = {}
    for name, _, bpe in variants:
        t = sorted(times[name])
        med[name] = statistics.median(t)
        emit('  %-16s %9.1f us [%9.1f .. %9.1f]   %7.1f GB/s' % (name, med[name], t[0], t[-1], n * bpe / med[name] / 1e3))
    l1 = med['l1_loss_fwd'] + med['l1_loss_bwd']
    ncc = med['local_ncc_fwd'] + med['local_ncc_bwd']
    for p, d in CONFIGS:
        m = med['mind_fwd %d,%d' % (p, d)] + med['mind_bwd %d,%d' % (p, d)]
        emit('  mind %d,%d fwd + bwd = %.1f us: %.2f x l1_loss (%.1f us), %.2f x local_ncc win %d (%.1f us)' % (p, d, m, m / l1, l1, m / ncc, WIN, ncc))


def ratios():
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(ROOT, 'tests', 'test_mind_gpu.py'), '-q', '-s', '-p', 'no:cacheprovider'],
                       capture_output=True, text=True, cwd=ROOT)
    worst = {}
    for line in r.stdout.splitlines():
        m = re.match(r'mind (\w+)\s.*ratio ([0-9.infa]+)', line)
        if m:
            fam = m.group(1) if m.group(1) not in ('symmetry', 'channels') else m.group(1) + ' (across)'
            v = float(m.group(2))
            if fam not in worst or v > worst[fam][0]:
                worst[fam] = (v, line.strip())
    tail = [l for l in r.stdout.splitlines() if ' passed' in l or ' failed' in l]
    emit('worst kernel / float32-yardstick ratios in tests/test_mind_gpu.py (%s); the rule is <= 4 (loss: <= 1 of its bound)' % (tail[-1].strip() if tail else 'exit status %d' % r.returncode))
    for fam, (v, line) in sorted(worst.items()):
        emit('  %-18s %6.2f   %s' % (fam, v, line))
    if r.returncode != 0:
        raise SystemExit(r.returncode)


def training(lam, steps, batch, eval_batches):
    import torch
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    from nemar_amd.train import _Options
    size = 256
    with tempfile.TemporaryDirectory() as ck:
        opt = _Options().parse(['--model', 'nemar', '--stn_type', 'unet', '--netG', 'resnet_3blocks', '--ngf', '16', '--ndf', '16', '--dataset_mode',
                                'gpupairs', '--dataroot', 'synthetic', '--synthetic_pairs', 'mapped', '--misalign', 'both', '--img_height', str(size),
                                '--img_width', str(size), '--crop_size', str(size), '--load_size', str(size + 30), '--batch_size', str(batch),
                                '--pool_size_pairs', '64', '--checkpoints_dir', ck, '--name', 'mind_%g' % lam, '--gpu_ids', '0', '--lambda_smooth', '10']
                               + (['--lambda_mind', str(lam)] if lam else []), quiet=True)
        torch.manual_seed(7)
        with contextlib.redirect_stdout(io.StringIO()):                       # (the networks' own report is not part of the record)
            dataset = create_dataset(opt)
            model = create_model(opt)
            model.setup(opt)
        step, block, curve = 0, [], []
        while step < steps:
            for data in dataset:
                model.set_input(data)
                model.optimize_parameters()
                block.append(model.registration_error()['epe_px'])
                step += 1
                if step % 50 == 0 or step >= steps:
                    curve.append((step, statistics.mean(block)))
                    block = []
                if step >= steps:
                    break
        losses = model.get_current_losses()
        rows, seen = [], 0
        for data in dataset:                                                  # further batches of the stream: never trained on
            model.set_input(data)
            model.test()
            rows.append(model.registration_error())
            seen += 1
            if seen >= eval_batches:
                break
    emit('  %s: after %d steps losses %s' % ('--lambda_mind %g' % lam if lam else 'without --lambda_mind', steps, '  '.join('%s %.4f' % kv for kv in losses.items())))
    emit('    registration/epe_px of the training batches, means over the steps up to: ' + '  '.join('%d: %.4f' % c for c in curve))
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
    ap.add_argument('--lambda_mind', type=float, default=10.0)
    ap.add_argument('--timeout', type=int, default=300, help='seconds, per section')
    ap.add_argument('--sections', default='timing:0,timing:1,ratios,training:0,training:1')
    ap.add_argument('--section', default=None, help='(internal) run one section in this process')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tools', 'profiles', 'mind_loss.txt'))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('mind_record: no GPU — a timing from anything else would say nothing')
    if a.section is not None:
        kind, _, arg = a.section.partition(':')
        if kind == 'timing':
            timing(SHAPES[int(arg)], a.rounds, a.calls)
        elif kind == 'ratios':
            ratios()
        else:
            training(a.lambda_mind if int(arg) else 0.0, a.steps, a.batch, a.eval_batches)
        raise SystemExit(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    lines = ['# %s' % torch.cuda.get_device_name(0),
             '# timing: rounds %d x %d calls, medians [min .. max]; GB/s over the algorithmic bytes of 3-channel x, y and gx (fwd 8 B, bwd 12 B per element)'
             % (a.rounds, a.calls),
             '# training: UNet STN, 256 x 256, batch %d, ngf = ndf = 16, resnet_3blocks, --misalign both (defaults), mapped synthetic pairs, seed 7, '
             '--lambda_smooth 10, %d steps; read-out on %d further batches of the stream' % (a.batch, a.steps, a.eval_batches)]
    for section in a.sections.split(','):
        cmd = [sys.executable, os.path.abspath(__file__), '--section', section, '--rounds', str(a.rounds), '--calls', str(a.calls), '--steps',
               str(a.steps), '--batch', str(a.batch), '--eval_batches', str(a.eval_batches), '--lambda_mind', str(a.lambda_mind)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            lines += r.stdout.splitlines()
            failed = r.returncode != 0
            if failed:
                lines.append('%s: exit status %d: %s' % (section, r.returncode, r.stderr.strip()[-400:]))
        except subprocess.TimeoutExpired:
            lines.append('%s: no result within %d s' % (section, a.timeout))
            failed = True
        print('\n'.join(lines[-12:]))
        sys.stdout.flush()
        if failed:                    # whatever went wrong on the device: nothing more is started on it
            break
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
