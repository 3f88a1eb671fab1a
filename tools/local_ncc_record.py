"""Two records of local NCC (csrc/local_ncc.hip, --lambda_lncc), no gate on either:

  timing    nemar_local_ncc_fwd / _bwd (gx only: the step's call) at 16 x 3 x 256^2 and 8 x 3 x 1024^2, win 9, next to ops.l1_loss's two
            calls (nemar_l1_loss_fwd / _bwd) at the same shapes: the HBM-bound yardstick of this code base.  Algorithmic bytes: forward
            a read of x and y (8 B/px), backward a read of x and y and a write of gx (12 B/px); the same for L1.  The calls ALTERNATE
            inside every round, each timed by device events around `--calls` back-to-back calls; a figure is the MEDIAN over `--rounds`
            rounds (min and max are printed: the spread).
  step      the bench configuration's step (bench.py: config 2, batch 8) with --lambda_lncc 0 and with --lambda_lncc 10 --lncc_win 9,
            same process, alternating blocks of `--steps` steps; medians over the blocks.

Every section runs in a child process of its own under its own time limit; a section that fails or runs out of time is recorded as
such and the others still run.

    python tools/local_ncc_record.py [--out tools/profiles/local_ncc.txt]"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((16, 3, 256, 256), (8, 3, 1024, 1024))
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
    y = (0.6 * x + 0.1 * torch.randn(N, C, H, W, device=dev, generator=g)).contiguous()
    gx, ga = torch.empty_like(x), torch.empty_like(x)
    loss, loss1, one = torch.empty(1, device=dev), torch.empty(1, device=dev), torch.ones(1, device=dev)
    wsb, wsb1 = lib.local_ncc_workspace(N, C, H, W, WIN), lib.loss_workspace()
    ws, ws1 = torch.empty(wsb // 4 + 1, device=dev), torch.empty(wsb1 // 4 + 1, device=dev)
    n = x.numel()
    variants = [
        ('local_ncc_fwd', lambda: lib.local_ncc_fwd(P(x), P(y), WIN, 1e-5, 1.0, P(loss), 0, None, P(ws), wsb, N, C, H, W, st()), 8),
        ('l1_loss_fwd', lambda: lib.l1_loss_fwd(P(x), P(y), n, 1.0, P(loss1), 0, P(ws1), wsb1, st()), 8),
        ('local_ncc_bwd', lambda: lib.local_ncc_bwd(P(x), P(y), WIN, 1e-5, P(one), 1.0, P(gx), None, 0, N, C, H, W, st()), 12),
        ('l1_loss_bwd', lambda: lib.l1_loss_bwd(P(x), P(y), n, P(one), 1.0, P(ga), 0, st()), 12),
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
    emit('%d x %d x %d x %d, win %d   (loss %.6f, L1 %.6f)' % (N, C, H, W, WIN, float(loss), float(loss1)))
    med = {}
    for name, _, bpp in variants:
        t = sorted(times[name])
        med[name] = statistics.median(t)
        emit('  %-16s %9.1f us [%9.1f .. %9.1f]   %7.1f GB/s' % (name, med[name], t[0], t[-1], n * bpp / med[name] / 1e3))
    emit('  local_ncc fwd + bwd = %.1f us, l1_loss fwd + bwd = %.1f us: ratio %.2f   (fwd %.2f, bwd %.2f)'
         % (med['local_ncc_fwd'] + med['local_ncc_bwd'], med['l1_loss_fwd'] + med['l1_loss_bwd'],
            (med['local_ncc_fwd'] + med['local_ncc_bwd']) / (med['l1_loss_fwd'] + med['l1_loss_bwd']),
            med['local_ncc_fwd'] / med['l1_loss_fwd'], med['local_ncc_bwd'] / med['l1_loss_bwd']))


def step(blocks, steps):
    import torch
    import bench
    dev = torch.device('cuda:0')
    runs = [('--lambda_lncc 0', ['--lambda_lncc', '0']), ('--lambda_lncc 10 --lncc_win %d' % WIN, ['--lambda_lncc', '10', '--lncc_win', str(WIN)])]
    models = []
    for name, extra in runs:
        model, data = bench._make(8, 256, extra, dev)
        for _ in range(3):
            model.set_input(data)
            model.optimize_parameters()
        models.append((name, model, data, []))
    for _ in range(blocks):
        for name, model, data, ms in models:
            ms.append(bench._time_steps(model, data, steps))
    emit('config-2 step (batch 8, 256 x 256), %d alternating blocks of %d eager steps, ms per step: median [min .. max]' % (blocks, steps))
    med = []
    for name, _, _, ms in models:
        med.append(statistics.median(ms))
        emit('  %-34s %8.3f [%8.3f .. %8.3f]' % (name, med[-1], min(ms), max(ms)))
    emit('  the terms cost %.3f ms per step (%.2f %%)' % (med[1] - med[0], 100 * (med[1] - med[0]) / med[0]))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--timeout', type=int, default=240, help='seconds, per section')
    ap.add_argument('--section', default=None, help='(internal) run one section in this process: timing:<index> or step')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tools', 'profiles', 'local_ncc.txt'))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('local_ncc_record: no GPU — a timing from anything else would say nothing')
    if a.section is not None:
        if a.section.startswith('timing:'):
            timing(SHAPES[int(a.section.split(':')[1])], a.rounds, a.calls)
        else:
            step(a.blocks, a.steps)
        raise SystemExit(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    lines = ['# %s' % torch.cuda.get_device_name(0),
             '# timing: rounds %d x %d calls, medians [min .. max]; GB/s over the algorithmic bytes (fwd 8 B/px, bwd 12 B/px)' % (a.rounds, a.calls)]
    for section in ['timing:%d' % i for i in range(len(SHAPES))] + ['step']:
        cmd = [sys.executable, os.path.abspath(__file__), '--section', section, '--rounds', str(a.rounds), '--calls', str(a.calls), '--blocks',
               str(a.blocks), '--steps', str(a.steps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            lines += r.stdout.splitlines() if r.returncode == 0 else ['%s: exit status %d: %s' % (section, r.returncode, r.stderr.strip()[-400:])]
            failed = r.returncode != 0
        except subprocess.TimeoutExpired:
            lines.append('%s: no result within %d s' % (section, a.timeout))
            failed = True
        if failed:                    # whatever went wrong on the device: nothing more is started on it
            break
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))
