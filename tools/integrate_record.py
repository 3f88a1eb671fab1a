"""Records of scaling and squaring (csrc/integrate.hip, ops.integrate_velocity, --stn_integrate), no gate on any of them:

  kernels   the chain of K = 6 steps, forward and backward, at 8 x 2 x 256^2 and 8 x 2 x 1024^2, field amplitudes 0.05 and 0.3 (the time
            must not depend on how far the field moves), next to the same chain composed from what the tree had before:
            ops.grid_sample with an explicit grid plus torch arithmetic, forward and autograd's backward.  That composition pads with
            zeros and carries the linspace zoom: a cost yardstick, not a parity one.  One process; the variants ALTERNATE inside every
            round, each timed by device events around `--calls` back-to-back calls; a figure is the MEDIAN over `--rounds` rounds (min
            and max are printed: the spread).  The step forward's compulsory bytes (8 B/px read, 8 B/px written; the gathers are L2
            hits) against its time.
  step      the training step's ms (median of `--step_rounds` steps after warm-up) with --stn_integrate 6 against without, and the
            kernel launches of one steady-state step by name (torch.profiler): all of them, and those of ATen.
  training  the seeded `--misalign both --synthetic_pairs mapped` UNet run of tools/fold_penalty_record.py, `--steps` steps, three
            times: plain, --lambda_fold 10, --stn_integrate 6; afterwards, on `--eval_batches` further batches of the same stream:
            registration/epe_px and the fold share (ops.jacobian_stats) of the prediction.

    python tools/integrate_record.py [--steps 300] [--out tools/profiles/integrate_velocity.txt]"""
import argparse
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = ((8, 256, 256), (8, 1024, 1024))
AMPS = (0.05, 0.3)
K = 6
_record = [None]


def emit(line):
    print(line)
    sys.stdout.flush()
    if _record[0] is not None:
        _record[0].write(line + '\n')
        _record[0].flush()


def composed_chain(v, steps):
    """the same recurrence from ops.grid_sample with an explicit grid and torch arithmetic (zero padding, the linspace identity)"""
    from nemar_amd import ops
    N, _, H, W = v.shape
    x, y = torch.linspace(-1, 1, W, device=v.device), torch.linspace(-1, 1, H, device=v.device)
    ident = torch.stack([x[None, :].expand(H, W), y[:, None].expand(H, W)], -1)[None]
    u = v * (1.0 / (1 << steps))
    for _ in range(steps):
        u = u + ops.grid_sample(u, ident + u.permute(0, 2, 3, 1))
    return u


def _timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls          # us per call


def kernels(rounds, calls):
    from nemar_amd import ops
    dev = torch.device('cuda:0')
    emit('# kernels: K = %d, rounds %d x %d calls, medians [min .. max] in us per chain' % (K, rounds, calls))
    for (N, H, W) in SHAPES:
        for amp in AMPS:
            g = torch.Generator(device=dev).manual_seed(1)
            v = F.interpolate(torch.randn(N, 2, 4, 5, device=dev, generator=g), size=(H, W), mode='bicubic')
            v = (v * (amp / v.abs().max())).contiguous().requires_grad_(True)
            gout = torch.randn(N, 2, H, W, device=dev, generator=g)
            u1, out1 = v.detach(), torch.empty_like(v)

            def fused_fb():
                v.grad = None
                ops.integrate_velocity(v, K).backward(gout)

            def composed_fb():
                v.grad = None
                composed_chain(v, K).backward(gout)

            variants = [
                ('one step forward (s = 1)', lambda: ops.L.svf_step_fwd(ops._p(u1), 1.0, ops._p(out1), N, H, W, ops._stream())),
                ('fused chain forward', lambda: ops.integrate_velocity(v.detach(), K)),
                ('composed chain forward', lambda: composed_chain(v.detach(), K)),
                ('fused chain fwd + bwd', fused_fb),
                ('composed chain fwd + bwd', composed_fb),
            ]
            for _, fn in variants:                                             # warm-up: code objects, workspaces, clocks
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {name: [] for name, _ in variants}
            for _ in range(rounds):
                for name, fn in variants:
                    times[name].append(_timed(fn, calls))
            emit('%d x 2 x %d x %d, amplitude %g (%.1f px)' % (N, H, W, amp, amp * W / 2))
            med = {}
            for name, _ in variants:
                t = sorted(times[name])
                med[name] = statistics.median(t)
                emit('  %-28s %9.1f us [%9.1f .. %9.1f]' % (name, med[name], t[0], t[-1]))
            emit('  step forward: 16 B/px compulsory = %.1f GB/s;  fused / composed: forward %.2f, fwd + bwd %.2f;  fused backward alone %.1f us, '
                 'composed %.1f us' % (N * H * W * 16 / med['one step forward (s = 1)'] / 1e3,
                                       med['fused chain forward'] / med['composed chain forward'],
                                       med['fused chain fwd + bwd'] / med['composed chain fwd + bwd'],
                                       med['fused chain fwd + bwd'] - med['fused chain forward'],
                                       med['composed chain fwd + bwd'] - med['composed chain forward']))


def _options(ck, name, batch, extra):
    from nemar_amd.train import _Options
    size = 256
    return _Options().parse(['--model', 'nemar', '--stn_type', 'unet', '--netG', 'resnet_3blocks', '--ngf', '16', '--ndf', '16', '--dataset_mode',
                             'gpupairs', '--dataroot', 'synthetic', '--synthetic_pairs', 'mapped', '--misalign', 'both', '--img_height', str(size),
                             '--img_width', str(size), '--crop_size', str(size), '--load_size', str(size + 30), '--batch_size', str(batch),
                             '--pool_size_pairs', '64', '--checkpoints_dir', ck, '--name', name, '--gpu_ids', '0', '--lambda_smooth', '10', *extra],
                            quiet=True)


def step_time(batch, step_rounds, ck):
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    emit('# step: UNet STN, 256 x 256, batch %d, ngf = ndf = 16; ms per optimize_parameters(), median of %d after 10 warm-up steps; launches of '
         'one further step' % (batch, step_rounds))
    for name, extra in (('plain', []), ('stn_integrate 6', ['--stn_integrate', '6'])):
        opt = _options(ck, 'step_' + name.replace(' ', '_'), batch, extra)
        torch.manual_seed(7)
        data = next(iter(create_dataset(opt)))
        model = create_model(opt)
        model.setup(opt)
        ms = []
        for i in range(10 + step_rounds):
            model.set_input(data)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            model.optimize_parameters()
            e1.record()
            torch.cuda.synchronize()
            if i >= 10:
                ms.append(e0.elapsed_time(e1))
        ms.sort()
        told = '  %-18s %8.3f ms [%8.3f .. %8.3f]' % (name, statistics.median(ms), ms[0], ms[-1])
        try:
            from torch.profiler import ProfilerActivity, profile
            model.set_input(data)
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                model.optimize_parameters()
                torch.cuda.synchronize()
            names = [e.name for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA') and 'Memcpy' not in e.name and 'Memset' not in e.name]
            aten = [n for n in names if 'at::' in n or 'aten' in n.lower()]
            svf = [n for n in names if 'svf_' in n]
            told += '   %d launches, %d of them svf_*, %d of ATen%s' % (len(names), len(svf), len(aten), (': ' + ', '.join(sorted(set(aten)))[:300]) if aten else '')
        except Exception as e:                                                  # (no profiler: the time alone)
            told += '   (launch count unavailable: %s)' % (str(e).splitlines()[0] if str(e) else type(e).__name__)
        emit(told)
        del model


def training(name, extra, steps, batch, eval_batches, ck):
    from nemar_amd import ops
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    opt = _options(ck, name.replace(' ', '_').replace('-', ''), batch, extra)
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
    counts, stats, errs = [], [], []
    seen = 0
    for data in dataset:
        model.set_input(data)
        c, s = model.cascade(1, regularity=True)[-1]
        counts.append(c)
        stats.append(s)
        errs.append(model.registration_error())
        seen += 1
        if seen >= eval_batches:
            break
    s = ops.regularity_summary(torch.cat(counts), torch.cat(stats))
    emit('  %-18s after %d steps losses %s' % (name, steps, '  '.join('%s %.4f' % kv for kv in losses.items())))
    emit('    registration/epe_px %8.4f (before %.4f)   folds %8d of %d = %.5f %%   det min %.4f   SDlogJ %s'
         % (statistics.mean(r['epe_px'] for r in errs), statistics.mean(r['epe_before_px'] for r in errs), s['folds'], s['interior'],
            100 * s['fold_frac'], s['det_min'], '%.4f' % s['log_det_std'] if s['log_det_std'] is not None else 'n/a'))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--step_rounds', type=int, default=21)
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--eval_batches', type=int, default=4)
    ap.add_argument('--skip_kernels', action='store_true')
    ap.add_argument('--skip_step', action='store_true')
    ap.add_argument('--skip_training', action='store_true')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'profiles', 'integrate_velocity.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('integrate_record: no GPU — a timing from anything else would say nothing')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    _record[0] = open(a.out, 'w')
    emit('# %s' % torch.cuda.get_device_name(0))
    with tempfile.TemporaryDirectory() as ck:
        if not a.skip_kernels:
            kernels(a.rounds, a.calls)
        if not a.skip_step:
            step_time(a.batch, a.step_rounds, ck)
        if not a.skip_training:
            emit('# training: UNet STN, 256 x 256, batch %d, ngf = ndf = 16, resnet_3blocks, --misalign both (defaults), mapped synthetic pairs, seed 7, '
                 '--lambda_smooth 10; read-out on %d further batches' % (a.batch, a.eval_batches))
            for name, extra in (('plain', []), ('--lambda_fold 10', ['--lambda_fold', '10']), ('--stn_integrate 6', ['--stn_integrate', '6'])):
                training(name, extra, a.steps, a.batch, a.eval_batches, ck)
    _record[0].close()
