"""The record of refinement on the pair (csrc/register.hip's backward, NEMARModel.refine), no gate on any of it:

  accuracy  the float64 cases of tests/register_grad_cases.py on the gfx950 library: per case the kernel's and torch-fp32's max-abs error
            against float64 and their ratio; the worst ratio per mode at the end.
  timing    nemar_warp_resampled_bwd against the composed route it replaces — nemar_grid_sample_bwd without grad_input on the field at
            full size, then nemar_bilinear_bwd down to the prediction's size — at 8 x 3 x 1024^2 from 256^2, 8 x 3 x 1000 x 1400 from
            256^2 and 8 x 3 x 256^2 from 64^2.  One process; the two ALTERNATE inside every round, each timed by device events around
            `--calls` back-to-back calls; a figure is the MEDIAN over `--rounds` rounds (min and max are printed: the spread).  With
            each shape: how many elements of the composed route's gradient differ in their bits from its first run, over 10 repeats on
            one input (its resize backward scatters with fp32 atomics off the x2 and integer ratios), and the same count for the fused one.
  step      one refinement step per image term (mind, lncc, l1) at 8 x 3 x 1024^2 from the 256^2 prediction of the trained model below:
            device time of refine(steps) divided by steps + 1 objective evaluations.
  sweep     the seeded `--misalign both --synthetic_pairs mapped` UNet run of tools/epe_record.py, `--steps` steps; then on `--eval_batches`
            further batches of the stream, which no step trained on: registration/epe_px and fold share of the network's prediction,
            and after refine(50 steps, term) from it, for every pair of `lr` and `lambda_smooth` of the grid.
  bench     with `--parent DIR` (a built checkout of the parent commit): the default training step, bench.py of DIR and of this tree in
            fresh processes, alternating, three runs each.

    python tools/refine_record.py [--steps 300] [--parent DIR] [--out tools/profiles/refine.txt]"""
import argparse
import ctypes
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = ((8, 3, (256, 256), (1024, 1024)), (8, 3, (256, 256), (1000, 1400)), (8, 3, (64, 64), (256, 256)))
LRS, SMOOTHS = (3e-4, 1e-3, 3e-3), (0.0, 0.1, 1.0)
_record = [None]


def emit(line):
    print(line)
    sys.stdout.flush()
    if _record[0] is not None:
        _record[0].write(line + '\n')
        _record[0].flush()


def accuracy():
    import register_grad_cases as K
    from backends import HipBackend
    from nemar_amd import _lib
    be = HipBackend(_lib.load())
    emit('# accuracy: max-abs error against float64 of the kernel and of torch-fp32 (the yardstick), N = 2')
    worst = {}
    for mode in K.MODES:
        for size in K.SIZES:
            err, yard = K.case_float64(be, mode, size)
            emit('  %-60s kernel %.3e  torch-fp32 %.3e  ratio %.2f' % (K._what(mode, size), err, yard, err / yard))
            worst[mode] = max(worst.get(mode, 0.0), err / yard)
    emit('  worst kernel / yardstick ratio: unet %.2f, affine %.2f (the tests allow %g)' % (worst[K.GRID_UNET], worst[K.GRID_AFFINE], K.MARGIN))


def _smooth(N, H, W, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    d = F.interpolate(torch.randn(N, 2, 4, 5, device=dev, generator=g), size=(H, W), mode='bicubic')
    return (d / d.abs().max()).contiguous()


def timing(rounds, calls):
    from nemar_amd import _lib, ops
    lib, dev = _lib.load(), torch.device('cuda:0')
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    U = ops.GRID_UNET
    emit('# timing: rounds %d x %d calls, medians [min .. max]' % (rounds, calls))
    for (N, C, (hf, wf), (H, W)) in SHAPES:
        g = torch.Generator(device=dev).manual_seed(5)
        img = torch.rand(N, C, H, W, device=dev, generator=g)
        gout = torch.randn(N, C, H, W, device=dev, generator=g)
        pred = (_smooth(N, hf, wf, 2, dev) * (8.0 / wf)).contiguous()                  # offsets of up to 4 px of the field
        field = torch.empty(N, 2, H, W, device=dev)
        lib.bilinear_fwd(P(pred), P(field), N * 2, hf, wf, H, W, st())
        wsb = lib.warp_resampled_bwd_workspace(U, N, hf, wf, H, W)
        ws = torch.empty(wsb // 4 + 1, dtype=torch.float32, device=dev)
        g_fused, g_field, g_comp = torch.empty_like(pred), torch.empty_like(field), torch.empty_like(pred)

        def fused():
            lib.warp_resampled_bwd(P(img), P(pred), U, P(gout), P(g_fused), 0, N, C, H, W, hf, wf, H, W, P(ws), wsb, st())

        def composed():
            lib.grid_sample_bwd(P(img), P(field), U, P(gout), None, 0, P(g_field), 0, N, C, H, W, H, W, None, 0, st())
            lib.bilinear_bwd(P(g_field), P(g_comp), N * 2, hf, wf, H, W, st())

        variants = [('fused warp_resampled_bwd', fused), ('composed gs_bwd + bilinear_bwd', composed)]
        for _, fn in variants:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in variants}
        for _ in range(rounds):
            for name, fn in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / calls)
        differ = {}
        for name, fn, res in (('fused', fused, g_fused), ('composed', composed, g_comp)):
            fn()
            first = res.clone().view(torch.int32)
            worst = 0
            for _ in range(10):
                fn()
                worst = max(worst, int((res.view(torch.int32) != first).sum().item()))
            differ[name] = worst
        gap = float((g_fused - g_comp).abs().max() / g_comp.abs().max())
        emit('%d x %d x %d x %d from %d x %d  (workspace %.1f MiB; fused against composed: max |difference| / max |gradient| %.2e)'
             % (N, C, H, W, hf, wf, wsb / 2 ** 20, gap))
        for name, _ in variants:
            t = sorted(times[name])
            emit('  %-32s %9.1f us [%9.1f .. %9.1f]' % (name, statistics.median(t), t[0], t[-1]))
        emit('  elements of %d whose bits differ from the first run, worst of 10 repeats: fused %d, composed %d'
             % (pred.numel(), differ['fused'], differ['composed']))


def _trained(steps, batch, ck):
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    from nemar_amd.train import _Options
    size = 256
    opt = _Options().parse(['--model', 'nemar', '--stn_type', 'unet', '--netG', 'resnet_3blocks', '--ngf', '16', '--ndf', '16', '--dataset_mode',
                            'gpupairs', '--dataroot', 'synthetic', '--synthetic_pairs', 'mapped', '--misalign', 'both', '--img_height', str(size),
                            '--img_width', str(size), '--crop_size', str(size), '--load_size', str(size + 30), '--batch_size', str(batch),
                            '--pool_size_pairs', '64', '--checkpoints_dir', ck, '--name', 'refine', '--gpu_ids', '0', '--lambda_smooth', '10'],
                           quiet=True)
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
    return model, dataset


def step_times(model, dataset, steps=20):
    data = next(iter(dataset))
    model.set_input(data)
    up = lambda t: F.interpolate(t, size=(1024, 1024), mode='bilinear', align_corners=False).contiguous()
    A, B = up(model.real_A), up(model.real_B)
    emit('# step: refine(%d steps) at %d x 3 x 1024^2 from the 256^2 prediction, device time / %d objective evaluations' % (steps, A.size(0), steps + 1))
    for term in ('mind', 'lncc', 'l1'):
        ts = []
        for _ in range(3):
            model.test()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            model.refine(A, B, steps, term=term)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / (steps + 1))
        emit('  %-5s %8.3f ms per step (median of 3 runs; the first includes the workspace growth: %s)' % (term, statistics.median(ts), ' '.join('%.3f' % t for t in ts)))


def sweep(model, dataset, eval_batches, term, refine_steps=50):
    batches = []
    for data in dataset:                                                      # further batches of the stream: never trained on
        batches.append(data)
        if len(batches) >= eval_batches:
            break
    mean = lambda rows, k: statistics.mean(r[k] for r in rows)

    def held_out(lr=None, lam=None):
        rows, objs = [], []
        for data in batches:
            model.set_input(data)
            model.test()
            if lr is not None:
                objs.append(model.refine(model.real_A, model.real_B, refine_steps, lr=lr, term=term, lambda_smooth=lam)['objective'][[0, -1]].tolist())
            rows.append(model.registration_error())
        return rows, objs

    rows, _ = held_out()
    emit('# sweep: refine(%d steps, term %r) on %d held-out batches; registration/epe_px (doing nothing: %.4f) and fold share'
         % (refine_steps, term, eval_batches, mean(rows, 'epe_before_px')))
    emit('  the network alone                       epe_px %8.4f   fold_frac %.5f' % (mean(rows, 'epe_px'), mean(rows, 'fold_frac')))
    best = None
    for lr in LRS:
        for lam in SMOOTHS:
            rows, objs = held_out(lr, lam)
            epe = mean(rows, 'epe_px')
            emit('  lr %-7g lambda_smooth %-5g           epe_px %8.4f   fold_frac %.5f   objective %.5f -> %.5f'
                 % (lr, lam, epe, mean(rows, 'fold_frac'), statistics.mean(o[0] for o in objs), statistics.mean(o[1] for o in objs)))
            if best is None or epe < best[0]:
                best = (epe, lr, lam)
    emit('  best pair: lr %g, lambda_smooth %g (epe_px %.4f); the defaults of NEMARModel.refine in this tree: lr %g, lambda_smooth %g'
         % (best[1], best[2], best[0], model.REFINE_LR, model.REFINE_LAMBDA_SMOOTH))


def bench_alternated(parent, runs=3, steps=40, warmup=10):
    """the default training step of `parent` (a checkout of the parent commit, built) and of this tree, bench.py in fresh processes, alternating"""
    import json
    import subprocess
    emit('# the default training step: bench.py --gpus 1 --steps %d --warmup %d, the parent commit and this tree alternating, ms per step' % (steps, warmup))
    ms = {'parent': [], 'this tree': []}
    for _ in range(runs):
        for name, root in (('parent', parent), ('this tree', ROOT)):
            r = subprocess.run(['timeout', '-k', '10', '300', sys.executable, 'bench.py', '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup)],
                               cwd=root, capture_output=True, text=True, check=True)
            ms[name].append(json.loads(r.stdout.strip().splitlines()[-1])['ms_per_step'])
    for name, v in ms.items():
        emit('  %-10s %s' % (name, '  '.join('%.3f' % x for x in v)))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--eval_batches', type=int, default=4)
    ap.add_argument('--term', default='mind')
    ap.add_argument('--skip_training', action='store_true')
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit: alternate its bench.py with this tree\'s')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tools', 'profiles', 'refine.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('refine_record: no GPU — a timing from anything else would say nothing')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    _record[0] = open(a.out, 'w')
    emit('# %s, %s (the name and the architecture the runtime reports for the MI355X)'
         % (torch.cuda.get_device_name(0), getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?')))
    accuracy()
    timing(a.rounds, a.calls)
    if not a.skip_training:
        emit('# model: UNet STN, 256 x 256, batch %d, ngf = ndf = 16, resnet_3blocks, --misalign both (defaults), mapped synthetic pairs, seed 7, '
             '--lambda_smooth 10, %d steps' % (a.batch, a.steps))
        with tempfile.TemporaryDirectory() as ck:
            model, dataset = _trained(a.steps, a.batch, ck)
            step_times(model, dataset)
            sweep(model, dataset, a.eval_batches, a.term)
            del model, dataset
    if a.parent:
        torch.cuda.empty_cache()
        bench_alternated(a.parent)
    _record[0].close()
