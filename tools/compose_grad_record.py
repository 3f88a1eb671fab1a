"""Records of the compose gradient and of cascade training (csrc/compose.hip nemar_compose_pred_bwd, ops.compose_predictions(grad=True),
--train_passes), no gate on any of them:

  kernels   nemar_compose_pred (forward) and nemar_compose_pred_bwd (both gradients) in us for the four mode pairs at 8 x 2 x 256^2 and
            2 x 2 x 1024^2, for operands near the identity (amplitude 0.01 px) and for a smooth 3 px field (an affine operand: a 3 px
            translation with a 1 % shear), next to nemar_svf_step_bwd at the same shape and on the same field: it moves the same bytes
            through the same 64-bit fixed-point atomics (max pass, scatter, fold), so it is the yardstick the backward is read against.
            One process; the variants ALTERNATE inside every round, each timed by device events around `--calls` back-to-back calls; a
            figure is the MEDIAN over `--rounds` rounds (min and max are printed: the spread).  Buffers are preallocated: the library
            calls alone are timed.  The tensor bytes of the (UNET, UNET) backward — first, second, gout read, gfirst and gsecond written,
            8 B/px each; the accumulator's own traffic (16 B/px scattered, read and cleared) is not counted — against its time.
  step      ms per optimize_parameters() of the smallest UNet-STN training configuration (256 x 256, ngf = ndf = 8, batch 2,
            --stn_no_identity_init) at --train_passes 1, 2 and 3: median of `--step_rounds` steps after 10 warm-up steps.

    python tools/compose_grad_record.py [--out tools/profiles/compose_grad.txt]"""
import argparse
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = ((8, 256, 256), (2, 1024, 1024))
FIELDS = (('near identity', 0.01), ('smooth 3 px', 3.0))      # name, amplitude in pixels
_record = [None]


def emit(line):
    print(line)
    sys.stdout.flush()
    if _record[0] is not None:
        _record[0].write(line + '\n')
        _record[0].flush()


def _timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls          # us per call


def _operand(mode, N, H, W, px, seed, dev):
    from nemar_amd import ops
    g = torch.Generator(device=dev).manual_seed(seed)
    if mode == ops.GRID_UNET:
        f = F.interpolate(torch.randn(N, 2, 4, 5, device=dev, generator=g), size=(H, W), mode='bicubic')
        return (f * (px * 2.0 / W / f.abs().max())).contiguous()
    th = torch.zeros(N, 6, device=dev)
    th[:, 2], th[:, 5] = px * 2.0 / W, -px * 2.0 / H
    th[:, 1] = 0.01 * min(px, 1.0)
    return th


def kernels(rounds, calls):
    from nemar_amd import ops
    L, P, U, A = ops.L, ops._p, ops.GRID_UNET, ops.GRID_AFFINE
    dev = torch.device('cuda:0')
    emit('# kernels: rounds %d x %d calls, medians [min .. max] in us per call' % (rounds, calls))
    for (N, H, W) in SHAPES:
        for fname, px in FIELDS:
            g = torch.Generator(device=dev).manual_seed(1)
            gout = torch.randn(N, 2, H, W, device=dev, generator=g)
            out = torch.empty(N, 2, H, W, device=dev)
            variants = []
            for m1, m2 in ((U, U), (U, A), (A, U), (A, A)):
                first, second = _operand(m1, N, H, W, px, 2, dev), _operand(m2, N, H, W, px, 3, dev)
                gfirst, gsecond = torch.empty_like(first), torch.empty_like(second)
                wsb = L.compose_pred_bwd_workspace(m1, m2, N, H, W)
                ws = torch.zeros(wsb // 4 + 64, dtype=torch.float32, device=dev)
                name = 'UA'[m1 == A] + 'UA'[m2 == A]

                def fwd(first=first, second=second, m1=m1, m2=m2):
                    L.compose_pred(P(first), m1, H, W, P(second), m2, H, W, P(out), None, None, 0, N, H, W, ops._stream())

                def bwd(first=first, second=second, m1=m1, m2=m2, gfirst=gfirst, gsecond=gsecond, ws=ws, wsb=wsb):
                    L.compose_pred_bwd(P(first), m1, H, W, P(second), m2, H, W, P(gout), P(gfirst), 0, P(gsecond), 0, P(ws), wsb, N, H, W,
                                       ops._stream())
                variants += [('compose %s forward' % name, fwd), ('compose %s backward' % name, bwd)]
            u, gu = _operand(U, N, H, W, px, 3, dev), torch.empty(N, 2, H, W, device=dev)
            svf_b = L.svf_step_bwd_workspace(N, H, W)
            svf_ws = torch.zeros(svf_b // 4 + 64, dtype=torch.float32, device=dev)
            variants.append(('svf step backward (s = 1)', lambda: L.svf_step_bwd(P(u), 1.0, P(gout), P(gu), 0, P(svf_ws), svf_b, N, H, W, ops._stream())))
            for _, fn in variants:                                             # warm-up: code objects, clocks
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {name: [] for name, _ in variants}
            for _ in range(rounds):
                for name, fn in variants:
                    times[name].append(_timed(fn, calls))
            emit('%d x 2 x %d x %d, %s (%g px)' % (N, H, W, fname, px))
            med = {}
            for name, _ in variants:
                t = sorted(times[name])
                med[name] = statistics.median(t)
                emit('  %-28s %9.1f us [%9.1f .. %9.1f]' % (name, med[name], t[0], t[-1]))
            emit('  compose UU backward: 40 B/px of tensors = %.1f GB/s;  against the svf step backward: %.2f x its time'
                 % (N * H * W * 40 / med['compose UU backward'] / 1e3, med['compose UU backward'] / med['svf step backward (s = 1)']))


def step_time(step_rounds, ck):
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    from nemar_amd.train import _Options
    size = 256
    emit('# step: UNet STN, %d x %d, batch 2, ngf = ndf = 8, resnet_3blocks, --stn_no_identity_init; ms per optimize_parameters(), median of %d '
         'after 10 warm-up steps' % (size, size, step_rounds))
    for passes in (1, 2, 3):
        opt = _Options().parse(['--model', 'nemar', '--stn_type', 'unet', '--netG', 'resnet_3blocks', '--ngf', '8', '--ndf', '8', '--dataset_mode',
                                'gpupairs', '--dataroot', 'synthetic', '--img_height', str(size), '--img_width', str(size), '--crop_size', str(size),
                                '--load_size', str(size + 12), '--batch_size', '2', '--pool_size_pairs', '6', '--checkpoints_dir', ck, '--name',
                                'passes_%d' % passes, '--no_dropout', '--gpu_ids', '0', '--lambda_smooth', '1.0', '--stn_no_identity_init',
                                '--train_passes', str(passes)], quiet=True)
        torch.manual_seed(7)
        data = next(iter(create_dataset(opt)))
        torch.manual_seed(11)
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
        emit('  --train_passes %d  %8.3f ms [%8.3f .. %8.3f]' % (passes, statistics.median(ms), ms[0], ms[-1]))
        del model


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--step_rounds', type=int, default=21)
    ap.add_argument('--skip_kernels', action='store_true')
    ap.add_argument('--skip_step', action='store_true')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'profiles', 'compose_grad.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('compose_grad_record: no GPU — a timing from anything else would say nothing')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    _record[0] = open(a.out, 'w')
    emit('# %s' % torch.cuda.get_device_name(0))
    with tempfile.TemporaryDirectory() as ck:
        if not a.skip_kernels:
            kernels(a.rounds, a.calls)
        if not a.skip_step:
            step_time(a.step_rounds, ck)
    _record[0].close()
