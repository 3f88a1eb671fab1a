"""Two records of the soft-Dice loss (csrc/dice.hip, --lambda_dice), no gate on either:

  timing    ops.dice_loss forward + backward (the sums, the finalising workgroup and the gather) next to ops.label_overlap — the score whose
            Dice the loss makes differentiable — and ops.epe_loss forward + backward on the same shapes: 8 x 256^2 (the training size)
            and 8 x 1024^2, K = 4 and 64, UNet offsets and affine dtheta, on BLOCKY maps (the K-level quantisation of a smooth
            function: most 2 x 2 cells hold one class, a pixel makes one LDS add to M and one to I) and on PER-PIXEL-RANDOM maps (four
            classes per cell: four adds to M, a wave spreads over all counters).  The prediction is a smooth field of a few pixels.  One
            process; the calls ALTERNATE inside every round, each timed by device events around `--calls` back-to-back calls; a figure is
            the MEDIAN over `--rounds` rounds (min and max are printed: the spread).
  training  the seeded `--misalign both --synthetic_pairs mapped --labels 4` UNet run of tools/epe_record.py, `--steps` steps, once with
            --lambda_dice 0 and once with it on; before and afterwards the HARD Dice (ops.label_overlap: nearest sampling, mean over the
            foreground classes present) on `--eval_batches` further batches of the same seeded stream, which no step trained on, next to
            the Dice of the unregistered pairs.

    python tools/dice_record.py [--steps 300] [--lambda_dice 10] [--out tools/profiles/dice_loss.txt]"""
import argparse
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = ((8, 256, 256), (8, 1024, 1024))
CLASSES = (4, 64)
_record = [None]


def emit(line):
    print(line)
    sys.stdout.flush()
    if _record[0] is not None:
        _record[0].write(line + '\n')
        _record[0].flush()


def _smooth(N, C, H, W, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    d = F.interpolate(torch.randn(N, C, 4, 5, device=dev, generator=g), size=(H, W), mode='bicubic')
    return (d / d.abs().max()).contiguous()


def _maps(kind, N, H, W, K, dev):
    if kind == 'blocky':
        f = _smooth(N, 1, H + 8, W + 8, 4, dev)[:, 0] * 0.5 + 0.5
        q = (f * K).floor().clamp_(0, K - 1)
        return q[:, 4:4 + H, 4:4 + W].contiguous(), q[:, 2:2 + H, 7:7 + W].contiguous()
    g = torch.Generator(device=dev).manual_seed(5)
    return (torch.randint(0, K, (N, H, W), device=dev, generator=g).float(), torch.randint(0, K, (N, H, W), device=dev, generator=g).float())


def timing(rounds, calls):
    from nemar_amd import ops
    dev = torch.device('cuda:0')
    emit('# timing: rounds %d x %d calls, us per call, medians [min .. max]' % (rounds, calls))
    for (N, H, W) in SHAPES:
        gt = (_smooth(N, 2, H, W, 1, dev) * 6.0).contiguous()
        offsets = (_smooth(N, 2, H, W, 2, dev) * (8.0 / W)).contiguous()              # offsets of up to 4 px, normalised units
        dtheta = ((torch.rand(N, 6, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) - 0.5) * 0.04).contiguous()
        for label, pred0, mode in (('unet', offsets, ops.GRID_UNET), ('affine', dtheta, ops.GRID_AFFINE)):
            pred = pred0.clone().requires_grad_(True)

            def both(loss_fn):
                def run():
                    pred.grad = None
                    loss_fn().backward()
                return run
            variants = [('epe_loss fwd+bwd', both(lambda: ops.epe_loss(pred, mode, gt, 0.01)))]
            for K in CLASSES:
                for kind in ('blocky', 'random'):
                    lm, lf = _maps(kind, N, H, W, K, dev)
                    variants.append(('dice_loss fwd+bwd K=%-2d %s' % (K, kind), both(lambda lm=lm, lf=lf, K=K: ops.dice_loss(pred, mode, lm, lf, K))))
                    variants.append(('label_overlap    K=%-2d %s' % (K, kind), lambda lm=lm, lf=lf, K=K: ops.label_overlap(pred.detach(), mode, lm, lf, K)))
            for _, fn in variants:                                            # warm-up: code objects, clocks, the allocator's pools
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
            emit('%d x %d x %d %s' % (N, H, W, label))
            for name, _ in variants:
                t = sorted(times[name])
                emit('  %-34s %9.1f us [%9.1f .. %9.1f]' % (name, statistics.median(t), t[0], t[-1]))


def _hard_dice(counts):
    """mean over samples and the foreground classes present in either map of 2 inter / (moving + fixed)"""
    c = counts.double()
    den = c[..., 1] + c[..., 2]
    present = den[:, 1:] > 0
    d = 2 * c[..., 0][:, 1:] / den[:, 1:].clamp_min(1)
    return float(d[present].mean())


def training(lam, steps, batch, eval_batches, ck, K=4):
    from nemar_amd import ops
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    from nemar_amd.train import _Options
    size = 256
    opt = _Options().parse(['--model', 'nemar', '--stn_type', 'unet', '--netG', 'resnet_3blocks', '--ngf', '16', '--ndf', '16', '--dataset_mode',
                            'gpupairs', '--dataroot', 'synthetic', '--synthetic_pairs', 'mapped', '--misalign', 'both', '--labels', str(K),
                            '--img_height', str(size), '--img_width', str(size), '--crop_size', str(size), '--load_size', str(size + 30),
                            '--batch_size', str(batch), '--pool_size_pairs', '64', '--checkpoints_dir', ck, '--name', 'dice_%g' % lam,
                            '--gpu_ids', '0', '--lambda_smooth', '10', '--lambda_dice', str(lam)], quiet=True)
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
    before, after, seen = [], [], 0
    for data in dataset:                                                      # further batches of the stream: never trained on
        model.set_input(data)
        model.test()
        pred, mode = model.netR.last_prediction()
        ident = torch.zeros(pred.size(0), 6, device=pred.device)
        before.append(_hard_dice(ops.label_overlap(ident, ops.GRID_AFFINE, model.labels_A, model.labels_B, K)))
        after.append(_hard_dice(ops.label_overlap(pred, mode, model.labels_A, model.labels_B, K)))
        seen += 1
        if seen >= eval_batches:
            break
    emit('  --lambda_dice %-5g: after %d steps losses %s' % (lam, steps, '  '.join('%s %.4f' % kv for kv in losses.items())))
    emit('    held-out hard Dice (label_overlap, foreground classes): unregistered %.4f   registered %.4f' % (statistics.mean(before), statistics.mean(after)))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--eval_batches', type=int, default=4)
    ap.add_argument('--lambda_dice', type=float, default=10.0)
    ap.add_argument('--skip_training', action='store_true')
    ap.add_argument('--skip_timing', action='store_true')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'profiles', 'dice_loss.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('dice_record: no GPU — a timing from anything else would say nothing')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    _record[0] = open(a.out, 'w')
    emit('# %s' % torch.cuda.get_device_name(0))
    if not a.skip_timing:
        timing(a.rounds, a.calls)
    if not a.skip_training:
        emit('# training: UNet STN, 256 x 256, batch %d, ngf = ndf = 16, resnet_3blocks, --misalign both (defaults), mapped synthetic pairs, --labels 4, '
             'seed 7, --lambda_smooth 10; read-out on %d further batches of the stream' % (a.batch, a.eval_batches))
        with tempfile.TemporaryDirectory() as ck:
            for lam in (0.0, a.lambda_dice):
                training(lam, a.steps, a.batch, a.eval_batches, ck)
    _record[0].close()
