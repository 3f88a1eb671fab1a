"""A record, not a test and not a gate: what composing predictions (csrc/compose.hip, NEMARModel.cascade) does on one MI355X.

1. The float64 table of tests/compose_cases.py on the gfx950 library: kernel error, numpy-fp32 error and their ratio per case.
2. Whether a cascade helps THIS model: N seeded steps (default 300) per STN type on `--synthetic_pairs mapped --misalign both`, as
   tools/misalign_record.py trains them, then registration_error() after 1, 2 and 3 passes on held-out seeded batches (another
   --data_seed: other textures, other misalignments).  Nobody has measured this; no threshold is attached.
3. The fused compose + warp launch against compose followed by nemar_warp_resampled_fwd, at 8 x 3 x 256^2 and 4 x 3 x 1024^2: alternating
   calls in one process, HIP events, median of repeats, outputs checked equal bit for bit first.  The fused form saves 8 B/px of field
   re-read and one launch; the ratio is written down whatever it is.

    python tools/cascade_record.py [--steps 300] [--held_out 8] [--out tools/profiles/cascade_record.txt]
"""
import argparse
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402


_record = [None]


def emit(line):
    """a line of the record: to the record file as it comes (stdout also carries the model's own banners)"""
    print(line)
    sys.stdout.flush()
    if _record[0] is not None:
        _record[0].write(line + '\n')
        _record[0].flush()


def float64_table():
    import compose_cases as K
    from backends import HipBackend
    from nemar_amd import _lib
    be = HipBackend(_lib.load())
    emit('# nemar_compose_pred against float64 (tests/compose_cases.py case_float64, N = 2): max-abs error in pixels; the bound is ratio <= %g' % K.MARGIN)
    emit('# %-5s %-10s %-10s %-10s %5s %12s %12s %7s' % ('modes', 'first', 'second', 'output', 'amp', 'kernel', 'numpy-fp32', 'ratio'))
    for size, amp in [(s, 0.15) for s in K.SIZES] + [(K.RAGGED, 1.5)]:
        for m1, m2 in K.MODE_PAIRS:
            err, yard = K.case_float64(be, size, m1, m2, amp=amp)
            emit('  %-5s %-10s %-10s %-10s %5g %12.3e %12.3e %7.2f' % ('UA'[m1 == K.A] + 'UA'[m2 == K.A], *('%dx%d' % s for s in size), amp, err, yard,
                                                                      err / yard if yard else 0.0))


def _options(stn, size, batch, ck, seed):
    from nemar_amd.train import _Options
    return _Options().parse(['--model', 'nemar', '--stn_type', stn, '--netG', 'resnet_3blocks', '--ngf', '16', '--ndf', '16', '--dataset_mode',
                             'gpupairs', '--dataroot', 'synthetic', '--synthetic_pairs', 'mapped', '--misalign', 'both', '--img_height', str(size),
                             '--img_width', str(size), '--crop_size', str(size), '--load_size', str(size + 30), '--batch_size', str(batch),
                             '--pool_size_pairs', '64', '--checkpoints_dir', ck, '--name', 'cascade_' + stn, '--gpu_ids', '0', '--lambda_smooth',
                             '10' if stn == 'unet' else '0', '--data_seed', str(seed)], quiet=True)


def cascade_error(stn, size, steps, held_out, batch, ck):
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    opt = _options(stn, size, batch, ck, 1234)
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
    emit('# %s STN, %d x %d, batch %d, ngf = ndf = 16, resnet_3blocks, --misalign both (defaults), mapped synthetic pairs, seed 7, %d steps;' %
         (stn, size, size, batch, steps))
    emit('# registration_error() on %d held-out batches (--data_seed 4321), means over the batches' % held_out)
    emit('# %6s %10s %14s %10s %10s' % ('passes', 'epe_px', 'epe_before_px', 'fold_frac', 'valid_frac'))
    batches = []
    for data in create_dataset(_options(stn, size, batch, ck, 4321)):
        batches.append(data)
        if len(batches) >= held_out:
            break
    for passes in (1, 2, 3):
        rows = []
        for data in batches:
            model.set_input(data)
            model.cascade(passes)
            rows.append(model.registration_error())
        mean = lambda k: statistics.fmean(r[k] for r in rows)
        emit('  %6d %10.4f %14.4f %10.5f %10.4f' % (passes, mean('epe_px'), mean('epe_before_px'), mean('fold_frac'), mean('valid_frac')))


def alternating(fns, warmup=10, iters=20, repeats=9):
    """per function: (median, min, max) over `repeats` of the mean time of `iters` back-to-back calls between two HIP events; the
    functions take turns inside every repeat, so that a drift of the machine meets all of them"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) * 1e-3 / iters)
    return [(statistics.median(t), min(t), max(t)) for t in out]


def fused_against_two_launches():
    from nemar_amd import ops
    dev = torch.device('cuda:0')
    emit('# compose + warp in ONE launch against nemar_compose_pred then nemar_warp_resampled_fwd (two UNet fields at the image size, preallocated')
    emit('# outputs, C-ABI calls): median us of 9 repeats x 20 calls, alternating (min .. max); outputs equal bit for bit')
    P = ops._p
    for (N, C, H, W) in ((8, 3, 256, 256), (4, 3, 1024, 1024)):
        g = torch.Generator(device=dev).manual_seed(1)
        first = (torch.rand(N, 2, H, W, device=dev, generator=g) - 0.5) * 0.1
        second = (torch.rand(N, 2, H, W, device=dev, generator=g) - 0.5) * 0.1
        img = torch.rand(N, C, H, W, device=dev, generator=g)
        f_a, f_b, o_a, o_b = torch.empty_like(first), torch.empty_like(first), torch.empty_like(img), torch.empty_like(img)
        U = ops.GRID_UNET

        def fused():
            ops.L.compose_pred(P(first), U, H, W, P(second), U, H, W, P(f_a), P(img), P(o_a), C, N, H, W, ops._stream())

        def two():
            ops.L.compose_pred(P(first), U, H, W, P(second), U, H, W, P(f_b), None, None, 0, N, H, W, ops._stream())
            ops.L.warp_resampled_fwd(P(img), P(f_b), U, 0, P(o_b), N, C, H, W, H, W, H, W, ops._stream())

        fused()
        two()
        torch.cuda.synchronize()
        if not (torch.equal(f_a, f_b) and torch.equal(o_a, o_b)):
            raise SystemExit('fused and two-launch outputs differ at %s' % ((N, C, H, W),))
        (tf, tf0, tf1), (tt, tt0, tt1) = alternating([fused, two])
        emit('  [%d,%d,%4d,%4d] fused %8.1f us (%.1f .. %.1f)   two launches %8.1f us (%.1f .. %.1f)   fused / two = %.3f' %
             (N, C, H, W, tf * 1e6, tf0 * 1e6, tf1 * 1e6, tt * 1e6, tt0 * 1e6, tt1 * 1e6, tf / tt))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--held_out', type=int, default=8)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--skip_training', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tools', 'profiles', 'cascade_record.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/cascade_record.py measures on an MI355X: no GPU here, nothing is recorded')
    _record[0] = open(a.out, 'w')
    emit('# %s' % torch.cuda.get_device_name(0))
    float64_table()
    fused_against_two_launches()
    with tempfile.TemporaryDirectory() as ck:
        if not a.skip_training:
            for stn, size in (('affine', 128), ('unet', 256)):
                cascade_error(stn, size, a.steps, a.held_out, a.batch, ck)
    _record[0].close()
