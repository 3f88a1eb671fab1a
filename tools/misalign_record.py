"""A record, not a test and not a gate: what the registration-error meter sees while NeMAR trains on known-misalignment pairs.

Runs N seeded steps (default 300) per STN type (affine at 128 x 128, UNet at 256 x 256; reduced widths, batch 8) on `--synthetic_pairs mapped
--misalign both` and prints the registration/* numbers every --every steps, then the achieved bandwidth of the deforming sampler next to
nemar_crop_flip_normalize at the same shape in the same process (warm-up, HIP events, median of repeats).  No threshold is attached to
anything: whether a few hundred steps of GAN training reduce the error on a synthetic texture is what the tool is there to find out.

    python tools/misalign_record.py [--steps 300] [--every 25] [--out profiles/misalign_record.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


_record = [None]


def emit(line):
    """a line of the record: to the record file as it comes (stdout also carries the model's own banners)"""
    print(line)
    sys.stdout.flush()
    if _record[0] is not None:
        _record[0].write(line + '\n')
        _record[0].flush()


def curve(stn, size, steps, every, batch, ck):
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    from nemar_amd.train import _Options
    from nemar_amd.util.visualizer import RegistrationMeter
    opt = _Options().parse(['--model', 'nemar', '--stn_type', stn, '--netG', 'resnet_3blocks', '--ngf', '16', '--ndf', '16', '--dataset_mode',
                            'gpupairs', '--dataroot', 'synthetic', '--synthetic_pairs', 'mapped', '--misalign', 'both', '--img_height', str(size),
                            '--img_width', str(size), '--crop_size', str(size), '--load_size', str(size + 30), '--batch_size', str(batch),
                            '--pool_size_pairs', '64', '--checkpoints_dir', ck, '--name', 'record_' + stn, '--gpu_ids', '0', '--lambda_smooth',
                            '10' if stn == 'unet' else '0'], quiet=True)
    torch.manual_seed(7)
    dataset = create_dataset(opt)
    model = create_model(opt)
    model.setup(opt)
    meter = RegistrationMeter(model.device)
    emit('# %s STN, %d x %d, batch %d, ngf = ndf = 16, resnet_3blocks, --misalign both (defaults), mapped synthetic pairs, seed 7' % (stn, size, size, batch))
    emit('# %6s %10s %14s %10s %10s %10s   (means over the steps since the previous row)' % ('step', 'epe_px', 'epe_before_px', 'max_px', 'fold_frac',
                                                                                              'valid_frac'))
    step = 0
    while step < steps:
        for data in dataset:
            model.set_input(data)
            model.optimize_parameters()
            pred, mode = model.netR.last_prediction()
            meter.update(pred, mode, model.gt_field)
            step += 1
            if step % every == 0 or step == steps:
                s = meter.read()
                emit('  %6d %10.4f %14.4f %10.3f %10.5f %10.4f' % (step, s['epe_px'], s['epe_before_px'], s['max_px'], s['fold_frac'], s['valid_frac']))
            if step >= steps:
                break


def event_time(fn, warmup=10, iters=20, repeats=7):
    """median over `repeats` of the mean time of `iters` back-to-back launches between two HIP events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / iters)
    return statistics.median(out), min(out), max(out)


def bandwidth():
    from nemar_amd import ops
    dev = torch.device('cuda:0')
    emit('# sampler bandwidth: compulsory bytes (pool texels read once + output written [+ the field read]) / median time; min .. max of 7 repeats')
    for (B, C, H, W, Hc, Wc) in ((8, 3, 286, 286, 256, 256), (8, 3, 542, 542, 512, 512), (16, 3, 1054, 1054, 1024, 1024)):
        g = torch.Generator(device=dev).manual_seed(1)
        pool = torch.rand(64, C, H, W, device=dev, generator=g)
        par = torch.stack([torch.randint(0, 64, (B,), generator=g, device=dev), torch.randint(0, H - Hc + 1, (B,), generator=g, device=dev),
                           torch.randint(0, W - Wc + 1, (B,), generator=g, device=dev), torch.randint(0, 2, (B,), generator=g, device=dev)], 1).int().contiguous()
        params = torch.zeros(B, 6 + 72, device=dev)
        params[:, 0] = params[:, 4] = 1.0
        params[:, 6:] = (torch.rand(B, 72, device=dev, generator=g) - 0.5) * 16
        field = ops.deform_field(params, B, Hc, Wc, 6, 6)
        y = torch.empty(B, C, Hc, Wc, device=dev)
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        plain = event_time(lambda: ops.L.crop_flip_normalize(P(pool), P(par), P(y), 64, B, C, H, W, Hc, Wc, 1.0, st()))
        deform = event_time(lambda: ops.L.crop_flip_deform_normalize(P(pool), P(par), P(field), P(y), 64, B, C, H, W, Hc, Wc, 1.0, st()))
        fld = event_time(lambda: ops.L.deform_field(P(params), P(field), B, Hc, Wc, 6, 6, st()))
        px = B * Hc * Wc
        for name, t, nbytes in (('crop_flip_normalize', plain, px * C * 8), ('crop_flip_deform_normalize', deform, px * (C * 8 + 8)),
                                ('deform_field (6 x 6 lattice)', fld, px * 8)):
            emit('  [%2d,%d,%4d,%4d] %-30s %8.1f us (%.1f .. %.1f)  %7.1f GB/s' % (B, C, Hc, Wc, name, t[0] * 1e6, t[1] * 1e6, t[2] * 1e6,
                                                                                  nbytes / t[0] / 1e9))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--every', type=int, default=25)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--skip_curves', action='store_true')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'misalign_record.txt'))
    a = ap.parse_args()
    _record[0] = open(a.out, 'w')
    emit('# %s' % torch.cuda.get_device_name(0))
    with tempfile.TemporaryDirectory() as ck:
        if not a.skip_curves:
            for stn, size in (('affine', 128), ('unet', 256)):
                curve(stn, size, a.steps, a.every, a.batch, ck)
        bandwidth()
    _record[0].close()
