"""`--norm batch` step configurations shared by the fixture generator (tests/golden/make_golden_batchnorm.py, which runs the REFERENCE)
and the GPU step-parity test (tests/test_batchnorm_step_gpu.py, which runs the build): network choice, size, batch, seeds.  Every
configuration runs with no_dropout (the build's dropout masks differ from torch's by design)."""
import numpy as np

import seeded
from step_configs import make_opt

_AFFINE_R = {'net.local.2.weight': 0.02, 'net.local.2.bias': 0.05}
_UNET_R = {'offset_map.output.conv2d.weight': 0.02}

BN_CONFIGS = {
    'bn_c1': dict(stn_type='affine', netG='resnet_6blocks', netD='basic', n_layers_D=3, ngf=32, ndf=32, size=128, batch=4, seed=71,
                  lambda_smooth=0.5, steps=2, overrides_R=_AFFINE_R),
    'bn_c3': dict(stn_type='unet', netG='resnet_9blocks', netD='basic', n_layers_D=3, ngf=16, ndf=16, size=256, batch=2, seed=89,
                  lambda_smooth=10.0, multi_resolution=2, steps=1, overrides_R=_UNET_R),
    'bn_unet': dict(stn_type='unet', netG='unet_256', netD='n_layers', n_layers_D=4, ngf=16, ndf=16, size=256, batch=2, seed=79,
                    lambda_smooth=10.0, gan_mode='lsgan', steps=1, overrides_R=_UNET_R),
    'bn_pixel': dict(stn_type='affine', netG='resnet_3blocks', netD='pixel', n_layers_D=3, ngf=16, ndf=16, size=128, batch=2, seed=83,
                     lambda_smooth=0.5, steps=1, overrides_R=_AFFINE_R),
}

BN_SUFFIXES = ('running_mean', 'running_var', 'num_batches_tracked')


def bn_opt(cfg, gpu_ids=()):
    opt = make_opt(cfg, gpu_ids=gpu_ids)
    opt.norm, opt.netD, opt.n_layers_D = 'batch', cfg['netD'], cfg['n_layers_D']
    return opt


def bn_seeded_state_dict(shapes, seed, overrides=None):
    """seeded.seeded_state_dict with the BatchNorm entries set to values a trained layer could hold — weight near 1, bias small,
    running_mean small, running_var positive, counter 0 — instead of the uniform noise (which would give negative variances).
    `shapes`: key -> shape in state_dict order.  Values: float32 arrays (the counter: an int64 0-d array)."""
    # (the 0-d counters are drawn as 1-element tensors — same stream indices — and replaced below)
    out = seeded.seeded_state_dict({k: (tuple(v) or (1,)) for k, v in shapes.items()}, seed, overrides)
    prefixes = [k[:-len('running_mean')] for k in shapes if k.endswith('running_mean')]
    for i, p in enumerate(prefixes):
        C = int(shapes[p + 'weight'][0])
        u = [seeded.uniform((C,), seed + 7919, 4 * i + j) for j in range(4)]
        out[p + 'weight'] = (1.0 + 0.1 * u[0]).astype(np.float32)
        out[p + 'bias'] = (0.05 * u[1]).astype(np.float32)
        out[p + 'running_mean'] = (0.1 * u[2]).astype(np.float32)
        out[p + 'running_var'] = (1.0 + 0.5 * np.abs(u[3])).astype(np.float32)
        out[p + 'num_batches_tracked'] = np.array(0, dtype=np.int64)
    return out


def load_bn_seeded(net, seed, overrides):
    import torch
    sd = net.state_dict()
    new = bn_seeded_state_dict({k: tuple(v.shape) for k, v in sd.items()}, seed, overrides)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in new.items()})


def seed_model(m, cfg):
    load_bn_seeded(m.netT, cfg['seed'] + 1, cfg.get('overrides_T'))
    load_bn_seeded(m.netR, cfg['seed'] + 2, cfg.get('overrides_R'))
    load_bn_seeded(m.netD, cfg['seed'] + 3, cfg.get('overrides_D'))
    for i, d in enumerate(m.netD_multiresolution):
        load_bn_seeded(d, cfg['seed'] + 10 + i, cfg.get('overrides_D'))


def bn_record(m, A, seed):
    """What the BatchNorm state of a model is reduced to after a step: every BatchNorm buffer (sum, abs-sum and seeded projection of the
    running statistics, the counter), and one eval-mode forward of T on A (mean, abs-mean, projection)."""
    import torch
    from full_record import proj
    out = {}
    nets = [('T', m.netT), ('D', m.netD)] + [('Dmr%d' % i, d) for i, d in enumerate(m.netD_multiresolution)]
    for nm, net in nets:
        for j, (k, b) in enumerate(net.named_buffers()):
            if k.endswith('num_batches_tracked'):
                out['bncount/%s/%s' % (nm, k)] = int(b)
            elif k.endswith(BN_SUFFIXES):
                out['bnsum/%s/%s' % (nm, k)] = b.detach().double().sum().item()
                out['bnabs/%s/%s' % (nm, k)] = b.detach().double().abs().sum().item()
                out['bnproj/%s/%s' % (nm, k)] = proj(b, seed, 2000 + j)
    p0 = next(m.netT.parameters())
    a = torch.from_numpy(A).to(p0.device, p0.dtype)
    was = m.netT.training
    m.netT.eval()
    with torch.no_grad():
        t = m.netT(a)
    m.netT.train(was)
    out['mean/eval_T'], out['absmean/eval_T'] = t.double().mean().item(), t.double().abs().mean().item()
    out['proj/eval_T'] = proj(t, seed, 2999)
    return out
