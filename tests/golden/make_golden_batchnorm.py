"""Generate the `--norm batch` fixtures by IMPORTING THE REFERENCE in the build container (as make_golden.py does) and recording what its
own code computes.  Data only; nothing of the reference is stored but its outputs.

  state_dict_keys_batchnorm.json   the state_dict keys and shapes of the reference's define_G / define_D with norm='batch' for every
                                   generator x discriminator the BatchNorm tests use, and the per-tensor init statistics (numel, mean,
                                   std) of define_G / define_D with norm='batch' (reference models/networks.py:62-113)
  step_bn_<name>.npz               per configuration of tests/bn_configs.py, the reference's NEMARModel in fp32 AND fp64 on the same
                                   seeded weights / inputs: full_step_record rows of every step (step k > 0: step_bn_<name>_s<k>.npz)
                                   plus bn_record (every BatchNorm buffer, one eval-mode forward of T)

    python tests/golden/make_golden_batchnorm.py [--only keys|<config name>]
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, '/root/reference')
tb = types.ModuleType('torch.utils.tensorboard')
tb.SummaryWriter = object
sys.modules['torch.utils.tensorboard'] = tb          # the only missing import on the model's import path

import torch  # noqa: E402

import seeded  # noqa: E402
from bn_configs import BN_CONFIGS, bn_opt, bn_record, seed_model  # noqa: E402
from full_record import full_step_record  # noqa: E402
from step_configs import hw  # noqa: E402

GENERATORS = ['resnet_9blocks', 'resnet_6blocks', 'resnet_3blocks', 'unet_256', 'unet_128']
DISCRIMINATORS = [('basic', 3), ('n_layers', 4), ('pixel', 3)]


def net_keys():
    from models import networks as ref_networks
    out = {'G': {}, 'D': {}}
    for g in GENERATORS:
        for drop in (False, True):
            net = ref_networks.define_G(3, 3, 16, g, 'batch', drop, 'normal', 0.02, [])
            out['G']['%s/dropout%d' % (g, drop)] = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    for d, n in DISCRIMINATORS:
        net = ref_networks.define_D(6, 16, d, n, 'batch', 'normal', 0.02, [])
        out['D']['%s/%d' % (d, n)] = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    return out


def init_stats():
    from models import networks as ref_networks
    torch.manual_seed(1234)
    nets = {'T': ref_networks.define_G(3, 3, 64, 'resnet_9blocks', 'batch', True, 'normal', 0.02, []),
            'D': ref_networks.define_D(6, 64, 'basic', 3, 'batch', 'normal', 0.02, [])}
    out = {}
    for nm, net in nets.items():
        out[nm] = [[k, int(v.numel()), float(v.double().mean()), float(v.double().std()) if v.numel() > 1 else 0.0]
                   for k, v in net.state_dict().items()]
    return out


def run_bn_config(name, cfg):
    from models.nemar_model import NEMARModel
    A, B = seeded.seeded_images(cfg['batch'], 3, *hw(cfg), cfg['seed'])
    outs = [{} for _ in range(cfg.get('steps', 1))]
    for tag, dt in (('f32', torch.float32), ('f64', torch.float64)):
        t0 = time.time()
        torch.set_default_dtype(dt)
        try:
            opt = bn_opt(cfg)
            torch.manual_seed(0)
            m = NEMARModel(opt)
            m.setup(opt)
            seed_model(m, cfg)
            assert next(m.netT.parameters()).dtype == dt
            for s in range(cfg.get('steps', 1)):
                rec = full_step_record(m, A, B, cfg['seed'])
                rec.update(bn_record(m, A, cfg['seed']))
                for k, v in rec.items():
                    outs[s]['%s/%s' % (tag, k)] = np.asarray(v, dtype=np.float64)
        finally:
            torch.set_default_dtype(torch.float32)
        print(name, tag, '%.1fs' % (time.time() - t0), flush=True)
        del m
    for s, out in enumerate(outs):
        np.savez_compressed(os.path.join(HERE, 'step_%s%s.npz' % (name, '_s%d' % s if s else '')), **out)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default=None)
    a = ap.parse_args()
    if a.only in (None, 'keys'):
        data = {'keys': net_keys(), 'init_stats': init_stats()}
        with open(os.path.join(HERE, 'state_dict_keys_batchnorm.json'), 'w') as f:
            json.dump(data, f, indent=0)
        print('wrote', {k: len(v) for k, v in data['keys'].items()})
    for name, cfg in BN_CONFIGS.items():
        if a.only in (None, name):
            run_bn_config(name, cfg)
