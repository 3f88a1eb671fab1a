"""CPU tier of `--norm batch`: the generator and discriminators built with BatchNorm have exactly the reference's state_dict keys and
shapes (checkpoints move in both directions), their initialisation matches the reference's statistically, and a checkpoint in the
reference's format loads with its running statistics and counters intact.  Expected values: tests/golden/state_dict_keys_batchnorm.json
(tests/golden/make_golden_batchnorm.py ran the reference's own define_G / define_D).  Nets are constructed, never run."""
import argparse
import json
import math
import os
from collections import OrderedDict

import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _fixture():
    with open(os.path.join(GOLD, 'state_dict_keys_batchnorm.json')) as f:
        return json.load(f)


def _layout(net):
    return [[k, list(v.shape)] for k, v in net.state_dict().items()]


@pytest.mark.parametrize("netG", ['resnet_9blocks', 'resnet_6blocks', 'resnet_3blocks', 'unet_256', 'unet_128'])
@pytest.mark.parametrize("dropout", [False, True])
def test_generator_state_dict_equals_reference(netG, dropout):
    from nemar_amd.models import networks
    want = _fixture()['keys']['G']['%s/dropout%d' % (netG, dropout)]
    net = networks.define_G(3, 3, 16, netG, 'batch', dropout, 'normal', 0.02, [])
    assert _layout(net) == want
    assert sum(isinstance(m, networks.BatchNormParams) for m in net.modules()) > 0


@pytest.mark.parametrize("netD,n_layers", [('basic', 3), ('n_layers', 4), ('pixel', 3)])
def test_discriminator_state_dict_equals_reference(netD, n_layers):
    from nemar_amd.models import networks
    want = _fixture()['keys']['D']['%s/%d' % (netD, n_layers)]
    assert _layout(networks.define_D(6, 16, netD, n_layers, 'batch', 'normal', 0.02, [])) == want


def test_other_norms_are_unchanged():
    """--norm instance / none build no BatchNorm containers and keep their key layouts"""
    from nemar_amd.models import networks
    for norm in ('instance', 'none'):
        for net in (networks.define_G(3, 3, 16, 'resnet_6blocks', norm, True, 'normal', 0.02, []),
                    networks.define_G(3, 3, 16, 'unet_128', norm, True, 'normal', 0.02, []),
                    networks.define_D(6, 16, 'basic', 3, norm, 'normal', 0.02, [])):
            assert not any(isinstance(m, networks.BatchNormParams) for m in net.modules())
            assert not [k for k in net.state_dict() if k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))]


@pytest.mark.parametrize("net", ['T', 'D'])
def test_init_statistics_match_reference(net):
    from nemar_amd.models import networks
    torch.manual_seed(4321)
    nets = {'T': lambda: networks.define_G(3, 3, 64, 'resnet_9blocks', 'batch', True, 'normal', 0.02, []),
            'D': lambda: networks.define_D(6, 64, 'basic', 3, 'batch', 'normal', 0.02, [])}
    want = _fixture()['init_stats'][net]
    sd = nets[net]().state_dict()
    assert [k for k, *_ in want] == list(sd.keys())
    for (k, n, mean, std), v in zip(want, sd.values()):
        assert v.numel() == n, k
        if k.endswith('num_batches_tracked'):
            assert v.dtype == torch.int64 and int(v) == 0, k
            continue
        v = v.double()
        if std == 0.0:                          # zero biases, running statistics 0 / 1
            assert float((v - mean).abs().max()) == 0.0, k
            continue
        s = float(v.std())
        assert abs(s - std) <= 5.0 * std * math.sqrt(1.0 / n) + 1e-12, (k, s, std)
        assert abs(float(v.mean()) - mean) <= 5.0 * std * math.sqrt(2.0 / n), (k, float(v.mean()), mean)


def test_checkpoint_in_reference_format_keeps_running_statistics(tmp_path):
    """BaseModel.load_networks on a `--norm batch` checkpoint (reference key names, `module.` prefixes of a DataParallel save): the
    running statistics and counters arrive as saved; an instance-norm network still drops such buffers."""
    from nemar_amd.models import networks
    from nemar_amd.models.base_model import BaseModel

    class _Holder:
        load_networks = BaseModel.load_networks
        _nets = BaseModel._nets

    torch.manual_seed(7)
    src = networks.define_G(3, 3, 8, 'resnet_3blocks', 'batch', False, 'normal', 0.02, [])
    sd = OrderedDict()
    for k, v in src.state_dict().items():
        if k.endswith('running_mean'):
            v = torch.randn_like(v)
        elif k.endswith('running_var'):
            v = torch.rand_like(v) + 0.5
        elif k.endswith('num_batches_tracked'):
            v = torch.tensor(1234, dtype=torch.long)
        sd['module.' + k] = v
    torch.save(sd, str(tmp_path / '5_net_T.pth'))
    h = _Holder()
    h.save_dir, h.model_names = str(tmp_path), ['T']
    h.netT = networks.define_G(3, 3, 8, 'resnet_3blocks', 'batch', False, 'normal', 0.02, [])
    h.load_networks(5)
    got = h.netT.state_dict()
    for k, v in sd.items():
        assert torch.equal(got[k[len('module.'):]], v), k
    # instance norm: a legacy checkpoint's norm buffers are dropped as before
    inst = networks.define_G(3, 3, 8, 'resnet_3blocks', 'instance', False, 'normal', 0.02, [])
    isd = OrderedDict(inst.state_dict())
    isd['model.2.running_mean'] = torch.zeros(8)
    torch.save(isd, str(tmp_path / '6_net_T.pth'))
    h.netT = inst
    h.load_networks(6)


def test_get_norm_layer_accepts_batch():
    from nemar_amd.models import networks
    assert networks.get_norm_layer('batch') == 'batch'
    with pytest.raises(NotImplementedError):
        networks.get_norm_layer('group')
