"""`-m gpu`: NEMARModel.optimize_parameters() with `--norm batch` against fixtures recorded from the REFERENCE itself
(tests/golden/make_golden_batchnorm.py: the reference's NEMARModel in fp32 AND fp64 on the same seeded weights and inputs,
tests/bn_configs.py), with the batched passes on (the default: T and D over stacked batches under ops.norm_segments) and off (the
reference's call order).  Compared per step: the losses, images, deformation, gradient rows and post-Adam checksums with
tests/test_step_full_gpu.compare's fp32-vs-fp64 tolerances; every BatchNorm buffer after the step (sum, abs-sum and projection of the
running statistics, on the same footing) and the counters exactly (2 per step for T, 5 for each discriminator); one eval-mode
forward of T on real_A."""
import os

import numpy as np
import pytest
import torch

import seeded
from bn_configs import BN_CONFIGS, bn_opt, bn_record, seed_model
from full_record import full_step_record
from step_configs import hw
from test_step_full_gpu import GOLD, _f32_tags, compare

pytestmark = pytest.mark.gpu

BN_BASE_REL, BN_BASE_ABS = 2e-5, 1e-6


def build(cfg):
    from nemar_amd.models import create_model
    opt = bn_opt(cfg, gpu_ids=[0])
    m = create_model(opt)
    m.setup(opt)
    seed_model(m, cfg)
    return m


def compare_bn(fixture, rec, slack=1.0):
    """rows (quantity, err, tol, ok) of the BatchNorm buffer rows (and, with `extra`, of further scalar rows); the counters must be equal.
    tol = base + 4 * slack * gap, gap = max(the quantity's own |f32 - f64|, the 90th-percentile relative gap of its class in its network
    x its scale): one quantity's own gap is a single draw of a heavy-tailed quantity, as test_step_full_gpu.compare says of gradient rows."""
    g = np.load(os.path.join(GOLD, 'step_%s.npz' % fixture))
    items = []
    for k in sorted(g.files):
        if not k.startswith('f64/') or k[4:] not in rec:
            continue
        q = k[4:]
        cls, tail = q.split('/', 1)
        want = float(g[k])
        if cls == 'bncount':
            items.append((q, cls, None, want, 0.0, 0.0))
            continue
        scale = max(float(g['f64/bnabs/' + tail]), 1e-30) if cls.startswith('bn') else max(abs(want), 1.0)
        gap = max(abs(float(g['%s/%s' % (t, q)]) - want) for t in _f32_tags(g))
        items.append((q, cls, tail.split('/')[0] if cls.startswith('bn') else cls, want, scale, gap))
    groups = {}
    for q, cls, net, want, scale, gap in items:
        if net is not None:
            groups.setdefault((cls, net), []).append(gap / scale)
    p90 = {key: float(np.quantile(v, 0.9)) for key, v in groups.items()}
    rows = []
    for q, cls, net, want, scale, gap in items:
        got = float(rec[q])
        if cls == 'bncount':
            rows.append((q, abs(got - want), 0.0, got == want))
            continue
        gap = max(gap, p90[(cls, net)] * scale)
        tol = BN_BASE_REL * scale + BN_BASE_ABS + 4.0 * slack * gap
        err = abs(got - want)
        rows.append((q, err, tol, err <= tol))
    return rows


# A second step runs free from the state the first one left: Adam's first update moves every element by lr * sign(g), so an element
# whose gradient sits at rounding distance of zero moves by 2 lr between ANY two fp32 implementations and every quantity of the second
# step inherits that.  The reference's one fp32-vs-fp64 gap samples it once: the BatchNorm and eval-mode rows of a second step take twice
# the gap.
SECOND_STEP_SLACK = 2.0


@pytest.mark.parametrize("batched", ["1", "0"])
@pytest.mark.parametrize("name", list(BN_CONFIGS))
def test_batchnorm_step_vs_reference(name, batched, monkeypatch):
    monkeypatch.setenv("NEMAR_BATCHED_PASSES", batched)
    cfg = BN_CONFIGS[name]
    m = build(cfg)
    assert m._batched == (batched == "1")
    A, B = seeded.seeded_images(cfg['batch'], 3, *hw(cfg), cfg['seed'])
    fan_in = {'R/' + k: int(p.shape[1]) for k, p in m.netR.named_parameters() if p.dim() == 2}
    n_mr = len(m.netD_multiresolution)
    for s in range(cfg.get('steps', 1)):
        rec = full_step_record(m, A, B, cfg['seed'])
        bn = bn_record(m, A, cfg['seed'])
        torch.cuda.synchronize()
        counts = {k: v for k, v in bn.items() if k.startswith('bncount/')}
        assert any(k.startswith('bncount/T/') for k in counts) and any(k.startswith('bncount/D/') for k in counts)
        for k, v in counts.items():
            assert v == (2 if k.startswith('bncount/T/') else 5) * (s + 1), (k, v)
        assert any(k.startswith('bncount/Dmr') for k in counts) == (n_mr > 0)
        fixture = name + ('_s%d' % s if s else '')
        if s == 0:
            rec.update({k: v for k, v in bn.items() if not k.startswith('bn')})      # the eval-mode forward of T: mean / absmean / proj rows
        rows = compare(fixture, rec, report=os.environ.get('NEMAR_FULL_REPORT'), fan_in=fan_in)
        rows_bn = compare_bn(fixture, bn, slack=1.0 if s == 0 else SECOND_STEP_SLACK)
        assert len(rows) > 40 and len(rows_bn) > 10, (len(rows), len(rows_bn))
        assert any(r[0] == 'proj/eval_T' for r in rows + rows_bn)
        bad = [r for r in rows + rows_bn if not r[3]]
        assert not bad, (fixture, len(bad), bad[:8])
