"""`-m gpu`: the soft-Dice loss above the kernels — ops.dice_loss's autograd node and ops.dice_sums against the entry points bit for bit,
label maps through the input pipeline (--labels K of the gpupairs dataset), and the term in the training step (--lambda_dice, --dice_eps,
--dice_classes, --dice_background) on known-misalignment batches of the mapped synthetic pool: absent or 0 with nothing changed, on as
one more loss and one more root of the translation + registration step, in both forward orders and as a captured step graph.  The
smallest configuration of the model tests (affine STN, 64 x 64, reduced widths)."""
import collections
import math

import numpy as np
import pytest
import torch

import dice_cases as K
from backends import HipBackend, _launches
from register_cases import GRID_AFFINE, GRID_UNET

pytestmark = pytest.mark.gpu

TODAY = ['L1_TR', 'GAN_TR', 'L1_RT', 'GAN_RT', 'smoothness', 'D_fake_TR', 'D_fake_RT', 'D']
MAPPED = ['--misalign', 'both', '--synthetic_pairs', 'mapped']
LABELS = MAPPED + ['--labels', '4']
LAMBDA = 20.0


def _argv(tmp, stn='affine', size=64, extra=()):
    return ['--model', 'nemar', '--stn_type', stn, '--netG', 'resnet_3blocks', '--ngf', '8', '--ndf', '8', '--dataset_mode', 'gpupairs',
            '--dataroot', 'synthetic', '--img_height', str(size), '--img_width', str(size), '--crop_size', str(size), '--load_size',
            str(size + 12), '--batch_size', '2', '--pool_size_pairs', '6', '--checkpoints_dir', str(tmp), '--name', 'dice', '--no_dropout',
            '--gpu_ids', '0', '--lambda_smooth', '1.0', *extra]


def _opt(tmp, **kw):
    from nemar_amd.train import _Options
    return _Options().parse(_argv(tmp, **kw), quiet=True)


bits = lambda a: np.asarray(a).view(np.uint32)


@pytest.mark.parametrize("mode,size,classes,background", [(GRID_UNET, (35, 67), 5, False), (GRID_UNET, (32, 64), 257, True),
                                                          (GRID_AFFINE, (35, 67), 5, False)], ids=str)
def test_ops_dice_loss_is_the_kernels_loss_and_gradient(hip_lib, mode, size, classes, background):
    from nemar_amd import ops
    be = HipBackend(hip_lib)
    N, (H, W) = 2, size
    pred, lm, lf, _, _ = K.draw(5, mode, N, H, W, classes, 'smooth')
    k0 = 0 if background else 1
    d_pred, d_lm, d_lf = be.dev(pred), be.dev(lm), be.dev(lf)
    want_loss, want_sums, d_coef = K.run_fwd(be, d_pred, mode, d_lm, d_lf, (N, H, W), classes, k0, 0.5, 0.25)
    want_grad = K.run_bwd(be, d_pred, mode, d_lm, d_lf, d_coef, (N, H, W), classes, 3.0)
    p = torch.from_numpy(pred).cuda().requires_grad_(True)
    tm, tf = torch.from_numpy(lm).cuda().requires_grad_(True), torch.from_numpy(lf).cuda()[:, None]      # ([N,H,W] and [N,1,H,W] both)
    loss = ops.dice_loss(p, mode, tm, tf, classes, eps=0.5, background=background, factor=0.25)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda and loss.requires_grad
    loss.backward(torch.full((), 3.0, device='cuda'))
    assert bits(loss.detach().cpu().numpy()) == bits(want_loss)
    assert np.array_equal(bits(p.grad.cpu().numpy()), bits(want_grad)) and float(p.grad.abs().max()) > 0
    assert tm.grad is None, "the label maps carry no gradient"
    sums = ops.dice_sums(p, mode, tm, tf, classes)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (N, classes, 3)
    assert np.array_equal(sums.cpu().numpy(), K.to_pixels(want_sums))
    other = GRID_AFFINE if mode == GRID_UNET else GRID_UNET
    for bad in (lambda: ops.dice_loss(p[:1], mode, tm, tf, classes), lambda: ops.dice_loss(p, mode, tm[:, :8], tf, classes),
                lambda: ops.dice_loss(p, mode, tm, tf, classes, eps=0.0), lambda: ops.dice_loss(p, mode, tm, tf, 1),
                lambda: ops.dice_loss(p, mode, tm, tf, 2000), lambda: ops.dice_loss(p, other, tm, tf, classes),
                lambda: ops.dice_loss(p, 0, tm, tf, classes)):
        with pytest.raises(ValueError, match="dice_loss"):
            bad()


# ---- the dataset ------------------------------------------------------------------------------------------------------------------------
def test_batch_keys_and_labels_follow_the_images(tmp_path):
    from nemar_amd import ops
    from nemar_amd.data import create_dataset
    from nemar_amd.data.gpupairs_dataset import GpuPairsDataset
    plain = GpuPairsDataset(_opt(tmp_path, extra=MAPPED))
    labelled = GpuPairsDataset(_opt(tmp_path, extra=LABELS))
    a, b = plain.batch([0, 3]), labelled.batch([0, 3])
    assert list(a) == ['A', 'B', 'A_paths', 'B_paths', 'gt_field'] and list(b) == list(a) + ['labels_A', 'labels_B']
    # the crop / flip / misalign streams of a seed do not move: the images and the field are the same bits
    assert all(torch.equal(a[k], b[k]) for k in ('A', 'B', 'gt_field')) and np.array_equal(plain._last_params, labelled._last_params)
    la, lb = b['labels_A'], b['labels_B']
    assert la.shape == (2, 1, 64, 64) and lb.shape == la.shape and la.dtype == torch.float32
    assert set(torch.unique(torch.cat([la, lb])).tolist()) <= {0.0, 1.0, 2.0, 3.0} and len(torch.unique(lb)) >= 2
    par = torch.from_numpy(labelled._last_params).cuda()
    assert torch.equal(la, ops.crop_flip_deform_labels(labelled.labels_A, par, b['gt_field'], 64, 64))
    assert torch.equal(lb, ops.crop_flip_deform_labels(labelled.labels_B, par, None, 64, 64))
    assert not torch.equal(la, lb), "labels_A is deformed by the batch's gt_field"
    # labels are those of the image they came with: the K-level quantisation of the pool's channel mean, cropped as image B is
    pool_mean = labelled.pool_A.mean(dim=1, keepdim=True)
    want = ops.crop_flip_deform_labels((pool_mean * 4).floor().clamp_(0, 3).contiguous(), par, None, 64, 64)
    assert torch.equal(lb, want)
    # without --misalign the two maps of an aligned pair are the same
    aligned = GpuPairsDataset(_opt(tmp_path, extra=['--synthetic_pairs', 'mapped', '--labels', '4'])).batch([1, 2])
    assert list(aligned) == ['A', 'B', 'A_paths', 'B_paths', 'labels_A', 'labels_B'] and torch.equal(aligned['labels_A'], aligned['labels_B'])
    with pytest.raises(ValueError, match="--synthetic_pairs mapped"):
        GpuPairsDataset(_opt(tmp_path, extra=['--labels', '4']))
    with pytest.raises(ValueError, match="at least 2"):
        GpuPairsDataset(_opt(tmp_path, extra=MAPPED + ['--labels', '1']))
    assert list(next(iter(create_dataset(_opt(tmp_path, extra=LABELS))))) == list(b)


def test_label_files_beside_the_images(tmp_path):
    from nemar_amd.data.gpupairs_dataset import GpuPairsDataset
    rng = np.random.default_rng(0)
    root = tmp_path / 'pairs'
    root.mkdir()
    np.save(root / 'A.npy', rng.random((3, 3, 40, 48)).astype(np.float32))
    np.save(root / 'B.npy', rng.random((3, 3, 40, 48)).astype(np.float32))
    argv = _argv(tmp_path, extra=['--labels', '3', '--preprocess', 'resize_and_crop'])
    argv[argv.index('--dataroot') + 1] = str(root)
    from nemar_amd.train import _Options
    with pytest.raises(FileNotFoundError, match="labels_A.npy"):
        GpuPairsDataset(_Options().parse(argv, quiet=True))
    lab = rng.integers(0, 3, (3, 40, 48)).astype(np.uint8)
    np.save(root / 'labels_A.npy', lab)
    np.save(root / 'labels_B.npy', lab[:, None])
    ds = GpuPairsDataset(_Options().parse(argv, quiet=True))
    assert ds.labels_A.shape == (3, 1, 76, 76) and torch.equal(ds.labels_A, ds.labels_B)       # resized with the images, by nearest
    assert set(torch.unique(ds.labels_A).tolist()) == {0.0, 1.0, 2.0}
    b = ds.batch([0, 1])
    assert b['labels_A'].shape == (2, 1, 64, 64) and torch.equal(b['labels_A'], b['labels_B'])


# ---- the step -----------------------------------------------------------------------------------------------------------------------------
class _Counting:
    """ops.L with every call of a launching entry point counted by name (backends._launches: the size queries, memoised per process, are
    not launches)"""

    def __init__(self, lib):
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not callable(fn) or not _launches(self._lib, name if name.startswith("nemar_") else "nemar_" + name):
            return fn

        def counted(*a):
            self.calls[name] += 1
            return fn(*a)
        return counted


def _run(tmp, extra, steps=1, batched=None, monkeypatch=None, data=None):
    """`steps` seeded optimize_parameters() on one batch from identical initial weights -> what the run left behind"""
    from nemar_amd import ops
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    if batched is not None:
        monkeypatch.setenv('NEMAR_BATCHED_PASSES', batched)
    opt = _opt(tmp, extra=extra)
    if data is None:
        torch.manual_seed(7)
        data = next(iter(create_dataset(opt)))
    torch.manual_seed(11)
    model = create_model(opt)
    model.setup(opt)
    ops.invalidate_packed_weights()
    real = ops.L
    ops.L = counting = _Counting(real)
    losses = []
    try:
        for _ in range(steps):
            model.set_input(data)
            model.optimize_parameters()
            losses.append(model.get_current_losses())
    finally:
        ops.L = real
    torch.cuda.synchronize()
    return {'loss_names': list(model.loss_names), 'losses': losses, 'calls': dict(counting.calls), 'data': data, 'model': model,
            'params': {net: [p.detach().clone() for p in getattr(model, 'net' + net).parameters()] for net in 'TRD'}}


def test_absent_or_zero_the_step_is_what_it_was(tmp_path):
    absent = _run(tmp_path / 'a', MAPPED)
    zero = _run(tmp_path / 'b', LABELS + ['--lambda_dice', '0'])
    assert not hasattr(_opt(tmp_path, extra=MAPPED), 'lambda_dice'), "the default option set carries the flag: the frozen option sets would change"
    for run in (absent, zero):
        assert run['loss_names'] == TODAY and list(run['losses'][0]) == TODAY
        assert not [k for k in run['calls'] if 'dice' in k], "a dice entry point ran with the term off"
        assert not hasattr(run['model'], 'loss_Dice')
    # the same launches (entry point by entry point), the same losses, the same parameters after the step, bit for bit
    assert absent['calls'] == zero['calls'] and sum(absent['calls'].values()) > 100
    assert absent['losses'] == zero['losses']
    for net in 'TRD':
        assert all(torch.equal(a, b) for a, b in zip(absent['params'][net], zero['params'][net]))


def test_on_it_is_a_loss_of_the_step_that_reaches_netR_only_and_decreases(tmp_path):
    from nemar_amd import ops
    off = _run(tmp_path / 'a', LABELS)
    on = _run(tmp_path / 'b', LABELS + ['--lambda_dice', str(LAMBDA), '--dice_eps', '0.5'], data=off['data'])
    assert on['loss_names'] == TODAY[:5] + ['Dice'] + TODAY[5:]
    extra = {k: v - off['calls'].get(k, 0) for k, v in on['calls'].items() if v != off['calls'].get(k, 0)}
    assert extra.pop('dice_loss_fwd') == 1 and extra.pop('dice_loss_bwd') == 1, "one forward and one backward launch pair per step"
    print("further calls with the term on:", extra)             # (the fan-out of the prediction has one more handle)
    assert not [k for k in extra if 'dice' in k], extra
    v = on['losses'][0]['Dice']
    assert math.isfinite(v) and 0 < v <= LAMBDA
    m = on['model']
    assert {k: x for k, x in on['losses'][0].items() if k != 'Dice'} == off['losses'][0]
    for net in 'TD':
        assert all(torch.equal(a, b) for a, b in zip(off['params'][net], on['params'][net])), "net%s differs: the Dice term reached it" % net
    assert any(not torch.equal(a, b) for a, b in zip(off['params']['R'], on['params']['R']))
    assert all(bool(torch.isfinite(p).all()) for p in on['params']['R'])
    # the logged value is the weight times ops.dice_loss of the step's prediction (the prediction of the step just taken)
    pred, mode = m.netR.last_prediction()
    again = LAMBDA * ops.dice_loss(pred, mode, m.labels_A, m.labels_B, 4, eps=0.5)
    assert float(again) == v
    # a handful of steps on the same batch: the term goes down
    more = _run(tmp_path / 'c', LABELS + ['--lambda_dice', str(LAMBDA), '--dice_eps', '0.5', '--lr', '0.001'], steps=8, data=off['data'])
    trace = [l['Dice'] for l in more['losses']]
    print("Dice over 8 steps:", trace)
    assert all(math.isfinite(x) for x in trace) and trace[-1] < trace[0], trace


def test_both_forward_orders_agree(tmp_path, monkeypatch):
    a = _run(tmp_path / 'a', LABELS + ['--lambda_dice', str(LAMBDA)], batched='1', monkeypatch=monkeypatch)
    b = _run(tmp_path / 'b', LABELS + ['--lambda_dice', str(LAMBDA)], batched='0', monkeypatch=monkeypatch, data=a['data'])
    assert a['loss_names'] == b['loss_names']
    # the prediction is netR's of the same pair with the same weights in either order: the term is the same bits
    assert a['losses'][0]['Dice'] == b['losses'][0]['Dice'] > 0


def test_options_and_batches_are_checked(tmp_path):
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    m = create_model(_opt(tmp_path, stn='unet', size=256, extra=LABELS + ['--lambda_fold', '1', '--lambda_epe', '1', '--lambda_dice', '1', '--lambda_lncc', '1']))
    assert m.loss_names == TODAY[:4] + ['LNCC_TR', 'LNCC_RT', 'smoothness', 'fold', 'EPE', 'Dice'] + TODAY[5:]
    assert create_model(_opt(tmp_path, extra=MAPPED + ['--lambda_dice', '1', '--dice_classes', '3']))._dice_classes == 3
    assert create_model(_opt(tmp_path, extra=LABELS + ['--lambda_dice', '1', '--dice_background']))._dice_background
    for bad, match in ((MAPPED + ['--lambda_dice', '1'], "at least 2 classes"), (LABELS + ['--lambda_dice', '1', '--dice_classes', '1'], "at least 2 classes"),
                       (LABELS + ['--lambda_dice', '1', '--dice_eps', '0'], "dice_eps")):
        with pytest.raises(ValueError, match=match):
            create_model(_opt(tmp_path, extra=bad))
    # a batch without labels, with labels of another size, or in the other direction
    opt = _opt(tmp_path, extra=MAPPED + ['--lambda_dice', '1', '--dice_classes', '4'])
    model = create_model(opt)
    model.setup(opt)
    model.set_input(next(iter(create_dataset(opt))))
    with pytest.raises(RuntimeError, match="--labels"):
        model.optimize_parameters()
    opt = _opt(tmp_path, extra=LABELS + ['--lambda_dice', '1'])
    data = next(iter(create_dataset(opt)))
    model.set_input(dict(data, labels_A=data['labels_A'][:, :, :32]))
    with pytest.raises(ValueError, match="labels_A"):
        model.optimize_parameters()
    model.set_input(data)
    model.optimize_parameters()
    assert math.isfinite(float(model.loss_Dice))
    rev = create_model(_opt(tmp_path, extra=LABELS + ['--lambda_dice', '1', '--direction', 'BtoA']))
    with pytest.raises(ValueError, match="AtoB"):
        rev.set_input(data)


def test_step_graph_replay_equals_eager_with_the_term_on(tmp_path):
    """the term makes no host sync and no allocation outside the caching allocator, and its two label maps are static buffers of the
    capture: three replays of the captured step on three different batches are three eager steps, bit for bit"""
    from nemar_amd import ops
    from nemar_amd.data import create_dataset
    from nemar_amd.models import create_model
    opt = _opt(tmp_path, extra=LABELS + ['--lambda_dice', str(LAMBDA)])
    torch.manual_seed(7)
    batches = []
    for data in create_dataset(opt):
        batches.append(data)
        if len(batches) == 3:
            break
    assert not torch.equal(batches[0]['labels_A'], batches[1]['labels_A'])
    snaps = []
    try:
        ops.step_params(True, torch.device('cuda:0'))
        for graph in (False, True):
            ops._step_params["step"] = 0
            torch.manual_seed(11)
            m = create_model(opt)
            m.setup(opt)
            ops.invalidate_packed_weights()
            m.set_input(batches[0])
            if graph:
                m.enable_step_graph(warmup=2)
            losses = []
            for data in batches:
                m.set_input(data)
                m.optimize_parameters()
                losses.append(m.get_current_losses())
            torch.cuda.synchronize()
            snaps.append(([p.detach().clone() for o in m.optimizers for p in (o.flat_p, o.m, o.v)], losses))
    finally:
        ops.step_params(False)
        ops.pin_workspaces(False)
    (p_eager, l_eager), (p_graph, l_graph) = snaps
    assert l_eager[0]['Dice'] > 0 and l_eager[0]['Dice'] != l_eager[1]['Dice']          # (each step saw its own maps)
    assert l_eager == l_graph, (l_eager, l_graph)
    assert all(torch.equal(a, b) for a, b in zip(p_eager, p_graph))
