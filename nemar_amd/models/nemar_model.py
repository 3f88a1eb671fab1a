"""NeMAR training step on MI355X — drop-in for reference models/nemar_model.py (NEMARModel :12-288).

Same flags (:30-45), same attributes (`netT`, `netR`, `netD`, `netD_multiresolution`, `loss_*`, `visual_names`,
`model_names`, `optimizers`), same call order inside optimize_parameters (:266-288): forward, discriminator step,
then translation+registration step against the freshly updated discriminator.  What differs is how the step
executes:
  * every operator is a gfx950 kernel (nemar_amd.ops); concatenations (real_A, X) are two-pointer conv inputs;
  * each loss term leaves its kernel already multiplied by its lambda, and the step back-propagates from the list
    of terms at once (`torch.autograd.backward(terms)` == backward of their sum), so no scalar arithmetic kernels
    run; the reference's `loss_*` scalars are formed lazily, only when somebody reads them;
  * the three Adam optimizers are single fused launches over flat buffers (ops.FlatAdam), whose gradient buffers are
    also the data-parallel all-reduce buckets (nemar_amd.distributed): one bucket after backward_D, two after
    backward_T_and_R.
"""
import argparse
import itertools
import os

import torch

from .. import distributed as dist
from .. import ops
from . import networks
from . import stn
from .base_model import BaseModel


class _LazyLoss:
    """sum_i scale_i * term_i, evaluated on first use (float(), .item(), arithmetic via .value())."""

    def __init__(self, parts):
        self.parts = parts            # list of (0-dim tensor, python scale)
        self._v = None

    def value(self):
        if self._v is None:
            with torch.no_grad():
                v = None
                for t, s in self.parts:
                    x = t.detach() * s if s != 1.0 else t.detach()
                    v = x if v is None else v + x
                self._v = v if v is not None else torch.zeros((), device='cuda')
        return self._v

    def __float__(self):
        return float(self.value())

    def item(self):
        return float(self)

    def detach(self):
        return self.value()

    def __repr__(self):
        return 'LazyLoss(%g)' % float(self)


def _loss_property(name):
    """`model.loss_<name>` is a 0-dim TENSOR, as in the reference (models/nemar_model.py:179-261) — arithmetic, .item(),
    SummaryWriter.add_scalar all work — but it is only FORMED when somebody reads it: the step itself back-propagates from the
    list of weighted terms and runs no scalar arithmetic kernels."""
    key = '_lazy_loss_' + name

    def get(self):
        try:
            return self.__dict__[key].value()
        except KeyError:        # as a plain attribute of the reference would: hasattr / getattr(default) keep working
            raise AttributeError('loss_%s has not been computed yet (no optimize_parameters() call so far)' % name) from None

    def put(self, parts):
        self.__dict__[key] = parts if isinstance(parts, _LazyLoss) else _LazyLoss([(parts, 1.0)])
    return property(get, put)


class NEMARModel(BaseModel):
    """netT: translation A->B; netR: registration (STN) A~>B; netD: PatchGAN on (A, B) pairs."""

    @staticmethod
    def modify_commandline_options(parser, is_train=True):
        parser = stn.modify_commandline_options(parser, is_train)
        if is_train:
            parser.add_argument('--lambda_GAN', type=float, default=1.0, help='Weight for the GAN loss.')
            parser.add_argument('--lambda_recon', type=float, default=100.0,
                                help='Weight for the L1 reconstruction loss.')
            parser.add_argument('--lambda_smooth', type=float, default=0.0, help='Regularization term used by the STN')
            # (MI355X build) train against folds: a hinge on the Jacobian determinant of the UNet STN's prediction (ops.fold_penalty).
            # Both default to 0.0 (_fold_options); a command line that does not carry them parses to the options it always parsed to
            parser.add_argument('--lambda_fold', type=float, default=argparse.SUPPRESS,
                                help='unet STN only: weight of the fold penalty, mean max(0, fold_margin - Jacobian determinant); '
                                     'default 0.0: switched off')
            parser.add_argument('--fold_margin', type=float, default=argparse.SUPPRESS,
                                help='determinant below which the fold penalty acts (default 0.0: folds only; the identity has determinant ~1)')
            # (MI355X build) train against local NCC: a windowed normalised cross-correlation of each generated image with real_B
            # (ops.local_ncc), next to the global L1 terms.  Read like --lambda_fold: a command line without them parses as it always did
            parser.add_argument('--lambda_lncc', type=float, default=argparse.SUPPRESS,
                                help='weight of the local NCC terms, 1 - mean cc of fake_TR_B / fake_RT_B with real_B; default 0.0: switched off')
            parser.add_argument('--lncc_win', type=int, default=argparse.SUPPRESS,
                                help='window size of the local NCC terms: odd, 3 .. 11 (default 9)')
            # (MI355X build) train across modalities: the distance of the MIND descriptors of registered_real_A and real_B (ops.mind_loss),
            # an image term that compares modality A with modality B directly and reaches netR alone.  Read like --lambda_fold
            parser.add_argument('--lambda_mind', type=float, default=argparse.SUPPRESS,
                                help='weight of the MIND term, the mean squared descriptor distance of registered_real_A and real_B; '
                                     'default 0.0: switched off')
            parser.add_argument('--mind_patch', type=int, default=argparse.SUPPRESS, help='patch size of the MIND term: 3 or 5 (default 3)')
            parser.add_argument('--mind_dilation', type=int, default=argparse.SUPPRESS,
                                help='distance of the four neighbouring patches of the MIND term: 1 or 2 (default 2)')
            parser.add_argument('--mind_eps', type=float, default=argparse.SUPPRESS,
                                help='constant added to the local variance of the MIND term, > 0 (default 1e-5)')
            # (MI355X build) train against known misalignment: the registration error of batches that carry a ground-truth field
            # (--misalign), as a loss on the prediction the warp reads (ops.epe_loss).  Read like --lambda_fold
            parser.add_argument('--lambda_epe', type=float, default=argparse.SUPPRESS,
                                help='weight of the supervised registration term, mean sqrt(|r|^2 + epe_eps^2) of the residual r against '
                                     'the known misalignment (needs --misalign affine|elastic|both); default 0.0: switched off')
            parser.add_argument('--epe_eps', type=float, default=argparse.SUPPRESS,
                                help='Charbonnier epsilon of the supervised registration term in pixels, > 0 (default 0.01)')
            # (MI355X build) train against label overlap: the soft Dice of the batch's label maps (--labels K), labels_A warped by the
            # prediction the warp reads against labels_B (ops.dice_loss).  Read like --lambda_fold
            parser.add_argument('--lambda_dice', type=float, default=argparse.SUPPRESS,
                                help='weight of the label-overlap term, mean 1 - soft Dice over samples and classes (needs batches with '
                                     'labels_A / labels_B: --labels K); default 0.0: switched off')
            parser.add_argument('--dice_eps', type=float, default=argparse.SUPPRESS,
                                help='smoothing constant of the soft Dice in pixels, > 0 (default 1.0)')
            parser.add_argument('--dice_classes', type=int, default=argparse.SUPPRESS,
                                help='number of classes of the label-overlap term (default: --labels)')
            parser.add_argument('--dice_background', action='store_true', default=argparse.SUPPRESS,
                                help='average the label-overlap term over class 0 too (default: the background is left out)')
            # (MI355X build) train the cascade: netR looks at the pair K times with shared weights, the predictions composed into the one
            # transformation every term acts on (UnetSTN.predict(passes=K), ops.compose_predictions(grad=True)).  Read like --lambda_fold
            parser.add_argument('--train_passes', type=int, default=argparse.SUPPRESS,
                                help='unet STN only: passes of the registration network per training step, 1 .. 8, composed into one '
                                     'transformation and trained end to end (default 1: a single look)')
            parser.add_argument('--enable_tbvis', action='store_true',
                                help='Enable tensorboard visualizer (default : False)')
            parser.add_argument('--multi_resolution', type=int, default=1,
                                help='Use of multi-resolution discriminator.'
                                     '(if equals to 1 then no multi-resolution training is applied)')
            # flags of the reference's TensorboardVisualizer (util/tb_visualizer.py:6-15), accepted for CLI parity
            parser.add_argument('--tbvis_iteration_update_rate', type=int, default=1000)
            parser.add_argument('--tbvis_disable_report_weights', action='store_true')
            parser.add_argument('--tbvis_disable_report_offsets', action='store_true')
            # (MI355X build) the registration-error scalars of batches that carry a ground-truth field (--misalign): on unless disabled
            parser.add_argument('--tbvis_disable_report_registration', action='store_true')
        return parser

    def __init__(self, opt):
        BaseModel.__init__(self, opt)
        self.train_stn = True
        # the fold penalty is a term of the training step only, and only a dense field has a per-pixel determinant to train against
        self._lambda_fold, self._fold_margin = float(getattr(opt, 'lambda_fold', 0.0)), float(getattr(opt, 'fold_margin', 0.0))
        self._fold_on = bool(self.isTrain and self._lambda_fold != 0.0)
        if self._fold_on and opt.stn_type != 'unet':
            raise ValueError('--lambda_fold %g needs --stn_type unet: the %s STN has no fold term (theta\'s determinant is one number per '
                             'sample, not a field to regularise)' % (self._lambda_fold, opt.stn_type))
        # the trained cascade: K looks of netR per training step, composed; only a dense field has a compose gradient at training size
        self._train_passes = int(getattr(opt, 'train_passes', 1)) if self.isTrain else 1
        if not 1 <= self._train_passes <= 8:
            raise ValueError('--train_passes %d: the passes of a training step are 1 .. 8' % self._train_passes)
        if self._train_passes > 1 and opt.stn_type != 'unet':
            raise ValueError('--train_passes %d needs --stn_type unet: cascade training composes dense fields (the %s STN composes in '
                             'closed form and is not trained that way)' % (self._train_passes, opt.stn_type))
        # the local NCC terms: two more image losses of the training step, any STN
        self._lambda_lncc, self._lncc_win = float(getattr(opt, 'lambda_lncc', 0.0)), int(getattr(opt, 'lncc_win', 9))
        self._lncc_on = bool(self.isTrain and self._lambda_lncc != 0.0)
        if self._lncc_on and not (3 <= self._lncc_win <= 11 and self._lncc_win % 2 == 1):
            raise ValueError('--lncc_win %d: the local NCC window is an odd size from 3 to 11' % self._lncc_win)
        # the MIND term: one more image loss of the training step, registered_real_A against real_B across the modalities, any STN
        self._lambda_mind = float(getattr(opt, 'lambda_mind', 0.0))
        self._mind_patch, self._mind_dil = int(getattr(opt, 'mind_patch', 3)), int(getattr(opt, 'mind_dilation', 2))
        self._mind_eps = float(getattr(opt, 'mind_eps', 1e-5))
        self._mind_on = bool(self.isTrain and self._lambda_mind != 0.0)
        if self._mind_on and self._mind_patch not in (3, 5):
            raise ValueError('--mind_patch %d: the patch of the MIND term is 3 or 5' % self._mind_patch)
        if self._mind_on and self._mind_dil not in (1, 2):
            raise ValueError('--mind_dilation %d: the dilation of the MIND term is 1 or 2' % self._mind_dil)
        if self._mind_on and not self._mind_eps > 0.0:
            raise ValueError('--mind_eps %g: the constant of the MIND term must be positive' % self._mind_eps)
        # the supervised registration term: one more loss of the training step on batches that carry a gt_field, any STN
        self._lambda_epe, self._epe_eps = float(getattr(opt, 'lambda_epe', 0.0)), float(getattr(opt, 'epe_eps', 0.01))
        self._epe_on = bool(self.isTrain and self._lambda_epe != 0.0)
        if self._epe_on and not self._epe_eps > 0.0:
            raise ValueError('--epe_eps %g: the Charbonnier epsilon of --lambda_epe must be positive' % self._epe_eps)
        # the label-overlap term: one more loss of the training step on batches that carry label maps, any STN
        self._lambda_dice, self._dice_eps = float(getattr(opt, 'lambda_dice', 0.0)), float(getattr(opt, 'dice_eps', 1.0))
        self._dice_classes = int(getattr(opt, 'dice_classes', 0) or getattr(opt, 'labels', 0) or 0)
        self._dice_background = bool(getattr(opt, 'dice_background', False))
        self._dice_on = bool(self.isTrain and self._lambda_dice != 0.0)
        if self._dice_on and self._dice_classes < 2:
            raise ValueError('--lambda_dice %g needs at least 2 classes: --dice_classes K, or --labels K (got %d)' % (self._lambda_dice, self._dice_classes))
        if self._dice_on and not (self._dice_eps > 0.0 and self._dice_eps < float('inf')):
            raise ValueError('--dice_eps %g: the smoothing constant of --lambda_dice must be positive and finite' % self._dice_eps)
        self.setup_visualizers()
        self.tb_visualizer = None
        # T's two applications and D's 3 + 2 applications per step run as single batches: the same graph with half the launches.  (With
        # --norm batch the batched calls run under ops.norm_segments(k): BatchNorm takes its statistics and running-stat updates per
        # segment of the batch, in segment order — those of the reference's k separate calls.)  Round 1 measured no gain (78.15 vs 78.00 ms/step: every layer
        # already filled the chip at batch 8); with the split-16 kernels, whose max / split / slab-sum passes are paid per launch,
        # it is 47.9 vs 50.2 ms/step on the same box, so it is the default.  NEMAR_BATCHED_PASSES=0 restores the reference's call
        # order (tests/test_step_gpu.py compares the two).
        self._batched = os.environ.get('NEMAR_BATCHED_PASSES', '1') == '1'
        # dropout masks: one Philox stream per process, governed by torch.manual_seed() and different on every rank
        ops.manual_seed(torch.initial_seed() + dist.rank())
        self.define_networks()
        if self.isTrain:
            self.criterionGAN = networks.GANLoss(opt.gan_mode)
            self.criterionL1 = ops.l1_loss
            self.setup_optimizers()
            if getattr(opt, 'enable_tbvis', False):
                # scalars the reference's TensorboardVisualizer reports (util/tb_visualizer.py:53-92): losses and the mean
                # deformation offsets, the latter reduced on the device (nemar_amd/util/visualizer.py)
                from ..util.visualizer import TrainingMonitor
                self.tb_visualizer = TrainingMonitor(self, opt)
            self._one = torch.ones((), dtype=torch.float32, device=self.device)
            self._lam_smooth = torch.full((), float(opt.lambda_smooth), dtype=torch.float32, device=self.device)
            if self._fold_on:
                self._lam_fold = torch.full((), self._lambda_fold, dtype=torch.float32, device=self.device)
            if self._epe_on:
                self._lam_epe = torch.full((), self._lambda_epe, dtype=torch.float32, device=self.device)
            if self._dice_on:
                self._lam_dice = torch.full((), self._lambda_dice, dtype=torch.float32, device=self.device)

    loss_L1_TR = _loss_property('L1_TR')
    loss_GAN_TR = _loss_property('GAN_TR')
    loss_L1_RT = _loss_property('L1_RT')
    loss_GAN_RT = _loss_property('GAN_RT')
    loss_smoothness = _loss_property('smoothness')
    loss_fold = _loss_property('fold')
    loss_EPE = _loss_property('EPE')
    loss_Dice = _loss_property('Dice')
    loss_LNCC_TR = _loss_property('LNCC_TR')
    loss_LNCC_RT = _loss_property('LNCC_RT')
    loss_MIND_R = _loss_property('MIND_R')
    loss_D_fake_TR = _loss_property('D_fake_TR')
    loss_D_fake_RT = _loss_property('D_fake_RT')
    loss_D = _loss_property('D')

    def setup_visualizers(self):
        # <loss>_TR: registration-first branch T(R(a)); <loss>_RT: translation-first branch R(T(a))
        self.loss_names = ['L1_TR', 'GAN_TR', 'L1_RT', 'GAN_RT', 'smoothness', 'D_fake_TR', 'D_fake_RT', 'D']
        if self._fold_on:
            self.loss_names.insert(self.loss_names.index('smoothness') + 1, 'fold')
        if self._epe_on:
            self.loss_names.insert(self.loss_names.index('fold' if self._fold_on else 'smoothness') + 1, 'EPE')
        if self._dice_on:
            after = 'EPE' if self._epe_on else ('fold' if self._fold_on else 'smoothness')
            self.loss_names.insert(self.loss_names.index(after) + 1, 'Dice')
        if self._lncc_on:
            at = self.loss_names.index('smoothness')
            self.loss_names[at:at] = ['LNCC_TR', 'LNCC_RT']
        if self._mind_on:
            self.loss_names.insert(self.loss_names.index('smoothness'), 'MIND_R')      # (after the local NCC names)
        self.visual_names = ['real_A', 'real_B', 'fake_TR_B', 'fake_RT_B', 'registered_real_A', 'fake_B']
        self.model_names = ['T', 'R'] + (['D'] if self.isTrain else [])

    def define_networks(self):
        opt = self.opt
        AtoB = opt.direction == 'AtoB'
        in_c = opt.input_nc if AtoB else opt.output_nc
        out_c = opt.output_nc if AtoB else opt.input_nc
        self.netT = networks.define_G(in_c, out_c, opt.ngf, opt.netG, opt.norm, not opt.no_dropout, opt.init_type,
                                      opt.init_gain, self.gpu_ids)
        self.netR = stn.define_stn(self.opt, self.opt.stn_type)
        if self.isTrain:
            self.netD = networks.define_D(opt.output_nc + opt.input_nc, opt.ndf, opt.netD, opt.n_layers_D, opt.norm,
                                          opt.init_type, opt.init_gain, self.gpu_ids)
            # extra discriminators on 1/2, 1/4, ... resolution inputs (reference :106-113)
            self.netD_multiresolution = []
            for _ in range(max(0, opt.multi_resolution - 1)):
                self.netD_multiresolution.append(
                    networks.define_D(opt.output_nc + opt.input_nc, opt.ndf, opt.netD, opt.n_layers_D, opt.norm,
                                      opt.init_type, opt.init_gain, self.gpu_ids))

    def reset_weights(self):
        opt = self.opt
        networks.init_weights(self.netT, opt.init_type, opt.init_gain)
        networks.init_weights(self.netD, opt.init_type, opt.init_gain)
        for netD_S in self.netD_multiresolution:
            networks.init_weights(netD_S, opt.init_type, opt.init_gain)

    def setup_optimizers(self):
        opt = self.opt
        betas = (opt.beta1, 0.999)
        self.optimizer_R = ops.FlatAdam(self.netR.parameters(), lr=opt.lr, betas=betas)
        self.optimizer_T = ops.FlatAdam(self.netT.parameters(), lr=opt.lr, betas=betas)
        d_params = itertools.chain(self.netD.parameters(), *[x.parameters() for x in self.netD_multiresolution])
        self.optimizer_D = ops.FlatAdam(d_params, lr=opt.lr, betas=betas)
        self.optimizers += [self.optimizer_T, self.optimizer_D, self.optimizer_R]
        # identical replicas on every rank before the first step; bucketed gradient averaging overlapped with backward
        dist.broadcast_parameters(self.optimizers)
        self.sync_T, self.sync_D, self.sync_R = dist.grad_sync_for([self.optimizer_T, self.optimizer_D, self.optimizer_R])

    def set_input(self, input):
        AtoB = self.opt.direction == 'AtoB'
        a, b = ('A', 'B') if AtoB else ('B', 'A')
        self.real_A = input[a].to(self.device, dtype=torch.float32, non_blocking=True).contiguous()
        self.real_B = input[b].to(self.device, dtype=torch.float32, non_blocking=True).contiguous()
        self.image_paths = input[a + '_paths']
        # known-misalignment pairs (data/gpupairs_dataset.py --misalign): the field that deformed modality A, [N,2,H,W] in pixels
        gt = input.get('gt_field')
        if gt is not None and not AtoB:
            raise ValueError('gt_field describes the deformation of modality A: the registration error is defined for --direction AtoB')
        self.gt_field = None if gt is None else gt.to(self.device, dtype=torch.float32, non_blocking=True).contiguous()
        # label maps (data/gpupairs_dataset.py --labels): float class ids [N,1,H,W] of the two modalities, for the label-overlap term
        la, lb = input.get('labels_A'), input.get('labels_B')
        if (la is not None or lb is not None) and not AtoB:
            raise ValueError('labels_A / labels_B: the label-overlap term warps the labels of modality A: it is defined for --direction AtoB')
        self.labels_A = None if la is None else la.to(self.device, dtype=torch.float32, non_blocking=True).contiguous()
        self.labels_B = None if lb is None else lb.to(self.device, dtype=torch.float32, non_blocking=True).contiguous()
        self._resized = {}

    def registration_error(self):
        """How far the last forward pass (a training step or test()) is from undoing the batch's known misalignment: a dict of Python
        floats — epe_px (mean |S(x) + g(S(x)) - x| over the pixels whose sampling position S(x) is inside the image), epe_before_px
        (mean |g|: the error of doing nothing), max_px, fold_frac, valid_frac.  One host synchronisation."""
        from ..util.visualizer import registration_summary
        if getattr(self, 'gt_field', None) is None:
            raise RuntimeError('registration_error: the current batch carries no gt_field (train with --misalign affine|elastic|both)')
        pred = self.netR.last_prediction()
        if pred is None:
            raise RuntimeError('registration_error: no forward pass yet')
        rows = ops.registration_error(pred[0], self.gt_field, pred[1])
        cols = rows.sum(0)
        cols[2] = rows[:, 2].max()
        return registration_summary(cols.tolist(), self.gt_field.size(0) * self.gt_field.size(2) * self.gt_field.size(3))

    def cascade(self, passes, regularity=False, similarity=False, bins=32):
        """test() with `passes` looks at the set_input pair (a "recursive cascade"): pass 1 is test() exactly as it is; every further pass
        predicts from (registered_real_A, real_B), composes that prediction ONTO the accumulated one (netR.compose: one transformation
        that samples where the two would in sequence) and warps the ORIGINAL real_A by the composite — one interpolation however many
        passes, the UNet STN's in the composing launch itself.  Afterwards netR.last_prediction() is the composite, registered_real_A and
        fake_RT_B are warps by it and fake_TR_B = netT(registered_real_A), so register() and registration_error() work unchanged.
        cascade(1) is test().  Inference only: no autograd, no regularisation term for the further passes (training the cascade is
        --train_passes K: UnetSTN.predict(passes=K)).
        With regularity=True returns a list of `passes` (counts, stats) pairs: netR.regularity of the accumulated transformation after
        each pass, at the network's size (composites are where folds appear); by default returns None, as before.
        With similarity=True returns a list of `passes` (counts, moments) pairs: netR.similarity of real_A under the accumulated
        transformation against real_B after each pass, at the network's size, `bins` bins over [-1, 1] (ops.similarity_summary turns a
        pair into mutual information and NCC).  With both flags: {'regularity': [...], 'similarity': [...]}."""
        passes = int(passes)
        if passes < 1:
            raise ValueError('cascade: %d passes (at least 1)' % passes)
        self.test()
        per_pass = [self.netR.regularity(self.netR.last_prediction())[:2]] if regularity else None
        agreement = [self.netR.similarity(self.netR.last_prediction(), self.real_A, self.real_B, bins)] if similarity else None
        told = {'regularity': per_pass, 'similarity': agreement} if regularity and similarity else (agreement if similarity else per_pass)
        if passes == 1:
            return told
        with torch.no_grad():
            acc = self.netR.last_prediction()
            dense = acc[1] == ops.GRID_UNET
            for _ in range(passes - 1):
                self.netR.predict(self.registered_real_A, self.real_B)
                new = self.netR.last_prediction()
                if dense:
                    field, self.registered_real_A = self.netR.compose(acc, new, self.real_A)
                else:
                    field = self.netR.compose(acc, new)
                    self.registered_real_A = self.netR.apply(field, [self.real_A])[0]
                acc = (field, acc[1])
                if regularity:
                    per_pass.append(self.netR.regularity(acc)[:2])
                if similarity:
                    agreement.append(self.netR.similarity(acc, self.real_A, self.real_B, bins))
            self.netR.set_last_prediction(acc[0])
            self.fake_RT_B = self.netR.apply(acc, [self.fake_B])[0]
            self.fake_TR_B = self.netT(self.registered_real_A)
            self.compute_visuals()
        return told

    def register(self, full_A, full_B=None, labels_A=None, translate=True, labels_B=None, landmarks_A=None, landmarks_B=None,
                 num_classes=None, regularity=False, jacobian_map=False, similarity=False, bins=32, intensity_range=(-1., 1.),
                 inverse=False, surface=False, surface_max_dist=64, surface_map=False):
        """Register images at their native size with the transformation the last forward pass (test() on the set_input batch, at the
        network's resolution) predicted: the sampling grid is in normalised coordinates, so the prediction holds at every size, and the
        warp kernel resizes a dense field on the fly (ops.warp_resampled).  full_A [N,C,H,W] is modality A of the same N pairs at any
        size; the warp is linear, so 'registered_A' comes back in whatever value range full_A has, but netT reads it as a network input:
        pass it in [-1, 1] (what set_input takes) when `translate` is on.  Returns a dict: 'registered_A' (full_A warped bilinearly, at its
        own size); 'fake_RT_B' (netT(full_A) warped, at that size too — a full-size generator pass, skipped with translate=False) only when
        netT can run at full_A's size — the key is absent otherwise, nothing is resized; 'registered_labels_A' (labels_A
        [N,*,H',W'] warped with nearest sampling: class ids are copied, never blended) when labels_A is given; 'offsets', the
        network-resolution prediction itself (offsets [N,2,h,w] or dtheta [N,6]).  full_B is accepted for symmetry with set_input and is
        not read: the prediction is made from the network-resolution pair.
        Scores, where there is something to score against (ops.label_overlap / ops.map_points; no further keys and no further launches
        otherwise): with labels_A and labels_B ([N,H,W] or [N,1,H,W], at the fixed image's size) 'overlap' and 'overlap_before', int32
        [N,K,3] per-class counts (inter, moving, fixed — Dice = 2 inter / (moving + fixed)) of the warped label map and of labels_A
        merely resampled to that size, K = num_classes or 1 + the largest id of the two maps (one host synchronisation); with
        landmarks_A and landmarks_B ([N,P,2] (x, y) in pixels of full_A and of the fixed image, which is full_B's size, or full_A's
        without full_B; NaN = missing) 'tre_px' and 'tre_before_px' [N,P]: |S(lm_B) - lm_A| with the prediction's S and with the
        identity's, NaN where either point is missing.
        With regularity=True (or jacobian_map=True, which implies it) 'jac_counts' int64 [N,2] and 'jac_stats' float32 [N,5]
        (netR.regularity: interior pixels and folds; min, max and sum of the Jacobian determinant and the two log sums — sums, for
        ops.regularity_summary) of the transformation at the fixed image's size — full_B's, or full_A's without full_B — and with
        jacobian_map=True 'jacobian_det' [N,H,W], the determinant map there (NaN in the last row and column).  One more launch pair;
        nothing else in the dict changes.
        With similarity=True (full_B is needed, and is read) 'similarity' = {'before': (counts, moments), 'after': (counts, moments)}:
        netR.similarity of full_A against full_B at full_B's size — the joint histogram int64 [N,bins,bins] of the two channel means
        over intensity_range (the value range of the images handed in) and the moments float32 [N,6] — under the identity and under
        the prediction (ops.similarity_summary: mutual information, NCC, MSE, MAE).  No annotation is needed.  Two more launch pairs;
        nothing else in the dict changes.
        With surface=True (labels_A, labels_B and num_classes are needed) 'surface' = {'before': (counts, hist), 'after': (counts, hist)}:
        netR.surface of labels_A against labels_B at labels_B's size — per class and direction the boundary pixels, those farther than
        surface_max_dist and the largest squared distance, int64 [N,K,2,3], and the histogram of the squared boundary distances, int32
        [N,K,2,surface_max_dist^2] — under the identity and under the prediction (ops.surface_summary: Hausdorff distance, HD95, ASSD);
        with surface_map=True also 'surface_dist2' int32 [N,2,H,W], the squared distance at every boundary pixel of the warped map
        (plane 0) and of labels_B (plane 1) under the prediction.  Nothing else in the dict changes.
        With inverse=True (needs --stn_integrate K > 0 and full_B, which is read) 'registered_B', full_B warped onto A at its own size by
        the inverse prediction, and 'inverse_offsets' [N,2,h,w], that prediction: exp(-v) of the velocity the network predicted
        (netR.inverse_prediction: K more squaring steps).  It inverts the integrated map in its true-identity convention and does not
        undo the slight zoom of the warp's grid."""
        pred = self.netR.last_prediction()
        if pred is None:
            raise RuntimeError('register: no forward pass yet')
        if surface and (labels_A is None or labels_B is None or num_classes is None):
            raise ValueError('register: surface=True needs labels_A, labels_B and num_classes, the two label maps and their class count')
        if inverse:
            if getattr(self.netR, 'integrate', 0) <= 0:
                raise ValueError('register: inverse=True needs a UNet STN built with --stn_integrate K > 0 (a velocity field to integrate '
                                 'backwards); this one predicts a displacement')
            if full_B is None:
                raise ValueError('register: inverse=True needs full_B, the images to warp onto A')
        with torch.no_grad():
            full_A = full_A.to(self.device, dtype=torch.float32).contiguous()
            if full_A.size(0) != pred[0].size(0):
                raise ValueError('register: %d images for a prediction of %d pairs' % (full_A.size(0), pred[0].size(0)))
            out = {'registered_A': self.netR.apply(pred, [full_A])[0], 'offsets': pred[0]}
            if translate and self._netT_runs_at(full_A.size(2), full_A.size(3)):
                out['fake_RT_B'] = self.netR.apply(pred, [self.netT(full_A)])[0]
            if labels_A is not None:
                labels_A = labels_A.to(self.device, dtype=torch.float32).contiguous()
                out['registered_labels_A'] = self.netR.apply(pred, [labels_A], sample='nearest')[0]
            score_labels = labels_A is not None and labels_B is not None
            score_points = landmarks_A is not None and landmarks_B is not None
            if score_labels or score_points:        # "before registration": the identity transformation, which also bridges two sizes
                identity = (torch.zeros((pred[0].size(0), 6), dtype=torch.float32, device=self.device), ops.GRID_AFFINE)
            if score_labels:
                labels_B = labels_B.to(self.device, dtype=torch.float32).contiguous()
                if num_classes is None:
                    num_classes = int(torch.maximum(labels_A.max(), labels_B.max()).item()) + 1
                out['overlap'] = ops.label_overlap(pred[0], pred[1], labels_A, labels_B, num_classes)
                out['overlap_before'] = ops.label_overlap(identity[0], identity[1], labels_A, labels_B, num_classes)
            if score_points:
                lm_A = landmarks_A.to(self.device, dtype=torch.float32).contiguous()
                lm_B = landmarks_B.to(self.device, dtype=torch.float32).contiguous()
                if lm_A.shape != lm_B.shape:
                    raise ValueError('register: landmarks_A %s and landmarks_B %s are no point pairs' % (tuple(lm_A.shape), tuple(lm_B.shape)))
                src_hw = tuple(full_A.shape[2:])
                out_hw = src_hw if full_B is None else tuple(full_B.shape[2:])
                for key, (p, mode) in (('tre_px', pred), ('tre_before_px', identity)):
                    out[key] = (ops.map_points(p, mode, lm_B, src_hw, out_hw) - lm_A).norm(dim=2)
            if regularity or jacobian_map:
                fixed_hw = tuple(full_A.shape[2:]) if full_B is None else tuple(full_B.shape[2:])
                out['jac_counts'], out['jac_stats'], det = self.netR.regularity(pred, fixed_hw, bool(jacobian_map))
                if jacobian_map:
                    out['jacobian_det'] = det
            if similarity:
                if full_B is None:
                    raise ValueError('register: similarity=True needs full_B, the fixed images')
                full_B = full_B.to(self.device, dtype=torch.float32).contiguous()
                zeros = torch.zeros((pred[0].size(0), 6), dtype=torch.float32, device=self.device)
                out['similarity'] = {'before': ops.joint_histogram(zeros, ops.GRID_AFFINE, full_A, full_B, bins, intensity_range, intensity_range),
                                     'after': self.netR.similarity(pred, full_A, full_B, bins, intensity_range, intensity_range)}
            if surface:
                zeros = torch.zeros((pred[0].size(0), 6), dtype=torch.float32, device=self.device)
                before = ops.surface_distance(zeros, ops.GRID_AFFINE, labels_A, labels_B, num_classes, surface_max_dist)
                after = self.netR.surface(pred, labels_A, labels_B, num_classes, surface_max_dist, bool(surface_map))
                out['surface'] = {'before': before[:2], 'after': after[:2]}
                if surface_map:
                    out['surface_dist2'] = after[2]
            if inverse:
                inv = self.netR.inverse_prediction()
                full_B = full_B.to(self.device, dtype=torch.float32).contiguous()
                if full_B.size(0) != inv[0].size(0):
                    raise ValueError('register: %d fixed images for a prediction of %d pairs' % (full_B.size(0), inv[0].size(0)))
                out['registered_B'] = self.netR.apply(inv, [full_B])[0]
                out['inverse_offsets'] = inv[0]
        return out

    REFINE_TERMS = ('mind', 'lncc', 'l1')
    REFINE_LR = 3e-3                   # normalised units per Adam step (0.38 px of a 256-wide image) and the weight of the smoothness
    REFINE_LAMBDA_SMOOTH = 1.0         # term: the best pair of tools/refine_record.py's sweep (tools/profiles/refine.txt)

    def refine(self, full_A, full_B, steps, lr=None, term='mind', lambda_smooth=None, lambda_fold=0.0, fold_margin=0.0, **term_options):
        """Test-time refinement ("instance optimisation"): `steps` Adam steps on THIS pair at its native size, starting from the last
        prediction — the network's, or the composite after cascade().  The parameter is a fresh leaf at the network's size: the offsets
        [N,2,h,w], the VELOCITY where netR was built with --stn_integrate K > 0 (the prediction inside the loop is its exponential, so
        the result stays diffeomorphic and keeps its inverse_prediction()), or dtheta [N,6].  No network weight receives a gradient or
        is read after the start.  Each step: full_A (for 'l1': netT(full_A), computed once) warped at full_B's size by the prediction
        with a gradient towards it (netR.apply(..., grad=True): nemar_warp_resampled_bwd), the image term against full_B — 'mind'
        (ops.mind_loss; across modalities, no generator pass), 'lncc' (ops.local_ncc) or 'l1' (ops.l1_loss; ValueError when netT
        cannot run at full_A's size); term_options go to that op — plus, for a UNet STN, lambda_smooth * ops.smoothness(parameter) and
        lambda_fold * ops.fold_penalty(prediction, fold_margin); then one nemar_adam_step (betas 0.9 / 0.999) on four plain buffers.
        No host synchronisation.  Returns {'objective': float32 [steps + 1] on the device — before, and after each step — and 'offsets':
        the refined prediction}, and installs it (and the refined velocity) as netR's last prediction: a following register() warps and
        scores with it."""
        steps = int(steps)
        if steps < 0:
            raise ValueError('refine: %d steps' % steps)
        if term not in self.REFINE_TERMS:
            raise ValueError('refine: term %r is not one of %s' % (term, self.REFINE_TERMS))
        last = self.netR.last_prediction()
        if last is None:
            raise RuntimeError('refine: no forward pass yet')
        mode = last[1]
        lr = self.REFINE_LR if lr is None else float(lr)
        lambda_smooth = self.REFINE_LAMBDA_SMOOTH if lambda_smooth is None else float(lambda_smooth)
        K = getattr(self.netR, 'integrate', 0) if mode == ops.GRID_UNET else 0
        velocity = getattr(self.netR, 'last_velocity', None) if K > 0 else None
        with torch.no_grad():
            full_A = full_A.to(self.device, dtype=torch.float32).contiguous()
            full_B = full_B.to(self.device, dtype=torch.float32).contiguous()
            if full_A.size(0) != last[0].size(0) or full_B.size(0) != last[0].size(0):
                raise ValueError('refine: %d / %d images for a prediction of %d pairs' % (full_A.size(0), full_B.size(0), last[0].size(0)))
            moving = full_A
            if term == 'l1':
                if not self._netT_runs_at(full_A.size(2), full_A.size(3)):
                    raise ValueError("refine: term 'l1' needs netT(full_A), and netT (%s) cannot run at %d x %d"
                                     % (self.opt.netG, full_A.size(2), full_A.size(3)))
                moving = self.netT(full_A).contiguous()
            start = last[0] if velocity is None else velocity
            param = start.detach().clone().contiguous().requires_grad_(True)
        image_term = {'mind': ops.mind_loss, 'lncc': ops.local_ncc, 'l1': ops.l1_loss}[term]
        out_hw = tuple(full_B.shape[2:])
        m, v = torch.zeros_like(param), torch.zeros_like(param)
        objective = torch.empty((steps + 1,), dtype=torch.float32, device=self.device)
        st = ops._stream

        def prediction():
            return self.netR._resized(ops.integrate_velocity(param, K)) if velocity is not None else param

        def total(pred):
            warped = self.netR.apply((pred, mode), [moving], out_hw=out_hw, grad=True)[0]
            loss = image_term(warped, full_B, **term_options)
            if mode == ops.GRID_UNET:
                if lambda_smooth:
                    loss = loss + ops.smoothness(param, None, 0.0, lambda_smooth)
                if lambda_fold:
                    loss = loss + ops.fold_penalty(pred, fold_margin, lambda_fold)
            return loss

        for k in range(steps):
            param.grad = None
            loss = total(prediction())
            objective[k].copy_(loss.detach())
            loss.backward()
            ops.L.adam_step(ops._p(param), ops._p(param.grad.contiguous()), ops._p(m), ops._p(v), param.numel(), lr, 0.9, 0.999, 1e-8, k + 1, st())
        with torch.no_grad():
            pred = prediction().detach()
            objective[steps].copy_(total(pred))
            param.grad = None
            refined = param.detach()
            if mode == ops.GRID_UNET:
                self.netR.set_refined(pred, refined if velocity is not None else None)
            else:
                self.netR.last_dtheta = refined
        return {'objective': objective, 'offsets': pred}

    def _netT_runs_at(self, h, w):
        """netT is fully convolutional, but its strided levels must divide the size: two for the ResNet generators (a transposed
        convolution doubles what a stride-2 convolution halved only for even sizes), `num_downs` for the U-Nets (their skips concatenate)"""
        g = self.opt.netG
        levels = networks._UNET_DOWNS.get(g, 2 if g in networks._RESNET_BLOCKS else None)
        return levels is not None and h % (1 << levels) == 0 and w % (1 << levels) == 0 and min(h, w) >= (1 << levels)

    # ---- forward -------------------------------------------------------------------------------------------
    def _fork_prediction(self, n_warps):
        """netR's prediction for the set_input pair as handles (netR.fork_field): one per warp, the regulariser's, and — None where the
        term is off — the fold term's, the EPE term's and the label-overlap term's"""
        kw = {}
        if self._fold_on:
            kw['fold'] = True
        extra = int(self._epe_on) + int(self._dice_on)
        if extra:
            kw['extra'] = extra
        # (the cascade is a matter of the training step: test() and what builds on it look once)
        looks = {'passes': self._train_passes} if self._train_passes > 1 and torch.is_grad_enabled() else {}
        out = self.netR.fork_field(self.netR.predict(self.real_A, self.real_B, **looks), n_warps, **kw)
        more = list(out[-1]) if extra else []
        return (out[0], out[1], (out[2] if self._fold_on else None), (more.pop(0) if self._epe_on else None),
                (more.pop(0) if self._dice_on else None))

    def _dice_labels(self, what):
        """the batch's two label maps, checked"""
        la, lb = getattr(self, 'labels_A', None), getattr(self, 'labels_B', None)
        if la is None or lb is None:
            raise RuntimeError('%s--lambda_dice %g: the current batch carries no labels_A / labels_B to train against (--labels K of the '
                               'gpupairs dataset)' % (what, self._lambda_dice))
        want = (self.real_A.size(0), 1, self.real_A.size(2), self.real_A.size(3))
        if tuple(la.shape) != want or tuple(lb.shape) != want:
            raise ValueError('--lambda_dice: labels_A %s / labels_B %s are not the size of the prediction, %s' % (tuple(la.shape), tuple(lb.shape), want))
        return la, lb

    def _further_stn_terms(self, f_fold, f_epe, f_dice=None):
        if self._fold_on:
            self.stn_fold_term = self.netR.fold_term(f_fold, self._fold_margin)
        if self._epe_on:
            gt = getattr(self, 'gt_field', None)
            if gt is None:
                raise RuntimeError('--lambda_epe %g: the current batch carries no gt_field to train against (train with --misalign '
                                   'affine|elastic|both)' % self._lambda_epe)
            want = (self.real_A.size(0), 2, self.real_A.size(2), self.real_A.size(3))
            if tuple(gt.shape) != want:
                raise ValueError('--lambda_epe: gt_field %s is not the size of the prediction, %s' % (tuple(gt.shape), want))
            self.stn_epe_term = self.netR.epe_term(f_epe, gt, self._epe_eps)
        if self._dice_on:
            la, lb = self._dice_labels('')
            self.stn_dice_term = self.netR.dice_term(f_dice, la, lb, self._dice_classes, self._dice_eps, self._dice_background)

    def _registered_for_netT(self):
        """registered_real_A as netT reads it.  With the MIND term on the image has two consumers, netT and the term: two handles
        (ops.fork), the term's kept for backward_T_and_R; self.registered_real_A stays the tensor visuals and cascade() read"""
        if not self._mind_on:
            return self.registered_real_A
        for_t, self._mind_handle = ops.fork(self.registered_real_A, 2)
        return for_t

    def forward(self):
        if not self._batched:
            # the reference's own order (models/nemar_model.py:161-176)
            self.fake_B = self.netT(self.real_A)
            if self._fold_on or self._epe_on or self._dice_on or self._train_passes > 1:
                # netR.forward() piece by piece, with one more handle of the field for each further term (or with several looks)
                (f_warp,), f_reg, f_fold, f_epe, f_dice = self._fork_prediction(1)
                warped = self.netR.warp(f_warp, [self.real_A, self.fake_B])
                reg_term = self.netR.regularization(f_reg, warped[0])
                self._further_stn_terms(f_fold, f_epe, f_dice)
            else:
                warped, reg_term = self.netR(self.real_A, self.real_B, apply_on=[self.real_A, self.fake_B])
            self.stn_reg_term = reg_term
            self.registered_real_A = warped[0]
            self.fake_TR_B = self.netT(self._registered_for_netT())     # registration first, then translation
            self.fake_RT_B = warped[1]                             # translation first, then registration
        else:
            # Same graph, evaluated with T's two applications as ONE batch: the deformation depends on (a, b) only, so
            # R(a) is available before T runs, and T (per-sample InstanceNorm, no cross-sample op) maps [a ; R(a)] to
            # [T(a) ; T(R(a))].  Every T layer then launches once on 2x the pixels (full second round of workgroups,
            # one weight-gradient reduction instead of two).
            n = self.real_A.size(0)
            # (the field has three consumers — two warps and the regulariser —, the batch of T two sources and two slices: the library's own
            # nodes for fan-out, concatenation and slicing, ops.fork / cat_batch / split_batch, instead of autograd's ATen kernels)
            (f_a, f_b), f_reg, f_fold, f_epe, f_dice = self._fork_prediction(2)
            self.registered_real_A = self.netR.warp(f_a, [self.real_A])[0]
            # (only the second half is differentiated: the stem's data gradient runs on it alone)
            with ops.norm_segments(2):
                both = self.netT(ops.grad_from(ops.cat_batch([self.real_A, self._registered_for_netT()]), n))
            self.fake_B, self.fake_TR_B = ops.split_batch(both, 2)
            self.fake_RT_B = self.netR.warp(f_b, [self.fake_B])[0]
            self.stn_reg_term = self.netR.regularization(f_reg, self.registered_real_A)
            self._further_stn_terms(f_fold, f_epe, f_dice)
        self._resized = {}
        if self.tb_visualizer is not None:
            # the reference runs netR a second time here (get_grid, :172-173); the field of the pass above is the same tensor
            self.deformation_field_A_to_B = getattr(self.netR, 'last_offsets', None)

    def _half(self, name, tensor, level):
        """tensor bilinearly resized to 1/2^level resolution (reference :185-188 etc.).  Only the step's INPUTS (real_A,
        real_B: `name` given) are cached — they are resized once instead of once per discriminator pass and the cache dies
        with set_input(); generated images are resized where they are used."""
        sh, sw = self.real_A.size(2) // (2 ** level), self.real_A.size(3) // (2 ** level)
        if name is None:
            return ops.resize_bilinear(tensor, sh, sw)
        key = (name, level)
        if key not in self._resized:
            self._resized[key] = ops.resize_bilinear(tensor, sh, sw)
        return self._resized[key]

    def _d_terms_batched(self, specs):
        """_d_terms for several (image, image_name, target_is_real, weight, detach) at once: the discriminators see the
        images as one batch (no cross-sample op in D), the loss terms are taken on the per-image slices."""
        k, n = len(specs), self.real_A.size(0)
        imgs = [(im.detach() if det else im) for (im, _, _, _, det) in specs]
        # an image every discriminator reads: one handle per reader (ops.fork: the readers' gradients are added by the library's kernel)
        readers = 1 + len(self.netD_multiresolution)
        handles = [ops.fork(im, readers) for im in imgs]
        a_rep = ops.cat_batch([self.real_A] * k)
        with ops.norm_segments(k):
            out = ops.split_batch(self.netD(a_rep, ops.cat_batch([h[0] for h in handles])), k)
        terms = [[self.criterionGAN(out[i], tr, w)] for i, (_, _, tr, w, _) in enumerate(specs)]
        for lvl, netD_S in enumerate(self.netD_multiresolution):
            a_r = self._half('real_A', self.real_A, lvl + 1)
            img_r = [self._half(name, h[lvl + 1], lvl + 1) for h, (_, name, _, _, det) in zip(handles, specs)]
            with ops.norm_segments(k):
                out = ops.split_batch(netD_S(ops.cat_batch([a_r] * k), ops.cat_batch(img_r)), k)
            for i, (_, _, tr, w, _) in enumerate(specs):
                terms[i].append(self.criterionGAN(out[i], tr, w))
        return terms

    def _d_terms(self, image, image_name, target_is_real, weight, detach):
        """[weight * GANLoss(D_i(real_A_i, image_i), target)] over the full-resolution discriminator and every
        reduced-resolution one."""
        img = image.detach() if detach else image
        terms = [self.criterionGAN(self.netD(self.real_A, img), target_is_real, weight)]
        for i, netD_S in enumerate(self.netD_multiresolution):
            a_r = self._half('real_A', self.real_A, i + 1)
            img_r = self._half(image_name, img, i + 1)
            terms.append(self.criterionGAN(netD_S(a_r, img_r), target_is_real, weight))
        return terms

    # ---- discriminator step ---------------------------------------------------------------------------------
    def backward_D(self):
        w = 0.5 * self.opt.lambda_GAN
        if self._batched:
            real, fake_tr, fake_rt = self._d_terms_batched([(self.real_B, 'real_B', True, w, True),
                                                            (self.fake_TR_B, None, False, w, True),
                                                            (self.fake_RT_B, None, False, w, True)])
        else:
            real = self._d_terms(self.real_B, 'real_B', True, w, detach=True)
            fake_tr = self._d_terms(self.fake_TR_B, None, False, w, detach=True)
            fake_rt = self._d_terms(self.fake_RT_B, None, False, w, detach=True)
        inv = 1.0 / w if w != 0 else 0.0
        self.loss_D_fake_TR = _LazyLoss([(t, inv) for t in fake_tr])
        self.loss_D_fake_RT = _LazyLoss([(t, inv) for t in fake_rt])
        terms = real + fake_tr + fake_rt
        self.loss_D = _LazyLoss([(t, 1.0) for t in terms])
        torch.autograd.backward(terms, [self._one] * len(terms))
        return self.__dict__['_lazy_loss_D']

    # ---- translation + registration step ----------------------------------------------------------------------
    def backward_T_and_R(self):
        opt = self.opt
        # each generated image is read by its L1 term and by the discriminators: two handles (ops.fork)
        if self._lncc_on:
            # ... and by its local NCC term: three handles
            tr_l1, tr_d, tr_cc = ops.fork(self.fake_TR_B, 3)
            rt_l1, rt_d, rt_cc = ops.fork(self.fake_RT_B, 3)
        else:
            tr_l1, tr_d = ops.fork(self.fake_TR_B, 2)
            rt_l1, rt_d = ops.fork(self.fake_RT_B, 2)
        l1_tr = self.criterionL1(tr_l1, self.real_B, opt.lambda_recon)
        l1_rt = self.criterionL1(rt_l1, self.real_B, opt.lambda_recon)
        if self._batched:
            gan_tr, gan_rt = self._d_terms_batched([(tr_d, None, True, opt.lambda_GAN, False),
                                                    (rt_d, None, True, opt.lambda_GAN, False)])
        else:
            gan_tr = self._d_terms(tr_d, None, True, opt.lambda_GAN, detach=False)
            gan_rt = self._d_terms(rt_d, None, True, opt.lambda_GAN, detach=False)
        self.loss_L1_TR = _LazyLoss([(l1_tr, 1.0)])
        self.loss_GAN_TR = _LazyLoss([(t, 1.0) for t in gan_tr])
        self.loss_L1_RT = _LazyLoss([(l1_rt, 1.0)])
        self.loss_GAN_RT = _LazyLoss([(t, 1.0) for t in gan_rt])
        self.loss_smoothness = _LazyLoss([(self.stn_reg_term, float(opt.lambda_smooth))])
        roots = [l1_tr, l1_rt] + gan_tr + gan_rt
        grads = [self._one] * len(roots)
        if opt.lambda_smooth != 0.0:
            roots.append(self.stn_reg_term)         # d(lambda * reg) = lambda * d(reg): the weight is the seed
            grads.append(self._lam_smooth)
        total = [(r, 1.0) for r in roots[:len(roots) - (1 if opt.lambda_smooth != 0.0 else 0)]] + [(self.stn_reg_term, float(opt.lambda_smooth))]
        if self._fold_on:
            self.loss_fold = _LazyLoss([(self.stn_fold_term, self._lambda_fold)])
            roots.append(self.stn_fold_term)        # one more root, seeded with its weight like the smoothness term
            grads.append(self._lam_fold)
            total.append((self.stn_fold_term, self._lambda_fold))
        if self._epe_on:
            self.loss_EPE = _LazyLoss([(self.stn_epe_term, self._lambda_epe)])
            roots.append(self.stn_epe_term)         # likewise
            grads.append(self._lam_epe)
            total.append((self.stn_epe_term, self._lambda_epe))
        if self._dice_on:
            self.loss_Dice = _LazyLoss([(self.stn_dice_term, self._lambda_dice)])
            roots.append(self.stn_dice_term)        # likewise
            grads.append(self._lam_dice)
            total.append((self.stn_dice_term, self._lambda_dice))
        if self._lncc_on:
            # two more roots, against real_B as the L1 terms are; the weight is the kernel's factor
            lncc = [ops.local_ncc(h, self.real_B.detach(), self._lncc_win, factor=self._lambda_lncc) for h in (tr_cc, rt_cc)]
            self.loss_LNCC_TR, self.loss_LNCC_RT = (_LazyLoss([(t, 1.0)]) for t in lncc)
            roots += lncc
            grads += [self._one] * 2
            total += [(t, 1.0) for t in lncc]
        if self._mind_on:
            # one more root: registered_real_A against real_B, descriptor against descriptor; it reaches netR through the warp and
            # neither netT nor netD.  The weight is the kernel's factor
            mind = ops.mind_loss(self._mind_handle, self.real_B.detach(), self._mind_patch, self._mind_dil, self._mind_eps, factor=self._lambda_mind)
            self._mind_handle = None
            self.loss_MIND_R = _LazyLoss([(mind, 1.0)])
            roots.append(mind)
            grads.append(self._one)
            total.append((mind, 1.0))
        torch.autograd.backward(roots, grads)
        return _LazyLoss(total)

    # ---- the step as a captured hipGraph (launch-bound small configurations: BASELINE config 1) ---------------------------------
    def enable_step_graph(self, warmup=3):
        """Capture optimize_parameters() for the CURRENT input shapes into a hipGraph and replay it from then on: one graph launch
        instead of ~1100 kernel launches per step.  Single process only (the gradient all-reduce is not captured).  Inputs are copied
        into static buffers; dropout offsets and Adam's step-dependent scalars live in device memory (ops.step_params), so every
        replay is a fresh step; an eager run in that mode produces the same bits (tests/test_step_gpu.py)."""
        if dist.is_distributed():
            raise RuntimeError('enable_step_graph: single-process only')
        if self.tb_visualizer is not None:
            raise RuntimeError('enable_step_graph: disable the tensorboard visualiser (it reads tensors between launches)')
        ops.step_params(True, self.device)
        self._static_A, self._static_B = self.real_A.clone(), self.real_B.clone()
        # the EPE term reads the batch's ground-truth field inside the captured step: a static buffer like the two images'
        self._static_gt = None
        if self._epe_on:
            if getattr(self, 'gt_field', None) is None:
                raise RuntimeError('enable_step_graph: --lambda_epe %g and the current batch carries no gt_field (train with --misalign '
                                   'affine|elastic|both)' % self._lambda_epe)
            self._static_gt = self.gt_field.clone()
            self.gt_field = self._static_gt
        # ... and the label-overlap term the batch's two label maps
        self._static_labels = None
        if self._dice_on:
            la, lb = self._dice_labels('enable_step_graph: ')
            self._static_labels = (la.clone(), lb.clone())
            self.labels_A, self.labels_B = self._static_labels
        opts =[self.optimizer_D, self.optimizer_R, self.optimizer_T]
        # The warm-up steps must not train: they run with lr = 0 (Adam leaves every parameter bit-unchanged: p - 0 * x) and the
        # moments, step counts and the dropout step counter are put back afterwards — the first replay is then step 1 of the same
        # schedule an eager loop would follow, on untouched weights.  (The packed-weight images are rebuilt from the same values, so
        # the state the capture sees — T and R to be re-packed, D's forward images valid — is the steady state of every later step.)
        saved = [(o.m.clone(), o.v.clone(), o.step_count, o.param_groups[0]["lr"]) for o in opts]
        # (--norm batch: the warm-up steps also move the running statistics and counters: put back as well)
        bn_bufs = [b for net in (self.netT, self.netD, *self.netD_multiresolution) for name, b in net.named_buffers()
                   if name.endswith(('running_mean', 'running_var', 'num_batches_tracked'))]
        bn_saved = [b.clone() for b in bn_bufs]
        saved_step = ops._step_params["step"]
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                         # warm-up on a side stream (allocator pools, lazy attributes, packs)
            try:
                for o in opts:
                    o.param_groups[0]["lr"] = 0.0
                for _ in range(warmup):
                    self.real_A, self.real_B = self._static_A, self._static_B
                    ops.begin_step()
                    self._optimize_parameters_eager()
            finally:
                for o, (m, v, n, lr) in zip(opts, saved):
                    o.m.copy_(m)
                    o.v.copy_(v)
                    o.step_count = n
                    o.param_groups[0]["lr"] = lr
                for b, v in zip(bn_bufs, bn_saved):
                    b.copy_(v)
                ops._step_params["step"] = saved_step
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self._graph = torch.cuda.CUDAGraph()
        self.real_A, self.real_B = self._static_A, self._static_B
        ops.begin_step()
        for o in opts:
            o.prepare_step(o.step_count + 1)
        ops._step_params["capturing"] = True
        try:
            with torch.cuda.graph(self._graph):
                self._optimize_parameters_eager()
        finally:
            ops._step_params["capturing"] = False
        # (the capture itself executed nothing: the step it describes is run by the first replay; undo its host book-keeping)
        for o in opts:
            o.step_count -= 1
        ops._step_params["step"] -= 1
        self._graph_losses = {k: v for k, v in self.__dict__.items() if k.startswith('_lazy_loss_')}
        ops.pin_workspaces(True)          # the graph holds their addresses: from now on they may grow but are never freed

    def _replay_step(self):
        static_gt = getattr(self, '_static_gt', None)
        gt_fits = static_gt is None or (getattr(self, 'gt_field', None) is not None and self.gt_field.shape == static_gt.shape)
        static_labels = getattr(self, '_static_labels', None)
        if static_labels is not None:
            la, lb = getattr(self, 'labels_A', None), getattr(self, 'labels_B', None)
            gt_fits = gt_fits and la is not None and lb is not None and la.shape == static_labels[0].shape and lb.shape == static_labels[1].shape
        if self.real_A.shape != self._static_A.shape or self.real_B.shape != self._static_B.shape or not gt_fits:
            # a batch of another shape (the ragged last batch of an epoch): the captured launches do not describe it — run this step
            # eagerly, in the same device-parameter mode (bit-identical arithmetic), and keep the graph for the next full batch
            ops.begin_step()
            return self._optimize_parameters_eager()
        if self.real_A is not self._static_A:
            self._static_A.copy_(self.real_A)
            self._static_B.copy_(self.real_B)
            self.real_A, self.real_B = self._static_A, self._static_B
        if static_gt is not None and self.gt_field is not static_gt:
            static_gt.copy_(self.gt_field)
            self.gt_field = static_gt
        if static_labels is not None and self.labels_A is not static_labels[0]:
            static_labels[0].copy_(self.labels_A)
            static_labels[1].copy_(self.labels_B)
            self.labels_A, self.labels_B = static_labels
        ops.begin_step()
        for o in (self.optimizer_D, self.optimizer_R, self.optimizer_T):
            o.prepare_step(o.step_count + 1)
        self._graph.replay()
        for o in (self.optimizer_D, self.optimizer_R, self.optimizer_T):
            o.replayed_step()
        # the loss_* attributes were created during the capture: their term buffers hold THIS step's values now, any sum formed by an
        # earlier read is stale
        for k, v in self._graph_losses.items():
            v._v = None
            self.__dict__[k] = v          # (an eager step in between — a ragged batch — had replaced them)

    def optimize_parameters(self):
        if getattr(self, '_graph', None) is not None:
            return self._replay_step()
        ops.begin_step()
        return self._optimize_parameters_eager()

    def _optimize_parameters_eager(self):
        # data parallel: how many gradient contributions each parameter will receive is COUNTED while the forward passes run
        # (T: once batched / twice; every discriminator: once batched / three times) — GradSync launches a bucket's all-reduce when
        # its last contribution has been issued
        self.sync_T.count_uses()
        self.sync_R.count_uses()
        self.forward()
        # D step
        self.set_requires_grad([self.netT, self.netR], False)
        self.optimizer_D.zero_grad()
        self.sync_D.count_uses()
        self.sync_D.begin()
        self.backward_D()
        self.sync_D.finish()
        self.optimizer_D.step()
        self.set_requires_grad([self.netT, self.netR], True)
        # T + R step (sees the updated D)
        self.set_requires_grad([self.netD, *self.netD_multiresolution], False)
        self.optimizer_R.zero_grad()
        self.optimizer_T.zero_grad()
        self.sync_T.begin()
        self.sync_R.begin()
        self.backward_T_and_R()
        self.sync_R.finish()
        self.sync_T.finish()
        self.optimizer_R.step()
        self.optimizer_T.step()
        self.set_requires_grad([self.netD, *self.netD_multiresolution], True)
        if self.tb_visualizer is not None:
            self.tb_visualizer.iteration_step()
