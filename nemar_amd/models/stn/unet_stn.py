"""Dense-deformation registration network — mirror of reference models/stn/unet_stn.py (ResUnet :28-102, UnetSTN
:105-201, cfg dicts :11-25) on the gfx950 kernels.

MI355X-first differences from the reference, none of which change results:
  * the identity grid (torch.linspace, :121-129) and the permute to NHWC (:167) are never materialised: the warp
    kernel synthesises `linspace(-1,1) + offsets` in registers from the planar offset field;
  * both `apply_on` images are warped by one autograd node, so d loss / d offsets is accumulated inside the
    backward kernels;
  * torch.cat([img_a, img_b]) and torch.cat([x, skip]) (:80,97) are two-pointer conv inputs;
  * the multi-resolution weights 1, 1/2, 1/4... of the regulariser (:186-200) are folded into the stencil kernel.
The reference's quirks are reproduced deliberately: the linspace identity under
align_corners=False is a slight zoom (B1); decoder convs ignore --init_type and use kaiming (B4: the `init_fun`
typo); the low-res upsample branch fires only if BOTH dims differ (B3).
"""
import torch.nn as nn

from ... import ops
from .layers import Conv, DownBlock, ResnetTransformer, prediction_mode, prediction_tensor
from .stn_losses import smoothness_loss

sampling_align_corners = False
sampling_mode = 'bilinear'

# encoder widths / decoder widths / options per configuration (reference :11-25).  'A' is the reference's only
# configuration.
# 'deep' (BASELINE.json config 5, 1024x1024): two more levels, so that the bottleneck is again 2x2 at 1024x1024 — not in the
# reference, whose ResUnet code builds it from the same dict entries (tests/golden/make_golden.py does exactly that).
ndf = {'A': [32, 64, 64, 64, 64, 64, 64], 'deep': [32, 64, 64, 64, 64, 64, 64, 64, 64], }
nuf = {'A': [64, 64, 64, 64, 64, 64, 32], 'deep': [64, 64, 64, 64, 64, 64, 64, 64, 32], }
use_down_resblocks = {'A': True, 'deep': True, }
resnet_nblocks = {'A': 3, 'deep': 3, }
refine_output = {'A': True, 'deep': True, }
down_activation = {'A': 'leaky_relu', 'deep': 'leaky_relu', }
up_activation = {'A': 'leaky_relu', 'deep': 'leaky_relu', }


class ResUnet(nn.Module):
    """(img_a, img_b) -> 2-channel offset field (reference :28-102)."""

    def __init__(self, nc_a, nc_b, cfg, init_func, init_to_identity):
        super().__init__()
        act = down_activation[cfg]
        self.ndown_blocks = len(ndf[cfg])
        self.nup_blocks = len(nuf[cfg])
        assert self.ndown_blocks >= self.nup_blocks
        in_nf = nc_a + nc_b
        skip_nf = {}
        for i, out_nf in enumerate(ndf[cfg], start=1):
            setattr(self, 'down_%d' % i, DownBlock(in_nf, out_nf, 3, 1, 1, activation=act, init_func=init_func,
                                                   bias=True, use_resnet=use_down_resblocks[cfg], use_norm=False))
            skip_nf[i] = out_nf
            in_nf = out_nf
        self.has_bottleneck = use_down_resblocks[cfg]
        if self.has_bottleneck:
            self.c1 = Conv(in_nf, 2 * in_nf, 1, 1, 0, activation=act, init_func=init_func, bias=True)
            self.t = ResnetTransformer(2 * in_nf, resnet_nblocks[cfg], init_func) if resnet_nblocks[cfg] else None
            self.c2 = Conv(2 * in_nf, in_nf, 1, 1, 0, activation=act, init_func=init_func, bias=True)
        act = up_activation[cfg]
        level = self.ndown_blocks
        for out_nf in nuf[cfg]:
            # the reference passes `init_fun=` (sic) here, which Conv swallows: decoder convs are always kaiming
            setattr(self, 'up_%d' % level, Conv(in_nf + skip_nf[level], out_nf, 3, 1, 1, bias=True, activation=act,
                                                init_func='kaiming'))
            in_nf = out_nf
            level -= 1
        if refine_output[cfg]:
            self.refine = nn.Sequential(ResnetTransformer(in_nf, 1, init_func),
                                        Conv(in_nf, in_nf, 1, 1, 0, init_func=init_func, activation=act))
        else:
            self.refine = None
        self.output = Conv(in_nf, 2, 3, 1, 1, bias=True, activation=None,
                           init_func=('zeros' if init_to_identity else init_func))

    def forward(self, img_a, img_b):
        skips = {}
        x, x2 = img_a, img_b                      # cat([img_a, img_b], 1) as two conv sources
        for i in range(1, self.ndown_blocks + 1):
            x, skips[i] = getattr(self, 'down_%d' % i)(x, x2)
            x2 = None
        if self.has_bottleneck:
            x = self.c1(x)
            if self.t is not None:
                x = self.t(x)
            x = self.c2(x)
        level = self.ndown_blocks
        while level > self.ndown_blocks - self.nup_blocks:
            s = skips[level]
            x = ops.resize_bilinear(x, s.size(2), s.size(3))
            x = getattr(self, 'up_%d' % level)(x, s)   # cat([x, s], 1) as two conv sources
            level -= 1
        if self.refine is not None:
            x = self.refine(x)
        return self.output(x)


class UnetSTN(nn.Module):
    """Predicts the deformation and applies it (reference :105-201)."""

    def __init__(self, in_channels_a, in_channels_b, height, width, cfg, init_func, stn_bilateral_alpha,
                 init_to_identity, multi_resolution_regularization, integrate=0):
        """integrate = K > 0 (--stn_integrate; not in the reference): the network's output is a stationary VELOCITY field and the warp
        reads exp(v), K scaling-and-squaring steps at the network's size (ops.integrate_velocity) — a composition of 2^K near-identity
        maps, free of folds up to discretisation and the clamp at the border.  0: the output is the displacement itself."""
        super().__init__()
        self.oh, self.ow = height, width
        self.in_channels_a, self.in_channels_b = in_channels_a, in_channels_b
        self.offset_map = ResUnet(in_channels_a, in_channels_b, cfg, init_func, init_to_identity)
        self.alpha = stn_bilateral_alpha
        self.multi_resolution_regularization = multi_resolution_regularization
        self.integrate = int(integrate)

    def _resized(self, d):
        """the reference's low-resolution branch (:139,165): `and`, as there"""
        if d.size(2) != self.oh and d.size(3) != self.ow:
            return ops.resize_bilinear(d, self.oh, self.ow)
        return d

    def _deformation(self, img_a, img_b):
        d = self.offset_map(img_a, img_b)
        if self.integrate > 0:
            # field[0] stays the velocity (the smoothness regulariser acts on it, as the diffeomorphic VoxelMorph line does); everything
            # that reads field[1] — the warp, the fold term, last_prediction() — sees the integrated field.  Two handles of the velocity,
            # one per consumer: their gradients are added by the library's kernel
            v_int, v_reg = ops.fork(d, 2)
            self.last_velocity = d.detach()        # no copy
            d_up = self._resized(ops.integrate_velocity(v_int, self.integrate))
            self.last_offsets = d_up.detach()
            return v_reg, d_up
        d_up = self._resized(d)
        self.last_offsets = d_up.detach()          # for the offset statistics (util/visualizer.OffsetMeter); no copy
        return d, d_up

    def inverse_prediction(self):
        """(offsets, grid mode) of the INVERSE of the last prediction: exp(-v), one more integration of the last velocity — usable
        wherever a prediction is (apply, overlap, map_points, regularity, similarity, compose).  It inverts exp(v) in the integration's
        true-identity convention: it does not undo the slight zoom the warp's linspace grid adds, so
        apply(inverse) after apply(forward) is two of those zooms away from the identity.  None before the first pass.  No autograd."""
        if self.integrate <= 0:
            raise RuntimeError('inverse_prediction: this UnetSTN predicts a displacement, not a velocity (integrate = 0: build it with '
                               '--stn_integrate K > 0)')
        v = getattr(self, 'last_velocity', None)
        if v is None:
            return None
        import torch
        with torch.no_grad():
            return self._resized(ops.integrate_velocity(v, self.integrate, -1.0)), ops.GRID_UNET

    def last_prediction(self):
        """(what the last forward pass handed to the warp kernel, its grid mode) — None before the first pass"""
        d = getattr(self, 'last_offsets', None)
        return None if d is None else (d, ops.GRID_UNET)

    def get_grid(self, img_a, img_b, return_offsets_only=False):
        """The sampling grid [N,H,W,2] aligning img_a with img_b (reference :131-146).  Built with torch ops: this is
        the inspection API, not the training path (the kernels never materialise the grid)."""
        import torch
        _, d = self._deformation(img_a, img_b)
        if return_offsets_only:
            return d.permute(0, 2, 3, 1)
        x = torch.linspace(-1.0, 1.0, self.ow, device=d.device)
        y = torch.linspace(-1.0, 1.0, self.oh, device=d.device)
        ident = torch.stack([x[None, :].expand(self.oh, self.ow), y[:, None].expand(self.oh, self.ow)], 0)
        return (ident[None] + d).permute(0, 2, 3, 1)

    # The forward pass in three pieces, so that a caller can evaluate the deformation once and warp several tensors at
    # different points of its own graph (NEMARModel runs T on [a, R(a)] as one batch): predict -> warp* -> regularization
    def predict(self, img_a, img_b, passes=1):
        """passes = K > 1 (--train_passes; not in the reference): a recursive cascade with SHARED weights, trained end to end.  The
        accumulated prediction starts as pass 1's field, taken where the warp reads it (after --stn_integrate and the low-resolution
        resize); every further pass warps the ORIGINAL img_a by it (one interpolation, as NEMARModel.cascade does), predicts from (that
        image, img_b) and composes the accumulated field with the new one (ops.compose_predictions(grad=True): both operands receive a
        gradient, the accumulated one a second through the warp — two handles, ops.fork).  Returns (composite, composite): the warps,
        the smoothness regulariser and the fold, EPE and Dice terms all act on the ONE transformation the warp reads — the regulariser
        sees the composite, not each pass's own field (nor, under --stn_integrate, the velocities).  Afterwards last_offsets is the
        detached composite, last_velocity None (a composite is the exponential of no single velocity) and last_pass_predictions the
        list of the K detached per-pass fields.  passes = 1 is the single look: exactly the code path without the argument."""
        passes = int(passes)
        if passes == 1:
            return self._deformation(img_a, img_b)
        if not 1 <= passes <= 8:
            raise ValueError('UnetSTN.predict: passes %d (1 .. 8)' % passes)
        _, acc = self._deformation(img_a, img_b)
        per_pass = [self.last_offsets]
        for _ in range(passes - 1):
            acc_warp, acc_comp = ops.fork(acc, 2)
            moved = ops.warp_unet(acc_warp, [img_a])[0]
            _, nxt = self._deformation(moved, img_b)
            per_pass.append(self.last_offsets)
            acc = ops.compose_predictions(acc_comp, ops.GRID_UNET, nxt, ops.GRID_UNET, (self.oh, self.ow), grad=True)
        self.last_offsets = acc.detach()
        self.last_velocity = None
        self.last_pass_predictions = per_pass
        return acc, acc

    def warp(self, field, imgs):
        return ops.warp_unet(field[1], list(imgs))

    def apply(self, field, imgs, out_hw=None, sample='bilinear', grad=False):
        """The prediction applied at ANY resolution, for inference: `field` is what predict() returned or last_prediction() (the offsets
        at the network's size, already past the reference's low-resolution branch); each image is sampled at out_hw (default: its own
        size) with the field resized inside the warp kernel (ops.warp_resampled).  sample='nearest' for label maps.  No autograd —
        unless grad=True: the same values with a gradient towards the prediction (refinement on the pair)."""
        return ops.warp_resampled(prediction_tensor(field), ops.GRID_UNET, list(imgs), out_hw, sample, grad)

    def set_refined(self, offsets, velocity=None):
        """what last_prediction() — and, with a velocity, inverse_prediction() — return from now on: a prediction refined on its own
        pair (NEMARModel.refine).  The velocity is the one `offsets` was integrated from."""
        self.last_offsets = offsets.detach()
        self.last_velocity = None if velocity is None else velocity.detach()

    def overlap(self, field, labels_moving, labels_fixed, num_classes):
        """Per-class overlap counts [N,K,3] (inter, moving, fixed) of labels_moving warped by the prediction — what
        apply(..., sample='nearest') gives, never written — against labels_fixed at its size (ops.label_overlap).  No autograd."""
        return ops.label_overlap(prediction_tensor(field), ops.GRID_UNET, labels_moving, labels_fixed, num_classes)

    def surface(self, field, labels_moving, labels_fixed, num_classes, max_dist=64, dist_map=False):
        """Boundary distances of labels_moving warped by the prediction — what apply(..., sample='nearest') gives, never written —
        against labels_fixed at its size: (counts [N,K,2,3] = boundary pixels, far, largest squared distance per class and direction;
        hist [N,K,2,max_dist^2] of the squared distances; the distance map [N,2,Ho,Wo] or None) — ops.surface_distance;
        ops.surface_summary turns counts and hist into the Hausdorff distance, HD95 and ASSD.  No autograd."""
        return ops.surface_distance(prediction_tensor(field), ops.GRID_UNET, labels_moving, labels_fixed, num_classes, max_dist, dist_map)

    def map_points(self, field, pts, src_hw, out_hw):
        """Where the prediction samples the src_hw source for points [N,P,2] (x, y) given in pixels of the out_hw fixed image
        (ops.map_points).  No autograd."""
        return ops.map_points(prediction_tensor(field), ops.GRID_UNET, pts, src_hw, out_hw)

    def regularity(self, field, out_hw=None, det_map=False):
        """How regular the prediction's transformation is at out_hw (default: the network's size): (counts [N,2] = interior pixels and
        folds, stats [N,5] = min / max / sum of the Jacobian determinant and the two log sums, the determinant map [N,Ho,Wo] or None) —
        ops.jacobian_stats; ops.regularity_summary turns counts and stats into fold share and SDlogJ.  No autograd."""
        return ops.jacobian_stats(prediction_tensor(field), ops.GRID_UNET, (self.oh, self.ow) if out_hw is None else out_hw, det_map)

    def similarity(self, field, moving, fixed, bins=32, range_moving=(-1., 1.), range_fixed=(-1., 1.), moments=True):
        """Intensity agreement of `moving` warped by the prediction — what apply() gives, never written — with `fixed` at its size:
        (counts [N,bins,bins], the joint histogram of the two channel means; moments [N,6] or None) — ops.joint_histogram;
        ops.similarity_summary turns them into mutual information, NCC, MSE and MAE.  Needs no annotation.  No autograd."""
        return ops.joint_histogram(prediction_tensor(field), ops.GRID_UNET, moving, fixed, bins, range_moving, range_fixed, moments)

    def compose(self, first, second, image=None, grad=False):
        """ONE prediction that samples where `first` and then `second` would in sequence — `second` was predicted from the pair `first`
        had already registered (a cascade pass), or `first` comes from an earlier run: the composite offsets [N,2,oh,ow] at the network's
        size (ops.compose_predictions), which apply(), overlap() and map_points() take like any prediction of this network.  Either
        operand may be a `(tensor, grid mode)` pair of another STN (an affine pre-registration).  With image [N,C,oh,ow] returns
        (offsets, image warped by them), from the same launch.  A zero field is the reference's slight zoom, not the identity, and
        composing keeps it: compose(first, zeros) != first.  No autograd — unless grad=True (no image then; a UNet operand at the
        network's size): the same values with a gradient towards both operands (ops.compose_predictions)."""
        return ops.compose_predictions(prediction_tensor(first), prediction_mode(first, ops.GRID_UNET), prediction_tensor(second),
                                       prediction_mode(second, ops.GRID_UNET), (self.oh, self.ow), image, grad)

    def set_last_prediction(self, offsets):
        """what last_prediction() returns from now on: a composite made outside the forward pass (NEMARModel.cascade)"""
        self.last_offsets = offsets.detach()
        self.last_velocity = None                  # a composite is the exponential of no single velocity: it has no inverse_prediction()

    def fork_field(self, field, n_warps, fold=False, extra=0):
        """-> ([one field per warp() call], the field for regularization()): handles of the same tensors (ops.fork), so that the
        consumers' gradients are added by the library's kernel instead of autograd's accumulation.  With fold=True a third element:
        one more handle of the field the warp reads, for fold_term().  With extra = k > 0 a last element: a list of k more such
        handles, one per further consumer of the field the warp reads (epe_term(), dice_term())."""
        d, d_up = field
        more = (1 if fold else 0) + int(extra)
        if d_up is d:
            hs = ops.fork(d, n_warps + 1 + more)
            out = [(h, h) for h in hs[:n_warps]], (hs[n_warps], hs[n_warps])
            rest = [(h, h) for h in hs[n_warps + 1:]]
        else:
            ups = ops.fork(d_up, n_warps + more)
            out = [(d, u) for u in ups[:n_warps]], (d, d_up)
            rest = [(d, u) for u in ups[n_warps:]]
        if fold:
            out = (*out, rest.pop(0))
        return (*out, rest) if extra else out

    def fold_term(self, field, margin=0.0):
        """mean over the interior pixels of max(0, margin - det) on the field the warp reads (ops.fold_penalty: the Jacobian
        determinant regularity() measures at the network's size).  The per-sample count of pixels with det <= margin stays on the
        device as `last_fold_active` (util/visualizer.FoldMeter)."""
        term, active = ops.fold_penalty(field[1], margin, 1.0, return_active=True)
        self.last_fold_active = active
        self.last_fold_interior = (field[1].size(2) - 1) * (field[1].size(3) - 1)      # per sample: what the counts are a share of
        return term

    def epe_term(self, field, gt_field, eps=0.01):
        """mean over all pixels of sqrt(|r|^2 + eps^2), r the residual registration_error measures against the ground-truth field
        gt_field [N,2,oh,ow] in pixels (ops.epe_loss), on the field the warp reads — past the integration and the low-resolution
        resize, where fold_term() acts."""
        return ops.epe_loss(field[1], ops.GRID_UNET, gt_field, eps, 1.0)

    def dice_term(self, field, labels_moving, labels_fixed, num_classes, eps=1.0, background=False):
        """mean over samples and classes of 1 - soft Dice of labels_moving warped bilinearly by the field the warp reads against
        labels_fixed, both [N,1,oh,ow] (or [N,oh,ow]) float class ids (ops.dice_loss) — where epe_term() acts."""
        return ops.dice_loss(field[1], ops.GRID_UNET, labels_moving, labels_fixed, num_classes, eps, background, 1.0)

    def regularization(self, field, warped_first):
        return self._calculate_regularization_term(field[0], warped_first)

    def forward(self, img_a, img_b, apply_on=None):
        """-> (list of warped tensors in `apply_on` order (default [img_a]), regularisation term)."""
        (f_warp,), f_reg = self.fork_field(self.predict(img_a, img_b), 1)
        warped = self.warp(f_warp, [img_a] if apply_on is None else apply_on)
        return warped, self.regularization(f_reg, warped[0])

    def _calculate_regularization_term(self, deformation, img):
        """sum_i 2^-i * smoothness(resize(d, /2^i), resize(img.detach(), /2^i), alpha) — reference :179-201."""
        dh, dw = deformation.size(2), deformation.size(3)
        img = None if img is None else img.detach()
        reg = None
        factor = 1.0
        for i in range(self.multi_resolution_regularization):
            if i != 0:
                d_r = ops.resize_bilinear(deformation, dh // (2 ** i), dw // (2 ** i))
                img_r = ops.resize_bilinear(img, dh // (2 ** i), dw // (2 ** i))
            elif img is not None and tuple(deformation.shape[2:]) != tuple(img.shape[2:]):
                d_r, img_r = deformation, ops.resize_bilinear(img, dh, dw)
            else:
                d_r, img_r = deformation, img
            term = smoothness_loss(d_r, img_r, alpha=self.alpha, factor=factor)
            reg = term if reg is None else reg + term
            factor /= 2.0
        return reg
