"""Affine registration network — mirror of reference models/stn/affine_stn.py (AffineNetwork :22-83, AffineSTN
:86-138).  theta = dtheta + I and F.affine_grid are fused into the warp kernel (GRID_AFFINE); the two nn.Linear
layers run as 1x1 convolutions on a 1x1 image through the same MFMA implicit-GEMM kernels."""
import torch.nn as nn

from ... import ops
from ..networks import LinearParams, Slots
from .layers import DownBlock, prediction_tensor

cfg_conv1_nf = {'A': 32, }
cfg_mlp_nf = {'A': 256}
cfg_use_norm = {'A': True, }
cfg_nconvs = {'A': 5, }
cfg_use_resnet = {'A': False, }
cfg_activation = {'A': 'relu'}


class AffineNetwork(nn.Module):
    """5 x [conv3x3 - InstanceNorm - ReLU - maxpool] then Linear(256) - ReLU - Linear(6) (reference :22-83)."""

    def __init__(self, in_channels_a, in_channels_b, height, width, cfg='A', init_func='kaiming'):
        super().__init__()
        self.h, self.w = height, width
        self.nconvs = cfg_nconvs[cfg]
        self.convs = Slots()
        prev_nf = in_channels_a + in_channels_b
        nf = cfg_conv1_nf[cfg]
        for i in range(self.nconvs):
            self.convs.put(i, DownBlock(prev_nf, nf, 3, 1, 1, bias=True, activation=cfg_activation[cfg],
                                        init_func=init_func, use_norm=cfg_use_norm[cfg],
                                        use_resnet=cfg_use_resnet[cfg], skip=False, refine=False, pool=True))
            prev_nf = nf
            nf = min(2 * nf, cfg_mlp_nf[cfg])
        self.local = Slots()
        self.local.put(0, LinearParams(prev_nf * (self.h // 2 ** self.nconvs) * (self.w // 2 ** self.nconvs), nf))
        self.local.put(2, LinearParams(nf, 6))
        # start at the identity transformation (reference :75-76)
        self.local.at(2).weight.data.normal_(mean=0.0, std=5e-4)
        self.local.at(2).bias.data.zero_()

    def forward(self, img_a, img_b):
        x, x2 = img_a, img_b
        for i in range(self.nconvs):
            x = self.convs.at(i)(x, x2)
            x2 = None
        n = x.size(0)
        x = x.reshape(n, -1, 1, 1)
        l0, l2 = self.local.at(0), self.local.at(2)
        x = ops.conv2d(x, l0.weight, l0.bias, act=ops.ACT_RELU, wshape=(l0.weight.size(0), l0.weight.size(1), 1, 1))
        x = ops.conv2d(x, l2.weight, l2.bias, wshape=(6, l2.weight.size(1), 1, 1))
        return x.reshape(n, 6)


class AffineSTN(nn.Module):
    """Predicts and applies the affine transformation (reference :86-138)."""

    def __init__(self, nc_a, nc_b, height, width, cfg, init_func):
        super().__init__()
        self.net = AffineNetwork(nc_a, nc_b, height, width, cfg, init_func)

    def _get_theta(self, img_a, img_b):
        import torch
        dtheta = self.net(img_a, img_b)
        ident = torch.tensor([1, 0, 0, 0, 1, 0], dtype=torch.float32, device=dtheta.device)
        return dtheta + ident[None]

    def get_grid(self, img_a, img_b):
        """F.affine_grid of the predicted theta (reference :102-106); inspection API, built with torch ops."""
        import torch.nn.functional as F
        theta = self._get_theta(img_a, img_b)
        return F.affine_grid(theta.view(-1, 2, 3), img_a.size(), align_corners=False)

    # predict -> warp* -> regularization: same split as UnetSTN (see there)
    def predict(self, img_a, img_b):
        dtheta = self.net(img_a, img_b)
        self.last_dtheta = dtheta.detach()         # for the registration-error meter (util/visualizer.RegistrationMeter); no copy
        return dtheta

    def last_prediction(self):
        """(what the last forward pass handed to the warp kernel, its grid mode) — None before the first pass"""
        d = getattr(self, 'last_dtheta', None)
        return None if d is None else (d, ops.GRID_AFFINE)

    def warp(self, field, imgs):
        return ops.warp_affine(field, list(imgs))

    def apply(self, field, imgs, out_hw=None, sample='bilinear', grad=False):
        """The prediction applied at ANY resolution, for inference: `field` is what predict() returned or last_prediction(); each image
        is sampled at out_hw (default: its own size) on affine_grid(theta) of that size (ops.warp_resampled).  sample='nearest' for
        label maps.  No autograd — unless grad=True: the same values with a gradient towards the prediction (refinement on the pair)."""
        return ops.warp_resampled(prediction_tensor(field), ops.GRID_AFFINE, list(imgs), out_hw, sample, grad)

    def overlap(self, field, labels_moving, labels_fixed, num_classes):
        """Per-class overlap counts [N,K,3] (inter, moving, fixed) of labels_moving warped by the prediction — what
        apply(..., sample='nearest') gives, never written — against labels_fixed at its size (ops.label_overlap).  No autograd."""
        return ops.label_overlap(prediction_tensor(field), ops.GRID_AFFINE, labels_moving, labels_fixed, num_classes)

    def surface(self, field, labels_moving, labels_fixed, num_classes, max_dist=64, dist_map=False):
        """Boundary distances of labels_moving warped by the prediction — what apply(..., sample='nearest') gives, never written —
        against labels_fixed at its size: (counts [N,K,2,3] = boundary pixels, far, largest squared distance per class and direction;
        hist [N,K,2,max_dist^2] of the squared distances; the distance map [N,2,Ho,Wo] or None) — ops.surface_distance;
        ops.surface_summary turns counts and hist into the Hausdorff distance, HD95 and ASSD.  No autograd."""
        return ops.surface_distance(prediction_tensor(field), ops.GRID_AFFINE, labels_moving, labels_fixed, num_classes, max_dist, dist_map)

    def map_points(self, field, pts, src_hw, out_hw):
        """Where the prediction samples the src_hw source for points [N,P,2] (x, y) given in pixels of the out_hw fixed image
        (ops.map_points).  No autograd."""
        return ops.map_points(prediction_tensor(field), ops.GRID_AFFINE, pts, src_hw, out_hw)

    def regularity(self, field, out_hw=None, det_map=False):
        """How regular the prediction's transformation is at out_hw (default: the network's size): (counts [N,2] = interior pixels and
        folds, stats [N,5] = min / max / sum of the Jacobian determinant and the two log sums, the determinant map [N,Ho,Wo] or None) —
        ops.jacobian_stats; an affine map has one determinant, theta's, at every pixel.  No autograd."""
        return ops.jacobian_stats(prediction_tensor(field), ops.GRID_AFFINE, (self.net.h, self.net.w) if out_hw is None else out_hw, det_map)

    def similarity(self, field, moving, fixed, bins=32, range_moving=(-1., 1.), range_fixed=(-1., 1.), moments=True):
        """Intensity agreement of `moving` warped by the prediction — what apply() gives, never written — with `fixed` at its size:
        (counts [N,bins,bins], the joint histogram of the two channel means; moments [N,6] or None) — ops.joint_histogram;
        ops.similarity_summary turns them into mutual information, NCC, MSE and MAE.  Needs no annotation.  No autograd."""
        return ops.joint_histogram(prediction_tensor(field), ops.GRID_AFFINE, moving, fixed, bins, range_moving, range_fixed, moments)

    def compose(self, first, second):
        """ONE dtheta [N,6] that samples where `first` and then `second` would in sequence — an affine cascade stays affine, in closed
        form and exactly: under align_corners=False the base coordinate of the position S2(x) samples is theta2 applied to the base
        coordinate of x, so theta12 = theta1 o theta2 as 3 x 3 matrices (formed in float64, rounded once).  No kernel, no autograd."""
        import torch
        d1, d2 = prediction_tensor(first).detach(), prediction_tensor(second).detach()
        eye = torch.eye(3, dtype=torch.float64, device=d1.device)

        def matrix(d):          # dtheta [N,6] -> [N,3,3]: theta = dtheta + I over the row (0, 0, 1)
            return torch.cat([d.to(torch.float64).view(-1, 2, 3), torch.zeros_like(eye[None, 2:]).expand(d.size(0), 1, 3)], 1) + eye
        return ((matrix(d1) @ matrix(d2)) - eye)[:, :2].reshape(-1, 6).to(torch.float32)

    def set_last_prediction(self, dtheta):
        """what last_prediction() returns from now on: a composite made outside the forward pass (NEMARModel.cascade)"""
        self.last_dtheta = dtheta.detach()

    def fork_field(self, field, n_warps, extra=0):
        """-> ([one theta handle per warp() call], the handle for regularization()) — ops.fork, as UnetSTN.fork_field; with
        extra = k > 0 a last element: a list of k more handles, one per further consumer (epe_term(), dice_term())"""
        hs = ops.fork(field, n_warps + 1 + int(extra))
        out = list(hs[:n_warps]), hs[n_warps]
        return (*out, list(hs[n_warps + 1:])) if extra else out

    def epe_term(self, field, gt_field, eps=0.01):
        """mean over all pixels of sqrt(|r|^2 + eps^2), r the residual registration_error measures against the ground-truth field
        gt_field [N,2,h,w] in pixels, for the sampling positions of affine_grid(theta) at the field's size (ops.epe_loss)"""
        return ops.epe_loss(field, ops.GRID_AFFINE, gt_field, eps, 1.0)

    def dice_term(self, field, labels_moving, labels_fixed, num_classes, eps=1.0, background=False):
        """mean over samples and classes of 1 - soft Dice of labels_moving warped bilinearly by affine_grid(theta) at the label maps'
        size against labels_fixed, both [N,1,h,w] (or [N,h,w]) float class ids (ops.dice_loss)"""
        return ops.dice_loss(field, ops.GRID_AFFINE, labels_moving, labels_fixed, num_classes, eps, background, 1.0)

    def regularization(self, field, warped_first=None):
        return self._calculate_regularization_term(field)

    def forward(self, img_a, img_b, apply_on=None):
        (f_warp,), f_reg = self.fork_field(self.predict(img_a, img_b), 1)
        warped = self.warp(f_warp, [img_a] if apply_on is None else apply_on)
        return warped, self.regularization(f_reg, warped[0])

    def _calculate_regularization_term(self, theta):
        """mean|dtheta| (reference :136-138)."""
        return ops.l1_loss(theta, None, 1.0)
