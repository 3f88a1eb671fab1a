"""`--dataset_mode gpupairs`: aligned A/B image pairs held in HBM, augmented on the GPU.

The pool is [M,3,H,W] per modality with values in [0,1] (what ToTensor produces): `--dataroot synthetic` builds it from
the seeded generator used by the tests, any other dataroot is a directory with `A.npy` / `B.npy` ([M,3,H,W] or [M,H,W,3],
uint8 or float).  A batch is ONE launch of nemar_crop_flip_normalize per modality: the crop position and flip of a pair are
drawn once on the host (reference get_params, data/base_dataset.py:63-78) and shipped as a [B,4] int32 tensor; crop,
flip, and Normalize((0.5,)*3, (0.5,)*3) (reference :81-112) happen in the kernel.  Returns the reference's dict:
{'A','B','A_paths','B_paths'} (README.md:18-25, nemar_model.py:151-159).

`--preprocess` as in the reference's get_transform (data/base_dataset.py:81-113):
  resize_and_crop       resize to load_size x load_size, random crop_size x crop_size crop
  crop                  random crop_size x crop_size crop of the image as it is
  scale_width           resize to width load_size (height follows), whole image
  scale_width_and_crop  ... then a random crop_size x crop_size crop
  none                  the whole image, sides rounded to multiples of 4 — the way to feed NON-SQUARE inputs such as the reference's
                        default --img_height 288 --img_width 384
The resize is a function of the image alone (the reference recomputes the same bicubic resize every epoch), so it is applied ONCE,
when the pool is brought into HBM (bicubic, antialiased, clamped to [0, 1] — the reference's PIL resize works on clamped 8-bit
values); per batch only the crop / flip / normalise launch runs.

`--misalign affine|elastic|both` (default none: aligned pairs, as above) turns the aligned pool into KNOWN-MISALIGNMENT training pairs: per
pair a smooth transformation is drawn on the host from a random stream of its own (the crop / flip sequence of a seed does not change),
its field g [B,2,Hc,Wc] — pixels, channel 0 = x, A'(q) = A_crop(q + g(q)) — is built on the device (nemar_deform_field: affine about the
crop centre + cubic B-spline lattice) and modality A is cropped, flipped AND deformed by one launch (nemar_crop_flip_deform_normalize,
border-clamped bilinear); B takes the plain launch.  The batch then carries 'gt_field', which the model's registration-error meter reads
(util/visualizer.RegistrationMeter).  `--synthetic_pairs mapped` makes the synthetic pool registrable: A is a band-limited random texture,
B a fixed per-channel non-linear remap of it (the default `independent` pools share nothing).

`--labels K` (default 0: off, every batch is what it is without the option, key for key) adds label maps for the soft-Dice term
(`--lambda_dice`): a label pool [M,1,H,W] of float class ids 0 .. K-1 per modality — `labels_A.npy` / `labels_B.npy` ([M,H,W] or
[M,1,H,W], the images' size) beside A.npy / B.npy, or for `--dataroot synthetic --synthetic_pairs mapped` the K-level quantisation of the
channel mean of pool A, shared by both modalities (the pairs are aligned).  The label pools follow the images' resize by NEAREST
interpolation, once, at load; a batch carries 'labels_A' and 'labels_B' [B,1,Hc,Wc] from the images' own crop window and flip
(nemar_crop_flip_deform_labels: nearest sampling, ids copied), and under --misalign labels_A is deformed by the batch's gt_field, as image A
is.  No random stream moves."""
import argparse
import ctypes
import math
import os
import random

import numpy as np
import torch

from .. import ops
from .base_dataset import BaseDataset, get_params


class GpuPairsDataset(BaseDataset):
    @staticmethod
    def modify_commandline_options(parser, is_train):
        parser.add_argument('--pool_size_pairs', type=int, default=64, help='synthetic pool: number of A/B pairs')
        parser.add_argument('--data_seed', type=int, default=1234)
        parser.add_argument('--misalign', type=str, default='none', choices=('none', 'affine', 'elastic', 'both'),
                            help='deform modality A by a known, seeded smooth transformation and return its field as gt_field')
        parser.add_argument('--misalign_max_px', type=float, default=8.0, help='largest translation and largest lattice displacement, pixels')
        parser.add_argument('--misalign_rot_deg', type=float, default=5.0, help='rotation drawn in +- this many degrees')
        parser.add_argument('--misalign_scale', type=float, default=0.05, help='scale drawn in 1 +- this')
        parser.add_argument('--misalign_grid', type=int, default=6, help='control points per side of the elastic lattice (>= 4)')
        parser.add_argument('--synthetic_pairs', type=str, default='independent', choices=('independent', 'mapped'),
                            help='synthetic pool: two independent noise pools, or a band-limited texture and a non-linear remap of it')
        # (read with getattr(opt, 'labels', 0): a command line without it parses to the options it always parsed to)
        parser.add_argument('--labels', type=int, default=argparse.SUPPRESS,
                            help='K >= 2: serve label maps labels_A / labels_B with K classes (labels_A.npy / labels_B.npy, or the quantised synthetic mapped pool); 0: none')
        return parser

    def __init__(self, opt):
        BaseDataset.__init__(self, opt)
        self.device = torch.device('cuda', opt.gpu_ids[0]) if opt.gpu_ids else torch.device('cuda')
        # crop positions / flips: one stream per rank (every rank augments its own samples)
        self.rng = random.Random(getattr(opt, 'data_seed', 1234) + 7919 * int(getattr(opt, 'shard_rank', 0)))
        # the misalignment parameters: a stream of their own, so that turning --misalign on leaves the crops and flips of a seed as they are
        self.misalign = getattr(opt, 'misalign', 'none')
        if self.misalign not in ('none', 'affine', 'elastic', 'both'):
            raise ValueError('--misalign %s is not one of none, affine, elastic, both' % self.misalign)
        self.rng_misalign = random.Random((getattr(opt, 'data_seed', 1234) + 7919 * int(getattr(opt, 'shard_rank', 0))) * 1000003 + 604)
        self.lattice = int(getattr(opt, 'misalign_grid', 6)) if self.misalign in ('elastic', 'both') else 0
        if self.misalign in ('elastic', 'both') and self.lattice < 4:
            raise ValueError('--misalign_grid %d: a cubic B-spline lattice needs at least 4 control points per side' % self.lattice)
        self.pre = getattr(opt, 'preprocess', 'resize_and_crop')
        if self.pre not in ('resize_and_crop', 'crop', 'scale_width', 'scale_width_and_crop', 'none'):
            raise ValueError('--preprocess %s is not one of the reference\'s modes' % self.pre)
        if self.root == 'synthetic':
            m = int(getattr(opt, 'pool_size_pairs', 64))
            g = torch.Generator(device=self.device).manual_seed(getattr(opt, 'data_seed', 1234))
            if 'crop' in self.pre:            # images a little larger than the crop, at the load size already
                size = max(opt.crop_size, getattr(opt, 'load_size', opt.crop_size))
                shape = (m, 3, size, size)
            else:                             # whole images of the network's input size
                shape = (m, 3, opt.img_height, opt.img_width)
            if getattr(opt, 'synthetic_pairs', 'independent') == 'mapped':
                self.pool_A = self._texture(shape, g)
                self.pool_B = self._remap(self.pool_A)
            else:
                self.pool_A = torch.rand(*shape, device=self.device, generator=g)
                self.pool_B = torch.rand(*shape, device=self.device, generator=g)
            self.paths_A = ['synthetic/A/%05d' % i for i in range(m)]
            self.paths_B = ['synthetic/B/%05d' % i for i in range(m)]
        else:
            self.pool_A, self.paths_A = self._load(os.path.join(self.root, 'A.npy'))
            self.pool_B, self.paths_B = self._load(os.path.join(self.root, 'B.npy'))
            assert self.pool_A.shape == self.pool_B.shape, "aligned pairs: A.npy and B.npy must have the same shape"
        self.num_labels = int(getattr(opt, 'labels', 0) or 0)
        self.labels_A = self.labels_B = None
        if self.num_labels:
            self.labels_A, self.labels_B = self._label_pools()
        self.pool_A, self.pool_B = self._resize(self.pool_A), self._resize(self.pool_B)
        self.M, _, self.H, self.W = self.pool_A.shape
        if self.num_labels:
            self.labels_A, self.labels_B = self._resize(self.labels_A, nearest=True), self._resize(self.labels_B, nearest=True)
            assert self.labels_A.shape == (self.M, 1, self.H, self.W) and self.labels_B.shape == (self.M, 1, self.H, self.W)
        # what a batch looks like: a square crop, or the whole image
        self.out_hw = (opt.crop_size, opt.crop_size) if 'crop' in self.pre else (self.H, self.W)
        assert self.H >= self.out_hw[0] and self.W >= self.out_hw[1], "images smaller than the crop"

    def _texture(self, shape, g):
        """band-limited random texture in [0, 1]: two octaves of seeded coarse noise (1/16 and 1/4 of the side), each upsampled once with the
        bicubic filter _resize uses, stretched to the full range per image — structure at the scales a registration network can lock on to"""
        m, c, h, w = shape
        out = None
        for div, weight in ((16, 0.65), (4, 0.35)):
            coarse = torch.rand(m, c, max(2, h // div), max(2, w // div), device=self.device, generator=g)
            up = torch.nn.functional.interpolate(coarse, size=(h, w), mode='bicubic', align_corners=False) * weight
            out = up if out is None else out + up
        lo, hi = out.amin(dim=(1, 2, 3), keepdim=True), out.amax(dim=(1, 2, 3), keepdim=True)
        return ((out - lo) / (hi - lo).clamp_min(1e-6)).clamp_(0.0, 1.0).contiguous()

    @staticmethod
    def _remap(a):
        """the second modality of a `mapped` synthetic pair: a fixed, per-channel, non-linear (one of them decreasing) map of the first"""
        maps = (lambda v: 1.0 - v * v, lambda v: 0.5 - 0.5 * torch.cos(math.pi * v), lambda v: v.sqrt())
        return torch.stack([maps[ch % 3](a[:, ch]) for ch in range(a.shape[1])], dim=1).clamp_(0.0, 1.0).contiguous()

    def _label_pools(self):
        """the two label pools [M,1,H,W] float32 at the size of the image pools as loaded (before _resize)"""
        K = self.num_labels
        if K < 2:
            raise ValueError('--labels %d: at least 2 classes (0 turns label maps off)' % K)
        if self.root == 'synthetic':
            if getattr(self.opt, 'synthetic_pairs', 'independent') != 'mapped':
                raise ValueError('--labels with --dataroot synthetic needs --synthetic_pairs mapped: independent noise pools have no structure to label')
            lab = (self.pool_A.mean(dim=1, keepdim=True) * K).floor().clamp_(0, K - 1).contiguous()
            return lab, lab
        pools = []
        for name in ('labels_A.npy', 'labels_B.npy'):
            path = os.path.join(self.root, name)
            if not os.path.exists(path):
                raise FileNotFoundError('--labels %d: %s not found (label maps [M,H,W] or [M,1,H,W] of the size of the images in A.npy / B.npy)' % (K, path))
            a = np.load(path)
            if a.ndim == 3:
                a = a[:, None]
            if a.ndim != 4 or a.shape[1] != 1 or (a.shape[0],) + a.shape[2:] != (self.pool_A.shape[0],) + tuple(self.pool_A.shape[2:]):
                raise ValueError('%s: shape %s, expected [M,H,W] or [M,1,H,W] with M, H, W = %s' % (path, a.shape, (self.pool_A.shape[0],) + tuple(self.pool_A.shape[2:])))
            pools.append(torch.from_numpy(np.ascontiguousarray(a)).to(self.device, torch.float32).contiguous())
        return pools

    def _draw_misalign(self, n):
        """[n, 6 + 2 L L] float32 parameter rows of nemar_deform_field: a11 a12 tx a21 a22 ty (scale * rotation about the crop centre +
        translation; the identity without `affine`), then the [2, L, L] lattice (L = 0 without `elastic`)"""
        opt, rng, L = self.opt, self.rng_misalign, self.lattice
        max_px = float(getattr(opt, 'misalign_max_px', 8.0))
        rows = np.zeros((n, 6 + 2 * L * L), dtype=np.float32)
        for b in range(n):
            a11, a12, tx, a21, a22, ty = 1.0, 0.0, 0.0, 0.0, 1.0, 0.0
            if self.misalign in ('affine', 'both'):
                th = math.radians(rng.uniform(-1.0, 1.0) * float(getattr(opt, 'misalign_rot_deg', 5.0)))
                sc = 1.0 + rng.uniform(-1.0, 1.0) * float(getattr(opt, 'misalign_scale', 0.05))
                a11, a12, a21, a22 = sc * math.cos(th), -sc * math.sin(th), sc * math.sin(th), sc * math.cos(th)
                tx, ty = rng.uniform(-max_px, max_px), rng.uniform(-max_px, max_px)
            rows[b, :6] = (a11, a12, tx, a21, a22, ty)
            for k in range(2 * L * L):
                rows[b, 6 + k] = rng.uniform(-max_px, max_px)
        return rows

    def _resize(self, pool, nearest=False):
        """the image-only part of get_transform: resize / scale_width / make_power_2 (reference data/base_dataset.py:86-99), once
        (nearest: a label pool — ids are picked, not blended)"""
        opt, (h, w) = self.opt, pool.shape[2:]
        if 'resize' in self.pre:
            nh, nw = opt.load_size, opt.load_size
        elif 'scale_width' in self.pre:
            nw, nh = opt.load_size, int(opt.load_size * h / w)
        elif self.pre == 'none':
            nh, nw = int(round(h / 4) * 4), int(round(w / 4) * 4)
        else:
            nh, nw = h, w
        if nearest:
            return pool if (nh, nw) == (h, w) else torch.nn.functional.interpolate(pool, size=(nh, nw), mode='nearest').contiguous()
        return self.resize_to(pool, nh, nw)

    @staticmethod
    def resize_to(pool, nh, nw):
        """pool [M,C,H,W] in [0, 1] at nh x nw: bicubic, antialiased, clamped (untouched when it has that size already)"""
        if (nh, nw) == tuple(pool.shape[2:]):
            return pool
        out = torch.nn.functional.interpolate(pool, size=(nh, nw), mode='bicubic', align_corners=False, antialias=True)
        return out.clamp_(0.0, 1.0).contiguous()

    @staticmethod
    def whole_images(pool, indices):
        """the images `indices` of pool [M,C,H,W] in [0, 1], whole and unflipped, as the network takes them: Normalize(0.5, 0.5) by the
        launch batch() uses, with the identity crop -> [len(indices),C,H,W] in [-1, 1]"""
        M, C, H, W = pool.shape
        params = torch.tensor([(i, 0, 0, 0) for i in indices], dtype=torch.int32).to(pool.device)
        y = torch.empty((len(indices), C, H, W), dtype=torch.float32, device=pool.device)
        ops.L.crop_flip_normalize(ctypes.c_void_p(pool.data_ptr()), ctypes.c_void_p(params.data_ptr()), ctypes.c_void_p(y.data_ptr()),
                                  M, len(indices), C, H, W, H, W, 1.0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        return y

    def _load(self, path):
        return self.load_pool(path, self.device)

    @staticmethod
    def load_pool(path, device):
        a = np.load(path)
        if a.ndim == 4 and a.shape[-1] == 3:
            a = a.transpose(0, 3, 1, 2)
        scale = 1.0 / 255.0 if a.dtype == np.uint8 else 1.0
        t = torch.from_numpy(np.ascontiguousarray(a)).to(device, torch.float32) * scale
        return t.contiguous(), ['%s[%d]' % (path, i) for i in range(t.shape[0])]

    def __len__(self):
        return self.M

    def batch(self, indices):
        opt = self.opt
        hc, wc = self.out_hw
        params = np.zeros((len(indices), 4), dtype=np.int32)
        for b, i in enumerate(indices):
            p = get_params(opt, (self.W, self.H), self.rng)
            x0, y0 = p['crop_pos'] if 'crop' in self.pre else (0, 0)
            params[b] = (i % self.M, y0, x0, int(p['flip']))
        d_params = torch.from_numpy(params).to(self.device, non_blocking=True)
        out = {}
        gt = None
        if self.misalign != 'none':
            self._last_misalign = self._draw_misalign(len(indices))
            d_mis = torch.from_numpy(self._last_misalign).to(self.device, non_blocking=True)
            gt = ops.deform_field(d_mis, len(indices), hc, wc, self.lattice, self.lattice)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for key, pool in (('A', self.pool_A), ('B', self.pool_B)):
            if key == 'A' and gt is not None:
                out[key] = ops.crop_flip_deform_normalize(pool, d_params, gt, hc, wc, 1.0)
                continue
            y = torch.empty((len(indices), 3, hc, wc), dtype=torch.float32, device=self.device)
            ops.L.crop_flip_normalize(ctypes.c_void_p(pool.data_ptr()), ctypes.c_void_p(d_params.data_ptr()),
                                      ctypes.c_void_p(y.data_ptr()), self.M, len(indices), 3, self.H, self.W, hc, wc, 1.0, st)
            out[key] = y
        out['A_paths'] = [self.paths_A[i % self.M] for i in indices]
        out['B_paths'] = [self.paths_B[i % self.M] for i in indices]
        if gt is not None:
            out['gt_field'] = gt
        if self.num_labels:
            out['labels_A'] = ops.crop_flip_deform_labels(self.labels_A, d_params, gt, hc, wc)
            out['labels_B'] = ops.crop_flip_deform_labels(self.labels_B, d_params, None, hc, wc)
        self._last_params = params
        return out

    def __getitem__(self, index):
        b = self.batch([index])
        return {k: v[0] for k, v in b.items()}
