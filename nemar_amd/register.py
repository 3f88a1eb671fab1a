"""Register image pairs at their native size with a trained model — inference only, no image decoding library:

    python -m nemar_amd.register --dataroot DIR --name EXPERIMENT --checkpoints_dir ./checkpoints --epoch latest \\
        --stn_type unet --img_height 256 --img_width 256 --batch_size 4 --results_dir ./results

DIR holds `A.npy` / `B.npy` in the format `--dataset_mode gpupairs` trains from ([M,3,H,W] or [M,H,W,3], uint8 or float in [0, 1]) and,
optionally, `labels_A.npy` ([M,H,W] or [M,C,H,W], any numeric dtype: a label map of modality A at any size).  Something to score the
result against is optional too: `labels_B.npy` ([M,H,W] or [M,1,H,W], the size of B.npy: the same classes in modality B) and
`landmarks_A.npy` / `landmarks_B.npy` ([M,P,2] (x, y) in pixels of A.npy and B.npy: annotated point pairs, a NaN row = missing).  Every pair is brought to the
network's --img_height x --img_width by the dataset's own resize and normalise path, netR predicts the transformation ONCE at that size
(weights of --epoch under --checkpoints_dir/--name, the flags the model was trained with), and NEMARModel.register() applies it to the
full-size images: the sampling grid is in normalised coordinates, so the prediction holds at every size (csrc/register.hip).
With --passes K (default 1) netR looks K times, each time at the pair its earlier predictions registered, and the K predictions are
composed into ONE transformation (NEMARModel.cascade, csrc/compose.hip): every image and label map is still interpolated once.

Written under --results_dir/--name/:
    registered_A.npy          modality A registered to B, in A.npy's own size, layout and dtype (uint8: rounded and clamped on the host)
    registered_labels_A.npy   labels_A.npy warped with nearest sampling (class ids are copied, never blended), in its own dtype
    offsets.npy               the network-resolution predictions: offsets [M,2,h,w] (unet) or dtheta [M,6] (affine); with --passes K > 1 the
                              composite of the K predictions, in the same form
    scores.json               only with labels_A.npy + labels_B.npy and / or the two landmark files (score_summary below): per-class and mean
                              Dice before and after registration, from the counts of the whole data set; mean, median and max
                              distance in pixels between the mapped landmarks of B and those of A, before and after, and how many
                              point pairs were used
    regularity.json           only with --regularity: how regular the transformation is at the images' native size (B.npy's), from the
                              counts and sums of the whole data set (ops.regularity_summary): interior pixels, folds (Jacobian
                              determinant <= 0) and their share, min / max / mean determinant, mean and standard deviation of the
                              log-determinant over the pixels that do not fold (SDlogJ); with --passes K > 1 also `per_pass`, K such
                              summaries of the accumulated transformation after each pass, at the network's size
    jacobian_det.npy          only with --jacobian_map (which implies --regularity): the determinant map [M,H,W] float32 at B.npy's
                              size, NaN in the last row and column (csrc/regularity.hip)
    similarity.json           only with --similarity: how well the intensities of A.npy agree with B.npy's at B.npy's size, `before`
                              (A merely resampled) and `after` registration, from the tables and sums of the whole data set
                              (ops.similarity_summary): counted pixels, the entropies, mutual information (nats) and its normalised
                              form from a --bins x --bins joint histogram of the channel means over [0, 1]; NCC, MSE and MAE; with
                              --passes K > 1 also `per_pass`, K such summaries of the network-size pair after each pass.  Needs no
                              annotation: A.npy and B.npy are enough (csrc/similarity.hip)
    surface.json              only with --surface (needs labels_A.npy and labels_B.npy): how far the class boundaries of the two label
                              maps are apart at labels_B.npy's size, `before` (labels_A merely resampled) and `after` registration
                              (ops.surface_summary): per class and as class means, with and without class 0, the Hausdorff distance,
                              its 95th percentile (HD95) and the average symmetric surface distance in pixels, averaged over the
                              pairs where both maps hold the class, and how many (pair, class) cases were used, skipped, or reach
                              beyond --surface_max_dist D (default 64 px: squared distances below D^2 are histogrammed, exactly);
                              with --passes K > 1 the composite is scored (csrc/surface.hip)
    surface_dist2.npy         only with --surface_map (which implies --surface): int32 [M,2,H,W], the squared distance at every
                              boundary pixel of the registered label map (plane 0) and of labels_B.npy (plane 1); -1 off the
                              boundaries, -2 where the other map has no boundary of the class
    registered_B.npy          only with --inverse (needs --stn_integrate K > 0, the flag the model was trained with, and --passes 1):
                              modality B warped onto A by the inverse prediction, in B.npy's own size, layout and dtype
    inverse_offsets.npy       only with --inverse: that prediction [M,2,h,w], exp(-v) of the velocity field the network predicted
                              (csrc/integrate.hip).  It inverts the integrated map in its true-identity convention; the slight zoom
                              of the warp's grid is not undone
    refine.json               only with --refine N: every batch's prediction is refined on its own pairs at their native size before it
                              is applied and scored — N Adam steps on the offsets (the velocity with --stn_integrate; dtheta) against
                              --refine_term mind | lncc | l1 (default mind: across modalities, no generator pass) and the regularisers
                              (--refine_lr, --refine_lambda_smooth, --refine_lambda_fold; NEMARModel.refine, csrc/register.hip's
                              backward): the steps, the term and the objective before and after, the mean over the data set.  Every
                              other file then holds the refined result ("before" in the score files stays the identity) — except
                              the `per_pass` lists of regularity.json and similarity.json under --passes K > 1: they are taken
                              while the network looks, BEFORE the refinement, so their last entry is the composite the refinement
                              started from and differs from "after" and the file's own totals, which are the refined one's
    offsets_before_refine.npy only with --refine N: what offsets.npy would have held without it
and one summary line on stdout: pairs, sizes, the scores (with --regularity: folds in per cent and SDlogJ; with --similarity:
MI before -> after; with --surface: HD95 before -> after; with --refine: the objective before -> after), seconds."""
import json
import os
import time

import numpy as np
import torch

from .data.gpupairs_dataset import GpuPairsDataset
from .models import create_model
from . import ops
from .options import TestOptions

def network_batch(pool_A, pool_B, indices, opt):
    """{'A','B','A_paths','B_paths'} for set_input: the pairs `indices` of the full-size pools at the network's size, in [-1, 1]"""
    hw = (opt.img_height, opt.img_width)
    sel = torch.as_tensor(list(indices), device=pool_A.device)
    a = GpuPairsDataset.resize_to(pool_A.index_select(0, sel), *hw)
    b = GpuPairsDataset.resize_to(pool_B.index_select(0, sel), *hw)
    local = list(range(len(indices)))
    paths = ['pair[%d]' % i for i in indices]
    return {'A': GpuPairsDataset.whole_images(a, local), 'B': GpuPairsDataset.whole_images(b, local), 'A_paths': paths, 'B_paths': paths}


def _like_input(t, ref, image):
    """device tensor [M,C,H,W] -> numpy in the layout and dtype of the array `ref` it was loaded from (images: channels-last when the
    loader took them as such)"""
    a = t.cpu().numpy()
    if ref.ndim == 3:
        a = a[:, 0]
    elif image and ref.shape[-1] == 3:
        a = a.transpose(0, 2, 3, 1)
    if ref.dtype == np.uint8:
        return np.clip(np.rint(a * 255.0), 0, 255).astype(np.uint8)
    if np.issubdtype(ref.dtype, np.integer):
        return np.rint(a).astype(ref.dtype)
    return a.astype(ref.dtype)


def score_summary(overlap_before=None, overlap=None, tre_before=None, tre=None):
    """What scores.json holds, from NEMARModel.register()'s score tensors of the whole data set (numpy; the batches concatenated along
    the first axis): overlap* int [M,K,3] counts (inter, moving, fixed), tre* float [M,P] in pixels with NaN for a missing pair.
    Dice per class is 2 * sum(inter) / (sum(moving) + sum(fixed)) with the sums over the data set — counts added, then divided —, over the
    classes present in either map, before or after; TRE statistics are over the pairs that are present."""
    scores = {}
    if overlap is not None:
        b, a = np.asarray(overlap_before, dtype=np.int64).sum(0), np.asarray(overlap, dtype=np.int64).sum(0)
        present = np.flatnonzero((b[:, 1] + b[:, 2] + a[:, 1] + a[:, 2]) > 0)
        dice = lambda c: [2.0 * int(c[k, 0]) / max(int(c[k, 1] + c[k, 2]), 1) for k in present]
        d_b, d_a = dice(b), dice(a)
        scores['dice'] = {'classes': [int(k) for k in present], 'before': d_b, 'after': d_a,
                          'mean_before': float(np.mean(d_b)) if d_b else None, 'mean_after': float(np.mean(d_a)) if d_a else None}
    if tre is not None:
        t_b, t_a = np.asarray(tre_before, dtype=np.float64).ravel(), np.asarray(tre, dtype=np.float64).ravel()
        used = np.isfinite(t_b) & np.isfinite(t_a)
        stats = lambda t: {'mean': float(t.mean()), 'median': float(np.median(t)), 'max': float(t.max())} if t.size else None
        scores['tre_px'] = {'points': int(used.sum()), 'before': stats(t_b[used]), 'after': stats(t_a[used])}
    return scores


def _optional(dataroot, name, M, what, ok):
    """DIR/name if it exists, checked: `ok(array)` or exit with `what`"""
    path = os.path.join(dataroot, name)
    if not os.path.exists(path):
        return None
    a = np.load(path)
    if a.shape[0] != M or not ok(a):
        raise SystemExit('%s %s: %s with M = %d expected' % (name, a.shape, what, M))
    return a


def main(argv=None):
    opt = TestOptions().parse(argv, quiet=True)
    if not opt.gpu_ids:
        raise SystemExit('nemar_amd.register runs on an MI355X only (pass --gpu_ids 0)')
    device = torch.device('cuda', opt.gpu_ids[0])
    torch.cuda.set_device(device)
    t0 = time.time()
    raw_A = np.load(os.path.join(opt.dataroot, 'A.npy'), mmap_mode='r')
    pool_A, _ = GpuPairsDataset.load_pool(os.path.join(opt.dataroot, 'A.npy'), device)
    pool_B, _ = GpuPairsDataset.load_pool(os.path.join(opt.dataroot, 'B.npy'), device)
    if pool_A.shape[0] != pool_B.shape[0]:
        raise SystemExit('A.npy holds %d images, B.npy %d: pairs expected' % (pool_A.shape[0], pool_B.shape[0]))
    labels_path = os.path.join(opt.dataroot, 'labels_A.npy')
    raw_labels = labels = None
    if os.path.exists(labels_path):
        raw_labels = np.load(labels_path)
        lab = raw_labels[:, None] if raw_labels.ndim == 3 else raw_labels
        if lab.ndim != 4 or lab.shape[0] != pool_A.shape[0]:
            raise SystemExit('labels_A.npy %s: [M,H,W] or [M,C,H,W] with M = %d expected' % (raw_labels.shape, pool_A.shape[0]))
        labels = torch.from_numpy(np.ascontiguousarray(lab).astype(np.float32)).to(device)
    M = pool_A.shape[0]
    # what to score against (scores.json): modality B's label map, annotated point pairs
    raw_labels_B = _optional(opt.dataroot, 'labels_B.npy', M, '[M,H,W] or [M,1,H,W] of B.npy\'s size',
                             lambda a: (a.ndim == 3 or (a.ndim == 4 and a.shape[1] == 1)) and tuple(a.shape[-2:]) == tuple(pool_B.shape[2:]))
    raw_lm = [_optional(opt.dataroot, n, M, '[M,P,2]', lambda a: a.ndim == 3 and a.shape[2] == 2) for n in ('landmarks_A.npy', 'landmarks_B.npy')]
    labels_B = lm_A = lm_B = num_classes = None
    if raw_labels_B is not None and labels is not None:
        if labels.shape[1] != 1:
            raise SystemExit('labels_A.npy %s: a single-channel map is needed to score it against labels_B.npy' % (raw_labels.shape,))
        labels_B = torch.from_numpy(np.ascontiguousarray(raw_labels_B.reshape(M, 1, *raw_labels_B.shape[-2:])).astype(np.float32)).to(device)
        num_classes = int(max(np.nanmax(raw_labels), np.nanmax(raw_labels_B))) + 1      # one K for every batch: the counts are added
    if raw_lm[0] is not None and raw_lm[1] is not None:
        if raw_lm[0].shape != raw_lm[1].shape:
            raise SystemExit('landmarks_A.npy %s and landmarks_B.npy %s: point pairs expected' % (raw_lm[0].shape, raw_lm[1].shape))
        lm_A, lm_B = (torch.from_numpy(np.ascontiguousarray(a).astype(np.float32)).to(device) for a in raw_lm)
    want_surface = bool(opt.surface or opt.surface_map)
    if want_surface and labels_B is None:
        raise SystemExit('--surface needs labels_A.npy and labels_B.npy under %s: the boundaries of the two label maps are what it measures' % opt.dataroot)
    if want_surface and not 1 <= opt.surface_max_dist <= ops.MAX_SURFACE_DIST:
        raise SystemExit('--surface_max_dist %d: 1 .. %d' % (opt.surface_max_dist, ops.MAX_SURFACE_DIST))
    surf = {'before': [], 'after': [], 'dist2': []}
    scored = {k: [] for k in ('overlap_before', 'overlap', 'tre_before_px', 'tre_px')}
    model = create_model(opt)
    model.setup(opt)
    if opt.eval:
        model.eval()
    want_reg = bool(opt.regularity or opt.jacobian_map)
    jac = {k: [] for k in ('jac_counts', 'jac_stats', 'jacobian_det')}
    per_pass = [[] for _ in range(opt.passes)] if want_reg and opt.passes > 1 else []
    sim = {'before': [], 'after': []}
    sim_per_pass = [[] for _ in range(opt.passes)] if opt.similarity and opt.passes > 1 else []
    want_inverse = bool(getattr(opt, 'inverse', False))
    if want_inverse and (int(getattr(opt, 'stn_integrate', 0)) <= 0 or opt.stn_type != 'unet'):
        raise SystemExit('--inverse needs --stn_type unet --stn_integrate K > 0: the inverse is exp(-v) of the velocity field such a model predicts')
    if want_inverse and opt.passes > 1:
        raise SystemExit('--inverse with --passes %d: a composite of several predictions is the exponential of no single velocity' % opt.passes)
    raw_B = np.load(os.path.join(opt.dataroot, 'B.npy'), mmap_mode='r') if want_inverse else None
    reg_B, inv_offsets = [], []
    reg, reg_labels, offsets = [], [], []
    refine_steps, refine_term = int(getattr(opt, 'refine', 0)), getattr(opt, 'refine_term', 'mind')
    if refine_steps < 0:
        raise SystemExit('--refine %d: a number of steps' % refine_steps)
    offsets_before, objectives = [], []
    for i0 in range(0, M, opt.batch_size):
        idx = list(range(i0, min(M, i0 + opt.batch_size)))
        model.set_input(network_batch(pool_A, pool_B, idx, opt))
        told_passes = model.cascade(opt.passes, regularity=want_reg, similarity=opt.similarity, bins=opt.bins)
        if want_reg and opt.similarity:
            reg_passes, sim_passes = told_passes['regularity'], told_passes['similarity']
        else:
            reg_passes, sim_passes = (told_passes, []) if want_reg else ([], told_passes or [])
        for k, pair in zip(per_pass, reg_passes):
            k.append(pair)
        for k, pair in zip(sim_per_pass, sim_passes):
            k.append(pair)
        part = lambda t: None if t is None else t[idx[0]:idx[-1] + 1]
        if refine_steps:
            offsets_before.append(model.netR.last_prediction()[0].clone())
            as_net = (lambda t: t * 2.0 - 1.0) if refine_term == 'l1' else (lambda t: t)      # (netT reads [-1, 1])
            refined = model.refine(as_net(part(pool_A)), as_net(part(pool_B)), refine_steps, lr=getattr(opt, 'refine_lr', None), term=refine_term,
                                   lambda_smooth=getattr(opt, 'refine_lambda_smooth', None), lambda_fold=getattr(opt, 'refine_lambda_fold', 0.0))
            objectives.append(refined['objective'][[0, -1]] * len(idx))
        out = model.register(part(pool_A), part(pool_B), part(labels), translate=False,          # (fake_RT_B is not among the files this command writes)
                             labels_B=part(labels_B), landmarks_A=part(lm_A), landmarks_B=part(lm_B), num_classes=num_classes,
                             **(dict(regularity=True, jacobian_map=opt.jacobian_map) if want_reg else {}),
                             **(dict(similarity=True, bins=opt.bins, intensity_range=(0.0, 1.0)) if opt.similarity else {}),
                             **(dict(inverse=True) if want_inverse else {}),
                             **(dict(surface=True, surface_max_dist=opt.surface_max_dist, surface_map=opt.surface_map) if want_surface else {}))
        if want_surface:
            surf['before'].append(out['surface']['before'])
            surf['after'].append(out['surface']['after'])
            if opt.surface_map:
                surf['dist2'].append(out['surface_dist2'])
        if want_inverse:
            reg_B.append(out['registered_B'])
            inv_offsets.append(out['inverse_offsets'].clone())
        for k in sim:
            if 'similarity' in out:
                sim[k].append(out['similarity'][k])
        for k in jac:
            if k in out:
                jac[k].append(out[k])
        for k in scored:
            if k in out:
                scored[k].append(out[k])
        reg.append(out['registered_A'])
        offsets.append(out['offsets'].clone())
        if labels is not None:
            reg_labels.append(out['registered_labels_A'])
    out_dir = os.path.join(opt.results_dir, opt.name)
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, 'registered_A.npy'), _like_input(torch.cat(reg), raw_A, True))
    np.save(os.path.join(out_dir, 'offsets.npy'), torch.cat(offsets).cpu().numpy())
    if labels is not None:
        np.save(os.path.join(out_dir, 'registered_labels_A.npy'), _like_input(torch.cat(reg_labels), raw_labels, False))
    if want_inverse:
        np.save(os.path.join(out_dir, 'registered_B.npy'), _like_input(torch.cat(reg_B), raw_B, True))
        np.save(os.path.join(out_dir, 'inverse_offsets.npy'), torch.cat(inv_offsets).cpu().numpy())
    told = ''
    if refine_steps:
        np.save(os.path.join(out_dir, 'offsets_before_refine.npy'), torch.cat(offsets_before).cpu().numpy())
        before, after = (torch.stack(objectives).sum(0) / M).tolist()          # the batches' objectives are means over their pairs
        with open(os.path.join(out_dir, 'refine.json'), 'w') as f:
            json.dump({'steps': refine_steps, 'term': refine_term, 'objective_before': before, 'objective_after': after}, f, indent=1)
    if scored['overlap'] or scored['tre_px']:
        host = {k: torch.cat(v).cpu().numpy() if v else None for k, v in scored.items()}
        scores = score_summary(host['overlap_before'], host['overlap'], host['tre_before_px'], host['tre_px'])
        with open(os.path.join(out_dir, 'scores.json'), 'w') as f:
            json.dump(scores, f, indent=1)
        if scores.get('dice', {}).get('classes'):
            told += ', mean Dice %.4f -> %.4f over %d classes' % (scores['dice']['mean_before'], scores['dice']['mean_after'], len(scores['dice']['classes']))
        if scores.get('tre_px', {}).get('points'):
            told += ', mean TRE %.3f -> %.3f px over %d points' % (scores['tre_px']['before']['mean'], scores['tre_px']['after']['mean'], scores['tre_px']['points'])
    if want_reg:
        regularity = ops.regularity_summary(torch.cat(jac['jac_counts']), torch.cat(jac['jac_stats']))
        if per_pass:
            regularity['per_pass'] = [ops.regularity_summary(torch.cat([c for c, _ in k]), torch.cat([s for _, s in k])) for k in per_pass]
        with open(os.path.join(out_dir, 'regularity.json'), 'w') as f:
            json.dump(regularity, f, indent=1)
        if opt.jacobian_map:
            np.save(os.path.join(out_dir, 'jacobian_det.npy'), torch.cat(jac['jacobian_det']).cpu().numpy())
        if regularity['fold_frac'] is not None:
            told += ', folds %.2f %%, SDlogJ %s' % (100.0 * regularity['fold_frac'],
                                                   'n/a' if regularity['log_det_std'] is None else '%.3f' % regularity['log_det_std'])
    if opt.similarity:
        whole = lambda pairs: ops.similarity_summary(torch.cat([c for c, _ in pairs]), torch.cat([m for _, m in pairs]))
        similarity = {k: whole(v) for k, v in sim.items()}
        if sim_per_pass:
            similarity['per_pass'] = [whole(k) for k in sim_per_pass]
        with open(os.path.join(out_dir, 'similarity.json'), 'w') as f:
            json.dump(similarity, f, indent=1)
        if similarity['after']['mi'] is not None and similarity['before']['mi'] is not None:
            told += ', MI %.4f -> %.4f' % (similarity['before']['mi'], similarity['after']['mi'])
    if want_surface:
        whole = lambda pairs: ops.surface_summary(torch.cat([c for c, _ in pairs]), torch.cat([h for _, h in pairs]))
        surface = {k: whole(surf[k]) for k in ('before', 'after')}
        with open(os.path.join(out_dir, 'surface.json'), 'w') as f:
            json.dump(surface, f, indent=1)
        if opt.surface_map:
            np.save(os.path.join(out_dir, 'surface_dist2.npy'), torch.cat(surf['dist2']).cpu().numpy())
        hd95 = [surface[k]['mean']['hd95'] for k in ('before', 'after')]
        told += ', HD95 %s -> %s px' % tuple('n/a' if v is None else '%.3f' % v for v in hd95)
    if refine_steps:
        told += ', refined %d steps: objective %.5f -> %.5f' % (refine_steps, before, after)
    torch.cuda.synchronize()
    print('registered %d pairs: %dx%d images with the %s prediction made at %dx%d%s%s%s, %.2f s -> %s'
          % (M, pool_A.shape[2], pool_A.shape[3], opt.stn_type, opt.img_height, opt.img_width, '' if opt.passes == 1 else ' in %d passes' % opt.passes,
             '' if labels is None else ', labels %dx%d' % tuple(labels.shape[2:]), told, time.time() - t0, out_dir))


if __name__ == '__main__':
    main()
