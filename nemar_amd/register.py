"""Register image pairs at their native size with a trained model — inference only, no image decoding library:

    python -m nemar_amd.register --dataroot DIR --name EXPERIMENT --checkpoints_dir ./checkpoints --epoch latest \\
        --stn_type unet --img_height 256 --img_width 256 --batch_size 4 --results_dir ./results

DIR holds `A.npy` / `B.npy` in the format `--dataset_mode gpupairs` trains from ([M,3,H,W] or [M,H,W,3], uint8 or float in [0, 1]) and,
optionally, `labels_A.npy` ([M,H,W] or [M,C,H,W], any numeric dtype: a label map of modality A at any size).  Every pair is brought to the
network's --img_height x --img_width by the dataset's own resize and normalise path, netR predicts the transformation ONCE at that size
(weights of --epoch under --checkpoints_dir/--name, the flags the model was trained with), and NEMARModel.register() applies it to the
full-size images: the sampling grid is in normalised coordinates, so the prediction holds at every size (csrc/register.hip).

Written under --results_dir/--name/:
    registered_A.npy          modality A registered to B, in A.npy's own size, layout and dtype (uint8: rounded and clamped on the host)
    registered_labels_A.npy   labels_A.npy warped with nearest sampling (class ids are copied, never blended), in its own dtype
    offsets.npy               the network-resolution predictions: offsets [M,2,h,w] (unet) or dtheta [M,6] (affine)
and one summary line on stdout: pairs, sizes, seconds."""
import os
import time

import numpy as np
import torch

from .data.gpupairs_dataset import GpuPairsDataset
from .models import create_model
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
    model = create_model(opt)
    model.setup(opt)
    if opt.eval:
        model.eval()
    M = pool_A.shape[0]
    reg, reg_labels, offsets = [], [], []
    for i0 in range(0, M, opt.batch_size):
        idx = list(range(i0, min(M, i0 + opt.batch_size)))
        model.set_input(network_batch(pool_A, pool_B, idx, opt))
        model.test()
        out = model.register(pool_A[idx[0]:idx[-1] + 1], pool_B[idx[0]:idx[-1] + 1], None if labels is None else labels[idx[0]:idx[-1] + 1],
                             translate=False)          # (fake_RT_B is not among the files this command writes)
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
    torch.cuda.synchronize()
    print('registered %d pairs: %dx%d images with the %s prediction made at %dx%d%s, %.2f s -> %s'
          % (M, pool_A.shape[2], pool_A.shape[3], opt.stn_type, opt.img_height, opt.img_width,
             '' if labels is None else ', labels %dx%d' % tuple(labels.shape[2:]), time.time() - t0, out_dir))


if __name__ == '__main__':
    main()
