"""CPU tier of the known-misalignment pipeline: the new flags and their defaults, the arithmetic of the five reported numbers, and a
monitor that stays silent about registration when the model carries no ground-truth field."""
import argparse
import json
import os

import pytest

NEW = {'misalign': 'none', 'misalign_max_px': 8.0, 'misalign_rot_deg': 5.0, 'misalign_scale': 0.05, 'misalign_grid': 6,
       'synthetic_pairs': 'independent', 'tbvis_disable_report_registration': False}

# the option names of `python -m nemar_amd.train --dataset_mode gpupairs` before this feature
PARENT = {'batch_size', 'beta1', 'checkpoints_dir', 'continue_train', 'crop_size', 'data_seed', 'dataroot', 'dataset_mode', 'direction',
          'display_env', 'display_freq', 'display_id', 'display_ncols', 'display_port', 'display_server', 'display_winsize', 'enable_tbvis',
          'epoch', 'epoch_count', 'gan_mode', 'gpu_ids', 'img_height', 'img_width', 'init_gain', 'init_type', 'input_nc', 'isTrain',
          'lambda_GAN', 'lambda_recon', 'lambda_smooth', 'load_iter', 'load_size', 'lr', 'lr_decay_iters', 'lr_policy', 'max_dataset_size',
          'model', 'multi_resolution', 'n_layers_D', 'name', 'ndf', 'netD', 'netG', 'ngf', 'niter', 'niter_decay', 'no_dropout', 'no_flip',
          'no_html', 'norm', 'num_threads', 'output_nc', 'phase', 'pool_size', 'pool_size_pairs', 'preprocess', 'print_freq', 'save_by_iter',
          'save_epoch_freq', 'save_latest_freq', 'seed', 'serial_batches', 'step_graph', 'stn_bilateral_alpha', 'stn_cfg', 'stn_multires_reg',
          'stn_no_identity_init', 'stn_type', 'suffix', 'tbvis_disable_report_offsets', 'tbvis_disable_report_weights',
          'tbvis_iteration_update_rate', 'update_html_freq', 'verbose'}


def test_new_flags_default_to_todays_behaviour():
    from nemar_amd.train import _Options
    opt = vars(_Options().parse(['--dataset_mode', 'gpupairs'], quiet=True))
    assert {k: opt[k] for k in NEW} == NEW
    assert set(opt) - set(NEW) == PARENT                       # nothing else was added, renamed or dropped
    opt = _Options().parse(['--dataset_mode', 'gpupairs', '--misalign', 'both', '--misalign_max_px', '3.5', '--misalign_rot_deg', '2',
                            '--misalign_scale', '0.1', '--misalign_grid', '5', '--synthetic_pairs', 'mapped',
                            '--tbvis_disable_report_registration'], quiet=True)
    assert (opt.misalign, opt.misalign_max_px, opt.misalign_rot_deg, opt.misalign_scale, opt.misalign_grid, opt.synthetic_pairs,
            opt.tbvis_disable_report_registration) == ('both', 3.5, 2.0, 0.1, 5, 'mapped', True)
    with pytest.raises(SystemExit):
        _Options().parse(['--dataset_mode', 'gpupairs', '--misalign', 'shear'], quiet=True)


def test_registration_summary_arithmetic():
    from nemar_amd.util.visualizer import registration_summary
    s = registration_summary([50.0, 125.0, 7.5, 300.0, 3.0, 60.0], 100)
    assert s == {'epe_px': 2.5, 'epe_before_px': 3.0, 'max_px': 7.5, 'fold_frac': 0.05, 'valid_frac': 0.5}
    s = registration_summary([0.0, 0.0, 0.0, 300.0, 0.0, 0.0], 100)          # nothing valid, a 1-pixel-wide image: no division by zero
    assert s == {'epe_px': 0.0, 'epe_before_px': 3.0, 'max_px': 0.0, 'fold_frac': 0.0, 'valid_frac': 0.0}


def test_monitor_writes_no_registration_scalars_without_a_ground_truth_field(tmp_path):
    import torch
    from nemar_amd.util import visualizer as V

    class Model:
        device = torch.device('cpu')
        netR = torch.nn.Linear(4, 2)

        def get_current_losses(self):
            return {'L1_TR': 1.5}

    opt = argparse.Namespace(checkpoints_dir=str(tmp_path), name='m', tbvis_iteration_update_rate=1, tbvis_disable_report_offsets=True,
                             tbvis_disable_report_weights=True)
    mon = V.TrainingMonitor(Model(), opt)
    assert mon.report_registration
    for _ in range(2):
        mon.iteration_step()
    mon.epoch_step()
    mon.end()
    tags = [json.loads(l)['tag'] for l in open(os.path.join(mon.log.dir, 'scalars.jsonl'))]
    assert tags == ['loss/L1_TR', 'loss/L1_TR']
