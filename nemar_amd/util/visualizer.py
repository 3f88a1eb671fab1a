"""Console / file loss log and scalar log — the observability surface of the reference that a training loop needs
(SURVEY.md §8 f4), without per-iteration host synchronisation:

  * LossLogger.print_current_losses reproduces the reference's line byte for byte (util/visualizer.py:211-227):
    '(epoch: %d, iters: %d, time: %.3f, data: %.3f) ' + '%s: %.3f ' per loss, printed and appended to loss_log.txt;
  * ScalarLog + OffsetMeter reproduce what TensorboardVisualizer reports (util/tb_visualizer.py:53-92): 'loss/<name>',
    'offset/mean_x', 'offset/mean_y' every --tbvis_iteration_update_rate iterations.  The reference copies the whole
    deformation field to the host every iteration (:71-74); here the per-channel sums are accumulated ON THE DEVICE by
    the bias-gradient reduction kernel into two floats and read back only when a report is written.
visdom / HTML image pages stay out of scope."""
import json
import os
import time

import torch

from .. import ops


class LossLogger:
    def __init__(self, opt):
        self.log_name = os.path.join(opt.checkpoints_dir, opt.name, 'loss_log.txt')
        os.makedirs(os.path.dirname(self.log_name), exist_ok=True)
        with open(self.log_name, "a") as f:
            f.write('================ Training Loss (%s) ================\n' % time.strftime("%c"))

    def print_current_losses(self, epoch, iters, losses, t_comp, t_data):
        message = '(epoch: %d, iters: %d, time: %.3f, data: %.3f) ' % (epoch, iters, t_comp, t_data)
        for k, v in losses.items():
            message += '%s: %.3f ' % (k, v)
        print(message)
        with open(self.log_name, "a") as f:
            f.write('%s\n' % message)
        return message


class ScalarLog:
    """add_scalar(tag, value, step): torch.utils.tensorboard.SummaryWriter when it is importable, and always a JSON-lines
    file next to the checkpoints (the build image has no tensorboard)."""

    def __init__(self, opt):
        self.dir = '{}/{}/{}_tensorboard_logs'.format(opt.checkpoints_dir, opt.name, opt.name)
        os.makedirs(self.dir, exist_ok=True)
        self.path = os.path.join(self.dir, 'scalars.jsonl')
        self.writer = None
        try:
            from torch.utils.tensorboard import SummaryWriter
            self.writer = SummaryWriter(self.dir)
        except Exception:
            pass

    def add_scalar(self, tag, value, step):
        with open(self.path, 'a') as f:
            f.write(json.dumps({'tag': tag, 'value': float(value), 'step': int(step)}) + '\n')
        if self.writer is not None:
            self.writer.add_scalar(tag, float(value), step)

    def add_histogram(self, tag, tensor, step, bins=30):
        """reference tb_visualizer.py:39 `writer.add_histogram(name, p.clone().cpu().data.numpy(), step)`: the SummaryWriter call
        when tensorboard is importable; the JSON-lines file always gets a 30-bin histogram computed ON the device (one
        torch.histc + min / max / mean: 33 floats cross PCIe instead of the whole parameter)."""
        t = tensor.detach().float().reshape(-1)
        lo, hi = float(t.min()), float(t.max())
        counts = torch.histc(t, bins=bins, min=lo, max=hi if hi > lo else lo + 1.0).tolist()
        with open(os.path.join(self.dir, 'histograms.jsonl'), 'a') as f:
            f.write(json.dumps({'tag': tag, 'step': int(step), 'min': lo, 'max': hi, 'mean': float(t.mean()), 'counts': counts}) + '\n')
        if self.writer is not None:
            self.writer.add_histogram(tag, t.cpu().numpy(), step)


class OffsetMeter:
    """Running mean of the deformation offsets per direction (reference tb_visualizer.py:59-74): update() adds the field's
    per-channel sums into a 2-float device accumulator (one kernel pair, no sync); means() reads it back and resets."""

    def __init__(self, device):
        self.acc = torch.zeros(2, dtype=torch.float32, device=device)
        self.weight = 0.0          # sum over updates of 1 (the reference averages per-iteration means)
        self.norm = []

    def update(self, offsets):
        n, c, h, w = offsets.shape
        assert c == 2
        # acc[c] += sum_{n,h,w} offsets / (n*h*w)  ==  += mean(offsets[:, c]) : scale folded in by accumulating raw sums of a
        # constant-size field; sizes may vary between calls, so keep the per-call normaliser on the host
        part = torch.zeros(2, dtype=torch.float32, device=offsets.device)
        ops._bias_grad(offsets.contiguous(), part, n, 2, h * w, ops._stream())
        self.acc.add_(part, alpha=1.0 / (n * h * w))
        self.weight += 1.0

    def means(self):
        if self.weight == 0:
            return 0.0, 0.0
        mx, my = (self.acc / self.weight).tolist()           # the only device->host transfer
        self.acc.zero_()
        self.weight = 0.0
        return mx, my


def registration_summary(cols, pixels):
    """the six column totals of ops.registration_error (ops.REG_COLUMNS; the maximum column max-ed) over `pixels` pixels -> the five
    reported numbers.  A batch without a single valid pixel has no error to average: epe_px and max_px are 0 and valid_frac says why."""
    valid, sum_r, max_r, sum_g, fold, interior = cols
    return {'epe_px': sum_r / valid if valid > 0 else 0.0, 'epe_before_px': sum_g / pixels if pixels > 0 else 0.0, 'max_px': max_r,
            'fold_frac': fold / interior if interior > 0 else 0.0, 'valid_frac': valid / pixels if pixels > 0 else 0.0}


class RegistrationMeter:
    """Registration error against the batch's ground-truth field (--misalign), accumulated ON THE DEVICE: update() runs the meter kernel
    on the step's own prediction and folds its [N,6] rows into a device accumulator (sums added, the maximum max-ed; no sync); read()
    transfers seven floats, returns the summary of everything since the last read (None if nothing was added) and resets."""

    def __init__(self, device):
        self.acc = torch.zeros(6, dtype=torch.float32, device=device)
        self.max = torch.zeros(1, dtype=torch.float32, device=device)
        self.pixels = 0

    def update(self, pred, mode, gt_field):
        rows = ops.registration_error(pred, gt_field, mode)
        self.acc.add_(rows.sum(0))
        self.max = torch.maximum(self.max, rows[:, 2].max().reshape(1))
        self.pixels += gt_field.size(0) * gt_field.size(2) * gt_field.size(3)

    def read(self):
        if self.pixels == 0:
            return None
        cols = torch.cat([self.acc, self.max]).tolist()          # the only device->host transfer
        cols[2] = cols.pop()
        out = registration_summary(cols, self.pixels)
        self.acc.zero_()
        self.max.zero_()
        self.pixels = 0
        return out


class FoldMeter:
    """Share of the interior pixels on which the fold penalty acts (--lambda_fold): update() adds the step's per-sample counts
    (ops.fold_penalty's `active`) into a device accumulator, no sync; read() transfers one integer, returns sum active / sum M of
    everything since the last read (None if nothing was added) and resets."""

    def __init__(self, device):
        self.acc = torch.zeros((), dtype=torch.int64, device=device)
        self.pixels = 0

    def update(self, active, interior_per_sample):
        self.acc.add_(active.sum())
        self.pixels += active.numel() * int(interior_per_sample)

    def read(self):
        if self.pixels == 0:
            return None
        frac = int(self.acc) / self.pixels                       # the only device->host transfer
        self.acc.zero_()
        self.pixels = 0
        return frac


class TrainingMonitor:
    """What train.py drives every iteration (reference TensorboardVisualizer.iteration_step, tb_visualizer.py:68-85)."""

    def __init__(self, model, opt):
        self.model, self.opt = model, opt
        self.rate = int(getattr(opt, 'tbvis_iteration_update_rate', 1000))
        self.report_offsets = not getattr(opt, 'tbvis_disable_report_offsets', False)
        self.report_weights = not getattr(opt, 'tbvis_disable_report_weights', False)
        self.log = ScalarLog(opt)
        self.report_registration = not getattr(opt, 'tbvis_disable_report_registration', False)
        self.meter = OffsetMeter(model.device)
        self.reg_meter = RegistrationMeter(model.device)
        self.fold_meter = FoldMeter(model.device) if getattr(model, '_fold_on', False) else None
        self.iteration_cnt = 0
        self.save_count = 0

    def iteration_step(self):
        field = getattr(self.model, 'deformation_field_A_to_B', None)
        if self.report_offsets and field is not None and field.dim() == 4 and field.size(1) == 2:
            self.meter.update(field)
        gt = getattr(self.model, 'gt_field', None)
        if self.report_registration and gt is not None:
            pred = self.model.netR.last_prediction()             # the prediction of the step's own forward pass: R is not run again
            if pred is not None:
                self.reg_meter.update(pred[0], pred[1], gt)
        active = getattr(self.model.netR, 'last_fold_active', None) if self.fold_meter is not None else None
        if active is not None:
            self.fold_meter.update(active, self.model.netR.last_fold_interior)
        if self.rate <= 0:
            return
        if self.iteration_cnt == 0:
            for name, v in self.model.get_current_losses().items():
                self.log.add_scalar('loss/{}'.format(name), v, self.save_count)
            if self.report_weights:
                self.save_current_weights()
            if self.report_offsets:
                mx, my = self.meter.means()
                self.log.add_scalar('offset/mean_x', mx, self.save_count)
                self.log.add_scalar('offset/mean_y', my, self.save_count)
            self.write_registration()
            self.save_count += 1
        self.iteration_cnt = (self.iteration_cnt + 1) % self.rate

    def save_current_weights(self):
        """'<net>/data/Weight|Bias/<parameter name>' histograms of every trainable parameter of T, R, D (reference
        tb_visualizer.py:34-40; gated by --tbvis_disable_report_weights like there)."""
        for net_name in ('netR', 'netT', 'netD'):             # the reference's list and order (models/nemar_model.py:58)
            net = getattr(self.model, net_name, None)
            if net is None:
                continue
            for n, p in net.named_parameters():
                if p.requires_grad:
                    self.log.add_histogram('{}/data/{}/{}'.format(net_name, 'Bias' if 'bias' in n else 'Weight', n), p, self.save_count)

    def epoch_step(self):
        if self.rate > 0:          # iteration-resolution reporting is on: nothing per epoch (reference :87-95)
            return
        for name, v in self.model.get_current_losses().items():
            self.log.add_scalar('loss/{}'.format(name), v, self.save_count)
        if self.report_weights:
            self.save_current_weights()
        if self.report_offsets:
            mx, my = self.meter.means()
            self.log.add_scalar('offset/mean_x', mx, self.save_count)
            self.log.add_scalar('offset/mean_y', my, self.save_count)
        self.write_registration()
        self.save_count += 1

    def write_registration(self):
        """'registration/<name>' of everything metered since the last report (nothing without a ground-truth field), and with the
        fold penalty on 'fold/active_frac'"""
        summary = self.reg_meter.read() if self.report_registration else None
        for name, v in (summary or {}).items():
            self.log.add_scalar('registration/{}'.format(name), v, self.save_count)
        frac = self.fold_meter.read() if self.fold_meter is not None else None
        if frac is not None:
            self.log.add_scalar('fold/active_frac', frac, self.save_count)

    def end(self):
        if self.log.writer is not None:
            self.log.writer.close()
