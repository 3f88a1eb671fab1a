"""The regularity read-out: the fused nemar_jacobian_stats (Jacobian determinant map + fold / log-Jacobian statistics in one pass,
csrc/regularity.hip) at N = 8 from a 256^2 field to 1024^2 and 2048^2 outputs:
  * statistics only (det_out = NULL): nothing per pixel is written;
  * statistics + the map: 4 B/px written;
  * the torch path a user had before: F.interpolate of the field + linspace + the positions + diff + products + sum and log — about ten
    full-resolution ATen passes (it evaluates the same formula, not the warp kernel's bits);
  * nemar_warp_resampled_fwd (bilinear, C = 1) alone at the same shape: the known floor for "one pass over the output" (4 B/px gathered,
    4 B/px written).

One process; the variants ALTERNATE inside every round, each timed by device events around `--calls` back-to-back calls; the figure
of a variant is the MEDIAN over `--rounds` rounds (min and max are printed: the spread).  A record, no gate.

    python tools/microbench_regularity.py [--out tools/profiles/regularity.txt]"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from nemar_amd import _lib

GRID_UNET, BILINEAR = 1, 0
SHAPES = ((8, 1024, 1024, 256, 256), (8, 2048, 2048, 256, 256))


def torch_path(pred, H, W):
    """what a user can do without the kernel: (interior, folds, min, max, sum det, sum log det, sum log^2) per sample"""
    f = F.interpolate(pred, size=(H, W), mode="bilinear", align_corners=False)
    gx = torch.linspace(-1, 1, W, device=pred.device)[None, None, :] + f[:, 0]
    gy = torch.linspace(-1, 1, H, device=pred.device)[None, :, None] + f[:, 1]
    px, py = ((gx + 1) * W - 1) / 2, ((gy + 1) * H - 1) / 2
    ax, ay = torch.diff(px, dim=2)[:, :-1], torch.diff(py, dim=2)[:, :-1]
    bx, by = torch.diff(px, dim=1)[:, :, :-1], torch.diff(py, dim=1)[:, :, :-1]
    det = ax * by - bx * ay
    pos = det > 0
    logs = torch.where(pos, torch.log(det.clamp_min(1e-30)), torch.zeros_like(det))
    return ((~pos).sum((1, 2)), det.amin((1, 2)), det.amax((1, 2)), det.sum((1, 2)), logs.sum((1, 2)), (logs * logs).sum((1, 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None, help="also append the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_regularity: no GPU — a timing from anything else would say nothing")
    lib, dev = _lib.load(), torch.device("cuda:0")
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = ["device: %s   rounds %d x %d calls, medians [min .. max]" % (torch.cuda.get_device_name(0), a.rounds, a.calls)]
    for (N, H, W, hf, wf) in SHAPES:
        g = torch.Generator(device=dev).manual_seed(1)
        pred = F.interpolate(torch.randn(N, 2, 4, 5, device=dev, generator=g), size=(hf, wf), mode="bicubic")
        pred = (pred * (0.6 / pred.abs().max())).contiguous()                # some folds, so that both branches of the statistics run
        img = torch.rand(N, 1, H, W, device=dev, generator=g)
        warped, det = torch.empty_like(img), torch.empty(N, H, W, device=dev)
        counts = torch.empty(N, 2, dtype=torch.int32, device=dev)
        stats, stats_map = torch.empty(N, 5, device=dev), torch.empty(N, 5, device=dev)
        wsb = lib.jacobian_stats_workspace(N, H, W)
        ws = torch.empty(wsb // 4, dtype=torch.int32, device=dev)
        today = {}

        def warp():
            lib.warp_resampled_fwd(P(img), P(pred), GRID_UNET, BILINEAR, P(warped), N, 1, H, W, hf, wf, H, W, st())

        def stats_only():
            lib.jacobian_stats(P(pred), GRID_UNET, None, P(counts), P(stats), P(ws), wsb, N, hf, wf, H, W, st())

        def stats_and_map():
            lib.jacobian_stats(P(pred), GRID_UNET, P(det), P(counts), P(stats_map), P(ws), wsb, N, hf, wf, H, W, st())

        def torch_today():
            today["out"] = torch_path(pred, H, W)

        variants = [("bilinear warp alone, C = 1", warp), ("jacobian_stats, stats only", stats_only), ("jacobian_stats, stats + map", stats_and_map),
                    ("torch: interpolate + diff + sums", torch_today)]
        for _, fn in variants:                                        # warm-up: code objects, clocks
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        assert torch.equal(stats.view(torch.int32), stats_map.view(torch.int32)), "stats differ with and without the map"
        folds, mn, mx, sm, sl, sl2 = today["out"]
        interior = (H - 1) * (W - 1)
        assert bool((counts[:, 0] == interior).all())
        agree = "folds %s vs torch %s of %d; sum log det %s vs torch %s" % (counts[:, 1].tolist(), folds.tolist(), interior,
                                                                           ["%.1f" % v for v in stats[:, 3].tolist()], ["%.1f" % v for v in sl.tolist()])
        times = {name: [] for name, _ in variants}
        for _ in range(a.rounds):
            for name, fn in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / a.calls)      # us per call
        lines.append("%dx%dx%d from a %dx%d field   (%s)" % (N, H, W, hf, wf, agree))
        med = {}
        for name, _ in variants:
            t = sorted(times[name])
            med[name] = statistics.median(t)
            lines.append("  %-34s %9.1f us [%9.1f .. %9.1f]   %7.1f Gpx/s" % (name, med[name], t[0], t[-1], N * H * W / med[name] / 1e3))
        lines.append("  stats only / warp alone = %.2f   (stats + map) / warp alone = %.2f   torch / stats only = %.1f   torch / (stats + map) = %.1f"
                     % (med[variants[1][0]] / med[variants[0][0]], med[variants[2][0]] / med[variants[0][0]], med[variants[3][0]] / med[variants[1][0]],
                        med[variants[3][0]] / med[variants[2][0]]))
        del img, warped, det, today
    report = "\n".join(lines)
    print(report)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
