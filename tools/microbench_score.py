"""Scoring a registration: the fused nemar_label_overlap (nearest warp + per-class counts in one pass, csrc/score.hip) against
  * nemar_warp_resampled_fwd(NEAREST, C = 1) alone at the same shape — a gather and a stream of the same bytes: the floor;
  * that call + torch.bincount over K * m + f — what a user had before;
  * on the measurement build, the fused kernel with every lane adding to the LDS histogram for itself (nemar_tune(45, 1)) next to the
    default (the lanes that share the wave's first key added once, by a ballot);
on three label contents: blocky (random ids on an 8 x 8-pixel lattice: what real label maps look like), single (one class: every lane
on one counter) and random (per-pixel ids: no two lanes agree), K = 8 and K = 256, N = 4, 1024^2 and 2048^2 from a 256^2 field.

One process; the variants ALTERNATE inside every round, each timed by device events around `--calls` back-to-back calls; the figure
of a variant is the MEDIAN over `--rounds` rounds (min and max are printed: the spread).  Bytes are the traffic MODEL of the fused
kernel, from shapes: 4 B/px of the moving map (read once through the caches) + 4 B/px of the fixed map; the coarse field and the
counts are noise.  The bare warp moves the same 8 B/px (4 read, 4 written)."""
import argparse
import ctypes
import os

os.environ.setdefault("NEMAR_AB_LIBRARY", "1")      # nemar_tune: the measurement build of the library (nemar_amd/_lib.py)
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from nemar_amd import _lib

GRID_UNET, NEAREST = 1, 1
SHAPES = ((4, 1024, 1024, 256, 256), (4, 2048, 2048, 256, 256))
CLASSES = (8, 256)
CONTENTS = ("blocky", "single", "random")


def labels(kind, N, H, W, K, dev, g):
    if kind == "random":
        a = torch.randint(0, K, (N, H, W), device=dev, generator=g)
    elif kind == "blocky":
        a = torch.randint(0, K, (N, H // 8, W // 8), device=dev, generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
    else:
        a = torch.full((N, H, W), K // 2, device=dev)
    return a.float().contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None, help="also append the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_score: no GPU — a timing from anything else would say nothing")
    lib, dev = _lib.load(), torch.device("cuda:0")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = ["device: %s   rounds %d x %d calls, medians [min .. max]" % (torch.cuda.get_device_name(0), a.rounds, a.calls)]
    for (N, H, W, hf, wf) in SHAPES:
        for K in CLASSES:
            for kind in CONTENTS:
                g = torch.Generator(device=dev).manual_seed(1)
                lm, lf = labels(kind, N, H, W, K, dev, g), labels(kind, N, H, W, K, dev, g)
                pred = torch.nn.functional.interpolate(torch.randn(N, 2, 4, 5, device=dev, generator=g), size=(hf, wf), mode="bicubic") * 0.05
                pred = pred.contiguous()
                warped = torch.empty(N, 1, H, W, device=dev)
                counts = torch.empty(N, K, 3, dtype=torch.int32, device=dev)
                base = (torch.arange(N, device=dev) * (K * K))[:, None, None]
                today = {}

                def warp():
                    lib.warp_resampled_fwd(P(lm), P(pred), GRID_UNET, NEAREST, P(warped), N, 1, H, W, hf, wf, H, W, st())

                def fused():
                    lib.label_overlap(P(lm), P(lf), P(pred), GRID_UNET, P(counts), N, K, H, W, hf, wf, H, W, st())

                def fused_per_lane():
                    lib.tune(45, 1)
                    fused()
                    lib.tune(45, 0)

                def warp_bincount():
                    warp()
                    today["joint"] = torch.bincount((warped[:, 0].long() * K + lf.long() + base).view(-1), minlength=N * K * K)

                variants = [("nearest warp alone", warp), ("label_overlap", fused), ("warp + torch.bincount", warp_bincount)]
                if lib.has_switches:
                    variants.insert(2, ("label_overlap, per-lane adds", fused_per_lane))
                for _, fn in variants:                                        # warm-up: code objects, clocks
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                joint = today["joint"].view(N, K, K)
                want = torch.stack([joint.diagonal(dim1=1, dim2=2), joint.sum(2), joint.sum(1)], dim=2)
                assert torch.equal(counts.long(), want), "label_overlap != warp + bincount"
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
                nbytes = 8 * N * H * W
                lines.append("%dx%dx%d from a %dx%d field, K = %d, %s labels (counts equal warp + bincount)   model %.1f MB" % (N, H, W, hf, wf, K, kind, nbytes / 1e6))
                med = {}
                for name, _ in variants:
                    t = sorted(times[name])
                    med[name] = statistics.median(t)
                    lines.append("  %-30s %8.1f us [%8.1f .. %8.1f]   %6.0f GB/s" % (name, med[name], t[0], t[-1], nbytes / med[name] / 1e3))
                lines.append("  label_overlap / nearest warp alone = %.2f   (warp + bincount) / label_overlap = %.2f"
                             % (med["label_overlap"] / med["nearest warp alone"], med["warp + torch.bincount"] / med["label_overlap"]))
                del lm, lf, warped, counts
    report = "\n".join(lines)
    print(report)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
