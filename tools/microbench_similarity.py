"""Intensity agreement of a registration: the fused nemar_joint_histogram (bilinear warp + channel means + joint histogram + moments in
one pass, csrc/similarity.hip) against
  * nemar_warp_resampled_fwd(BILINEAR) of the same moving image at the same shape — the same gather plus a store of Cm planes that the
    fused kernel does not do: the yardstick;
  * itself without the moments (moments = NULL: no partial records, no merge launch);
  * on the measurement build, the fused kernel with every lane adding to the LDS table for itself (nemar_tune(46, 1): the default and
    the product's path) next to the lanes that share the wave's first cell being added once, by a ballot (nemar_tune(46, 0));
on three image contents: smooth (noise on a 16 x 20 lattice, bicubic in between: what natural images look like to a 32-bin histogram —
neighbouring lanes in the same cell), blocky (one value per 8 x 8 pixels) and random (per-pixel noise: no two lanes agree by design),
Cm = 3, Cf = 1, N = 4, 32 and 64 bins, 1024^2 and 2048^2 from a 256^2 field.

One process; the variants ALTERNATE inside every round, each timed by device events around `--calls` back-to-back calls; the figure
of a variant is the MEDIAN over `--rounds` rounds (min and max are printed: the spread).  Bytes are the traffic MODEL of the fused
kernel, from shapes: 4 B/px per moving channel (read once through the caches) + 4 B/px per fixed channel; the coarse field and the
table are noise.  The bare warp reads the same moving bytes and writes 4 B/px per channel."""
import argparse
import ctypes
import os

os.environ.setdefault("NEMAR_AB_LIBRARY", "1")      # nemar_tune: the measurement build of the library (nemar_amd/_lib.py)
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from nemar_amd import _lib

GRID_UNET, BILINEAR = 1, 0
SHAPES = ((4, 1024, 1024, 256, 256), (4, 2048, 2048, 256, 256))
BINS = (32, 64)
CONTENTS = ("smooth", "blocky", "random")
CM, CF = 3, 1


def image(kind, N, C, H, W, dev, g):
    if kind == "random":
        a = torch.rand(N, C, H, W, device=dev, generator=g)
    elif kind == "blocky":
        a = torch.rand(N, C, H // 8, W // 8, device=dev, generator=g).repeat_interleave(8, 2).repeat_interleave(8, 3)
    else:
        a = torch.nn.functional.interpolate(torch.rand(N, C, 16, 20, device=dev, generator=g), size=(H, W), mode="bicubic", align_corners=False)
    return (a.clamp_(0, 1) * 2 - 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None, help="also append the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_similarity: no GPU — a timing from anything else would say nothing")
    lib, dev = _lib.load(), torch.device("cuda:0")
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = ["device: %s   rounds %d x %d calls, medians [min .. max]" % (torch.cuda.get_device_name(0), a.rounds, a.calls)]
    for (N, H, W, hf, wf) in SHAPES:
        for kind in CONTENTS:
            g = torch.Generator(device=dev).manual_seed(1)
            moving, fixed = image(kind, N, CM, H, W, dev, g), image(kind, N, CF, H, W, dev, g)
            pred = torch.nn.functional.interpolate(torch.randn(N, 2, 4, 5, device=dev, generator=g), size=(hf, wf), mode="bicubic") * 0.05
            pred = pred.contiguous()
            warped = torch.empty(N, CM, H, W, device=dev)
            wsb = int(lib.joint_histogram_workspace(N, H, W))
            ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
            moments = torch.empty(N, 6, device=dev)
            for B in BINS:
                counts = torch.empty(N, B, B, dtype=torch.int32, device=dev)
                kept = {}

                def warp():
                    lib.warp_resampled_fwd(P(moving), P(pred), GRID_UNET, BILINEAR, P(warped), N, CM, H, W, hf, wf, H, W, st())

                def fused(mom=moments):
                    lib.joint_histogram(P(moving), P(fixed), P(pred), GRID_UNET, P(counts), P(mom), P(ws), wsb, N, CM, CF, B, -1.0, 1.0, -1.0, 1.0,
                                        H, W, hf, wf, H, W, st())

                def switched(value, name):
                    def run():
                        lib.tune(46, value)
                        fused()
                        lib.tune(46, 1)                                       # (the default)
                        if name not in kept:
                            kept[name] = (counts.clone(), moments.clone())
                    return run

                variants = [("bilinear warp alone, C = %d" % CM, warp)]
                if lib.has_switches:
                    variants += [("joint_histogram, wave-aggregated adds", switched(0, "agg")), ("joint_histogram, per-lane adds", switched(1, "lane"))]
                else:
                    variants += [("joint_histogram", fused)]
                variants += [("joint_histogram, no moments", lambda: fused(None))]
                for _, fn in variants:                                        # warm-up: code objects, clocks
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                if lib.has_switches:
                    assert torch.equal(kept["agg"][0], kept["lane"][0]) and torch.equal(kept["agg"][1], kept["lane"][1]), "the two LDS-add variants differ"
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
                nbytes = 4 * (CM + CF) * N * H * W
                lines.append("%dx%dx%dx%d + %d from a %dx%d field, %d bins, %s images (counted %d of %d px)   model %.1f MB"
                             % (N, CM, H, W, CF, hf, wf, B, kind, int(counts.long().sum()), N * H * W, nbytes / 1e6))
                med = {}
                for name, _ in variants:
                    t = sorted(times[name])
                    med[name] = statistics.median(t)
                    lines.append("  %-40s %8.1f us [%8.1f .. %8.1f]   %6.0f GB/s" % (name, med[name], t[0], t[-1], nbytes / med[name] / 1e3))
                base = med["bilinear warp alone, C = %d" % CM]
                lines.append("  " + "   ".join("%s / warp alone = %.2f" % (name, med[name] / base) for name, _ in variants[1:]))
            del moving, fixed, warped
    report = "\n".join(lines)
    print(report)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
