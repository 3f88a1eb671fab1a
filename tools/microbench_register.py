"""Registration at native size: the fused nemar_warp_resampled_fwd against the composed pair it replaces (nemar_bilinear_fwd of the offset
field to the output size, then nemar_grid_sample_fwd), bilinear, UNet mode — and, on the measurement build of the library, the fused kernel's
other shape (nemar_tune(44, 1): 4 consecutive pixels per lane, 16-byte stores) next to the default (one pixel per lane).

One process; the variants ALTERNATE inside every round, each timed by device events around `--calls` back-to-back calls; the figure
of a variant is the MEDIAN over `--rounds` rounds (min and max are printed: the spread).  Bytes are the traffic MODEL, from shapes:
    fused     4 * 2C B/px          (source read once through the caches + output written; the coarse field is noise)
    composed  4 * (2C + 4) B/px    (+ the 2-channel field written at the output size and read back)
Run through tools/gpu_run.sh:   tools/gpu_run.sh register py:tools/microbench_register.py"""
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
SHAPES = ((8, 3, 2048, 2048, 256, 256), (8, 3, 1024, 1024, 256, 256))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None, help="also append the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_register: no GPU — a timing from anything else would say nothing")
    lib, dev = _lib.load(), torch.device("cuda:0")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = ["device: %s   rounds %d x %d calls, medians [min .. max]" % (torch.cuda.get_device_name(0), a.rounds, a.calls)]
    for (N, C, H, W, hf, wf) in SHAPES:
        g = torch.Generator(device=dev).manual_seed(1)
        img = torch.rand(N, C, H, W, device=dev, generator=g)
        pred = torch.nn.functional.interpolate(torch.randn(N, 2, 4, 5, device=dev, generator=g), size=(hf, wf), mode="bicubic") * 0.05
        pred = pred.contiguous()
        out = torch.empty(N, C, H, W, device=dev)
        out_c = torch.empty(N, C, H, W, device=dev)
        field = torch.empty(N, 2, H, W, device=dev)

        def fused():
            lib.warp_resampled_fwd(P(img), P(pred), GRID_UNET, BILINEAR, P(out), N, C, H, W, hf, wf, H, W, st())

        def composed():
            lib.bilinear_fwd(P(pred), P(field), N * 2, hf, wf, H, W, st())
            lib.grid_sample_fwd(P(img), P(field), GRID_UNET, P(out_c), N, C, H, W, H, W, st())

        def fused_vec4():
            lib.tune(44, 1)
            fused()
            lib.tune(44, 0)

        variants = [("fused", fused, 2 * C), ("composed", composed, 2 * C + 4)]
        if lib.has_switches:
            variants.append(("fused, 16-B stores", fused_vec4, 2 * C))
        for _, fn, _ in variants:                                        # warm-up: code objects, clocks
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        assert torch.equal(out, out_c), "fused != composed"
        times = {name: [] for name, _, _ in variants}
        for _ in range(a.rounds):
            for name, fn, _ in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / a.calls)      # us per call
        lines.append("%dx%dx%dx%d from a %dx%d field (outputs equal bit for bit)" % (N, C, H, W, hf, wf))
        med = {}
        for name, _, bpp in variants:
            t = sorted(times[name])
            med[name] = statistics.median(t)
            nbytes = 4 * bpp * N * H * W
            lines.append("  %-18s %8.1f us [%8.1f .. %8.1f]   model %7.1f MB   %6.0f GB/s" % (name, med[name], t[0], t[-1], nbytes / 1e6,
                                                                                             nbytes / med[name] / 1e3))
        lines.append("  composed / fused = %.2f   (traffic model: %d / %d = %.2f)" % (med["composed"] / med["fused"], 4 * (2 * C + 4), 4 * 2 * C,
                                                                                      (2 * C + 4) / (2 * C)))
        del img, out, out_c, field
    report = "\n".join(lines)
    print(report)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
