"""The row-vector forms of the plain data-movement passes (nemar_tune key 47) against the one-element-per-lane kernels behind the same entry
points, at the shapes one BASELINE configs[1] training step launches them with (batch 8, 256 x 256; the registration net's seven levels:
32 / 64 channels, 256^2 .. 4^2 maps — plane counts from nemar_amd/models/stn/unet_stn.py cfg 'A'):
    nemar_bilinear_fwd / nemar_bilinear_bwd   2x up, 512 planes, source 2^2 .. 128^2
    nemar_maxpool2_bwd                        256 planes of 256^2 with the skip addend, 512 planes of 128^2 .. 4^2
    the reflect fold                          no entry point of its own: timed THROUGH nemar_conv2d_bwd_data (3x3 reflect, the 16-bit route's
                                              padded-domain gradient + fold); the column `delta` (switch 0 - switch 1) is the fold's gain, the
                                              absolute figures are the whole call's.  The kernel trace has the fold's own duration.
One process, one stream, the measurement build of the library.  Per shape the two settings ALTERNATE inside every round; each is timed by
device events around `--calls` back-to-back calls; the figure is the MEDIAN over `--rounds` rounds, [min .. max] the spread.  GB/s are
ALGORITHMIC bytes (every tensor of the call once).  The yardstick is nemar_instnorm_fwd over 16 x 64 x 256^2 (268 MB read + 268 MB
written) in the same process: the library's best streaming pass on the box the run landed on.
    python tools/microbench_pointwise.py --out profiles/pointwise_rows.txt"""
import argparse
import ctypes
import os

os.environ.setdefault("NEMAR_AB_LIBRARY", "1")      # nemar_tune: the measurement build of the library (nemar_amd/_lib.py)
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from nemar_amd import _lib

KEY = 47
LEVELS = (128, 64, 32, 16, 8, 4, 2)
PAD_REFLECT = 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_pointwise: no GPU — a timing from anything else would say nothing")
    lib, dev = _lib.load(), torch.device("cuda:0")
    if not lib.has_switches:
        raise SystemExit("microbench_pointwise: needs the measurement build of the library (nemar_tune)")
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.calls      # us per call

    # the yardstick
    x, y, stats = rnd(16 * 64, 256 * 256), torch.empty(16 * 64, 256 * 256, device=dev), torch.empty(16 * 64, 2, device=dev)
    inorm = lambda: lib.instnorm_fwd(P(x), None, P(y), P(stats), 16 * 64, 256 * 256, 1e-5, 0, 0.0, st())
    for _ in range(3):
        inorm()
    torch.cuda.synchronize()
    t = sorted(timed(inorm) for _ in range(a.rounds))
    yard = 2 * x.numel() * 4 / statistics.median(t) / 1e3
    lines = ["device: %s   rounds %d x %d calls, medians [min .. max]" % (torch.cuda.get_device_name(0), a.rounds, a.calls),
             "yardstick nemar_instnorm_fwd 16x64x256^2: %.1f us [%.1f .. %.1f] = %.0f GB/s" % (statistics.median(t), t[0], t[-1], yard),
             "%-44s %28s %28s %7s %7s %6s %s" % ("call", "switch 0: us [min .. max]", "switch 1: us [min .. max]", "GB/s 0", "GB/s 1", "/yard",
                                                  "verdict")]
    del x, y, stats

    def ab(name, fn, out, nbytes, through_conv=False):
        """fn() at switch 0 and 1, alternating; `out` must come out bit for bit the same"""
        res = {}
        for v in (0, 1):
            lib.tune(KEY, v)
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            res[v] = out.clone()
        assert torch.equal(res[0].view(torch.int32), res[1].view(torch.int32)), "%s: the two forms differ" % name
        times = {0: [], 1: []}
        for _ in range(a.rounds):
            for v in (0, 1):
                lib.tune(KEY, v)
                times[v].append(timed(fn))
        lib.tune(KEY, 1)
        s0, s1 = sorted(times[0]), sorted(times[1])
        m0, m1 = statistics.median(s0), statistics.median(s1)
        spread = max(s0[-1] - s0[0], s1[-1] - s1[0])
        verdict = "faster" if m0 - m1 > spread else ("SLOWER" if m1 - m0 > spread else "same within the spread")
        if through_conv:
            lines.append("%-44s %9.1f [%7.1f .. %7.1f] %9.1f [%7.1f .. %7.1f]   delta %6.1f us (fold bytes %5.1f MB)        %s" % (
                name, m0, s0[0], s0[-1], m1, s1[0], s1[-1], m0 - m1, nbytes / 1e6, verdict))
        else:
            lines.append("%-44s %9.1f [%7.1f .. %7.1f] %9.1f [%7.1f .. %7.1f] %7.0f %7.0f %6.2f %s" % (
                name, m0, s0[0], s0[-1], m1, s1[0], s1[-1], nbytes / m0 / 1e3, nbytes / m1 / 1e3, nbytes / m1 / 1e3 / yard, verdict))

    planes = 8 * 64
    for h in LEVELS:
        src, dst = rnd(planes, h, h), torch.empty(planes, 2 * h, 2 * h, device=dev)
        ab("bilinear_fwd %d x %d^2 -> %d^2" % (planes, h, 2 * h),
           lambda: lib.bilinear_fwd(P(src), P(dst), planes, h, h, 2 * h, 2 * h, st()), dst, 4 * (src.numel() + dst.numel()))
    for h in LEVELS:
        gy, gx = rnd(planes, 2 * h, 2 * h), torch.empty(planes, h, h, device=dev)
        ab("bilinear_bwd %d x %d^2 -> %d^2" % (planes, 2 * h, h),
           lambda: lib.bilinear_bwd(P(gy), P(gx), planes, h, h, 2 * h, 2 * h, st()), gx, 4 * (gy.numel() + gx.numel()))
    for pl, h, with_add in ((8 * 32, 256, True),) + tuple((planes, h, True) for h in LEVELS[:-1]):
        x, gy, add, gx = rnd(pl, h, h), rnd(pl, h // 2, h // 2), rnd(pl, h, h) if with_add else None, torch.empty(pl, h, h, device=dev)
        ab("maxpool2_bwd %d x %d^2 + addend" % (pl, h),
           lambda: lib.maxpool2_bwd(P(x), P(gy), P(add), P(gx), pl, h, h, st()), gx, 4 * (3 * x.numel() + gy.numel()))
    for N, C, h in ((8, 32, 256), (8, 64, 128), (8, 64, 64)):
        gy, w, gx, add = rnd(N, C, h, h), rnd(C, C, 3, 3) * 0.05, torch.empty(N, C, h, h, device=dev), rnd(N, C, h, h)
        wsb = lib.conv2d_bwd_data_workspace(N, C, h, h, C, 3, 3, 1, 1, PAD_REFLECT)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        for with_add in (False, True):
            e = _lib.ConvExtras()
            e.addend = add.data_ptr() if with_add else None
            ab("conv2d_bwd_data %dx%dx%d^2 3x3 reflect%s" % (N, C, h, " + addend" if with_add else ""),
               lambda: lib.conv2d_bwd_data_ex(P(gy), P(w), None, 0, 0.0, P(gx), C, None, 0, N, h, h, C, h, h, 3, 3, 1, 1, PAD_REFLECT, P(ws), wsb, 0,
                                              st(), ctypes.byref(e)),
               gx, 4 * (N * C * (h + 2) * (h + 2) + (3 if with_add else 2) * gx.numel() - gx.numel()), through_conv=True)
            assert lib.last_route() == 3, "the reflect data gradient left the 16-bit route (%d)" % lib.last_route()
    report = "\n".join(lines)
    print(report)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
