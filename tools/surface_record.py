"""A record of nemar_surface_distance (csrc/surface.hip), no gate: times on the MI355X at 1024 x 1024, N = 4, blocky label maps
(random ids on a 64-pixel lattice; the fixed map is the moving map displaced by 5 rows and 7 columns), a 256 x 256 UNet field (the
resampled route), for K in {2, 16, 64} and for K = 1024 with three classes present — next to nemar_label_overlap on the same inputs,
and next to K = 3 with the same three classes (what the 1021 absent classes cost).  One process; the calls ALTERNATE inside every
round, each timed by device events around `--calls` back-to-back calls; a figure is the MEDIAN over `--rounds` rounds (min and max are
printed: the spread).  The bytes each pass moves are the model of DESIGN.md "Surface distances", from the counts the call itself returns.

    python tools/surface_record.py [--rounds 11] [--calls 10] [--out tools/profiles/surface_distance.txt]"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

N, H, W, FIELD, BLOCK, MAX_DIST = 4, 1024, 1024, 256, 64, 64
_record = [None]


def emit(line):
    print(line)
    sys.stdout.flush()
    if _record[0] is not None:
        _record[0].write(line + '\n')
        _record[0].flush()


def blocky(seed, ids):
    rng = np.random.default_rng(seed)
    a = np.asarray(ids)[rng.integers(0, len(ids), (N, H // BLOCK, W // BLOCK))].repeat(BLOCK, 1).repeat(BLOCK, 2)
    return np.ascontiguousarray(a).astype(np.float32)


def run(rounds, calls):
    from nemar_amd import _lib
    lib, dev = _lib.load(), torch.device('cuda:0')
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device=dev).manual_seed(1)
    pred = F.interpolate(torch.randn(N, 2, 4, 5, device=dev, generator=g), size=(FIELD, FIELD), mode='bicubic')
    pred = (pred * (0.02 / pred.abs().max())).contiguous()                    # up to ~10 px at 1024
    px = N * H * W
    emit('# N %d, %d x %d, field %d x %d, max_dist %d: rounds %d x %d calls, medians [min .. max]' % (N, H, W, FIELD, FIELD, MAX_DIST, rounds, calls))
    cases = [('K = 2', 2, range(2)), ('K = 16', 16, range(16)), ('K = 64', 64, range(64)), ('K = 3, three classes', 3, range(3)),
             ('K = 1024, three classes present', 1024, (0, 511, 1023))]
    results = {}
    for name, K, ids in cases:
        lm = torch.from_numpy(blocky(2, ids)).to(dev)
        lf = torch.roll(lm, (5, -7), (1, 2)).contiguous()
        counts = torch.empty((N, K, 2, 3), dtype=torch.int32, device=dev)
        hist = torch.empty((N, K, 2, MAX_DIST * MAX_DIST), dtype=torch.int32, device=dev)
        dist2 = torch.empty((N, 2, H, W), dtype=torch.int32, device=dev)
        overlap = torch.empty((N, K, 3), dtype=torch.int32, device=dev)
        wsb = lib.surface_distance_workspace(N, K, H, W)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        surface = lambda d2: lib.surface_distance(P(lm), P(lf), P(pred), 1, P(counts), P(hist), P(d2), P(ws), wsb, N, K, MAX_DIST, H, W, FIELD, FIELD,
                                                  H, W, st())
        variants = [('surface_distance', lambda: surface(None)), ('surface_distance + dist2', lambda: surface(dist2)),
                    ('label_overlap', lambda: lib.label_overlap(P(lm), P(lf), P(pred), 1, P(overlap), N, K, H, W, FIELD, FIELD, H, W, st()))]
        for _, fn in variants:                                                # warm-up: code objects, clocks
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {v: [] for v, _ in variants}
        for _ in range(rounds):
            for v, fn in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[v].append(e0.elapsed_time(e1) * 1e3 / calls)            # us per call
        c = counts.cpu().numpy().view(np.uint32).astype(np.int64)
        defined = (c[..., 0].min(-1) > 0)                                     # [N,K]
        boundary = int(c[..., 0].sum())
        chunk = (wsb - 8 * px) // (4 * px)
        chunks = -(-K // chunk)
        emit('%s   (%d defined (sample, class) pairs, %d boundary pixels, far %d, largest d2 %d; workspace %.1f MiB, %d classes per chunk, %d chunk%s)'
             % (name, int(defined.sum()), boundary, int(c[..., 1].sum()), int(c[..., 2].max()), wsb / 2 ** 20, chunk, chunks, '' if chunks == 1 else 's'))
        for v, _ in variants:
            t = sorted(times[v])
            results[name, v] = statistics.median(t)
            emit('  %-28s %9.1f us [%9.1f .. %9.1f]' % (v, results[name, v], t[0], t[-1]))
        # the model: bytes per pass: 0a reads 12 B/px (two maps, the field is 1/16 of a plane) and writes 4; 0b reads 4 and
        # writes 4 (+ 8 with dist2); 1 per DEFINED (sample, class, map) plane reads 2 and writes 2 going down, reads 2 and writes < 2 coming
        # up; 2 reads 4 B/px of codes per chunk and sample that has a defined class and, per boundary pixel, the g values of its search
        swept = sum(int(defined[:, k0:k0 + chunk].any(1).sum()) for k0 in range(0, K, chunk))       # (sample, chunk) pairs with a defined class
        b0a, b0b, b1, b2 = 16 * px, 8 * px, int(defined.sum()) * 2 * 8 * H * W, swept * 4 * H * W
        emit('  model, MB moved: pass 0a %.1f   0b %.1f (+ %.1f with dist2)   1 %.1f (%d planes swept)   2 %.1f (%d sweeps of the codes of one sample) + the searches of %d boundary pixels'
             % (b0a / 1e6, b0b / 1e6, 8 * px / 1e6, b1 / 1e6, int(defined.sum()) * 2, b2 / 1e6, swept, boundary))
    t3, t1024 = results['K = 3, three classes', 'surface_distance'], results['K = 1024, three classes present', 'surface_distance']
    launches = 2 * (-(-1024 // ((lib.surface_distance_workspace(N, 1024, H, W) - 8 * px) // (4 * px))) - 1)
    emit('# absent classes: K = 1024 with three classes present takes %.2f x the time of K = 3 with the same three: %.1f us more, %.2f us per '
         'absent class against %.1f us per present class (%d more launches, %.1f MB more of hist and counts to clear, workgroups that read two '
         'counts and return) - no sweep of a plane is paid for an absent class, the launches of its chunk are'
         % (t1024 / t3, t1024 - t3, (t1024 - t3) / 1021, t3 / 3, launches, (1024 - 3) * N * 2 * (MAX_DIST * MAX_DIST + 3) * 4 / 1e6))
    per_launch = (t1024 - t3) / launches                                      # an upper estimate: the clearing is in it too
    emit('# classes as a grid dimension: one launch pair per chunk besides passes 0a and 0b, per class '
         'present %.1f -> %.1f -> %.1f us.  A launch pair per class was NOT built and NOT measured; at the <= %.1f us a launch costs above it would add '
         'about %.0f us to the %.0f us of K = 64: not a win that shows at this size, where the sweeps and the searches are the time'
         % (*(results[k, 'surface_distance'] / n for k, n in (('K = 2', 2), ('K = 16', 16), ('K = 64', 64))), per_launch,
            per_launch * (2 * 64 - 2 * -(-64 // ((lib.surface_distance_workspace(N, 64, H, W) - 8 * px) // (4 * px)))), results['K = 64', 'surface_distance']))
    emit('# label_overlap (one pass, 12 B/px read) is the floor of any label read-out: surface_distance is %.0f x that at K = 2 and %.0f x at K = 64'
         % (results['K = 2', 'surface_distance'] / results['K = 2', 'label_overlap'], results['K = 64', 'surface_distance'] / results['K = 64', 'label_overlap']))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'profiles', 'surface_distance.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('surface_record: no GPU — a timing from anything else would say nothing')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    _record[0] = open(a.out, 'w')
    emit('# %s' % torch.cuda.get_device_name(0))
    run(a.rounds, a.calls)
    _record[0].close()
