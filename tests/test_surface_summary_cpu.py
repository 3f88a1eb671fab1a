"""CPU tier: ops.surface_summary (the host arithmetic behind surface.json) on hand-built counts and histograms, against
numpy.percentile / numpy.mean over the distance lists the histograms stand for.  Floating point enters only here: a distance is
sqrt(d2) in float64, the percentile is numpy's own interpolation of two such values (equal bit for bit), and a mean over n <= 400
distances taken from the histogram instead of the list differs by the order of the additions: n * 2^-53 relative, bounded by 1e-12."""
import json

import numpy as np
import pytest
import torch

RTOL = 1e-12
D = 8
B = D * D


def _pair(d2_mf, d2_fm, max_dist=D):
    """counts [2,3] and hist [2,B] of one defined (sample, class) pair from the two directions' lists of squared distances"""
    counts, hist = np.zeros((2, 3), dtype=np.int64), np.zeros((2, max_dist * max_dist), dtype=np.int64)
    for d, v in enumerate((np.asarray(d2_mf), np.asarray(d2_fm))):
        near = v[v < max_dist * max_dist]
        hist[d] = np.bincount(near, minlength=max_dist * max_dist)
        counts[d] = [len(v), len(v) - len(near), v.max()]
    return counts, hist


def _want(d2_mf, d2_fm):
    mf, fm = np.sqrt(np.asarray(d2_mf, dtype=np.float64)), np.sqrt(np.asarray(d2_fm, dtype=np.float64))
    return {'hd': max(mf.max(), fm.max()), 'hd95': np.percentile(np.concatenate([mf, fm]), 95), 'asd_mf': mf.mean(), 'asd_fm': fm.mean(),
            'assd': (mf.mean() + fm.mean()) / 2}


@pytest.fixture(scope="module")
def ops():
    from nemar_amd import ops
    return ops


def _lists(seed, n_mf, n_fm, top=B):
    rng = np.random.default_rng(seed)
    return rng.integers(0, top, n_mf), rng.integers(0, top, n_fm)


def test_against_numpy_on_the_expanded_lists(ops):
    """M = 3 samples x K = 3 classes, every pair defined, list lengths from 1 to 211 (percentile ranks that interpolate and that do not)"""
    M, K = 3, 3
    counts, hist = np.zeros((M, K, 2, 3), dtype=np.int64), np.zeros((M, K, 2, B), dtype=np.int64)
    want = [[None] * K for _ in range(M)]
    sizes = [(1, 1), (2, 1), (20, 21), (211, 190), (7, 100), (41, 1), (3, 3), (64, 64), (5, 16)]
    for i, (a, b) in enumerate(sizes):
        n, k = divmod(i, K)
        lists = _lists(i, a, b)
        counts[n, k], hist[n, k] = _pair(*lists)
        want[n][k] = _want(*lists)
    s = ops.surface_summary(counts, hist)
    assert s['classes'] == [0, 1, 2] and (s['pairs'], s['undefined'], s['far']) == (9, 0, 0)
    for k in range(K):
        assert s['per_class']['hd'][k] == np.mean([want[n][k]['hd'] for n in range(M)])              # exact: square roots of integers
        assert s['per_class']['hd95'][k] == np.mean([want[n][k]['hd95'] for n in range(M)])          # numpy's own interpolation
        for name in ('asd_mf', 'asd_fm', 'assd'):
            assert s['per_class'][name][k] == pytest.approx(np.mean([want[n][k][name] for n in range(M)]), rel=RTOL, abs=0)
    for name in ('hd', 'hd95', 'asd_mf', 'asd_fm', 'assd'):
        assert s['mean'][name] == pytest.approx(np.mean(s['per_class'][name]), rel=RTOL)
        assert s['mean_foreground'][name] == pytest.approx(np.mean(s['per_class'][name][1:]), rel=RTOL)       # class 0 reported, and left out here
    # tensors, and the batches of a data set concatenated, give the same numbers; the result is plain JSON
    t = ops.surface_summary(torch.from_numpy(counts), torch.from_numpy(hist).to(torch.int32))
    assert t == s and json.loads(json.dumps(s)) == s
    assert ops.surface_summary(np.concatenate([counts[:1], counts[1:]]), np.concatenate([hist[:1], hist[1:]])) == s


def test_the_far_tail(ops):
    """asd / assd are None exactly for a sample with far > 0; hd95 is None exactly when one of the two ranks numpy interpolates between
    lies beyond the histogram; hd stays exact"""
    near = np.full(99, 4)
    # (a) one far pixel among 200: ranks 0.95 * 199 = 189.05 -> 189 and 190 are both inside the histogram
    mf = np.concatenate([near, [B + 36]])
    c, h = _pair(mf, np.full(100, 9))
    s = ops.surface_summary(c[None, None], h[None, None])
    assert (s['pairs'], s['far']) == (1, 1)
    assert s['per_class']['assd'] == [None] and s['per_class']['asd_mf'] == [None] and s['per_class']['asd_fm'] == [None]
    assert s['per_class']['hd'] == [10.0]                                       # sqrt(64 + 36), from max_d2
    assert s['per_class']['hd95'] == [np.percentile(np.sqrt(np.concatenate([mf, np.full(100, 9)])), 95)] == [3.0]
    assert s['mean']['assd'] is None and s['mean']['hd95'] == 3.0
    # (b) 11 far of 200: rank 189 is the first far value -> None; (c) 10 far: rank 189 is the last near value, rank 190 far -> None;
    # (d) 9 far: both ranks near
    for n_far, known in ((11, False), (10, False), (9, True)):
        mf = np.concatenate([np.full(100 - n_far, 4), np.full(n_far, B + 1)])
        c, h = _pair(mf, np.full(100, 9))
        s = ops.surface_summary(c[None, None], h[None, None])
        assert (s['per_class']['hd95'] == [3.0]) if known else (s['per_class']['hd95'] == [None]), n_far
        assert s['per_class']['assd'] == [None] and s['far'] == 1
    # a far sample leaves the class's other samples their values
    c2, h2 = _pair(np.full(10, 1), np.full(10, 4))
    s = ops.surface_summary(np.stack([c, c2])[:, None], np.stack([h, h2])[:, None])
    assert (s['pairs'], s['far']) == (2, 1) and s['per_class']['assd'] == [1.5] and s['per_class']['hd'] == [(np.sqrt(B + 1) + 2.0) / 2]


def test_undefined_pairs_and_class_zero(ops):
    """a (sample, class) pair without boundary pixels in one of the maps is skipped and counted; a class defined nowhere reports None and
    is left out of the class means; class 0 is reported like any class and additionally left out of mean_foreground"""
    M, K = 2, 4
    counts, hist = np.zeros((M, K, 2, 3), dtype=np.int64), np.zeros((M, K, 2, B), dtype=np.int64)
    lists = {(0, 0): _lists(1, 30, 31), (1, 0): _lists(2, 12, 9), (0, 1): _lists(3, 5, 8), (1, 3): _lists(4, 17, 3)}
    for (n, k), l in lists.items():
        counts[n, k], hist[n, k] = _pair(*l)
    counts[1, 1, 0, 0] = 44                                   # class 1 of sample 1: a boundary in the moving map only
    s = ops.surface_summary(counts, hist)
    assert (s['pairs'], s['undefined'], s['far']) == (4, 4, 0)
    w = {nk: _want(*l) for nk, l in lists.items()}
    assert s['per_class']['hd'] == [(w[0, 0]['hd'] + w[1, 0]['hd']) / 2, w[0, 1]['hd'], None, w[1, 3]['hd']]
    assert s['per_class']['hd95'][2] is None and s['per_class']['assd'][2] is None
    for name in ('hd', 'hd95', 'assd'):
        per = s['per_class'][name]
        assert s['mean'][name] == pytest.approx(np.mean([per[0], per[1], per[3]]), rel=RTOL)
        assert s['mean_foreground'][name] == pytest.approx(np.mean([per[1], per[3]]), rel=RTOL)
    # nothing defined at all
    s = ops.surface_summary(np.zeros((1, 2, 2, 3), dtype=np.int64), np.zeros((1, 2, 2, 4), dtype=np.int64))
    assert (s['pairs'], s['undefined']) == (0, 2) and s['mean']['hd'] is None and s['mean_foreground']['hd95'] is None
