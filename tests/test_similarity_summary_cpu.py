"""ops.similarity_summary: the host-side float64 arithmetic on nemar_joint_histogram's tables and sums (no GPU, no kernel)."""
import numpy as np
import pytest
import torch

from nemar_amd import ops


def _moments(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.array([[a.sum(), b.sum(), (a * a).sum(), (b * b).sum(), (a * b).sum(), np.abs(a - b).sum()]])


def test_independent_marginals_have_no_mutual_information():
    p, q = np.array([3, 1, 4, 2]), np.array([5, 9, 2, 6])
    s = ops.similarity_summary(np.outer(p, q)[None])
    assert s['valid'] == int(p.sum() * q.sum()) and isinstance(s['valid'], int)
    assert abs(s['mi']) <= 1e-12
    assert s['entropy_joint'] == pytest.approx(s['entropy_moving'] + s['entropy_fixed'], abs=1e-12) and s['nmi'] == pytest.approx(1.0, abs=1e-12)
    pm = p / p.sum()
    assert s['entropy_moving'] == pytest.approx(-(pm * np.log(pm)).sum(), abs=1e-12)      # rows are the moving image's bins
    assert 'ncc' not in s                                                                   # no moments were given


@pytest.mark.parametrize("B", [2, 32, 64])
def test_uniform_diagonal_table(B):
    s = ops.similarity_summary((7 * np.eye(B, dtype=np.int64))[None])
    assert s['valid'] == 7 * B
    assert s['mi'] == pytest.approx(np.log(B), abs=1e-12) and s['nmi'] == pytest.approx(2.0, abs=1e-12)


def test_moments_reproduce_numpy():
    rng = np.random.default_rng(0)
    a = rng.random(500)
    b = 0.3 * a * a + 0.1 * rng.random(500)
    table = np.zeros((1, 4, 4), dtype=np.int64)
    table[0, 1, 2], table[0, 2, 1] = 300, 200                        # (only its sum, the number of counted pixels, matters to the moments)
    s = ops.similarity_summary(table, _moments(a, b))
    assert s['ncc'] == pytest.approx(np.corrcoef(a, b)[0, 1], abs=1e-10)
    assert s['mse'] == pytest.approx(((a - b) ** 2).mean(), abs=1e-12)
    assert s['mae'] == pytest.approx(np.abs(a - b).mean(), abs=1e-12)
    assert all(isinstance(s[k], float) for k in ('ncc', 'mse', 'mae', 'mi', 'nmi', 'entropy_joint'))


def test_nothing_to_divide_by_is_none():
    s = ops.similarity_summary(np.zeros((2, 8, 8), dtype=np.int64), np.zeros((2, 6)))
    assert s['valid'] == 0
    assert all(s[k] is None for k in ('entropy_moving', 'entropy_fixed', 'entropy_joint', 'mi', 'nmi', 'ncc', 'mse', 'mae'))
    one_cell = np.zeros((1, 8, 8), dtype=np.int64)
    one_cell[0, 3, 5] = 40                                           # every pixel in one cell: zero joint entropy
    a = np.full(40, 0.5)
    s = ops.similarity_summary(one_cell, _moments(a, a + 0.25))      # constant images: zero variance
    assert s['valid'] == 40 and s['entropy_joint'] == 0 and s['mi'] == 0 and s['nmi'] is None
    assert s['ncc'] is None and s['mse'] == 0.0625 and s['mae'] == 0.25
    b = np.linspace(0, 1, 40)
    assert ops.similarity_summary(one_cell, _moments(a, b))['ncc'] is None      # one side constant


def test_batches_concatenate_tables_and_sums_are_added_then_divided():
    rng = np.random.default_rng(1)
    tables = rng.integers(0, 50, (5, 6, 6))
    vecs = [(rng.random(n), rng.random(n)) for n in tables.reshape(5, -1).sum(1)]
    moments = np.concatenate([_moments(a, b) for a, b in vecs])
    whole = ops.similarity_summary(tables, moments)
    parts = ops.similarity_summary(np.concatenate([tables[:2], tables[2:]]), np.concatenate([moments[:2], moments[2:]]))
    assert whole == parts
    assert whole == ops.similarity_summary(tables.sum(0, keepdims=True), moments.sum(0, keepdims=True))
    a, b = np.concatenate([v[0] for v in vecs]), np.concatenate([v[1] for v in vecs])
    assert whole['valid'] == a.size and whole['ncc'] == pytest.approx(np.corrcoef(a, b)[0, 1], abs=1e-9)
    assert whole['mae'] == pytest.approx(np.abs(a - b).mean(), abs=1e-12)
    # torch tensors (what ops.joint_histogram returns, brought to the host or not) are taken as well
    assert ops.similarity_summary(torch.from_numpy(tables), torch.from_numpy(moments.astype(np.float32))) == \
        ops.similarity_summary(tables, moments.astype(np.float32))
