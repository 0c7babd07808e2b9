"""-m gpu: the three kernels of the global registration (csrc/cloud_features.hip: atvs_cloud_fpfh, atvs_cloud_feature_nearest;
csrc/cloud_ransac.hip: atvs_cloud_ransac_score; ops/cloud.py) held to tests/cloud_global_restated.py.

cloud_fpfh: the zero rows exactly, every part's sum within 2^-22 of 1, every other entry within the float32-rounding bar the
restatement derives from the operation counts (GR.FPFH_BAR), rows with a pair near a bin edge left out (at most 1 %).
cloud_feature_nearest and cloud_ransac: bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd                                   # noqa: F401
from atvsnet_amd import ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_global_restated as GR  # noqa: E402

pytestmark = pytest.mark.gpu


def _up(dev, a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize('case', ['plane', 'room', 'sphere', 'sparse', 'edited'])
def test_fpfh_equals_the_restatement(cuda, case):
    pts, k, radius = GR.fpfh_case(case)
    dev = _up(cuda, pts)
    idx = ops.cloud_knn(ops.cloud_grid(dev, radius), dev, k, exclude_same_index=True)[1]
    nrm = ops.cloud_normals(dev, dev, idx, self_counts=True)
    idx, nrm = GR.fpfh_edits(case, idx.cpu().numpy(), nrm.cpu().numpy())
    args = (dev, _up(cuda, idx, np.int32), _up(cuda, nrm))
    got, again = ops.cloud_fpfh(*args).cpu().numpy(), ops.cloud_fpfh(*args).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (len(pts), 33) and _bits(got) == _bits(again)
    want, near = GR.fpfh(pts, idx, nrm)
    zero = ~want.any(axis=1)
    assert np.array_equal(~got.any(axis=1), zero) and _bits(got[zero]) == _bits(np.zeros((int(zero.sum()), 33), np.float32))
    padded = int((idx < 0).any(axis=1).sum())
    print('%s: %d rows, %d zero, %d with padding, %d near an edge' % (case, len(pts), zero.sum(), padded, near.sum()))
    if case == 'sparse':
        assert 2 * padded > len(pts) and 0 < zero.sum() < len(pts)
    if case == 'edited':
        assert zero[7] and zero[::17].all() and zero[5] and zero[6] and not zero.all()
    else:
        assert (~zero).sum() >= 0.5 * len(pts) or case == 'sparse'
    assert np.isfinite(got).all() and (got >= 0).all()
    parts = got[~zero].astype(np.float64).reshape(-1, 3, 11).sum(axis=2)
    assert np.abs(parts - 1.0).max() <= GR.PART_SUM_BAR
    assert near.sum() <= 0.01 * len(pts)
    held = ~zero & ~near
    err = np.abs(got[held].astype(np.float64) - want[held].astype(np.float64)).max()
    print('largest difference %.3e, the bar %.3e' % (err, GR.FPFH_BAR))
    assert err <= GR.FPFH_BAR


@pytest.mark.parametrize('n,m', [(1, 1), (257, 4097), (4097, 65)])
def test_feature_nearest_is_the_restatement_bit_for_bit(cuda, n, m):
    ref, query = GR.features(n, 1), GR.features(m, 2)
    if n > 16 and m > 16:
        query[8] = ref[n // 2]                               # an exact hit on a duplicated row
        query[9] = ref[n - 1]
    d2, idx = (t.cpu().numpy() for t in ops.cloud_feature_nearest(_up(cuda, ref), _up(cuda, query)))
    again = ops.cloud_feature_nearest(_up(cuda, ref), _up(cuda, query))
    want_d2, want_idx = GR.feature_nearest(ref, query)
    assert d2.dtype == np.float32 and idx.dtype == np.int32 and d2.shape == idx.shape == (m,)
    assert _bits(idx) == _bits(want_idx) and _bits(d2) == _bits(want_d2)
    assert _bits(again[0].cpu().numpy()) == _bits(d2) and _bits(again[1].cpu().numpy()) == _bits(idx)
    zero_q = ~query.any(axis=1)
    assert (idx[zero_q] == -1).all() and np.isinf(d2[zero_q]).all() and (idx[~zero_q] >= 0).all()
    assert ref[idx[~zero_q]].any(axis=1).all()                   # a zero reference row is never a match
    if n > 16 and m > 16:
        assert idx[8] == 3 and idx[9] == 3 and d2[8] == 0.0
    # a cloud against itself: every row that is not zero finds itself (the lowest of its duplicates) at distance 0
    plain = GR.features(max(n, m), 3)
    first = np.array([int(np.flatnonzero((plain == row).all(axis=1))[0]) for row in plain])
    d2, idx = (t.cpu().numpy() for t in ops.cloud_feature_nearest(_up(cuda, plain), _up(cuda, plain)))
    live = plain.any(axis=1)
    assert np.array_equal(idx[live], first[live]) and (d2[live] == 0.0).all() and (idx[~live] == -1).all()
    # no reference row at all, and only zero ones
    for empty in (np.zeros((0, 33), np.float32), np.zeros((3, 33), np.float32)):
        d2, idx = (t.cpu().numpy() for t in ops.cloud_feature_nearest(_up(cuda, empty), _up(cuda, query)))
        assert (idx == -1).all() and np.isinf(d2).all()


@pytest.mark.parametrize('with_scale', [False, True])
@pytest.mark.parametrize('c,h', [(3, 1), (3, 65), (257, 65), (257, 4097), (4097, 65), (4097, 4097)])
def test_ransac_is_the_restatement_bit_for_bit(cuda, c, h, with_scale):
    src, dst, triples, tau, planted, M = GR.ransac_case(c, h, with_scale)
    args = (_up(cuda, src), _up(cuda, dst), _up(cuda, triples, np.int32), tau, with_scale)
    _, valid, reason = GR.hypotheses(src, dst, triples, with_scale)
    if h >= 65:
        assert 'index' in reason and (c == 3 or {'edge', 'area', 'ratio'} <= set(reason.tolist()))      # every rule is exercised
    for best in (1, 8):
        got, again = ops.cloud_ransac(*args, best=best), ops.cloud_ransac(*args, best=best)
        want, counts, _ = GR.ransac(src, dst, triples, tau, with_scale, best=best)
        assert len(got) == best == len(want)
        for g, a, w in zip(got, again, want):
            assert (g['count'], g['index']) == (w['count'], w['index'])                          # counts and order: exact
            assert _bits(np.float64(g['sum'])) == _bits(np.float64(w['sum'])) and _bits(g['matrix']) == _bits(w['matrix'])
            assert (g['count'], g['index'], _bits(np.float64(g['sum'])), _bits(g['matrix'])) == (
                a['count'], a['index'], _bits(np.float64(a['sum'])), _bits(a['matrix']))
        n_valid = int(valid.sum())
        assert [g['index'] for g in got[n_valid:]] == [-1] * max(0, best - n_valid)               # best beyond the valid ones
        assert all(g['count'] == -1 and not g['matrix'].any() for g in got[n_valid:])
    # the hypothesis through three planted inliers wins, with the planted count
    assert got[0]['count'] == planted and valid[0] and counts[0] == planted
    T = np.vstack([got[0]['matrix'], [0, 0, 0, 1]])
    assert np.abs(T - M).max() <= 1e-5
    if h == 1:
        assert [g['index'] for g in got] == [0] + [-1] * 7
