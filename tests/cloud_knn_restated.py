"""The neighbourhood kernels' definitions restated with numpy and Python numbers (include/atvsnet_hip.h, csrc/cloud_knn.hip): brute
force, no grid.

A candidate of query j is every finite reference point i, except i == j under exclude_same_index.  d2 is cloud_restated's float32
expression.  A candidate is kept when double(d2) <= double(R) * double(R); kept candidates are ordered by (bits(d2), i) ascending.
knn: the first k of that order, padded with (+inf, -1).  radius_count: how many are kept.  knn_mean: Python float additions of
sqrt(double(d2)) in ascending t, divided by k; +inf for a row with a padded entry.  sor_stats: math.fsum.  clean: the steps of
atvsnet/clean_cloud.py over these.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_register_restated as RR  # noqa: E402


def _d2_block(q, Pk):
    with np.errstate(over='ignore', invalid='ignore'):
        dx, dy, dz = q[:, 0:1] - Pk[:, 0][None, :], q[:, 1:2] - Pk[:, 1][None, :], q[:, 2:3] - Pk[:, 2][None, :]
        d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == np.float32
    return d


def _blocks(Q, P, R, exclude_same_index, chunk_elems=1 << 23):
    """Yields (first row, d2 (rows, finite reference points) float32, kept (the same shape) bool, the finite reference points'
    indices) over slices of Q."""
    Q = np.ascontiguousarray(Q, np.float32).reshape(-1, 3)
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
    if exclude_same_index:
        assert len(Q) == len(P)
    keep = np.flatnonzero(np.isfinite(P).all(axis=1))
    r2 = float(np.float32(R)) * float(np.float32(R))
    Pk = P[keep]
    rows = max(1, chunk_elems // max(1, len(Pk)))
    for s in range(0, len(Q), rows):
        q = Q[s:s + rows]
        d = _d2_block(q, Pk)
        ok = np.isfinite(q).all(axis=1)[:, None] & (d.astype(np.float64) <= r2)
        if exclude_same_index:
            ok &= keep[None, :] != (s + np.arange(len(q)))[:, None]
        yield s, d, ok, keep


def knn(Q, P, R, k, exclude_same_index=False):
    """-> (d2 (m,k) float32, idx (m,k) int32)"""
    m = len(np.asarray(Q).reshape(-1, 3))
    d2 = np.full((m, k), np.inf, np.float32)
    idx = np.full((m, k), -1, np.int32)
    for s, d, ok, keep in _blocks(Q, P, R, exclude_same_index):
        r, c = np.nonzero(ok)                                              # the kept candidates, row by row
        kept = (d[r, c].view(np.uint32).astype(np.uint64) << np.uint64(32)) | keep[c].astype(np.uint64)
        order = np.lexsort((kept, r))                                      # by row, then by (bits(d2), index)
        r, kept = r[order], kept[order]
        rank = np.arange(len(r)) - np.searchsorted(r, np.arange(len(d)))[r]
        first = rank < k
        r, rank, kept = r[first], rank[first], kept[first]
        d2[s + r, rank] = (kept >> np.uint64(32)).astype(np.uint32).view(np.float32)
        idx[s + r, rank] = (kept & np.uint64(0xffffffff)).astype(np.int32)
    return d2, idx


def knn_by_tuples(Q, P, R, k, exclude_same_index=False):
    """The same by a second formulation: per query a Python list of (bits(d2), index) tuples, sorted."""
    Q = np.asarray(Q, np.float32).reshape(-1, 3)
    P = np.asarray(P, np.float32).reshape(-1, 3)
    r2 = float(np.float32(R)) * float(np.float32(R))
    d2 = np.full((len(Q), k), np.inf, np.float32)
    idx = np.full((len(Q), k), -1, np.int32)
    for j, q in enumerate(Q):
        if not np.isfinite(q).all():
            continue
        cand = []
        for i, p in enumerate(P):
            if not np.isfinite(p).all() or (exclude_same_index and i == j):
                continue
            with np.errstate(over='ignore'):
                dx, dy, dz = q[0] - p[0], q[1] - p[1], q[2] - p[2]
                d = np.float32(np.float32(dx * dx + dy * dy) + dz * dz)
            if float(d) <= r2:
                cand.append((int(np.float32(d).view(np.uint32)), i))
        for t, (bits, i) in enumerate(sorted(cand)[:k]):
            d2[j, t] = np.uint32(bits).view(np.float32)
            idx[j, t] = i
    return d2, idx


def radius_count(Q, P, R, exclude_same_index=False):
    """-> count (m,) int32"""
    m = len(np.asarray(Q).reshape(-1, 3))
    out = np.zeros(m, np.int32)
    for s, _, ok, _ in _blocks(Q, P, R, exclude_same_index):
        out[s:s + len(ok)] = ok.sum(axis=1)
    return out


def knn_mean(d2):
    """d2 (m,k) float32 -> s (m,) float64"""
    d2 = np.asarray(d2, np.float32)
    m, k = d2.shape
    root = np.sqrt(d2.astype(np.float64))
    s = np.zeros(m, np.float64)
    for t in range(k):                       # ascending t, one rounded float64 addition each (what a Python float loop does)
        s = s + root[:, t]
    s = s / float(k)
    s[~np.isfinite(d2).all(axis=1)] = np.inf
    return s


def sor_stats(s):
    """-> (count, mean, std, (sum |s|, sum (s - mean)^2) by math.fsum): over the finite entries; std with count - 1 below the root."""
    s = np.asarray(s, np.float64)
    f = s[np.isfinite(s)].tolist()
    c = len(f)
    mean = math.fsum(f) / c if c else 0.0
    dev = math.fsum((x - mean) * (x - mean) for x in f)
    std = math.sqrt(dev / (c - 1)) if c >= 2 else 0.0
    return c, mean, std, (math.fsum(abs(x) for x in f), dev)


def clean(points, colors=None, voxel=None, sor=None, radius_filter=None, detail=None):
    """clean_cloud.clean restated -> (points, colors, kept: the surviving rows' indices into the input).  detail: a dict that
    receives the sor step's s, threshold and the rows it saw."""
    p = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
    rows = np.arange(len(p))
    if voxel is not None:
        ok = p[np.isfinite(p).all(axis=1)]
        origin = np.floor(ok.astype(np.float64).min(axis=0)) if len(ok) else np.zeros(3)
        p, first = RR.voxel_downsample(p, voxel, origin)
        rows = rows[first]
    if sor is not None:
        k, ratio, radius = sor
        s = knn_mean(knn(p, p, radius, k, exclude_same_index=True)[0])
        c, mean, std, _ = sor_stats(s)
        threshold = mean + ratio * std
        if detail is not None:
            detail.update(s=s, threshold=threshold, rows=rows.copy(), count=c, mean=mean, std=std)
        keep = s <= threshold
        p, rows = p[keep], rows[keep]
    if radius_filter is not None:
        radius, least = radius_filter
        keep = radius_count(p, p, radius, exclude_same_index=True) >= least
        p, rows = p[keep], rows[keep]
    return p, (None if colors is None else np.asarray(colors)[rows]), rows
