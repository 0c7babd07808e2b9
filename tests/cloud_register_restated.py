"""The registration kernels' definitions (include/atvsnet_hip.h, csrc/cloud_register.hip) restated with numpy and Python integers,
the ICP loop of atvsnet/register_cloud.py restated over cloud_restated.nearest, and a test shape without symmetry.

Nothing here imports the product: the fit is Umeyama's closed form from explicit, centred correspondences (the product fits from
18 sums), the sums are exact (math.fsum / Python integers)."""
import math
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_restated as CR  # noqa: E402


def transform(points, T):
    """Per coordinate k, in float64: ((T[k][0] x + T[k][1] y) + T[k][2] z) + T[k][3], rounded once to float32."""
    T = np.asarray(T, np.float64)
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(over='ignore', invalid='ignore'):
        return np.stack([(((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * z) + T[k, 3]) for k in range(3)], 1).astype(np.float32)


def pair_terms(src, dst, idx, d2, trim=np.inf, pivot_src=(0, 0, 0), pivot_dst=(0, 0, 0)):
    """-> (k,18) float64: the 18 terms of every pair that takes part (0 <= idx < n and double(d2) <= trim * trim), formed as the
    header states them: a = double(src) - pivot_src, b = double(dst[idx]) - pivot_dst; a (3), b (3), a_r * b_c (9),
    (a0 a0 + a1 a1) + a2 a2, (b0 b0 + b1 b1) + b2 b2, double(d2)."""
    src, dst = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(dst, np.float32).reshape(-1, 3)
    idx, d2 = np.asarray(idx, np.int32), np.asarray(d2, np.float32)
    with np.errstate(invalid='ignore'):
        keep = (idx >= 0) & (idx < len(dst)) & (d2.astype(np.float64) <= float(trim) * float(trim))
    a = src[keep].astype(np.float64) - np.asarray(pivot_src, np.float64)
    b = dst[idx[keep]].astype(np.float64) - np.asarray(pivot_dst, np.float64)
    cross = [a[:, r] * b[:, c] for r in range(3) for c in range(3)]
    aa = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    bb = (b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2]
    cols = [a[:, 0], a[:, 1], a[:, 2], b[:, 0], b[:, 1], b[:, 2]] + cross + [aa, bb, d2[keep].astype(np.float64)]
    return np.stack(cols, 1).reshape(-1, 18)


def pair_moments(src, dst, idx, d2, trim=np.inf, pivot_src=(0, 0, 0), pivot_dst=(0, 0, 0)):
    """-> (count, sums (18,) float64 = math.fsum of every column of pair_terms, abs (18,) = math.fsum of their magnitudes)."""
    t = pair_terms(src, dst, idx, d2, trim, pivot_src, pivot_dst)
    sums = np.array([math.fsum(t[:, k].tolist()) for k in range(18)], np.float64)
    mags = np.array([math.fsum(np.abs(t[:, k]).tolist()) for k in range(18)], np.float64)
    return len(t), sums, mags


CELL_LIMIT = 1 << 21


def voxel_downsample(points, voxel, origin):
    """-> (means (k,3) float32, first (k,) int32), in ascending order of each voxel's lowest original index.  Per axis, in
    float64: g = (double(x) - origin) / voxel, c = floor(g), u = int(floor((g - c) * 2^32)) clamped to 2^32 - 1; per voxel the
    Python-integer sum S of u and the count k; mean = origin + voxel * (c + (double(S) / double(k)) / 2^32), rounded once to
    float32.  Non-finite points are dropped; a cell outside [0, 2^21) raises ValueError."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    origin = np.asarray(origin, np.float64).reshape(3)
    voxel = float(voxel)
    ok = np.isfinite(p).all(axis=1)
    with np.errstate(over='ignore', invalid='ignore'):
        g = (p.astype(np.float64) - origin) / voxel
    c = np.floor(g)
    if ((c[ok] < 0) | (c[ok] >= CELL_LIMIT)).any():
        raise ValueError('a cell coordinate leaves [0, 2^21)')
    with np.errstate(invalid='ignore'):
        u = np.minimum(np.floor((g - c) * 4294967296.0), 4294967295.0)
    voxels = {}                                        # cell -> [first index, count, Sx, Sy, Sz]; dicts keep insertion order
    for i in np.flatnonzero(ok).tolist():
        key = (int(c[i, 0]), int(c[i, 1]), int(c[i, 2]))
        v = voxels.get(key)
        if v is None:
            v = voxels[key] = [i, 0, 0, 0, 0]
        v[1] += 1
        v[2] += int(u[i, 0])
        v[3] += int(u[i, 1])
        v[4] += int(u[i, 2])
    means = np.zeros((len(voxels), 3), np.float32)
    first = np.zeros(len(voxels), np.int32)
    for j, (key, v) in enumerate(voxels.items()):
        first[j] = v[0]
        for a in range(3):
            frac = (float(v[2 + a]) / float(v[1])) / 4294967296.0
            means[j, a] = np.float32(origin[a] + voxel * (float(key[a]) + frac))
    return means, first


def nearest(Q, P, R, threads=None):
    """cloud_restated.nearest over slices of the queries in threads (numpy releases the lock): the same result, per query."""
    Q = np.ascontiguousarray(Q, np.float32).reshape(-1, 3)
    threads = threads or max(1, min(16, os.cpu_count() or 1))
    if len(Q) < 2048 or threads == 1:
        return CR.nearest(Q, P, R)
    parts = np.array_split(np.arange(len(Q)), threads * 4)
    with ThreadPoolExecutor(threads) as pool:
        res = list(pool.map(lambda s: CR.nearest(Q[s], P, R, chunk_elems=1 << 21), parts))
    return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])


def fit(P, Q, with_scale):
    """Umeyama: the least-squares Q ~ s R P + t from explicit pairs (float64), never a reflection -> 4x4."""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    mp, mq = P.mean(axis=0), Q.mean(axis=0)
    X, Y = P - mp, Q - mq
    H = Y.T @ X / len(P)
    U, D, Vt = np.linalg.svd(H)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    s = float(np.trace(np.diag(D) @ S) / (X * X).sum(axis=1).mean()) if with_scale else 1.0
    T = np.eye(4)
    T[:3, :3] = s * R
    T[:3, 3] = mq - s * (R @ mp)
    return T


def corners_of(points):
    p = np.asarray(points, np.float32).reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)].astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    return np.array([[(lo, hi)[(c >> k) & 1][k] for k in range(3)] for c in range(8)])


def icp(recon, gt, init=None, with_scale=False, distances=(0.2, 0.1, 0.05), max_iterations=100, min_move=0.0):
    """The loop of register_cloud.register with voxel = 0: per stage distance r, repeat { q = transform(recon, T); nearest within
    r; T = fit(original recon -> matched gt) } until the corners of recon's box move by at most min_move.
    -> (T, [(iterations, pairs)] per stage)."""
    recon, gt = np.asarray(recon, np.float32).reshape(-1, 3), np.asarray(gt, np.float32).reshape(-1, 3)
    T = np.eye(4) if init is None else np.array(init, np.float64).reshape(4, 4)
    corners = corners_of(recon)
    stages = []
    for r in distances:
        its, pairs = 0, 0
        for _ in range(max_iterations):
            d2, idx = nearest(transform(recon, T), gt, r)
            keep = idx >= 0
            pairs = int(keep.sum())
            if pairs < 3:
                raise ValueError('%d pairs within %g' % (pairs, r))
            T_new = fit(recon[keep].astype(np.float64), gt[idx[keep]].astype(np.float64), with_scale)
            d = (corners @ T_new[:3, :3].T + T_new[:3, 3]) - (corners @ T[:3, :3].T + T[:3, 3])
            T, its = T_new, its + 1
            if float(np.sqrt((d * d).sum(axis=1)).max()) <= min_move:
                break
        stages.append((its, pairs))
    return T, stages


def shape(n, seed, noise=0.0):
    """n float64 points on a shape without symmetry: three unequal wall patches meeting in a corner (2.0 x 1.2 floor, 2.0 x 0.8 and
    1.2 x 0.8 walls) and a half-ball of radius 0.25 standing on the floor at (1.3, 0.4, 0); Gaussian noise of sigma `noise`."""
    rng = np.random.default_rng(seed)
    areas = np.array([2.0 * 1.2, 2.0 * 0.8, 1.2 * 0.8, 2.0 * np.pi * 0.25 ** 2])
    part = rng.choice(4, size=n, p=areas / areas.sum())
    u, v = rng.uniform(size=n), rng.uniform(size=n)
    p = np.zeros((n, 3))
    k = part == 0
    p[k] = np.stack([2.0 * u[k], 1.2 * v[k], np.zeros(k.sum())], 1)
    k = part == 1
    p[k] = np.stack([2.0 * u[k], np.zeros(k.sum()), 0.8 * v[k]], 1)
    k = part == 2
    p[k] = np.stack([np.zeros(k.sum()), 1.2 * u[k], 0.8 * v[k]], 1)
    k = part == 3
    d = rng.normal(size=(int(k.sum()), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:, 2] = np.abs(d[:, 2])
    p[k] = np.array([1.3, 0.4, 0.0]) + 0.25 * d
    if noise:
        p += rng.normal(0.0, noise, p.shape)
    return p


def rotation(axis, degrees):
    """Rodrigues: the rotation by `degrees` about `axis`."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(degrees)
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


def similarity(R, t, s=1.0, centre=(0, 0, 0)):
    """4x4 of x -> s R (x - centre) + centre + t."""
    c = np.asarray(centre, np.float64)
    T = np.eye(4)
    T[:3, :3] = s * np.asarray(R, np.float64)
    T[:3, 3] = c + np.asarray(t, np.float64) - T[:3, :3] @ c
    return T


def moved_pair(shift=(0, 0, 0), scale=1.0, n_gt=40000, n_src=15000, seed=7):
    """The ground truth (n_gt,3) float32 at `shift`, a source (n_src,3) float32 that is an exact subset of it moved by the INVERSE
    of M = (rotation of 4 degrees about (1,2,3) through the centroid, translation (0.06, -0.04, 0.05), `scale`) and rounded to
    float32, the subset's indices, and M: M moves the source back onto its partners."""
    gt = (shape(n_gt, seed) + np.asarray(shift, np.float64)).astype(np.float32)
    pick = np.random.default_rng(seed + 1).permutation(n_gt)[:n_src]
    g = gt.astype(np.float64)
    M = similarity(rotation((1, 2, 3), 4.0), (0.06, -0.04, 0.05), scale, g.mean(axis=0))
    Mi = np.linalg.inv(M)
    src = (g[pick] @ Mi[:3, :3].T + Mi[:3, 3]).astype(np.float32)
    return gt, src, pick, M


def ulp_bar(gt):
    """2 ulp(float32) of the largest coordinate magnitude of the ground truth."""
    return 2.0 * float(np.spacing(np.float32(np.abs(np.asarray(gt, np.float32)).max())))
