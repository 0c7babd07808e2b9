"""Normals by PCA over the k nearest (include/atvsnet_hip.h: atvs_cloud_normals) and point-to-plane registration over the TARGET's
normals (atvs_cloud_plane_moments_target, register_cloud.register normal_side='target'), restated with numpy float64, math.fsum and
numpy.linalg.eigh / lstsq.

normals: per row the samples d = double(points[idx]) - double(query) for idx >= 0; s = fsum(d), S_ab = fsum(d_a d_b);
c = samples (+ 1 with self_counts); C_ab = S_ab - s_a s_b / c; numpy.linalg.eigh; the eigenvector of the smallest eigenvalue.  The
zero normal (variation NaN): c < 3, a non-finite sample or query, an idx >= n, lambda_1 <= 1e-12 lambda_2.  The sign: towards the
row's viewpoint when n . (viewpoint - query) is not 0, else canonical (the component of largest magnitude, lowest index on ties,
positive).

The target side of tests/cloud_plane_restated.py: the same pair rule with the normal of the MATCHED target point, unrotated, and
J = [q x n, n, q . n].

Nothing here imports the product."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_knn_restated as KR  # noqa: E402
import cloud_plane_restated as PR  # noqa: E402
import cloud_register_restated as RR  # noqa: E402

RANK_RATIO = 1e-12
GAP_FLOOR = 1e-6           # rows with (lambda_1 - lambda_0) / lambda_2 below this are left out of the angle bar only
NORMAL_K, NORMAL_RADIUS = 16, 0.2          # the comparison's neighbourhoods


def canonical(v):
    """v with its component of largest magnitude (lowest index on ties) made positive."""
    v = np.asarray(v, np.float64)
    lead = int(np.argmax(np.abs(v)))                      # argmax returns the first of equals
    return -v if v[lead] < 0.0 else v


def covariance(points, query, row, self_counts):
    """One row -> (C (3,3) or None for the zero normal by the sample rules, c)."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    q = np.asarray(query, np.float32).astype(np.float64)
    row = [int(i) for i in row if int(i) >= 0]
    c = len(row) + (1 if self_counts else 0)
    if any(i >= len(points) for i in row) or not np.isfinite(q).all():
        return None, c
    d = points[row].astype(np.float64).reshape(-1, 3) - q
    if c < 3 or not np.isfinite(d).all():
        return None, c
    s = [math.fsum(d[:, a].tolist()) for a in range(3)]
    C = np.zeros((3, 3))
    for a in range(3):
        for b in range(a, 3):
            C[a, b] = C[b, a] = math.fsum((d[:, a] * d[:, b]).tolist()) - s[a] * s[b] / c
    return C, c


def normals(points, queries, idx, self_counts=False, viewpoints=None, view_of=None):
    """-> (normals (m,3) float64, variation (m,) float64, lam (m,3) float64 ascending, count (m,) int): zero rows have the zero
    normal and NaN variation and lam."""
    queries = np.asarray(queries, np.float32).reshape(-1, 3)
    idx = np.asarray(idx, np.int32).reshape(len(queries), -1)
    views = None if viewpoints is None else np.asarray(viewpoints, np.float64).reshape(-1, 3)
    m = len(queries)
    out, var, lam, count = np.zeros((m, 3)), np.full(m, np.nan), np.full((m, 3), np.nan), np.zeros(m, np.int64)
    for j in range(m):
        C, count[j] = covariance(points, queries[j], idx[j], self_counts)
        if C is None:
            continue
        w, V = np.linalg.eigh(C)
        if not np.isfinite(w).all() or w[1] <= RANK_RATIO * w[2]:
            continue
        n = V[:, 0]
        v = 0 if view_of is None else int(view_of[j])
        dot = 0.0
        if views is not None and 0 <= v < len(views):
            e = views[v] - queries[j].astype(np.float64)
            dot = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2]
        out[j] = -n if dot < 0.0 else (n if dot > 0.0 else canonical(n))
        var[j], lam[j] = w[0] / ((w[0] + w[1]) + w[2]), w
    return out, var, lam, count


def normals_plain(points, queries, idx, self_counts=False):
    """The same, unoriented, by a second formulation: Python floats one sample at a time, exact rational sums
    (fractions.Fraction), the eigenvector from numpy.linalg.svd of C.  -> normals (m,3) float64 in the canonical sign."""
    from fractions import Fraction
    points = np.asarray(points, np.float32).reshape(-1, 3)
    queries = np.asarray(queries, np.float32).reshape(-1, 3)
    out = np.zeros((len(queries), 3))
    for j, q in enumerate(queries):
        samples, bad = [], not all(math.isfinite(float(v)) for v in q)
        for i in idx[j]:
            i = int(i)
            if i < 0:
                continue
            if i >= len(points) or not all(math.isfinite(float(v)) for v in points[i]):
                bad = True
                continue
            samples.append([float(points[i, a]) - float(q[a]) for a in range(3)])
        c = len(samples) + (1 if self_counts else 0)
        if bad or c < 3:
            continue
        s = [float(sum(Fraction(d[a]) for d in samples)) for a in range(3)]
        C = np.array([[float(sum(Fraction(d[a] * d[b]) for d in samples)) - s[a] * s[b] / c for b in range(3)] for a in range(3)])
        U, w, _ = np.linalg.svd(C)
        if w[1] <= RANK_RATIO * w[0]:
            continue
        out[j] = canonical(U[:, 2])
    return out


def angle_bar(lam, count, S=128):
    """The bound on sin(angle) between the kernel's normal and the restated one, per row: 2^-22 (the float32 rounding of the
    components) + B 2^-53 (l0 + l1 + l2) / (l1 - l0), B = 2 (c + 3 + S): c + 3 roundings of the serial covariance sums and the
    centring, S the solver's stated backward error, both in units of 2^-53 |C|, doubled by Davis-Kahan."""
    lam, c = np.asarray(lam, np.float64), np.asarray(count, np.float64)
    B = 2.0 * (c + 3.0 + S)
    with np.errstate(divide='ignore', invalid='ignore'):
        return 2.0 ** -22 + B * 2.0 ** -53 * lam.sum(axis=1) / (lam[:, 1] - lam[:, 0]), B


def sin_angle(a, b):
    """|a x b| / (|a| |b|) per row: the sine of the angle between the lines of a and b (sign-blind)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(np.cross(a, b), axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


# ---- the target side of the point-to-plane step ------------------------------------------------------------------------------------

def plane_pairs(src, T, dst, dst_normals, idx, d2, trim=np.inf, pivot=(0, 0, 0)):
    """-> (q, g, n, r, J (k,7), d2 (k,)) of the pairs that take part: 0 <= idx < n, double(d2) <= trim * trim (NaN: no),
    dst_normals[idx] finite and (nx nx + ny ny) + nz nz > 0."""
    src, dst = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(dst, np.float32).reshape(-1, 3)
    nrm = np.asarray(dst_normals, np.float32).reshape(-1, 3)
    assert len(nrm) == len(dst)
    idx, d2 = np.asarray(idx, np.int32), np.asarray(d2, np.float32)
    T, p = np.asarray(T, np.float64), np.asarray(pivot, np.float64).reshape(3)
    with np.errstate(invalid='ignore', over='ignore'):
        keep = (idx >= 0) & (idx < len(dst)) & (d2.astype(np.float64) <= float(trim) * float(trim))
        nd = nrm[np.where(keep, idx, 0)].astype(np.float64).reshape(-1, 3) if len(dst) else np.zeros((len(idx), 3))
        keep &= np.isfinite(nd).all(axis=1) & ((nd[:, 0] * nd[:, 0] + nd[:, 1] * nd[:, 1]) + nd[:, 2] * nd[:, 2] > 0.0)
    s, n = src[keep].astype(np.float64), nd[keep]
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    q = np.stack([(((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * z) + T[k, 3]) - p[k] for k in range(3)], 1).reshape(-1, 3)
    g = (dst[idx[keep]].astype(np.float64) - p).reshape(-1, 3)
    e = q - g
    r = (e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2]
    J = np.stack([q[:, 1] * n[:, 2] - q[:, 2] * n[:, 1], q[:, 2] * n[:, 0] - q[:, 0] * n[:, 2], q[:, 0] * n[:, 1] - q[:, 1] * n[:, 0],
                  n[:, 0], n[:, 1], n[:, 2], (q[:, 0] * n[:, 0] + q[:, 1] * n[:, 1]) + q[:, 2] * n[:, 2]], 1).reshape(-1, 7)
    return q, g, n, r, J, d2[keep].astype(np.float64)


def plane_terms(src, T, dst, dst_normals, idx, d2, trim=np.inf, pivot=(0, 0, 0)):
    """-> (k,37) float64: per pair J_a J_b for a <= b row-major (28), J_a r (7), r r, double(d2)."""
    _, _, _, r, J, dd = plane_pairs(src, T, dst, dst_normals, idx, d2, trim, pivot)
    cols = [J[:, a] * J[:, b] for a in range(7) for b in range(a, 7)] + [J[:, a] * r for a in range(7)] + [r * r, dd]
    return np.stack(cols, 1).reshape(-1, 37)


def plane_moments(src, T, dst, dst_normals, idx, d2, trim=np.inf, pivot=(0, 0, 0)):
    """-> (count, sums (37,) by math.fsum, mags (37,) = math.fsum of the terms' magnitudes)."""
    t = plane_terms(src, T, dst, dst_normals, idx, d2, trim, pivot)
    sums = np.array([math.fsum(t[:, k].tolist()) for k in range(37)], np.float64)
    mags = np.array([math.fsum(np.abs(t[:, k]).tolist()) for k in range(37)], np.float64)
    return len(t), sums, mags


def register_plane_target(recon, gt, gt_normals, init=None, with_scale=False, distances=PR.STAGES, max_iterations=100, min_move=0.0):
    """cloud_plane_restated.register_plane over the target's normals: the same loop, stop rule and least-squares step
    (PR.motion_from_points) with the rows above.  -> (T, [(iterations, pairs)] per stage)."""
    recon, gt = np.asarray(recon, np.float32).reshape(-1, 3), np.asarray(gt, np.float32).reshape(-1, 3)
    T = np.eye(4) if init is None else np.array(init, np.float64).reshape(4, 4)
    corners = RR.corners_of(recon)
    lo, hi = PR.box(gt)
    pivot = (lo + hi) / 2.0
    stages = []
    for rad in distances:
        its, pairs = 0, 0
        for _ in range(max_iterations):
            d2, idx = RR.nearest(RR.transform(recon, T), gt, rad)
            _, _, _, r, J, _ = plane_pairs(recon, T, gt, gt_normals, idx, d2, np.inf, pivot)
            pairs = len(r)
            if pairs < 3:
                raise ValueError('%d pairs within %g' % (pairs, rad))
            T_new = PR.motion_from_points(J, r, pivot, with_scale) @ T
            d = (corners @ T_new[:3, :3].T + T_new[:3, 3]) - (corners @ T[:3, :3].T + T[:3, 3])
            T, its = T_new, its + 1
            if float(np.sqrt((d * d).sum(axis=1)).max()) <= (1e-3 * rad if min_move is None else min_move):
                break
        stages.append((its, pairs))
    return T, stages


def self_normals(cloud, k=NORMAL_K, radius=NORMAL_RADIUS):
    """The cloud's own normals as register estimates them: the k nearest OTHERS within the radius, the point itself counted,
    unoriented.  -> (normals float32 (n,3), variation, lam, count, idx)."""
    cloud = np.asarray(cloud, np.float32).reshape(-1, 3)
    idx = KR.knn(cloud, cloud, radius, k, exclude_same_index=True)[1]
    n, var, lam, count = normals(cloud, cloud, idx, self_counts=True)
    return n.astype(np.float32), var, lam, count, idx


@functools.lru_cache(maxsize=None)
def comparison_normals():
    """The restated PCA normals of the comparison pair's ground truth (k = 16, radius 0.2) -> self_normals' tuple; computed once per
    process, read-only."""
    return self_normals(PR.comparison_pair()[0])


@functools.lru_cache(maxsize=None)
def comparison_plane_target():
    """The restated target-side loop on the comparison's pair with those normals, under the comparison's stop rule -> (T, stages)."""
    gt, src, _, _ = PR.comparison_pair()
    return register_plane_target(src, gt, comparison_normals()[0], distances=PR.STAGES, max_iterations=100, min_move=PR.MIN_MOVE)
