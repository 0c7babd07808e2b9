"""The point-to-plane moments (include/atvsnet_hip.h: atvs_cloud_plane_moments) restated with numpy float64 and math.fsum, an
independent Gauss-Newton step from explicit per-pair Jacobians (numpy.linalg.lstsq; the product solves normal equations built from
37 sums), the point-to-plane loop of atvsnet/register_cloud.py restated over cloud_restated.nearest, and the test shape of
tests/cloud_register_restated.py with its analytic normals.

Nothing here imports the product."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_register_restated as RR  # noqa: E402

STAGES = (0.2, 0.1, 0.05)
MIN_MOVE = 1e-6          # the comparison's stop rule for both loops: the box corners move by at most a micrometre on a 2 m shape


def rotation_of(T):
    """The pure rotation of a similarity T: its 3x3 block divided by the cube root of its determinant (what ops.cloud_plane_moments
    hands the kernel as rot9)."""
    A = np.asarray(T, np.float64)[:3, :3]
    return A / np.cbrt(float(np.linalg.det(A)))


def plane_pairs(src, normals, T, dst, idx, d2, trim=np.inf, pivot=(0, 0, 0)):
    """The pairs that take part and their quantities, per pair in float64 in the stated order -> (q, g, n', r, J (k,7), d2 (k,)).
    Takes part: 0 <= idx < n, double(d2) <= trim * trim (NaN: no), the normal finite and (nx nx + ny ny) + nz nz > 0."""
    src, dst = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(dst, np.float32).reshape(-1, 3)
    nrm = np.asarray(normals, np.float32).reshape(-1, 3)
    idx, d2 = np.asarray(idx, np.int32), np.asarray(d2, np.float32)
    T, R, p = np.asarray(T, np.float64), rotation_of(T), np.asarray(pivot, np.float64).reshape(3)
    with np.errstate(invalid='ignore', over='ignore'):
        nd = nrm.astype(np.float64)
        keep = (idx >= 0) & (idx < len(dst)) & (d2.astype(np.float64) <= float(trim) * float(trim))
        keep &= np.isfinite(nrm).all(axis=1) & ((nd[:, 0] * nd[:, 0] + nd[:, 1] * nd[:, 1]) + nd[:, 2] * nd[:, 2] > 0.0)
    s, nd = src[keep].astype(np.float64), nd[keep]
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    q = np.stack([(((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * z) + T[k, 3]) - p[k] for k in range(3)], 1).reshape(-1, 3)
    g = (dst[idx[keep]].astype(np.float64) - p).reshape(-1, 3)
    n = np.stack([(R[k, 0] * nd[:, 0] + R[k, 1] * nd[:, 1]) + R[k, 2] * nd[:, 2] for k in range(3)], 1).reshape(-1, 3)
    e = q - g
    r = (e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2]
    J = np.stack([g[:, 1] * n[:, 2] - g[:, 2] * n[:, 1], g[:, 2] * n[:, 0] - g[:, 0] * n[:, 2], g[:, 0] * n[:, 1] - g[:, 1] * n[:, 0],
                  n[:, 0], n[:, 1], n[:, 2], (q[:, 0] * n[:, 0] + q[:, 1] * n[:, 1]) + q[:, 2] * n[:, 2]], 1).reshape(-1, 7)
    return q, g, n, r, J, d2[keep].astype(np.float64)


def plane_terms(src, normals, T, dst, idx, d2, trim=np.inf, pivot=(0, 0, 0)):
    """-> (k,37) float64: per pair J_a J_b for a <= b row-major (28), J_a r (7), r r, double(d2)."""
    _, _, _, r, J, dd = plane_pairs(src, normals, T, dst, idx, d2, trim, pivot)
    cols = [J[:, a] * J[:, b] for a in range(7) for b in range(a, 7)] + [J[:, a] * r for a in range(7)] + [r * r, dd]
    return np.stack(cols, 1).reshape(-1, 37)


def plane_moments(src, normals, T, dst, idx, d2, trim=np.inf, pivot=(0, 0, 0)):
    """-> (count, sums (37,) = math.fsum of every column of plane_terms, mags (37,) = math.fsum of their magnitudes)."""
    t = plane_terms(src, normals, T, dst, idx, d2, trim, pivot)
    sums = np.array([math.fsum(t[:, k].tolist()) for k in range(37)], np.float64)
    mags = np.array([math.fsum(np.abs(t[:, k]).tolist()) for k in range(37)], np.float64)
    return len(t), sums, mags


def motion_from_points(J, r, pivot=(0, 0, 0), with_scale=False):
    """The Gauss-Newton step from explicit rows: x = argmin |J x + r| by numpy.linalg.lstsq over the first 6 (or all 7) columns ->
    the 4x4 of x -> pivot + (1 + sigma) Exp(omega) (x - pivot) + t."""
    J, r = np.asarray(J, np.float64).reshape(-1, 7), np.asarray(r, np.float64).reshape(-1)
    dim = 7 if with_scale else 6
    x = np.linalg.lstsq(J[:, :dim], -r, rcond=None)[0]
    w = x[:3]
    theta = float(np.linalg.norm(w))
    R = RR.rotation(w, np.rad2deg(theta)) if theta > 0.0 else np.eye(3)
    return RR.similarity(R, x[3:6], 1.0 + float(x[6]) if with_scale else 1.0, pivot)


def box(points):
    """(lo, hi) float64 over the finite rows of a float32 cloud."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)].astype(np.float64)
    return p.min(axis=0), p.max(axis=0)


def register_plane(recon, normals, gt, init=None, with_scale=False, distances=STAGES, max_iterations=100, min_move=0.0):
    """The point-to-plane loop of register_cloud.register with voxel = 0: per stage distance r, repeat { moved = transform(recon,
    T); nearest within r; T = step(original recon under T, its normals, matched gt) T } about the centre of gt's box until the
    corners of recon's box move by at most min_move (None: 1e-3 r, register's default).  -> (T, [(iterations, pairs)] per
    stage)."""
    recon, gt = np.asarray(recon, np.float32).reshape(-1, 3), np.asarray(gt, np.float32).reshape(-1, 3)
    T = np.eye(4) if init is None else np.array(init, np.float64).reshape(4, 4)
    corners = RR.corners_of(recon)
    lo, hi = box(gt)
    pivot = (lo + hi) / 2.0
    stages = []
    for rad in distances:
        its, pairs = 0, 0
        for _ in range(max_iterations):
            d2, idx = RR.nearest(RR.transform(recon, T), gt, rad)
            _, _, _, r, J, _ = plane_pairs(recon, normals, T, gt, idx, d2, np.inf, pivot)
            pairs = len(r)
            if pairs < 3:
                raise ValueError('%d pairs within %g' % (pairs, rad))
            T_new = motion_from_points(J, r, pivot, with_scale) @ T
            d = (corners @ T_new[:3, :3].T + T_new[:3, 3]) - (corners @ T[:3, :3].T + T[:3, 3])
            T, its = T_new, its + 1
            if float(np.sqrt((d * d).sum(axis=1)).max()) <= (1e-3 * rad if min_move is None else min_move):
                break
        stages.append((its, pairs))
    return T, stages


def corner_error(T, M, points):
    """The largest distance between a corner of `points`' box under T and under M."""
    c = RR.corners_of(points)
    d = (c @ T[:3, :3].T + T[:3, 3]) - (c @ M[:3, :3].T + M[:3, 3])
    return float(np.sqrt((d * d).sum(axis=1)).max())


def shape_with_normals(n, seed, noise=0.0, normal_noise=0.0):
    """cloud_register_restated.shape(n, seed, noise) -- the same draws, so the same points -- and the unit normal of the surface each
    point was drawn on: (0,0,1) on the floor, (0,1,0) and (1,0,0) on the walls, the radius on the half-ball.  normal_noise: Gaussian
    noise of that sigma per component (from a generator of its own), renormalised.  -> (points (n,3), normals (n,3)) float64."""
    rng = np.random.default_rng(seed)
    areas = np.array([2.0 * 1.2, 2.0 * 0.8, 1.2 * 0.8, 2.0 * np.pi * 0.25 ** 2])
    part = rng.choice(4, size=n, p=areas / areas.sum())
    u, v = rng.uniform(size=n), rng.uniform(size=n)
    p, nrm = np.zeros((n, 3)), np.zeros((n, 3))
    k = part == 0
    p[k], nrm[k] = np.stack([2.0 * u[k], 1.2 * v[k], np.zeros(k.sum())], 1), (0.0, 0.0, 1.0)
    k = part == 1
    p[k], nrm[k] = np.stack([2.0 * u[k], np.zeros(k.sum()), 0.8 * v[k]], 1), (0.0, 1.0, 0.0)
    k = part == 2
    p[k], nrm[k] = np.stack([np.zeros(k.sum()), 1.2 * u[k], 0.8 * v[k]], 1), (1.0, 0.0, 0.0)
    k = part == 3
    d = rng.normal(size=(int(k.sum()), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:, 2] = np.abs(d[:, 2])
    p[k], nrm[k] = np.array([1.3, 0.4, 0.0]) + 0.25 * d, d
    if noise:
        p += rng.normal(0.0, noise, p.shape)
    if normal_noise:
        nrm = nrm + np.random.default_rng(seed + 1000).normal(0.0, normal_noise, nrm.shape)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return p, nrm


def sampled_pair(n_gt, n_src, seed_gt, seed_src, scale=1.0, noise=0.0, normal_noise=0.0):
    """Two INDEPENDENT samples of the shape: the ground truth (n_gt,3) float32, and a source (n_src,3) float32 with its normals
    (n_src,3) float32 in its own frame, moved by the inverse of M = (4 degrees about (1,2,3) through the ground truth's centroid,
    translation (0.06, -0.04, 0.05), `scale`).  -> (gt, src, normals, M): M moves the source back."""
    gt = RR.shape(n_gt, seed_gt, noise=noise).astype(np.float32)
    R = RR.rotation((1, 2, 3), 4.0)
    M = RR.similarity(R, (0.06, -0.04, 0.05), scale, gt.mean(axis=0).astype(np.float64))
    Mi = np.linalg.inv(M)
    p, nrm = shape_with_normals(n_src, seed_src, noise, normal_noise)
    return gt, (p @ Mi[:3, :3].T + Mi[:3, 3]).astype(np.float32), (nrm @ R).astype(np.float32), M            # R^T n, row-wise: n @ R


COMPARISON = dict(n_gt=8000, n_src=4000, seed_gt=21, seed_src=22)


@functools.lru_cache(maxsize=None)
def comparison_pair():
    """The pair of the comparison of DESIGN.md section 12.1a: exact samples, analytic normals -> (gt, src, normals, M).  Computed
    once per process, like the two loops below; treat what they return as read-only."""
    return sampled_pair(**COMPARISON)


@functools.lru_cache(maxsize=None)
def comparison_point():
    """The restated point-to-point loop on the comparison's pair -> (T, stages)."""
    gt, src, _, _ = comparison_pair()
    return RR.icp(src, gt, distances=STAGES, max_iterations=100, min_move=MIN_MOVE)


@functools.lru_cache(maxsize=None)
def comparison_plane():
    """The restated point-to-plane loop on the comparison's pair, under the same stop rule -> (T, stages)."""
    gt, src, nrm, _ = comparison_pair()
    return register_plane(src, nrm, gt, distances=STAGES, max_iterations=100, min_move=MIN_MOVE)
