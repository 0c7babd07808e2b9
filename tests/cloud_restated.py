"""The point-cloud kernels' definition restated with numpy (include/atvsnet_hip.h, csrc/cloud.hip): brute force, no grid.

For a finite query q and a finite reference point p, in float32 with every operation rounded:
    dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z,   d2 = (dx*dx + dy*dy) + dz*dz
d2min = the minimum over all finite reference points, idx = the lowest index attaining it (numpy's argmin returns the first
minimum); (+inf, -1) when double(d2min) > double(R) * double(R), the query is not finite, or no reference point is finite.
"""
import numpy as np


def d2_pairs(q, p):
    """The float32 expression for matching rows of q and p ((k,3) each) -> (k,) float32."""
    q, p = np.asarray(q, np.float32), np.asarray(p, np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        dx, dy, dz = q[:, 0] - p[:, 0], q[:, 1] - p[:, 1], q[:, 2] - p[:, 2]
        return ((dx * dx + dy * dy) + dz * dz).astype(np.float32)


def nearest(Q, P, R, chunk_elems=1 << 25, unique=False):
    """-> (d2 (m,) float32, idx (m,) int32) [, unique (m,) bool: the minimum is attained by exactly one reference point]."""
    Q = np.ascontiguousarray(Q, np.float32).reshape(-1, 3)
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
    m = len(Q)
    d2 = np.full(m, np.inf, np.float32)
    idx = np.full(m, -1, np.int32)
    uniq = np.zeros(m, bool)
    keep = np.flatnonzero(np.isfinite(P).all(axis=1))
    r2 = float(np.float32(R)) * float(np.float32(R))
    if len(keep) and m:
        Pk = P[keep]
        px, py, pz = Pk[:, 0][None, :], Pk[:, 1][None, :], Pk[:, 2][None, :]
        rows = max(1, chunk_elems // len(Pk))
        with np.errstate(over='ignore', invalid='ignore'):
            for s in range(0, m, rows):
                q = Q[s:s + rows]
                dx, dy, dz = q[:, 0:1] - px, q[:, 1:2] - py, q[:, 2:3] - pz
                d = (dx * dx + dy * dy) + dz * dz
                assert d.dtype == np.float32
                a = d.argmin(axis=1)
                best = d[np.arange(len(q)), a]
                ok = np.isfinite(q).all(axis=1) & (best.astype(np.float64) <= r2)
                d2[s:s + rows] = np.where(ok, best, np.float32(np.inf))
                idx[s:s + rows] = np.where(ok, keep[a], -1)
                if unique:
                    uniq[s:s + rows] = ok & ((d == best[:, None]).sum(axis=1) == 1)
    return (d2, idx, uniq) if unique else (d2, idx)


def counts(d2, tolerances):
    return [int((np.asarray(d2, np.float32).astype(np.float64) <= float(t) * float(t)).sum()) for t in tolerances]


def surface(n, seed, noise=0.002):
    """n float32 points on a noisy unit sphere (a synthetic scan)."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v *= 1.0 + noise * rng.normal(size=(n, 1))
    return v.astype(np.float32)
