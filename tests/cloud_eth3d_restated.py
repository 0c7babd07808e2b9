"""The definitions of atvs_cloud_scan_excess and atvs_cloud_voxel_shares (include/atvsnet_hip.h) restated in numpy float64, and
once more as literal Python loops.

scan_excess: the projection is scan_render_restated.project (the renderer's own), one face at a time over all points; IEEE float64
division and square root (numpy's are correctly rounded).  voxel_shares: the cells of cloud_register_restated.voxel_downsample,
np.unique on the packed 3 x 21-bit key, Python integers for q.  The *_loop forms say the same one point at a time with Python
numbers -- slow, for a few hundred points: they are what the vectorised forms are checked against."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_render_restated as SR  # noqa: E402

CELL_LIMIT = 1 << 21


def scan_excess(points, cams, maps, pixel_centre=0.5, window=1):
    """points (m,3), cams (6 S,16), maps (6 S,N,N) float32 -> (excess (m,) float32, scanner (m,) int32)."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    maps = np.asarray(maps, np.float32)
    size = maps.shape[1]
    assert maps.shape == (len(cams), size, size) and len(cams) % 6 == 0 and 0 <= window <= 2
    m = len(p)
    finite = np.isfinite(p).all(axis=1)
    best = np.full(m, np.inf, np.float64)
    best_s = np.full(m, -1, np.int32)
    for s in range(len(cams) // 6):
        face = np.full(m, -1, np.int64)
        c2 = np.zeros(m)
        xs = np.zeros(m)
        ys = np.zeros(m)
        for f in range(6):
            k2, kx, ky = SR.project(p, cams[6 * s + f], pixel_centre)
            with np.errstate(all='ignore'):
                z = k2.astype(np.float32)
                ok = finite & (face < 0) & (k2 > 0.0) & np.isfinite(z) & (z > 0)
                ok &= (kx >= 0.0) & (kx < float(size)) & (ky >= 0.0) & (ky < float(size))
            face[ok] = f
            c2[ok], xs[ok], ys[ok] = k2[ok], kx[ok], ky[ok]
        seen = np.flatnonzero(face >= 0)
        if not seen.size:
            continue
        u = np.floor(xs[seen]).astype(np.int64)
        v = np.floor(ys[seen]).astype(np.int64)
        z_scan = np.full(seen.size, np.inf, np.float32)
        for dv in range(-window, window + 1):
            for du in range(-window, window + 1):
                uu, vv = u + du, v + dv
                inside = (uu >= 0) & (uu < size) & (vv >= 0) & (vv < size)
                d = maps[6 * s + face[seen], np.clip(vv, 0, size - 1), np.clip(uu, 0, size - 1)]
                take = inside & (d != 0) & (d < z_scan)
                z_scan[take] = d[take]
        hit = np.isfinite(z_scan)
        seen, z_scan = seen[hit], z_scan[hit]
        c = np.asarray(cams[6 * s:6 * s + 6])[face[seen]]
        q = p[seen].astype(np.float64)
        X, Y, Z = q[:, 0], q[:, 1], q[:, 2]
        c0 = ((c[:, 0] * X + c[:, 1] * Y) + c[:, 2] * Z) + c[:, 9]
        c1 = ((c[:, 3] * X + c[:, 4] * Y) + c[:, 5] * Z) + c[:, 10]
        k2 = c2[seen]
        r = np.sqrt((c0 * c0 + c1 * c1) + k2 * k2)
        e = r * (1.0 - z_scan.astype(np.float64) / k2)
        better = e < best[seen]
        best[seen[better]] = e[better]
        best_s[seen[better]] = s
    return np.where(best_s >= 0, best, np.inf).astype(np.float32), best_s


def scan_excess_loop(points, cams, maps, pixel_centre=0.5, window=1):
    """The definition one (point, scanner) pair at a time."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    maps = np.asarray(maps, np.float32)
    size = maps.shape[1]
    pc = float(pixel_centre)
    excess = np.full(len(p), np.inf, np.float32)
    scanner = np.full(len(p), -1, np.int32)
    for i, row in enumerate(p):
        if not np.isfinite(row).all():
            continue
        X, Y, Z = float(row[0]), float(row[1]), float(row[2])
        best, best_s = math.inf, -1
        for s in range(len(cams) // 6):
            found = None
            for f in range(6):
                c = [float(t) for t in cams[6 * s + f]]
                c2 = ((c[6] * X + c[7] * Y) + c[8] * Z) + c[11]
                if not c2 > 0.0:
                    continue
                with np.errstate(over='ignore'):
                    z = np.float32(c2)
                if not (np.isfinite(z) and z > 0):
                    continue
                c0 = ((c[0] * X + c[1] * Y) + c[2] * Z) + c[9]
                c1 = ((c[3] * X + c[4] * Y) + c[5] * Z) + c[10]
                xs = ((c0 / c2) * c[12] + c[14] - pc) + 0.5
                ys = ((c1 / c2) * c[13] + c[15] - pc) + 0.5
                if xs >= 0.0 and xs < size and ys >= 0.0 and ys < size:
                    found = (f, c0, c1, c2, int(math.floor(xs)), int(math.floor(ys)))
                    break
            if found is None:
                continue
            f, c0, c1, c2, u, v = found
            z_scan = None
            for dv in range(-window, window + 1):
                for du in range(-window, window + 1):
                    if 0 <= u + du < size and 0 <= v + dv < size:
                        d = float(maps[6 * s + f, v + dv, u + du])
                        if d != 0.0 and (z_scan is None or d < z_scan):
                            z_scan = d
            if z_scan is None:
                continue
            e = math.sqrt((c0 * c0 + c1 * c1) + c2 * c2) * (1.0 - z_scan / c2)
            if e < best:
                best, best_s = e, s
        if best_s >= 0:
            excess[i], scanner[i] = np.float32(best), best_s
    return excess, scanner


def cells(points, voxel, origin):
    """-> (rows of the finite points, their packed cell keys as uint64); a cell outside [0, 2^21) raises ValueError."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    origin = np.asarray(origin, np.float64).reshape(3)
    ok = np.flatnonzero(np.isfinite(p).all(axis=1))
    c = np.floor((p[ok].astype(np.float64) - origin) / float(voxel))
    if ((c < 0) | (c >= CELL_LIMIT)).any():
        raise ValueError('a cell coordinate leaves [0, 2^21)')
    c = c.astype(np.uint64)
    return ok, c[:, 0] | (c[:, 1] << np.uint64(21)) | (c[:, 2] << np.uint64(42))


def voxel_shares(points, d2, excess, voxel, origin, tolerances, margin=0.0):
    """-> (T,4) Python-integer rows: sum q, voxels counted, sum hit, sum den."""
    rows, key = cells(points, voxel, origin)
    d2 = np.asarray(d2, np.float32).reshape(-1)[rows].astype(np.float64)
    _, inverse = np.unique(key, return_inverse=True)
    inverse = inverse.reshape(-1)
    n_vox = int(inverse.max()) + 1 if inverse.size else 0
    with np.errstate(invalid='ignore'):
        observed = np.ones(len(rows), bool) if excess is None else \
            np.asarray(excess, np.float32).reshape(-1)[rows].astype(np.float64) <= float(margin)
    out = []
    for t in tolerances:
        with np.errstate(invalid='ignore'):
            hit = d2 <= float(t) * float(t)
        h = np.bincount(inverse[hit], minlength=n_vox)
        den = h + np.bincount(inverse[~hit & observed], minlength=n_vox)
        sq = sum((int(a) << 32) // int(b) for a, b in zip(h.tolist(), den.tolist()) if b)
        out.append([sq, int((den > 0).sum()), int(h.sum()), int(den.sum())])
    return out


def voxel_shares_loop(points, d2, excess, voxel, origin, tolerances, margin=0.0):
    """The definition one point at a time, voxels in a dict."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    out = []
    for t in tolerances:
        voxels = {}
        for i, row in enumerate(p):
            if not np.isfinite(row).all():
                continue
            cell = tuple(int(math.floor((float(row[a]) - float(origin[a])) / float(voxel))) for a in range(3))
            if min(cell) < 0 or max(cell) >= CELL_LIMIT:
                raise ValueError('a cell coordinate leaves [0, 2^21)')
            v = voxels.setdefault(cell, [0, 0])
            if float(d2[i]) <= float(t) * float(t):
                v[0] += 1
                v[1] += 1
            elif excess is None or float(excess[i]) <= float(margin):
                v[1] += 1
        counted = [v for v in voxels.values() if v[1]]
        out.append([sum((h << 32) // d for h, d in counted), len(counted), sum(h for h, _ in counted), sum(d for _, d in counted)])
    return out


# ---- shared scenes ---------------------------------------------------------------------------------------------------------

def box_walls(n, half, rng, centre=(0.0, 0.0, 0.0)):
    """n points on the six walls of the cube |x - centre| = half (float32)."""
    p = rng.uniform(-half, half, (n, 3))
    axis = rng.integers(0, 3, n)
    p[np.arange(n), axis] = np.where(rng.random(n) < 0.5, -half, half)
    return (p + np.asarray(centre, np.float64)).astype(np.float32)
