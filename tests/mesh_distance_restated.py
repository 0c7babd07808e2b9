"""The point-to-triangle distance of include/atvsnet_hip.h restated in numpy, operation for operation, by brute force over all faces
(`nearest`: what csrc/mesh_distance.hip is held to bit for bit), and a second reference written independently of it
(`nearest_by_projection`: the foot of the perpendicular on the face's plane where it falls inside the triangle, else the nearest of
the three edge segments), which the restatement is held to within BAR.

BAR, the relative bar between the two references' d2 (both float32), beside its derivation.  Both compute in double from the same
float32 inputs and round once to float32.  The rounding: half a unit in the last place each, 2^-24 relative, 2 * 2^-24 between them.
The double terms: each reference forms a closest point x from differences, dot products, one or two quotients and a combination,
about 40 operations of 2^-53 relative to the quantities they combine, which are bounded by the squared extent L^2 of (face, query)
while d2 may be as small as the result allows: the double error of d2 is at most about 2 * 40 * 2^-53 * L * sqrt(d2) + 40 * 2^-53 *
L^2 absolute.  So |d2 - d2'| <= 2^-22 * max(d2, d2') + DOUBLE_TERM * L * (L + sqrt(d2)) with DOUBLE_TERM = 2^-45 (160 * 2^-53 rounded
up to a power of two), L the largest |coordinate difference| between the query and the face's corners."""
import numpy as np

REGIONS = ('A', 'B', 'AB', 'C', 'AC', 'BC', 'interior', 'segment', 'point')
BAR_REL = 2.0 ** -22
DOUBLE_TERM = 2.0 ** -45
CHUNK = 1 << 21                       # (query, face) pairs per block of the brute force


def usable_faces(vertices, faces):
    """(F,) bool: three indices in 0..V-1 and nine finite coordinates."""
    V = len(vertices)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < V)).all(1)
    fin = np.isfinite(np.asarray(vertices, np.float32)).all(1) if V else np.zeros(0, bool)
    ok[ok] = fin[f[ok]].all(1)
    return ok


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _quot(num, den):
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(den > 0.0, num / np.where(den > 0.0, den, 1.0), 0.0)


def _segment(p, X, Y):
    e, w = Y - X, p - X
    t = _quot(_dot(w, e), _dot(e, e))
    t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
    x = X + t[..., None] * e
    r = p - x
    return _dot(r, r), x


def closest_points(p, a, b, c):
    """p, a, b, c broadcastable (...,3) float64 -> (dd (...) float64, x (...,3) float64, region (...) int8 index into REGIONS): the
    header's sequence."""
    p, a, b, c = np.broadcast_arrays(p, a, b, c)
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    n0 = ab[..., 1] * ac[..., 2] - ab[..., 2] * ac[..., 1]
    n1 = ab[..., 2] * ac[..., 0] - ab[..., 0] * ac[..., 2]
    n2 = ab[..., 0] * ac[..., 1] - ab[..., 1] * ac[..., 0]
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    s = (va + vb) + vc
    flat = (n0 == 0.0) & (n1 == 0.0) & (n2 == 0.0)
    tests = [(d1 <= 0.0) & (d2 <= 0.0),
             (d3 >= 0.0) & (d4 <= d3),
             (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0),
             (d6 >= 0.0) & (d5 <= d6),
             (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0),
             (va <= 0.0) & (d4 - d3 >= 0.0) & (d5 - d6 >= 0.0),
             s > 0.0]
    t_ab, t_ac = _quot(d1, d1 - d3), _quot(d2, d2 - d6)
    u = d4 - d3
    t_bc = _quot(u, u + (d5 - d6))
    v, w = _quot(vb, s), _quot(vc, s)
    points = [a, b, a + t_ab[..., None] * ab, c, a + t_ac[..., None] * ac, b + t_bc[..., None] * (c - b),
              (a + v[..., None] * ab) + w[..., None] * ac]
    # the segment rule: AB, AC, BC, the first smallest
    best, x_seg = _segment(p, a, b)
    for X, Y in ((a, c), (b, c)):
        dd, y = _segment(p, X, Y)
        take = dd < best
        best = np.where(take, dd, best)
        x_seg = np.where(take[..., None], y, x_seg)
    is_point = (ab == 0.0).all(-1) & (ac == 0.0).all(-1)
    region = np.where(is_point, 8, 7).astype(np.int8)
    x = x_seg
    undecided = ~flat
    chosen = np.zeros(flat.shape, bool)
    for k, (test, point) in enumerate(zip(tests, points)):
        take = undecided & ~chosen & test
        x = np.where(take[..., None], point, x)
        region = np.where(take, np.int8(k), region)
        chosen |= take
    r = p - x
    return _dot(r, r), x, region


def nearest(vertices, faces, queries, radius, closest=False, census=False):
    """The definition by brute force -> (d2 (m,) float32, face (m,) int32[, closest (m,3) float32][, region (m,) int8 of the attaining
    face, -1 where none])."""
    v32, q32 = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(queries, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    m = len(q32)
    ids = np.nonzero(usable_faces(v32, f))[0]
    best = np.full(m, (0x7f800000 << 32) | 0xffffffff, np.uint64)
    best_x = np.full((m, 3), np.nan, np.float64)
    best_region = np.full(m, -1, np.int8)
    finite = np.isfinite(q32).all(1)
    rows = np.nonzero(finite)[0]
    if len(ids) and len(rows):
        v = v32.astype(np.float64)
        p = q32[rows].astype(np.float64)[:, None, :]
        step = max(1, CHUNK // len(rows))
        for lo in range(0, len(ids), step):
            part = ids[lo:lo + step]
            a, b, c = v[f[part, 0]][None], v[f[part, 1]][None], v[f[part, 2]][None]
            dd, x, region = closest_points(p, a, b, c)
            with np.errstate(over='ignore'):
                bits = dd.astype(np.float32).view(np.uint32).astype(np.uint64)
            key = (bits << np.uint64(32)) | part.astype(np.uint64)[None, :]
            k = key.argmin(1)                          # the smallest key: ties in d2 go to the lowest face
            pick = key[np.arange(len(rows)), k]
            take = pick < best[rows]
            best[rows[take]] = pick[take]
            best_x[rows[take]] = x[np.arange(len(rows)), k][take]
            best_region[rows[take]] = region[np.arange(len(rows)), k][take]
    d2 = (best >> np.uint64(32)).astype(np.uint32).view(np.float32)
    face = (best & np.uint64(0xffffffff)).astype(np.uint32).view(np.int32).copy()
    r2 = float(np.float32(radius)) * float(np.float32(radius))
    found = (face >= 0) & (d2.astype(np.float64) <= r2)
    d2 = np.where(found, d2, np.float32(np.inf)).astype(np.float32)
    face = np.where(found, face, -1).astype(np.int32)
    out = [d2, face]
    if closest:
        with np.errstate(invalid='ignore'):
            out.append(np.where(found[:, None], best_x, np.nan).astype(np.float32))
    if census:
        out.append(np.where(found, best_region, -1).astype(np.int8))
    return tuple(out)


def second_best_gap(vertices, faces, queries):
    """(m,) float64: the relative gap (d2_second - d2_best) / max(d2_second, tiny) between a query's two smallest DISTINCT-face
    double distances (inf where fewer than two usable faces): below the bar the `face` of a query may legitimately differ."""
    v, q = np.asarray(vertices, np.float32).astype(np.float64), np.asarray(queries, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ids = np.nonzero(usable_faces(vertices, f))[0]
    gap = np.full(len(q), np.inf)
    rows = np.nonzero(np.isfinite(q).all(1))[0]
    if len(ids) < 2 or not len(rows):
        return gap
    two = np.full((len(rows), 2), np.inf)
    step = max(1, CHUNK // len(rows))
    for lo in range(0, len(ids), step):
        part = ids[lo:lo + step]
        dd = closest_points(q[rows][:, None, :], v[f[part, 0]][None], v[f[part, 1]][None], v[f[part, 2]][None])[0]
        two = np.sort(np.concatenate([two, dd], 1), 1)[:, :2]
    with np.errstate(invalid='ignore', divide='ignore'):
        gap[rows] = np.where(two[:, 1] > 0.0, (two[:, 1] - two[:, 0]) / two[:, 1], 0.0)
    return gap


# ------------------------------------------------------------------------------------------------- the second, independent reference
def _seg_d2(p, X, Y):
    e = Y - X
    L2 = np.einsum('...k,...k->...', e, e)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.clip(np.where(L2 > 0.0, np.einsum('...k,...k->...', p - X, e) / np.where(L2 > 0.0, L2, 1.0), 0.0), 0.0, 1.0)
    r = p - (X + t[..., None] * e)
    return np.einsum('...k,...k->...', r, r)


def distances_by_projection(p, a, b, c):
    """(...,) float64 squared distances: the perpendicular's foot where it lies inside the triangle (three same-side tests against
    the normal), else the smallest of the three segment distances."""
    p, a, b, c = np.broadcast_arrays(p, a, b, c)
    n = np.cross(b - a, c - a)
    nn = np.einsum('...k,...k->...', n, n)
    with np.errstate(divide='ignore', invalid='ignore'):
        h = np.einsum('...k,...k->...', p - a, n) / np.where(nn > 0.0, nn, 1.0)
    foot = p - h[..., None] * n
    inside = (nn > 0.0)
    for X, Y in ((a, b), (b, c), (c, a)):
        inside &= np.einsum('...k,...k->...', np.cross(Y - X, foot - X), n) >= 0.0
    plane = h * h * nn
    edges = np.minimum(np.minimum(_seg_d2(p, a, b), _seg_d2(p, b, c)), _seg_d2(p, c, a))
    return np.where(inside, np.minimum(plane, edges), edges)


def nearest_by_projection(vertices, faces, queries, radius):
    """-> (d2 (m,) float32, extent (m,) float64): the smallest distance by the second reference, +inf beyond the radius, and the L of
    the bar: the largest coordinate difference between the query and any usable face's corner."""
    v32, q32 = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(queries, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ids = np.nonzero(usable_faces(v32, f))[0]
    m = len(q32)
    best = np.full(m, np.inf)
    extent = np.zeros(m)
    rows = np.nonzero(np.isfinite(q32).all(1))[0]
    if len(ids) and len(rows):
        v = v32.astype(np.float64)
        p = q32[rows].astype(np.float64)
        used = v[np.unique(f[ids])]
        extent[rows] = np.maximum(np.abs(p - used.min(0)), np.abs(p - used.max(0))).max(1)
        step = max(1, CHUNK // len(rows))
        for lo in range(0, len(ids), step):
            part = ids[lo:lo + step]
            dd = distances_by_projection(p[:, None, :], v[f[part, 0]][None], v[f[part, 1]][None], v[f[part, 2]][None])
            best[rows] = np.minimum(best[rows], dd.min(1))
    with np.errstate(over='ignore'):
        d2 = best.astype(np.float32)
    r2 = float(np.float32(radius)) * float(np.float32(radius))
    return np.where(d2.astype(np.float64) <= r2, d2, np.float32(np.inf)).astype(np.float32), extent


def bar(d2_a, d2_b, extent):
    """The absolute bar between the two references' float32 d2 (module docstring)."""
    big = np.maximum(d2_a, d2_b).astype(np.float64)
    return BAR_REL * big + DOUBLE_TERM * extent * (extent + np.sqrt(big))


# ------------------------------------------------------------------------------------- the grid's reference count and its coarsening
def grid_refs(vertices, faces, h):
    """The face references csrc/mesh_distance.hip needs at cell edge h: per usable face the cells of the box of its corners,
    cell = floor((x - origin) / h) in double with origin the minimum corner of the usable faces' corners."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[usable_faces(vertices, f)]
    if not len(f):
        return 0
    corners = v[f]                                     # (F,3,3)
    origin = corners.reshape(-1, 3).min(0)
    lo = np.floor((corners.min(1) - origin) / h)
    hi = np.floor((corners.max(1) - origin) / h)
    return int((hi - lo + 1.0).prod(1).sum())


def coarsening(vertices, faces, h, budget):
    """ops.mesh_grid's loop from a first cell edge h (the device's: it holds the cell cap's rule) -> [(h, references)] per build."""
    steps = []
    for _ in range(128):
        refs = grid_refs(vertices, faces, h)
        steps.append((h, refs))
        if refs <= budget:
            return steps
        h = 2.0 * h
    raise AssertionError('the coarsening did not end')
