"""The definitions of the mesh smoothing section of include/atvsnet_hip.h (atvs_mesh_adjacency .. atvs_mesh_vertex_normals) and of
ops.mesh_smooth / ops.mesh_vertex_normals, restated in numpy: np.add.at on int64 for the sums, np.rint for llrint, numpy's int64 ->
float64 conversions (round to nearest even, as the device's).  numpy never fuses a product into a sum, which is what the library's
-ffp-contract=off gives the kernels.  Rows of `neighbours` come sorted here; the device's order is not defined."""
import math

import numpy as np

ADJACENCY_INFO = ('pairs', 'boundary_pairs', 'nonmanifold_pairs', 'skipped_index_faces', 'self_pairs', 'nonfinite_pairs', 'unplaced_pairs')
FINITE, BOUNDARY, NONMANIFOLD = 1, 2, 4
CLAMP = 1 << 32


def adjacency(vertices, faces):
    """-> dict(degree, flags, offsets, neighbours (rows sorted), info)."""
    V = len(vertices)
    finite = np.isfinite(vertices).all(1) if V else np.zeros(0, bool)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < V)).all(1)
    info = dict.fromkeys(ADJACENCY_INFO, 0)
    info['skipped_index_faces'] = int((~ok).sum())
    f = f[ok]
    a, b = f[:, [0, 1, 2]].reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    same = a == b
    info['self_pairs'] = int(same.sum())
    a, b = a[~same], b[~same]
    bad = ~(finite[a] & finite[b])
    info['nonfinite_pairs'] = int(bad.sum())
    a, b = a[~bad], b[~bad]
    key, count = np.unique((np.minimum(a, b) << 32) | np.maximum(a, b), return_counts=True)
    lo, hi = key >> 32, key & 0xffffffff
    info.update(pairs=len(key), boundary_pairs=int((count == 1).sum()), nonmanifold_pairs=int((count > 2).sum()))
    degree = np.zeros(V, np.int32)
    flags = finite.astype(np.int32)
    bits = ((count == 1) * BOUNDARY | (count > 2) * NONMANIFOLD).astype(np.int32)
    for end in (lo, hi):
        np.add.at(degree, end, 1)
        np.bitwise_or.at(flags, end, bits)
    offsets = np.concatenate([[0], np.cumsum(degree, dtype=np.int64)]).astype(np.int32)
    src, dst = np.concatenate([lo, hi]), np.concatenate([hi, lo])
    neighbours = dst[np.lexsort((dst, src))].astype(np.int32)
    return dict(degree=degree, flags=flags, offsets=offsets, neighbours=neighbours, info=info)


def sorted_rows(offsets, neighbours):
    """`neighbours` with every row offsets[v] .. offsets[v+1]-1 sorted: the form in which two adjacencies compare."""
    out = np.array(neighbours[:offsets[-1]], np.int32)
    for v in range(len(offsets) - 1):
        out[offsets[v]:offsets[v + 1]].sort()
    return out


def quantize(vertices, origin, step):
    """-> (q (V,3) int64, dict(nonfinite_vertices, far_coordinates))."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    finite = np.isfinite(v).all(1)
    with np.errstate(invalid='ignore', over='ignore'):
        t = np.rint((v.astype(np.float64) - np.asarray(origin, np.float64)) / np.float64(step))
    t[~finite] = 0.0
    return t.astype(np.int64), dict(nonfinite_vertices=int((~finite).sum()), far_coordinates=int((np.abs(t) > 2.0 ** 31).sum()))


def smooth_pass(q, adj, factor, pin_mask=0):
    """-> (q_out, clamped coordinates)."""
    q = np.asarray(q, np.int64)
    degree, flags = adj['degree'].astype(np.int64), adj['flags']
    V = len(q)
    S = np.zeros((V, 3), np.int64)
    np.add.at(S, np.repeat(np.arange(V), degree), q[adj['neighbours'][:adj['offsets'][-1]]])
    moves = ((flags & FINITE) != 0) & (degree != 0) & ((flags & pin_mask) == 0)
    m = S.astype(np.float64) / np.maximum(degree, 1).astype(np.float64)[:, None]
    d = m - q.astype(np.float64)
    r = q + np.rint(np.float64(factor) * d).astype(np.int64)
    r = np.where(moves[:, None], r, q)
    clamped = int((np.abs(r) > CLAMP).sum())
    return np.clip(r, -CLAMP, CLAMP), clamped


def dequantize(q, q0, vertices, origin, step):
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    with np.errstate(over='ignore'):
        moved = (np.asarray(origin, np.float64) + np.float64(step) * q.astype(np.float64)).astype(np.float32)
    return np.where(q == q0, v.view(np.uint32), moved.view(np.uint32)).view(np.float32)


def lattice(vertices):
    """(origin (3,) float64, step) as ops.mesh_smooth takes them from the bounding box of the finite vertices."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    v = v[np.isfinite(v).all(1)].astype(np.float64)
    lo, hi = (v.min(0), v.max(0)) if len(v) else (np.zeros(3), np.zeros(3))
    extent = float((hi - lo).max())
    e = math.frexp(extent)[1] if extent > 0.0 else 0
    return (lo + hi) / 2.0, math.ldexp(1.0, e - 32)


def smooth(vertices, faces, iterations, lam=0.5, mu=-0.53, pin_boundary=False, trace=None):
    """-> (vertices_out, info): ops.mesh_smooth.  trace: a list that receives q after every pass (q0 first)."""
    adj = adjacency(vertices, faces)
    origin, step = lattice(vertices)
    q0, qinfo = quantize(vertices, origin, step)
    assert qinfo['far_coordinates'] == 0
    q, clamped = q0, 0
    if trace is not None:
        trace.append(q0)
    for factor in ([lam] if mu is None else [lam, mu]) * iterations:
        q, c = smooth_pass(q, adj, factor, BOUNDARY if pin_boundary else 0)
        clamped += c
        if trace is not None:
            trace.append(q)
    info = dict(adj['info'], origin=[float(x) for x in origin], step=step, passes=iterations * (1 if mu is None else 2),
                nonfinite_vertices=qinfo['nonfinite_vertices'], clamped=clamped)
    return dequantize(q, q0, vertices, origin, step), info


def _cross(vertices, faces):
    """(m (F',3) float64, the usable faces (F',3), the mask of faces with indices in range): atvs_mesh_sample_counts' form."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(1)
    f = f[ok]
    with np.errstate(invalid='ignore', over='ignore'):
        e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
        m = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    return m, f, ok


def _extent(m):
    with np.errstate(invalid='ignore', over='ignore'):
        return np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])


def face_extent(vertices, faces):
    m, f, ok = _cross(vertices, faces)
    s = _extent(m)
    fin = np.isfinite(s)
    return dict(max_extent=float(s[fin].max()) if fin.any() else 0.0, usable_faces=int(fin.sum()), skipped_index_faces=int((~ok).sum()),
                nonfinite_faces=int((~fin).sum()))


def vertex_normal_sums(vertices, faces, area_unit):
    """-> (sums (V,3) int64, incidences (V,) int32)."""
    V = len(vertices)
    m, f, _ = _cross(vertices, faces)
    s = _extent(m)
    use = np.isfinite(s) & (s > 0.0)
    m, f, s = m[use], f[use], s[use]
    w = np.minimum(1.0, s / np.float64(area_unit))
    t = np.rint((w[:, None] * (m / s[:, None])) * 2.0 ** 30).astype(np.int64)
    sums, incidences = np.zeros((V, 3), np.int64), np.zeros(V, np.int32)
    for c in range(3):
        np.add.at(sums, f[:, c], t)
        np.add.at(incidences, f[:, c], 1)
    return sums, incidences


def normals_from_sums(sums):
    N = np.asarray(sums, np.int64).astype(np.float64)
    L = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(L[:, None] > 0.0, (N / L[:, None]).astype(np.float32), np.float32(0.0))


def vertex_normals(vertices, faces, area_unit=None):
    if area_unit is None:
        area_unit = face_extent(vertices, faces)['max_extent'] or 1.0
    return normals_from_sums(vertex_normal_sums(vertices, faces, area_unit)[0])
