"""The definitions of the mesh simplification (include/atvsnet_hip.h: atvs_mesh_cluster, atvs_mesh_cluster_quadrics,
atvs_mesh_cluster_place, atvs_mesh_cluster_max_move, atvs_mesh_cluster_faces) restated in vectorised numpy: float64 operations in
the header's order, integer sums by np.add.at, the Jacobi written out rotation by rotation.  It returns every intermediate, and per
cluster a MARGIN: how far the cluster is from a decision the placement takes (an eigenvalue at the rank threshold, lambda_max at
2^-20, the minimiser on the cell's wall), so that a test can leave out the clusters where a last bit decides.
tests/test_mesh_simplify_host.py holds this file to its own invariants; tests/test_gpu_mesh_simplify.py holds the kernels to it."""
import numpy as np

import mesh_topology_restated as T

FIX = 2.0 ** 30
SLIVER = 2.0 ** -20
CELL_LIMIT = 1 << 21
PLACEMENTS = ('mean', 'quadric')


def coords(x, origin, cell):
    """x (n,) float32 of one axis -> (g, c, u): the quotient, its floor, the 32-bit fraction (uint64), all per the header."""
    with np.errstate(all='ignore'):
        g = (x.astype(np.float64) - float(origin)) / float(cell)
        c = np.floor(g)
        f = np.floor((g - c) * 4294967296.0)
    u = np.where(f >= 4294967295.0, 4294967295.0, f)
    return g, c, u


def cluster(vertices, colors, cell, origin):
    """-> dict(vertex_cluster (V,) int32, cells (C,3) int32, counts (C,) int32, position_sums (C,3) uint64, color_sums (C,3) int64
    or None).  A finite vertex whose cell leaves [0, 2^21) raises ValueError."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    finite = np.isfinite(v).all(1)
    idx = np.nonzero(finite)[0]
    c = np.zeros((len(idx), 3), np.int64)
    u = np.zeros((len(idx), 3), np.uint64)
    for a in range(3):
        _, ca, ua = coords(v[idx, a], origin[a], cell)
        if ((ca < 0) | (ca >= CELL_LIMIT)).any():
            raise ValueError('a vertex leaves the 2^21 cells on axis %d' % a)
        c[:, a], u[:, a] = ca.astype(np.int64), ua.astype(np.uint64)
    key = c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)        # first: the lowest position, so the lowest index
    inverse = inverse.reshape(-1)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind='stable')] = np.arange(len(first))
    ids = rank[inverse]
    C = len(first)
    vertex_cluster = np.full(len(v), -1, np.int32)
    vertex_cluster[idx] = ids
    cells = np.zeros((C, 3), np.int32)
    cells[ids] = c
    counts = np.bincount(ids, minlength=C).astype(np.int32)
    position_sums = np.zeros((C, 3), np.uint64)
    np.add.at(position_sums, ids, u)
    color_sums = None
    if colors is not None:
        color_sums = np.zeros((C, 3), np.int64)
        np.add.at(color_sums, ids, np.asarray(colors, np.uint8).reshape(-1, 3)[idx].astype(np.int64))
    return dict(vertex_cluster=vertex_cluster, cells=cells, counts=counts, position_sums=position_sums, color_sums=color_sums)


def check_faces(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(f) and ((f < 0) | (f >= V)).any():
        raise ValueError('a face index outside 0..%d' % (V - 1))
    return f


def quadrics(vertices, faces, vertex_cluster, C, cell, origin):
    """-> (quadrics (C,10) int64, incidences (C,) int32)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = check_faces(faces, len(v))
    Q = np.zeros((C, 10), np.int64)
    inc = np.zeros(C, np.int32)
    if not len(f):
        return Q, inc
    k = vertex_cluster[f].astype(np.int64)                                   # (F,3)
    ok = (k >= 0).all(1)
    f, k = f[ok], k[ok]
    x = v[f].astype(np.float64)                                              # (F', 3 vertices, 3 axes)
    with np.errstate(all='ignore'):
        e, h = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0]
        m0 = e[:, 1] * h[:, 2] - e[:, 2] * h[:, 1]
        m1 = e[:, 2] * h[:, 0] - e[:, 0] * h[:, 2]
        m2 = e[:, 0] * h[:, 1] - e[:, 1] * h[:, 0]
        L2 = (m0 * m0 + m1 * m1) + m2 * m2
    ok = (L2 > 0.0) & np.isfinite(L2)
    k, x, m0, m1, m2, L2 = k[ok], x[ok], m0[ok], m1[ok], m2[ok], L2[ok]
    r = np.sqrt(L2)
    n = [m0 / r, m1 / r, m2 / r]
    ratio = r / (float(cell) * float(cell))
    w = np.where(ratio < 1.0, ratio, 1.0)
    for j in range(3):
        use = np.ones(len(k), bool)
        if j > 0:
            use &= k[:, j] != k[:, 0]
        if j > 1:
            use &= k[:, j] != k[:, 1]
        p = []
        for a in range(3):
            g = (x[:, j, a] - float(origin[a])) / float(cell)
            p.append((g - np.floor(g)) - 0.5)
        d = -((n[0] * p[0] + n[1] * p[1]) + n[2] * p[2])
        w0, w1, w2, wd = w * n[0], w * n[1], w * n[2], w * d
        terms = [w0 * n[0], w0 * n[1], w0 * n[2], w1 * n[1], w1 * n[2], w2 * n[2], wd * n[0], wd * n[1], wd * n[2], wd * d]
        fixed = np.stack([np.rint(t * FIX).astype(np.int64) for t in terms], 1)
        np.add.at(Q, k[use, j], fixed[use])
        np.add.at(inc, k[use, j], 1)
    return Q, inc


def _rotate(app, aqq, apq, apr, aqr, V, p, q):
    """jacobi_rotate of csrc/jacobi3.h on a batch -> (app, aqq, apq = 0, apr, aqr); V (n,3,3) in place."""
    with np.errstate(all='ignore'):
        theta = (aqq - app) / (2.0 * apq)
        mag = np.abs(theta) + np.sqrt(theta * theta + 1.0)
        t = np.where(apq == 0.0, 0.0, np.where(theta < 0.0, -1.0 / mag, 1.0 / mag))
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    h = t * apq
    app, aqq = app - h, aqq + h
    apr, aqr = c * apr - s * aqr, s * apr + c * aqr
    vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
    V[:, :, p] = c[:, None] * vp - s[:, None] * vq
    V[:, :, q] = s[:, None] * vp + c[:, None] * vq
    return app, aqq, np.zeros_like(apq), apr, aqr


def jacobi3(a00, a01, a02, a11, a12, a22):
    """-> (lam (n,3) the diagonal, V (n,3,3): eigenvector i in column i), six sweeps of (0,1), (0,2), (1,2)."""
    a00, a01, a02, a11, a12, a22 = (np.array(a, np.float64) for a in (a00, a01, a02, a11, a12, a22))
    V = np.tile(np.eye(3), (len(a00), 1, 1))
    for _ in range(6):
        a00, a11, a01, a02, a12 = _rotate(a00, a11, a01, a02, a12, V, 0, 1)
        a00, a22, a02, a01, a12 = _rotate(a00, a22, a02, a01, a12, V, 0, 2)
        a11, a22, a12, a01, a02 = _rotate(a11, a22, a12, a01, a02, V, 1, 2)
    return np.stack([a00, a11, a22], 1), V


def place(cells, counts, position_sums, color_sums, Q, cell, origin, placement='quadric', rank_epsilon=1e-3):
    """-> dict(positions (C,3) float32, colors (C,3) uint8 or None, placed (C,) uint8, margin (C,) float64, x (C,3) the position in
    cell units about the centre)."""
    if placement not in PLACEMENTS:
        raise ValueError('placement %r' % (placement,))
    C = len(counts)
    k = np.maximum(np.asarray(counts, np.int64), 1)
    kd = k.astype(np.float64)
    S = np.asarray(position_sums).view(np.uint64).reshape(C, 3) if C else np.zeros((0, 3), np.uint64)
    x0 = np.stack([(S[:, a].astype(np.float64) / kd) / 4294967296.0 - 0.5 for a in range(3)], 1) if C else np.zeros((0, 3))
    x = x0.copy()
    use = np.zeros(C, bool)
    margin = np.full(C, np.inf)
    if placement == 'quadric' and C:
        scale = 1.0 / FIX
        q = np.asarray(Q, np.int64).astype(np.float64) * scale
        A00, A01, A02, A11, A12, A22, b0, b1, b2 = (q[:, i] for i in range(9))
        lam, V = jacobi3(A00, A01, A02, A11, A12, A22)
        lmax = lam[:, 0].copy()
        lmax = np.where(lam[:, 1] > lmax, lam[:, 1], lmax)
        lmax = np.where(lam[:, 2] > lmax, lam[:, 2], lmax)
        thr = float(rank_epsilon) * lmax
        g0 = ((A00 * x0[:, 0] + A01 * x0[:, 1]) + A02 * x0[:, 2]) + b0
        g1 = ((A01 * x0[:, 0] + A11 * x0[:, 1]) + A12 * x0[:, 2]) + b1
        g2 = ((A02 * x0[:, 0] + A12 * x0[:, 1]) + A22 * x0[:, 2]) + b2
        y0, y1, y2 = x0[:, 0].copy(), x0[:, 1].copy(), x0[:, 2].copy()
        with np.errstate(all='ignore'):
            for i in range(3):
                t = ((V[:, 0, i] * g0 + V[:, 1, i] * g1) + V[:, 2, i] * g2) / lam[:, i]
                on = lam[:, i] > thr
                y0 = np.where(on, y0 - V[:, 0, i] * t, y0)
                y1 = np.where(on, y1 - V[:, 1, i] * t, y1)
                y2 = np.where(on, y2 - V[:, 2, i] * t, y2)
            y = np.stack([y0, y1, y2], 1)
            use = np.isfinite(lmax) & (lmax > SLIVER) & np.isfinite(y).all(1) & (np.abs(y) <= 0.5).all(1)
            # the margin: the least distance to a decision, each on its own scale
            m_sliver = np.abs(lmax * 2.0 ** 20 - 1.0)
            m_rank = np.abs(lam / lmax[:, None] - float(rank_epsilon)).min(1) / float(rank_epsilon)
            m_wall = np.abs(0.5 - np.abs(y)).min(1)
        solid = np.isfinite(lmax) & (lmax > SLIVER)
        margin = np.where(solid, np.minimum(m_sliver, np.minimum(np.nan_to_num(m_rank, nan=0.0), np.nan_to_num(m_wall, nan=0.0))), m_sliver)
        margin = np.nan_to_num(margin, nan=0.0)
        x = np.where(use[:, None], y, x0)
    org = np.asarray(origin, np.float64)
    positions = np.stack([org[a] + float(cell) * ((np.asarray(cells)[:, a].astype(np.float64) + 0.5) + x[:, a]) for a in range(3)],
                         1).astype(np.float32) if C else np.zeros((0, 3), np.float32)
    colors = None
    if color_sums is not None:
        cs = np.asarray(color_sums, np.int64).reshape(C, 3)
        colors = ((2 * cs + k[:, None]) // (2 * k[:, None])).astype(np.uint8)
    return dict(positions=positions, colors=colors, placed=use.astype(np.uint8), margin=margin, x=x)


def max_move(vertices, vertex_cluster, positions):
    """-> the largest distance of a clustered vertex to its cluster's position: sqrt of the largest float32 squared distance."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    on = vertex_cluster >= 0
    if not on.any():
        return 0.0
    with np.errstate(all='ignore'):
        e = positions[vertex_cluster[on]].astype(np.float64) - v[on].astype(np.float64)
        d = ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]).astype(np.float32)
    return float(np.sqrt(np.float64(d.max())))


def rewrite_faces(faces, vertex_cluster):
    """-> dict(faces (F,3) int32 the cluster ids, keep (F,) uint8, nonfinite_faces, degenerate_faces, duplicate_faces)."""
    f = check_faces(faces, len(vertex_cluster))
    F = len(f)
    ids = vertex_cluster[f].astype(np.int32).reshape(F, 3)
    nonfinite = (ids < 0).any(1)
    degenerate = ~nonfinite & ((ids[:, 0] == ids[:, 1]) | (ids[:, 1] == ids[:, 2]) | (ids[:, 0] == ids[:, 2]))
    live = np.nonzero(~nonfinite & ~degenerate)[0]
    keep = np.zeros(F, np.uint8)
    if len(live):
        triples = np.sort(ids[live].astype(np.int64), 1)
        _, first = np.unique(triples, axis=0, return_index=True)            # the first occurrence: the lowest face index of the set
        keep[live[first]] = 1
    return dict(faces=ids, keep=keep, nonfinite_faces=int(nonfinite.sum()), degenerate_faces=int(degenerate.sum()),
                duplicate_faces=int(len(live) - keep.sum()))


def simplify(vertices, colors, faces, cell, origin, placement='quadric', rank_epsilon=1e-3):
    """Everything: the intermediates of every stage under their names, and the result `out` = (vertices, colors, faces) after
    mesh_topology_restated.select (`cluster_map` (C,): a cluster's row in it, or -1), with `counts` (clusters, vertices_in/out, faces_in/out, the three drops, placed_by_quadric,
    fell_back) and `max_move`."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = check_faces(faces, len(v))
    cl = cluster(v, colors, cell, origin)
    C = len(cl['counts'])
    Q, inc = quadrics(v, f, cl['vertex_cluster'], C, cell, origin)
    pl = place(cl['cells'], cl['counts'], cl['position_sums'], cl['color_sums'], Q, cell, origin, placement, rank_epsilon)
    rw = rewrite_faces(f, cl['vertex_cluster'])
    out_v, out_c, out_f, vertex_map = T.select(pl['positions'], pl['colors'], rw['faces'], rw['keep'])
    placed = int(pl['placed'].sum())
    counts = dict(clusters=C, vertices_in=len(v), vertices_out=len(out_v), faces_in=len(f), faces_out=len(out_f),
                  nonfinite_faces=rw['nonfinite_faces'], degenerate_faces=rw['degenerate_faces'], duplicate_faces=rw['duplicate_faces'],
                  placed_by_quadric=placed, fell_back=(C - placed) if placement == 'quadric' else 0)
    return dict(cluster=cl, quadrics=Q, incidences=inc, place=pl, rewrite=rw, out=(out_v, out_c, out_f), cluster_map=vertex_map, counts=counts,
                max_move=max_move(v, cl['vertex_cluster'], pl['positions']))
