"""The definitions of ops.tsdf_integrate and ops.tsdf_mesh (include/atvsnet_hip.h) restated in numpy on a DENSE grid, independent
of the kernels' block structure: `integrate` visits every voxel of the box for every view, `mesh` walks the cubes of a dense
[z][y][x] array.  The blocks only give the ORDER of vertices and faces (blocks ascending, x fastest inside a block).

The orientation rule is not tabulated here: each triangle's normal is computed from the midpoints of its edges and tested
against (centroid of the outside corners - centroid of the inside corners), in exact integer arithmetic on doubled lattice
coordinates.  With it the helpers the tests share: analytic sphere depth maps, edge statistics of a mesh."""
import itertools
from collections import Counter

import numpy as np

EDGES = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]       # offsets (x, y, z) of the owned edge types
PERMS = list(itertools.permutations(range(3)))          # xyz, xzy, yxz, yzx, zxy, zyx


def centres(origin, voxel, n, axis):
    """float64 (n,): the centres of the voxels 0..n-1 along one axis, origin + ((double)i + 0.5) * voxel."""
    return float(origin[axis]) + (np.arange(n, dtype=np.float64) + 0.5) * float(voxel)


def integrate(depths, cams, voxel, trunc, origin, dims, images=None, pixel_centre=0.0):
    """-> dict(tsdf, weight (nz,ny,nx) float32, color (nz,ny,nx,3) float32 or None, blocks (nb,3) int32): every voxel of the box
    (dims blocks of 8^3) against every view, float64 in the stated order."""
    depths = np.asarray(depths, np.float32)
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    n, rows, cols = depths.shape
    bx, by, bz = dims
    nx, ny, nz = bx * 8, by * 8, bz * 8
    Z, Y, X = np.meshgrid(centres(origin, voxel, nz, 2), centres(origin, voxel, ny, 1), centres(origin, voxel, nx, 0), indexing='ij')
    S = np.zeros((nz, ny, nx), np.float64)
    W = np.zeros((nz, ny, nx), np.float64)
    C = np.zeros((nz, ny, nx, 3), np.float64)
    trunc = float(trunc)
    for k in range(n):
        c = cams[k]
        with np.errstate(all='ignore'):
            c2 = ((c[6] * X + c[7] * Y) + c[8] * Z) + c[11]
            z = c2.astype(np.float32)
            c0 = ((c[0] * X + c[1] * Y) + c[2] * Z) + c[9]
            c1 = ((c[3] * X + c[4] * Y) + c[5] * Z) + c[10]
            x = (c0 / c2) * c[12] + c[14]
            y = (c1 / c2) * c[13] + c[15]
            xs = (x - float(pixel_centre)) + 0.5
            ys = (y - float(pixel_centre)) + 0.5
            ok = (c2 > 0.0) & np.isfinite(z) & (z > 0) & (xs >= 0.0) & (xs < float(cols)) & (ys >= 0.0) & (ys < float(rows))
        u = np.where(ok, np.floor(np.where(ok, xs, 0.0)), 0).astype(np.int64)
        v = np.where(ok, np.floor(np.where(ok, ys, 0.0)), 0).astype(np.int64)
        d = depths[k][v, u]
        with np.errstate(all='ignore'):
            sdf = d.astype(np.float64) - c2
            ok &= (d > 0) & np.isfinite(d) & (sdf >= -trunc) & (sdf <= trunc)
        S[ok] += sdf[ok] / trunc
        W[ok] += 1.0
        if images is not None:
            C[ok] += np.asarray(images[k], np.float32)[v[ok], u[ok], :3].astype(np.float64)
    has = W > 0
    with np.errstate(all='ignore'):
        tsdf = np.where(has, S / W, 0.0).astype(np.float32)
        color = None if images is None else np.where(has[..., None], C / W[..., None], 0.0).astype(np.float32)
    weight = W.astype(np.float32)
    occupied = has.reshape(bz, 8, by, 8, bx, 8).any(axis=(1, 3, 5))
    zz, yy, xx = np.nonzero(occupied)                    # ascending in (z by + y) bx + x
    return dict(tsdf=tsdf, weight=weight, color=color, blocks=np.stack([xx, yy, zz], axis=1).astype(np.int32).reshape(-1, 3))


def _order_key(v, bx, by):
    """Where voxel v = (i, j, k) stands in the kernels' order: its block's linear index, then [z][y][x] inside the block."""
    i, j, k = v
    return (((k >> 3) * by + (j >> 3)) * bx + (i >> 3)) * 512 + (k & 7) * 64 + (j & 7) * 8 + (i & 7)


def _tetra_triangles(corners, inside):
    """The triangles of one tetrahedron: corners = 4 lattice points (local vertices 0..3), inside = 4 bools -> a list of triangles,
    each 3 edges, an edge = (local vertex, local vertex); oriented from the geometry."""
    ins = [q for q in range(4) if inside[q]]
    out = [q for q in range(4) if not inside[q]]
    if not ins or not out:
        return []
    if len(ins) == 1 or len(out) == 1:
        s = ins[0] if len(ins) == 1 else out[0]
        tris = [[(s, q) for q in range(4) if q != s]]
    else:
        (a, b), (c, d) = ins, out
        tris = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
    P = [np.array(c, np.int64) for c in corners]
    # (centroid of outside - centroid of inside) * len(ins) * len(out): integers
    direction = len(ins) * sum(P[q] for q in out) - len(out) * sum(P[q] for q in ins)
    oriented = []
    for tri in tris:
        m = [P[x] + P[y] for x, y in tri]                # twice the midpoints
        normal = np.cross(m[1] - m[0], m[2] - m[0])
        if int(normal @ direction) < 0:
            tri = [tri[0], tri[2], tri[1]]
        oriented.append(tri)
    return oriented


def mesh(tsdf, weight, color, origin, voxel, min_weight=1.0, with_edges=False):
    """Dense [z][y][x] arrays -> (vertices (V,3) float32, colors (V,3) uint8 r, g, b or None, faces (F,3) int32); with_edges: and
    every vertex's edge as (lower voxel (i, j, k), edge type).
    Special values: valid is weight >= min_weight and inside is tsdf < 0 as float32 comparisons (a NaN is neither), t, p and the
    colour expression are plain IEEE double arithmetic, and a colour is floor(x + 0.5), then 0 unless >= 0, then 255 unless <= 255."""
    f = np.asarray(tsdf, np.float32)
    w = np.asarray(weight, np.float32)
    nz, ny, nx = f.shape
    bx, by = -(-nx // 8), -(-ny // 8)
    with np.errstate(invalid='ignore'):
        valid = w >= np.float32(min_weight)
        inside = f < 0
    ok = np.ones((nz - 1, ny - 1, nx - 1), bool)
    n_in = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        sl = (slice(dz, nz - 1 + dz), slice(dy, ny - 1 + dy), slice(dx, nx - 1 + dx))
        ok &= valid[sl]
        n_in += inside[sl]
    kk, jj, ii = np.nonzero(ok & (n_in > 0) & (n_in < 8))
    cubes = sorted(zip(ii.tolist(), jj.tolist(), kk.tolist()), key=lambda v: _order_key(v, bx, by))
    unit = np.eye(3, dtype=np.int64)
    tri_edges = []                                        # per triangle 3 edges, an edge = (lower voxel, edge type)
    for cube in cubes:
        o = np.array(cube, np.int64)
        for p in PERMS:
            corners = [o, o + unit[p[0]], o + unit[p[0]] + unit[p[1]], o + 1]
            ins = [bool(inside[c[2], c[1], c[0]]) for c in corners]
            for tri in _tetra_triangles(corners, ins):
                edges = []
                for x, y in tri:
                    lo, hi = (x, y) if x < y else (y, x)
                    edges.append((tuple(corners[lo].tolist()), EDGES.index(tuple((corners[hi] - corners[lo]).tolist()))))
                tri_edges.append(edges)
    owned = sorted({e for tri in tri_edges for e in tri}, key=lambda e: (_order_key(e[0], bx, by), e[1]))
    index = {e: n for n, e in enumerate(owned)}
    vertices = np.zeros((len(owned), 3), np.float32)
    colors = None if color is None else np.zeros((len(owned), 3), np.uint8)
    org = [float(v) for v in origin]
    voxel = float(voxel)
    for n, (a, kind) in enumerate(owned):
        b = tuple(a[c] + EDGES[kind][c] for c in range(3))
        fa, fb = float(f[a[2], a[1], a[0]]), float(f[b[2], b[1], b[0]])
        assert (fa < 0) != (fb < 0)
        t = fa / (fa - fb)
        for c in range(3):
            pa = org[c] + (float(a[c]) + 0.5) * voxel
            pb = org[c] + (float(b[c]) + 0.5) * voxel
            vertices[n, c] = np.float32(pa + t * (pb - pa))
        if color is not None:
            for c in range(3):
                ca, cb = float(color[a[2], a[1], a[0], c]), float(color[b[2], b[1], b[0], c])
                x = float(np.floor((ca + t * (cb - ca)) + 0.5))     # plain IEEE: inf - inf and 0 * inf are NaN
                x = x if x >= 0.0 else 0.0                           # a NaN and -inf go to 0
                x = x if x <= 255.0 else 255.0                       # +inf to 255
                colors[n, 2 - c] = int(x)
    faces = np.zeros((len(tri_edges), 3), np.int32)
    for n, tri in enumerate(tri_edges):
        v = [index[e] for e in tri]
        r = v.index(min(v))
        faces[n] = v[r:] + v[:r]
    if with_edges:
        return vertices, colors, faces.reshape(-1, 3), owned
    return vertices, colors, faces.reshape(-1, 3)


def mesh_of_volume(volume, min_weight=1.0):
    """The restated mesh of an ops.TsdfVolume (through to_dense)."""
    f, w, c = volume.to_dense()
    return mesh(f, w, c, volume.origin, volume.voxel, min_weight)


# ----------------------------------------------------------------------------------------------------------------------------------
# what the tests share
# ----------------------------------------------------------------------------------------------------------------------------------
def sphere_field(n=32, h=1.0, r=10.3, centre=(15.7, 16.2, 15.1)):
    """The exact distance field of a sphere on an n^3 grid of spacing h with origin 0, [z][y][x], cast to float32."""
    a = (np.arange(n, dtype=np.float64) + 0.5) * h
    Z, Y, X = np.meshgrid(a, a, a, indexing='ij')
    return (np.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) - r).astype(np.float32)


def sphere_depths(cams, rows, cols, radius, pixel_centre=0.0):
    """Analytic z-depth maps of the sphere of `radius` at the origin: ray-sphere through every pixel centre -> (depths (n,rows,cols)
    float32, 0 where the ray misses; images (n,rows,cols,3) float32 b, g, r in 0..255, a smooth function of the hit point)."""
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    depths = np.zeros((len(cams), rows, cols), np.float32)
    images = np.zeros((len(cams), rows, cols, 3), np.float32)
    v, u = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing='ij')
    for k, c in enumerate(cams):
        R, t = c[:9].reshape(3, 3), c[9:12]
        centre = -R.T @ t
        ray = np.stack([(u + pixel_centre - c[14]) / c[12], (v + pixel_centre - c[15]) / c[13], np.ones_like(u)], axis=-1)     # z = 1
        dirs = ray @ R                                    # R^T ray, per pixel
        A = (dirs * dirs).sum(-1)
        B = 2.0 * (dirs @ centre)
        Cc = centre @ centre - radius * radius
        disc = B * B - 4.0 * A * Cc
        hit = disc > 0
        s = np.where(hit, (-B - np.sqrt(np.where(hit, disc, 0.0))) / (2.0 * A), 0.0)          # the ray is scaled to z = 1: s is the z-depth
        hit &= s > 0
        depths[k] = np.where(hit, s, 0.0).astype(np.float32)
        point = centre + dirs * s[..., None]
        images[k] = np.where(hit[..., None], 127.5 + 120.0 * np.sin(3.0 * point + np.array([0.0, 1.0, 2.0])), 0.0).astype(np.float32)
    return depths, images


def edge_stats(faces):
    """-> (directed: Counter of (a, b) over the faces' directed edges, undirected: Counter of frozenset((a, b)))."""
    directed, undirected = Counter(), Counter()
    for t in np.asarray(faces).tolist():
        for q in range(3):
            a, b = t[q], t[(q + 1) % 3]
            directed[(a, b)] += 1
            undirected[(min(a, b), max(a, b))] += 1
    return directed, undirected
