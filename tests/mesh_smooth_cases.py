"""The meshes of the smoothing tests (tests/test_mesh_smooth_host.py, tests/test_gpu_mesh_smooth.py): the smallest shapes at which
the kernels of csrc/mesh_smooth.hip can go wrong.  mesh(name) -> (vertices (V,3) float32, faces (F,3) int32), the same arrays every
time; restated(name, pin) -> the restatement's results for the case, computed once and shared (read-only).

    tetra         4 vertices, 4 faces, closed
    sheet         a flat 7 x 7 regular grid of spacing 1/8, one diagonal direction, at an offset of (1000, -3, 0.25): with the
                  boundary pinned every interior vertex's mean is itself exactly
    noisy_sheet   the same with z noise
    noisy_sphere  an icosphere of 3 subdivisions (642 vertices, 1280 faces), radii times 1 + 0.02 default_rng(7).standard_normal(V)
    sphere4       4 subdivisions (2562 vertices, 5120 faces): rows cross the scan's 2048 tile, the table exceeds its minimum slots
    fan           a hub of valence 300 (more than a wavefront, more than a workgroup's 256 threads) with its rim
    dirty         a duplicated face, faces (a,a,b) and (a,a,a), two faces on one edge with opposite windings, an edge with three
                  faces, a vertex no face names, a NaN and an Inf vertex that faces name, negative coordinates
    no_vertices   V = 0, F = 0;   no_faces   V = 5, F = 0
"""
import functools

import numpy as np

import mesh_smooth_restated as R

NAMES = ('tetra', 'sheet', 'noisy_sheet', 'noisy_sphere', 'sphere4', 'fan', 'dirty', 'no_vertices', 'no_faces')
TAUBIN = (0.5, -0.53)
ITERATIONS = 3                      # six passes


def icosphere(subdivisions):
    """The icosahedron subdivided `subdivisions` times (each face into four, midpoints pushed to the unit sphere), in float64;
    faces wound so that their normals point outward."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        middle, out = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in middle:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                middle[key] = len(v) - 1
            return middle[key]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return np.asarray(v, np.float64), np.asarray(f, np.int32)


def _sheet(noise):
    n, h = 7, 0.125
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    v = np.stack([1000.0 + h * x, -3.0 + h * y, np.full(x.shape, 0.25)], -1).reshape(-1, 3)
    if noise:
        v[:, 2] += 0.01 * np.random.default_rng(11).standard_normal(len(v))
    i = (y[:-1, :-1] * n + x[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([i, i + 1, i + n + 1], 1), np.stack([i, i + n + 1, i + n], 1)])
    return v.astype(np.float32), f.astype(np.int32)


def _fan():
    k = 300
    a = 2.0 * np.pi * np.arange(k) / k
    v = np.concatenate([[[0.0, 0.0, 0.3]], np.stack([np.cos(a), np.sin(a), 0.05 * np.sin(7 * a)], 1)])
    i = np.arange(k)
    return v.astype(np.float32), np.stack([np.zeros(k, np.int64), 1 + i, 1 + (i + 1) % k], 1).astype(np.int32)


def _dirty():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.2], [-1, -1, -1], [0.5, 0.5, 1], [5, 5, 5], [np.nan, 0, 0], [2, np.inf, 0],
                  [2, 0, 0.1], [2, 1, -0.1]], np.float32)
    f = np.array([[0, 1, 2], [0, 1, 2], [1, 3, 2], [1, 3, 9], [4, 4, 0], [5, 5, 5], [3, 9, 10], [2, 3, 7], [3, 10, 8]], np.int32)
    return v, f


# what the dirty case says, by hand: the distinct pairs with their faces are (0,1) 2, (0,2) 2, (1,2) 3, (1,3) 2, (2,3) 2, (3,9) 2,
# (1,9) 1, (0,4) 2, (9,10) 1, (3,10) 2; vertices 5 (only (5,5,5) names it) and 6 (no face) are isolated, 7 and 8 are not finite
DIRTY = dict(degree=[3, 4, 3, 4, 1, 0, 0, 0, 0, 3, 2], flags=[1, 7, 5, 1, 1, 1, 1, 0, 0, 3, 3],
             info=dict(pairs=10, boundary_pairs=2, nonmanifold_pairs=1, skipped_index_faces=0, self_pairs=4, nonfinite_pairs=4, unplaced_pairs=0))


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == 'tetra':
        v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float32)
        f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
    elif name in ('sheet', 'noisy_sheet'):
        v, f = _sheet(name == 'noisy_sheet')
    elif name == 'noisy_sphere':
        v, f = icosphere(3)
        v = (v * (1.0 + 0.02 * np.random.default_rng(7).standard_normal(len(v)))[:, None]).astype(np.float32)
    elif name == 'sphere4':
        v, f = icosphere(4)
        v = v.astype(np.float32)
    elif name == 'fan':
        v, f = _fan()
    elif name == 'dirty':
        v, f = _dirty()
    elif name == 'no_vertices':
        v, f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    elif name == 'no_faces':
        v, f = np.random.default_rng(3).standard_normal((5, 3)).astype(np.float32), np.zeros((0, 3), np.int32)
    else:
        raise KeyError(name)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def mesh(name):
    return _mesh(name)


@functools.lru_cache(maxsize=None)
def restated(name, pin=False):
    """dict(adjacency, origin, step, trace = [q0, q after each of the six passes], out, info, sums, incidences, normals, extent)."""
    v, f = mesh(name)
    trace = []
    out, info = R.smooth(v, f, ITERATIONS, TAUBIN[0], TAUBIN[1], pin, trace=trace)
    extent = R.face_extent(v, f)
    unit = extent['max_extent'] or 1.0
    sums, incidences = R.vertex_normal_sums(v, f, unit)
    return dict(adjacency=R.adjacency(v, f), origin=np.asarray(info['origin']), step=info['step'], trace=trace, out=out, info=info,
                extent=extent, sums=sums, incidences=incidences, normals=R.normals_from_sums(sums))
