"""The meshes the simplification is held to (tests/test_mesh_simplify_host.py on the restatement alone, tests/test_gpu_mesh_simplify.py
on the kernels).  A case is a dict: name, vertices (V,3) float32, colors (V,3) uint8 or None, faces (F,3) int32, cell, origin (3
floats).  The largest is the plane: 4900 vertices and about 310 clusters, so it crosses the 256-lane workgroup and the 2048-counter
scan tile; every small case runs the duplicate table at its minimum size."""
import functools

import numpy as np

import mesh_simplify_restated as S

NAMES = ['cube', 'cube_far', 'sphere', 'plane', 'sheets', 'debris', 'one_cell', 'big_triangles', 'single_face']
CUBE_CORNER, CUBE_EDGE, CUBE_QUADS = (0.013, 0.027, 0.041), 1.0, 12
FAR = 1000.0
SPHERE_CENTRE = (0.011, 0.023, 0.037)          # off the lattice's symmetry: no eigenvalue pair or cell wall is hit exactly


def _colors(V, seed):
    return np.random.RandomState(seed).randint(0, 256, (V, 3)).astype(np.uint8)


def _grid_faces(index, flip=False):
    """index (n,m) of vertex ids -> the 2 (n-1)(m-1) triangles of the grid's quads, wound one way (flip: the other)."""
    a, b, c, d = index[:-1, :-1].ravel(), index[1:, :-1].ravel(), index[1:, 1:].ravel(), index[:-1, 1:].ravel()
    f = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    return f[:, ::-1] if flip else f


def cube_surface(corner, edge, quads):
    """The surface of an axis-aligned cube as quads x quads quads per side, vertices shared along the edges, wound outward."""
    n = quads + 1
    ijk = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing='ij'), -1).reshape(-1, 3)
    on = ((ijk == 0) | (ijk == quads)).any(1)
    ids = np.full(n ** 3, -1, np.int64)
    ids[on] = np.arange(on.sum())
    ids = ids.reshape(n, n, n)
    vertices = np.asarray(corner, np.float64) + ijk[on] * (float(edge) / quads)
    faces = []
    for axis in range(3):
        for side in (0, quads):
            index = np.take(ids, side, axis=axis)
            faces.append(_grid_faces(index, flip=(side == 0) != (axis == 1)))
    return vertices, np.concatenate(faces)


def uv_sphere(segments, rings, radius):
    theta = np.pi * np.arange(1, rings) / rings
    phi = 2.0 * np.pi * np.arange(segments) / segments
    body = np.stack([np.outer(np.sin(theta), np.cos(phi)), np.outer(np.sin(theta), np.sin(phi)),
                     np.outer(np.cos(theta), np.ones(segments))], -1).reshape(-1, 3)
    vertices = radius * np.concatenate([[[0.0, 0.0, 1.0]], body, [[0.0, 0.0, -1.0]]])
    index = 1 + np.arange((rings - 1) * segments).reshape(rings - 1, segments)
    index = np.concatenate([index, index[:, :1]], 1)
    faces = [_grid_faces(index)]
    south = 1 + (rings - 1) * segments
    for s in range(segments):
        faces.append(np.array([[0, index[0, s], index[0, s + 1]], [south, index[-1, s + 1], index[-1, s]]]))
    return vertices, np.concatenate(faces)


def _case(name, vertices, faces, cell, origin, colors='random'):
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    if isinstance(colors, str):
        colors = _colors(len(v), len(name))
    return dict(name=name, vertices=v, colors=colors, faces=np.ascontiguousarray(faces, np.int32).reshape(-1, 3), cell=float(cell),
                origin=tuple(float(o) for o in origin))


@functools.lru_cache(maxsize=None)
def case(name):
    if name == 'cube':
        v, f = cube_surface(CUBE_CORNER, CUBE_EDGE, CUBE_QUADS)
        return _case(name, v, f, 0.25, (-0.1, -0.1, -0.1))
    if name == 'cube_far':
        v, f = cube_surface(CUBE_CORNER, CUBE_EDGE, CUBE_QUADS)
        return _case(name, v + FAR, f, 0.25, (FAR - 0.1, FAR - 0.1, FAR - 0.1), colors=None)
    if name == 'sphere':
        v, f = uv_sphere(64, 32, 1.0)
        return _case(name, v + SPHERE_CENTRE, f, 0.25, (-1.0, -1.0, -1.0))
    if name == 'plane':
        rng = np.random.RandomState(11)
        x, y = np.meshgrid(0.02 * np.arange(70), 0.02 * np.arange(70), indexing='ij')
        z = 0.3 * x + 0.2 * y + 0.002 * rng.standard_normal(x.shape)
        f = _grid_faces(np.arange(4900).reshape(70, 70))
        return _case(name, np.stack([x, y, z], -1), f, 0.1, (-0.013, -0.017, -0.05))
    if name == 'sheets':
        x, y = np.meshgrid(0.02 * np.arange(30), 0.02 * np.arange(30), indexing='ij')
        index = np.arange(900).reshape(30, 30)
        v = np.concatenate([np.stack([x, y, np.full_like(x, 0.03)], -1).reshape(-1, 3), np.stack([x, y, np.full_like(x, 0.05)], -1).reshape(-1, 3)])
        f = np.concatenate([_grid_faces(index), _grid_faces(index + 900, flip=True)])
        return _case(name, v, f, 0.1, (-0.007, -0.003, 0.0), colors=None)
    if name == 'debris':
        return _debris()
    if name == 'one_cell':
        v, f = uv_sphere(12, 6, 0.2)
        return _case(name, v + 0.5, f, 1.0, (0.0, 0.0, 0.0))
    if name == 'big_triangles':
        v = np.array([[0.3, 0.2, 0.1], [10.4, 0.3, 0.2], [0.2, 10.1, 0.4], [10.3, 10.2, 3.3]])
        return _case(name, v, [[0, 1, 2], [1, 3, 2]], 1.0, (0.0, 0.0, 0.0))
    if name == 'single_face':
        return _case(name, [[0.1, 0.1, 0.1], [0.9, 0.2, 0.1], [0.2, 0.8, 0.6]], [[0, 1, 2]], 0.35, (0.0, 0.0, 0.0))
    raise KeyError(name)


def _debris():
    """One mesh holding: a zero-area face, faces (a,a,b) and (a,a,a), an unreferenced vertex, a vertex with NaN and one with inf and
    faces naming them, two faces with the same three clusters in another order, and colours whose channel sums need the rounding
    rule (k = 2 with an odd sum rounds up, k = 3 with remainders 1 and 2)."""
    v = np.array([[0.10, 0.10, 0.10],      # 0  cell (0,0,0)
                  [0.30, 0.20, 0.10],      # 1  cell (0,0,0)
                  [1.20, 0.10, 0.30],      # 2  cell (1,0,0)
                  [0.20, 1.30, 0.20],      # 3  cell (0,1,0)
                  [1.40, 1.10, 0.40],      # 4  cell (1,1,0)
                  [1.60, 0.30, 0.20],      # 5  cell (1,0,0)
                  [0.40, 1.70, 0.10],      # 6  cell (0,1,0)
                  [1.80, 0.50, 0.60],      # 7  cell (1,0,0)
                  [2.50, 2.50, 2.50],      # 8  unreferenced, a cluster of its own
                  [np.nan, 0.5, 0.5],      # 9
                  [0.5, np.inf, 0.5],      # 10
                  [2.20, 0.20, 0.20],      # 11 cell (2,0,0)
                  [2.40, 0.20, 0.20],      # 12 cell (2,0,0), collinear with 11 and 13
                  [2.80, 0.20, 0.20],      # 13 cell (2,0,0)
                  [3.30, 0.40, 0.20]],     # 14 cell (3,0,0)
                 np.float64)
    f = [[0, 2, 3],        # clusters A B C
         [5, 6, 1],        # the same set from other vertices, another order: a duplicate
         [2, 4, 3],
         [11, 12, 13],     # zero area, one cluster
         [2, 14, 12],      # a live face over cells (1,0,0), (3,0,0), (2,0,0)
         [2, 12, 14],      # the same set, the other winding: a duplicate
         [0, 0, 2],        # (a, a, b)
         [4, 4, 4],        # (a, a, a)
         [0, 9, 2],        # names the NaN vertex
         [10, 3, 4],       # names the inf vertex
         [3, 7, 4],
         [0, 1, 2]]        # two vertices in one cluster: degenerate
    c = np.zeros((len(v), 3), np.uint8)
    c[0], c[1] = (10, 255, 1), (11, 254, 2)                 # k = 2: sums 21 (odd: 10.5 -> 11), 509 (254.5 -> 255), 3 (1.5 -> 2)
    c[2], c[5], c[7] = (1, 2, 200), (1, 3, 100), (2, 3, 101)    # k = 3: sums 4 (1.33 -> 1), 8 (2.67 -> 3), 401 (133.67 -> 134)
    c[3:5] = (7, 8, 9)
    c[6] = (8, 8, 8)
    c[8:] = (50, 60, 70)
    return _case('debris', v, f, 1.0, (0.0, 0.0, 0.0), colors=c)


@functools.lru_cache(maxsize=None)
def restated(name, placement='quadric'):
    """The restatement of a case, computed once and shared: treat it as read-only."""
    c = case(name)
    return S.simplify(c['vertices'], c['colors'], c['faces'], c['cell'], c['origin'], placement)
