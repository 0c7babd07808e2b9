"""The meshes and queries the point-to-triangle distance is held to (tests/test_mesh_distance_host.py on the restatement alone,
tests/test_gpu_mesh_distance.py on the kernels).  The meshes of tests/mesh_simplify_cases.py and mesh_sample_cases' `debris_bad_index`
are imported read-only; three small meshes are made here:

    single_face      one face, radius 1/8, queries constructed to land in each of the seven regions, the three corners themselves
                     (distance 0), and beside corner a a query at distance EXACTLY the radius (found) and four steps further (not found)
    axis_face        one face in the plane z = 0 with representable coordinates: queries exactly on the plane, on an edge, on a vertex
    cube             1728 faces: more than a workgroup of queries, many cells
    big_triangles    two faces that span tens of cells per axis: the reference budget and its coarsening
    sheets           two surfaces 0.02 apart, radius 0.05
    debris_bad_index faces with an index out of range, NaN and inf vertices, zero-area faces
    zero_area        a repeated vertex (a, a, b), a point (a, a, a), a collinear triple, beside one proper face
    twice            one face given twice and a third over a shared edge, queries straight above that edge: the lowest index wins

Every case has queries near the surface (on a face, moved up to 1.6 radii in a random direction: some are beyond the radius), a few
more than a cell outside the box, and a NaN and two inf rows.  A few hundred to 1500 queries per case."""
import functools

import numpy as np

import mesh_distance_restated as R
import mesh_sample_cases as SC
import mesh_simplify_cases as K

NAMES = ['single_face', 'axis_face', 'cube', 'big_triangles', 'sheets', 'debris_bad_index', 'zero_area', 'twice']
RADIUS = {'single_face': 0.125, 'axis_face': 0.25, 'cube': 0.05, 'big_triangles': 0.3, 'sheets': 0.05, 'debris_bad_index': 0.3,
          'zero_area': 0.5, 'twice': 0.5}
NEAR = {'single_face': 300, 'axis_face': 200, 'cube': 1500, 'big_triangles': 1200, 'sheets': 1200, 'debris_bad_index': 600,
        'zero_area': 600, 'twice': 300}


def _f32(x):
    return np.ascontiguousarray(np.asarray(x, np.float64).astype(np.float32).reshape(-1, 3))


@functools.lru_cache(maxsize=None)
def mesh(name):
    """-> (vertices (V,3) float32, faces (F,3) int32): read-only."""
    if name == 'axis_face':
        return _f32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.array([[0, 1, 2]], np.int32)
    if name == 'zero_area':
        v = _f32([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.5],      # a proper face
                  [2.0, 0.5, 0.25], [3.0, 1.5, 0.75],                      # (a, a, b): the segment 3-4
                  [1.5, 2.0, 1.0],                                         # (a, a, a): a point
                  [2.0, -1.0, 0.0], [2.5, -1.0, 0.0], [3.5, -1.0, 0.0]])   # a collinear triple along x: the segment 6-8
        return v, np.array([[0, 1, 2], [3, 3, 4], [5, 5, 5], [7, 6, 8], [4, 3, 4]], np.int32)
    if name == 'twice':
        v = _f32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0]])
        return v, np.array([[0, 1, 2], [0, 1, 2], [1, 0, 3]], np.int32)
    if name == 'debris_bad_index':
        v, _, f = SC.mesh(name)
        return v, f
    c = K.case(name)
    return c['vertices'], c['faces']


def _near(v, f, radius, n, seed):
    """n queries: a uniform point of a random usable face, moved by up to 1.6 radii in a random direction."""
    rng = np.random.RandomState(seed)
    ids = np.nonzero(R.usable_faces(v, f))[0]
    pick = ids[rng.randint(0, len(ids), n)]
    a, b, c = (v[f[pick, k]].astype(np.float64) for k in range(3))
    u, w = rng.uniform(size=(2, n))
    flip = u + w > 1.0
    u, w = np.where(flip, 1.0 - u, u), np.where(flip, 1.0 - w, w)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return a + u[:, None] * (b - a) + w[:, None] * (c - a) + d * (1.6 * radius * rng.uniform(size=(n, 1)) ** 0.5)


def _constructed(name, v, f, radius):
    a, b, c = (v[f[0, k]].astype(np.float64) for k in range(3))
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n)
    g = (a + b + c) / 3.0
    if name == 'single_face':
        out = [a, b, c]                                                   # on a vertex: distance 0
        for lift in (0.0, 0.03, -0.06):
            out += [g + lift * n,                                         # interior
                    a + 0.15 * (a - g) + lift * n, b + 0.15 * (b - g) + lift * n, c + 0.15 * (c - g) + lift * n,      # A, B, C
                    0.5 * (a + b) + 0.1 * (0.5 * (a + b) - c) + lift * n,                                              # AB
                    0.5 * (a + c) + 0.1 * (0.5 * (a + c) - b) + lift * n,                                              # AC
                    0.5 * (b + c) + 0.1 * (0.5 * (b + c) - a) + lift * n,                                              # BC
                    0.5 * (a + b), 0.5 * (a + c), 0.5 * (b + c)]                                                       # on the edges
        a32 = v[f[0, 0]]
        exact = a32 - np.array([radius, 0, 0], np.float32)               # 0.1f - 0.125 is a float32: distance exactly the radius
        assert float(a32[0]) - float(exact[0]) == radius
        beyond = exact.copy()
        for _ in range(4):                                               # four steps: one alone still rounds to the radius squared
            beyond[0] = np.nextafter(beyond[0], np.float32(-np.inf))
        return np.concatenate([np.asarray(out), exact[None].astype(np.float64), beyond[None].astype(np.float64)])
    if name == 'axis_face':
        return np.array([[0.25, 0.25, 0.0], [0.5, 0.0, 0.0], [0.5, 0.5, 0.0], [0.0, 0.25, 0.0], [0, 0, 0], [1, 0, 0], [0, 1, 0],
                         [0.25, 0.25, 0.25], [0.25, 0.25, -0.25], [0.25, 0.25, 0.2500001], [0.5, -0.125, 0.0], [-0.125, -0.125, 0.0],
                         [1.125, 0.0, 0.0], [0.75, 0.75, 0.0], [0.0, 1.25, 0.0], [-0.25, 0.5, 0.0]])
    if name == 'twice':
        return np.array([[0.5, 0.0, 0.2], [0.25, 0.0, 0.125], [0.75, 0.0, -0.25], [0.5, 0.0, 0.0], [0.0, 0.0, 0.25], [1.0, 0.0, 0.25]])
    return np.zeros((0, 3))


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(name, vertices, faces, radius, queries (m,3) float32): read-only."""
    v, f = mesh(name)
    radius = RADIUS[name]
    used = v[np.unique(f[R.usable_faces(v, f)])].astype(np.float64)
    lo, hi = used.min(0), used.max(0)
    rng = np.random.RandomState(len(name))
    outside = np.concatenate([hi + radius * rng.uniform(2.2, 4.0, (6, 3)), lo - radius * rng.uniform(2.2, 4.0, (6, 3)),
                              [[lo[0] - 2.5 * radius, 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])]]])
    bad = np.array([[np.nan, lo[1], lo[2]], [lo[0], np.inf, lo[2]], [-np.inf, np.inf, hi[2]]])
    first = _f32(_constructed(name, v, f, radius))
    q = _f32(np.concatenate([_near(v, f, radius, NEAR[name], 3 + len(name)), outside, bad]))
    q = q[np.random.RandomState(1).permutation(len(q))]                  # the kinds interleaved: no workgroup holds one kind alone
    return dict(name=name, vertices=v, faces=f, radius=radius, queries=np.ascontiguousarray(np.concatenate([first, q])),
                constructed=len(first))


@functools.lru_cache(maxsize=None)
def restated(name):
    """(d2, face, closest, region) of the restatement, computed once and shared: treat it as read-only."""
    c = case(name)
    return R.nearest(c['vertices'], c['faces'], c['queries'], c['radius'], closest=True, census=True)
