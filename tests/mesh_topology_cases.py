"""The meshes the topology kernels are held to (tests/test_gpu_mesh_topology.py), with what each promises; the host test
(tests/test_mesh_topology_cases_host.py) asserts the promises on the restatement alone, so that a pass on the GPU means something.
A case is a dict: name, faces (F,3) int32, V, vertices (V,3) float32 and colors (V,3) uint8 (absent where V is too large to carry
them: census only), promise {what the restatement must find}."""
import functools

import numpy as np

import mesh_topology_restated as T
import tsdf_restated as R

H, RADIUS, CENTRE = 1.0, 10.3, (15.7, 16.2, 15.1)                 # the sphere of tests/test_tsdf_host.py
VERTEX_LIMIT = 1 << 30                                           # the wrappers' limit on vertices (ops.CLOUD_MAX_POINTS)
SHELLS = 40

NAMES = ['two_tetrahedra', 'strip_shuffled', 'strip_ascending', 'strip_descending', 'star_highest', 'star_lowest', 'isolated',
         'sphere_and_shells', 'fan', 'duplicated_face', 'self_edges', 'clipped_sphere', 'collisions', 'high_bits', 'last_vertices',
         'empty_v0', 'empty_v7', 'one_face']


def permuted(vertices, faces, V, seed, fixed=()):
    """Vertex indices renamed by a seeded shuffle (indices in `fixed` stay) and the faces reordered by another."""
    rng = np.random.RandomState(seed)
    free = np.setdiff1d(np.arange(V), np.asarray(fixed, np.int64))
    perm = np.arange(V)
    perm[free] = rng.permutation(free)
    faces = perm[np.asarray(faces, np.int64)][rng.permutation(len(faces))].astype(np.int32)
    if vertices is not None:
        out = np.empty_like(vertices)
        out[perm] = vertices
        vertices = out
    return vertices, faces


def _coordinates(V, seed):
    rng = np.random.RandomState(seed)
    return rng.standard_normal((V, 3)).astype(np.float32), rng.randint(0, 256, (V, 3)).astype(np.uint8)


TETRAHEDRON = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [0, 2, 3]], np.int64)
OCTAHEDRON_V = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
OCTAHEDRON_F = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int64)


@functools.lru_cache(maxsize=None)
def _sphere(clipped=False):
    field = R.sphere_field(32, H, RADIUS, CENTRE)
    weight = np.ones_like(field)
    if clipped:
        weight[:, :, 20:] = 0
    v, _, f = R.mesh(field, weight, None, (0.0, 0.0, 0.0), H)
    return v, f


@functools.lru_cache(maxsize=None)
def sphere_and_shells():
    """-> (vertices, faces, sphere faces' flags): the restated marching-tetrahedra sphere and SHELLS scaled octahedra outside it,
    vertex indices and face order shuffled."""
    v, f = _sphere()
    vs, fs = [v.astype(np.float64)], [f.astype(np.int64)]
    for k in range(SHELLS):
        a = 2.0 * np.pi * k / SHELLS
        centre = np.array(CENTRE) + 14.0 * np.array([np.cos(a), np.sin(a), 0.3 * np.sin(3 * a)])
        fs.append(OCTAHEDRON_F + sum(len(x) for x in vs))
        vs.append(centre + 0.3 * OCTAHEDRON_V)
    vertices, faces = np.concatenate(vs).astype(np.float32), np.concatenate(fs)
    of_sphere = np.arange(len(faces)) < len(f)
    rng = np.random.RandomState(5)
    order = rng.permutation(len(faces))
    perm = rng.permutation(len(vertices))
    out = np.empty_like(vertices)
    out[perm] = vertices
    return out, perm[faces][order].astype(np.int32), of_sphere[order]


@functools.lru_cache(maxsize=None)
def case(name):
    vertices = None
    promise = {}
    if name == 'two_tetrahedra':
        V = 16                                               # 4 + 4 + 3 referenced, 5 not: 0 and V - 1 among those
        faces = np.concatenate([TETRAHEDRON, TETRAHEDRON + 4, [[8, 9, 10]]]) + 1
        _, faces = permuted(None, faces, V, 1, fixed=(0, V - 1))
        promise = dict(C=3, sizes=[1, 4, 4], boundary=3, unreferenced=5, unreferenced_ends=True)
    elif name.startswith('strip_'):
        n = 20000
        V = n + 2
        faces = (np.arange(n)[:, None] + np.arange(3)[None, :]).astype(np.int32)
        if name == 'strip_shuffled':
            _, faces = permuted(None, faces, V, 2)
        elif name == 'strip_descending':
            faces = (V - 1 - faces).astype(np.int32)
        promise = dict(C=1, sizes=[n], boundary=n + 2)
    elif name.startswith('star_'):
        n = 8192
        V = 1 + 2 * n
        hub = V - 1 if name == 'star_highest' else 0
        rim = np.arange(2 * n).reshape(n, 2) + (1 if hub == 0 else 0)
        faces = np.concatenate([np.full((n, 1), hub), rim], axis=1)
        _, faces = permuted(None, faces, V, 3, fixed=(hub,))
        promise = dict(C=1, sizes=[n], boundary=3 * n)
    elif name == 'isolated':
        n = 5000                                             # C crosses the scan tile of 2048
        V = 3 * n
        _, faces = permuted(None, np.arange(V).reshape(n, 3), V, 4)
        promise = dict(C=n, sizes=[1] * 16, boundary=3 * n)
    elif name == 'sphere_and_shells':
        vertices, faces, _ = sphere_and_shells()
        V = len(vertices)
        promise = dict(C=SHELLS + 1, sizes=[8] * 15 + [11888], boundary=0)
    elif name == 'fan':
        V, faces = 5, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]])
        promise = dict(C=1, nonmanifold=1, max_faces_per_edge=3, boundary=6)
    elif name == 'duplicated_face':
        V, faces = 3, np.array([[0, 1, 2], [0, 1, 2]])
        promise = dict(C=1, misoriented=3, manifold=3, boundary=0)
    elif name == 'self_edges':
        V, faces = 5, np.array([[1, 1, 2], [3, 3, 3]])       # (1,1), (1,2) twice; (3,3) three times
        promise = dict(C=2, self_edges=2, edges=3, boundary=1, manifold=1, nonmanifold=1, max_faces_per_edge=3, unreferenced=2)
    elif name == 'clipped_sphere':
        vertices, faces = _sphere(clipped=True)
        V = len(vertices)
        vertices, faces = permuted(vertices, faces, V, 6)
        promise = dict(C=1, boundary_over=20)
    elif name == 'collisions':
        V = 24
        faces = np.random.RandomState(7).randint(0, V, (6000, 3))
        promise = dict(C=1, edges_at_most=V * (V + 1) // 2, max_over=20)
    elif name == 'high_bits':                                # census only: keys use the high bits of both halves
        V = VERTEX_LIMIT
        faces = np.array([[V - 1, V - 2, V - 3], [V - 2, V - 1, V - 4], [V - 5, V - 5, V - 1], [0, V - 1, 1 << 29]])
        promise = dict(census_only=True, edges=10, self_edges=1, manifold=2)
    elif name == 'last_vertices':
        V = (1 << 20) + 3
        faces = np.array([[V - 1, V - 2, V - 3], [V - 2, V - 1, V - 4], [V - 5, V - 5, V - 1], [0, V - 1, 1 << 19], [7, 8, 9]])
        promise = dict(C=2, sizes=[1, 4], self_edges=1)
    elif name == 'empty_v0':
        V, faces = 0, np.zeros((0, 3))
        promise = dict(C=0, edges=0)
    elif name == 'empty_v7':
        V, faces = 7, np.zeros((0, 3))
        promise = dict(C=0, edges=0, unreferenced=7)
    elif name == 'one_face':
        V, faces = 3, np.array([[2, 0, 1]])
        promise = dict(C=1, sizes=[1], boundary=3, edges=3)
    else:
        raise KeyError(name)
    out = dict(name=name, V=int(V), faces=np.ascontiguousarray(faces, np.int32).reshape(-1, 3), promise=promise)
    if not promise.get('census_only'):
        seed = NAMES.index(name)
        out['vertices'], out['colors'] = _coordinates(V, 100 + seed)
        if vertices is not None:
            out['vertices'] = np.ascontiguousarray(vertices, np.float32)
    return out


def check_promise(c):
    """Asserts on the restatement alone that case `c` has what it promises."""
    p, faces, V = c['promise'], c['faces'], c['V']
    census = T.edge_census(faces, V)
    assert census['error'] == 0 and census['edges'] == census['boundary'] + census['manifold'] + census['nonmanifold']
    _, undirected = R.edge_stats(faces)
    assert census['boundary'] == sum(1 for n in undirected.values() if n == 1) and census['edges'] == len(undirected)
    for word in ('edges', 'boundary', 'manifold', 'nonmanifold', 'misoriented', 'self_edges', 'max_faces_per_edge'):
        if word in p:
            assert census[word] == p[word], (word, census[word])
    if 'boundary_over' in p:
        assert census['boundary'] > p['boundary_over']
    if 'edges_at_most' in p:
        assert census['edges'] <= p['edges_at_most'] and census['max_faces_per_edge'] > p['max_over']
    if p.get('census_only'):
        assert V == VERTEX_LIMIT and int(faces.max()) == V - 1
        return
    vc, fc, face_count, vertex_count = T.components(faces, V)
    assert len(face_count) == len(vertex_count) == p['C']
    assert int(face_count.sum()) == len(faces) and int(vertex_count.sum()) == int((vc >= 0).sum())
    if 'sizes' in p:
        assert sorted(face_count.tolist())[-16:] == p['sizes']
    if 'unreferenced' in p:
        assert int((vc < 0).sum()) == p['unreferenced']
    if p.get('unreferenced_ends'):
        assert vc[0] == -1 and vc[-1] == -1
    if p['C']:
        first = np.array([np.flatnonzero(vc == k)[0] for k in range(min(p['C'], 64))])
        assert (np.diff(first) > 0).all()                    # ids in ascending order of the smallest vertex


def select_keeps(c):
    """The `keep` arrays a case is selected with: all, none, every third face."""
    F = len(c['faces'])
    return {'all': np.ones(F, np.uint8), 'none': np.zeros(F, np.uint8), 'third': (np.arange(F) % 3 == 0).astype(np.uint8) * 7}


def poisoned(vertices):
    """A copy with NaNs of several payloads, infinities and -0.0 among the coordinates."""
    v = vertices.copy()
    bits = v.view(np.uint32)
    bits[0::7, 0] = 0x7fc00001
    bits[1::7, 1] = 0xffc12345
    bits[2::7, 2] = 0x80000000
    bits[3::11, 0] = 0x7f800000
    bits[4::11, 1] = 0x7f800001                              # a signalling NaN
    return v


def bad_index_cases():
    """-> (faces, V, the number of faces with a bad index): an index of -1 and an index of V in one face each."""
    V = 4
    faces = np.array([[0, 1, 2], [2, -1, 3], [1, 2, 3], [3, 2, V], [0, 3, 1]], np.int32)
    return faces, V, 2
