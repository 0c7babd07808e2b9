"""The mesh topology kernels' definitions (include/atvsnet_hip.h, csrc/mesh_topology.hip) restated in numpy alone: connected
components by a sequential union-find, the selection of faces with the vertices compacted, the edge census by numpy.unique.
What the GPU tests compare the ops against, bit for bit, and what the host tests hold to known answers."""
import numpy as np

CENSUS_WORDS = ('edges', 'boundary', 'manifold', 'nonmanifold', 'misoriented', 'max_faces_per_edge', 'self_edges', 'error')


def bad_faces(faces, num_vertices):
    """The number of faces with an index outside 0..num_vertices-1."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return int(((f < 0) | (f >= int(num_vertices))).any(axis=1).sum())


def components(faces, num_vertices):
    """-> (vertex_component (V,) int32, face_component (F,) int32, face_count (C,) int32, vertex_count (C,) int32): the label of a
    vertex is the smallest vertex index it is connected to, by a plain sequential union-find in which the smaller root stays the
    root; the dense ids number the labels in ascending order."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = int(num_vertices)
    if bad_faces(f, V):
        raise ValueError('%d of %d faces have a vertex index outside 0..%d' % (bad_faces(f, V), len(f), V - 1))
    parent = list(range(V))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for a, b, c in f.tolist():
        for x, y in ((a, b), (b, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)                             # the smaller index stays the root
    label = np.array([find(x) for x in range(V)], np.int64).reshape(-1)
    referenced = np.zeros(V, bool)
    referenced[f.reshape(-1)] = True
    roots = np.flatnonzero(referenced & (label == np.arange(V)))              # ascending: the dense order
    dense = np.full(V, -1, np.int64)
    dense[roots] = np.arange(len(roots))
    vertex_component = np.where(referenced, dense[label], -1).astype(np.int32)
    face_component = vertex_component[f[:, 0]].astype(np.int32) if len(f) else np.zeros(0, np.int32)
    face_count = np.bincount(face_component, minlength=len(roots)).astype(np.int32)
    vertex_count = np.bincount(vertex_component[referenced], minlength=len(roots)).astype(np.int32)
    return vertex_component, face_component, face_count, vertex_count


def select(vertices, colors, faces, keep):
    """-> (vertices (V',3), colors (V',3) or None, faces (F',3) int32, vertex_map (V,) int32).  Rows are copied as bytes."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    kept = f[np.asarray(keep).reshape(-1) != 0]
    if bad_faces(kept, len(v)):
        raise ValueError('%d of %d faces have a vertex index outside 0..%d' % (bad_faces(kept, len(v)), len(f), len(v) - 1))
    used = np.zeros(len(v), bool)
    used[kept.reshape(-1)] = True
    vertex_map = np.where(used, np.cumsum(used) - 1, -1).astype(np.int32)
    out_v = v.view(np.uint32)[used].view(np.float32)                          # as bits
    out_c = None if colors is None else np.asarray(colors, np.uint8).reshape(-1, 3)[used]
    return out_v, out_c, vertex_map[kept].astype(np.int32).reshape(-1, 3), vertex_map


def edge_census(faces, num_vertices):
    """-> {word: int} over the distinct sorted pairs of the faces' 3F pairs (f0,f1), (f1,f2), (f2,f0)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = int(num_vertices)
    if bad_faces(f, V):
        raise ValueError('%d of %d faces have a vertex index outside 0..%d' % (bad_faces(f, V), len(f), V - 1))
    out = dict.fromkeys(CENSUS_WORDS, 0)
    if not len(f):
        return out
    pairs = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    lo, hi = pairs.min(axis=1), pairs.max(axis=1)
    forward = pairs[:, 0] <= pairs[:, 1]                                      # given as (lo, hi); a pair with lo == hi is
    keys, inverse = np.unique((lo << 32) | hi, return_inverse=True)
    inverse = inverse.reshape(-1)
    fwd = np.bincount(inverse[forward], minlength=len(keys))
    bwd = np.bincount(inverse[~forward], minlength=len(keys))
    n = fwd + bwd
    out.update(edges=int(len(keys)), boundary=int((n == 1).sum()), manifold=int((n == 2).sum()), nonmanifold=int((n > 2).sum()),
               misoriented=int(((fwd >= 2) | (bwd >= 2)).sum()), max_faces_per_edge=int(n.max()),
               self_edges=int(((keys >> 32) == (keys & 0xffffffff)).sum()))
    return out


def clean(vertices, colors, faces, keep_components):
    """The mesh without the components whose flag in keep_components (C,) is false -> select's outputs."""
    _, face_component, _, _ = components(faces, len(vertices))
    return select(vertices, colors, faces, np.asarray(keep_components, bool)[face_component].astype(np.uint8))
