"""The connectivity of a triangle mesh on the device (csrc/mesh_topology.hip): `mesh_components` labels the connected components
and counts their faces and vertices, `mesh_select` keeps a choice of faces with the vertices compacted and the faces renumbered,
`mesh_edge_census` counts the edges by the number of faces that share them.  The definitions are in include/atvsnet_hip.h and
restated in tests/mesh_topology_restated.py; atvsnet/clean_mesh.py (a mesh without its fragments) and mesh_fusion.mesh_report (the
boundary edges of a mesh on the device) are built on them.  Integer atomics only: the same inputs give the same bits."""

import torch

from .. import _lib
from .base import _call, _p, _size, _stream
from .cloud import CLOUD_MAX_POINTS, _int_in, _same_device
from .mesh import _launchable, _mesh_arg

MESH_TOPOLOGY_MAX_FACES = _lib.header_macro('ATVS_MESH_TOPOLOGY_MAX_FACES')
MESH_CENSUS_MIN_SLOTS = _lib.header_macro('ATVS_MESH_CENSUS_MIN_SLOTS')
MESH_CENSUS_WORDS = ('edges', 'boundary', 'manifold', 'nonmanifold', 'misoriented', 'max_faces_per_edge', 'self_edges', 'error')


def _bad_faces(op, bad, nf, nv):
    return ValueError('%s: %d of %d faces have a vertex index outside 0..%d' % (op, bad, nf, nv - 1))


def mesh_components(faces, num_vertices):
    """faces (F,3) int32, num_vertices V -> (vertex_component (V,) int32, face_component (F,) int32, face_count (C,) int32,
    vertex_count (C,) int32).  Two vertices are connected when one face names both (a face with repeated indices still connects
    what it names); vertex_component is -1 for a vertex no face names, else the dense id of its component, ids 0..C-1 in ascending
    order of the component's smallest vertex index; face_component is the component of the face's first vertex.  A face with an
    index outside 0..V-1 raises ValueError.  Synchronises once (the error word and C)."""
    nv = _int_in(num_vertices, 'num_vertices', 0, CLOUD_MAX_POINTS)
    _mesh_arg(faces, 'faces', torch.int32, (3,), MESH_TOPOLOGY_MAX_FACES)
    nf, dev = int(faces.shape[0]), faces.device
    most = max(1, min(nv, nf))
    vertex_component = torch.empty(nv, dtype=torch.int32, device=dev)
    face_component = torch.empty(nf, dtype=torch.int32, device=dev)
    face_count = torch.empty(most, dtype=torch.int32, device=dev)
    vertex_count = torch.empty(most, dtype=torch.int32, device=dev)
    if not _launchable(faces, 'faces'):
        return vertex_component, face_component, face_count[:0], vertex_count[:0]
    scratch = torch.empty(_size('atvs_mesh_components_scratch_size', nv, nf), dtype=torch.uint8, device=dev)
    info = torch.empty(2, dtype=torch.int32, device=dev)
    _call('atvs_mesh_components', _p(faces), nf, nv, _p(scratch), scratch.numel(), _p(vertex_component), _p(face_component),
          _p(face_count), _p(vertex_count), _p(info), _stream())
    bad, n_comp = (int(x) for x in info.cpu().tolist())
    if bad:
        raise _bad_faces('mesh_components', bad, nf, nv)
    return vertex_component, face_component, face_count[:n_comp], vertex_count[:n_comp]


def mesh_select(vertices, colors, faces, keep):
    """vertices (V,3) float32, colors (V,3) uint8 or None, faces (F,3) int32, keep (F,) uint8 -> (vertices (V',3), colors (V',3) or
    None, faces (F',3), vertex_map (V,) int32): the faces with keep != 0 in their order, the vertices they name in their order, the
    faces renumbered; vertex_map sends an old index to its new one, or to -1.  Coordinates and colours are copied as bits.  A kept
    face with an index outside 0..V-1 raises ValueError.  The outputs are views of the first rows of buffers of V and F rows.
    Synchronises once (the error word, V' and F')."""
    _mesh_arg(vertices, 'vertices', torch.float32, (3,), CLOUD_MAX_POINTS)
    if colors is not None:
        _mesh_arg(colors, 'colors', torch.uint8, (3,))
        _same_device(colors, 'colors', vertices, 'vertices')
        if int(colors.shape[0]) != int(vertices.shape[0]):
            raise ValueError('colors: %d rows for %d vertices' % (int(colors.shape[0]), int(vertices.shape[0])))
    _mesh_arg(faces, 'faces', torch.int32, (3,), MESH_TOPOLOGY_MAX_FACES)
    _mesh_arg(keep, 'keep', torch.uint8, ())
    _same_device(faces, 'faces', vertices, 'vertices')
    _same_device(keep, 'keep', vertices, 'vertices')
    nv, nf, dev = int(vertices.shape[0]), int(faces.shape[0]), vertices.device
    if int(keep.shape[0]) != nf:
        raise ValueError('keep: %d flags for %d faces' % (int(keep.shape[0]), nf))
    vertices_out = torch.empty_like(vertices)
    colors_out = None if colors is None else torch.empty_like(colors)
    faces_out = torch.empty_like(faces)
    vertex_map = torch.empty(nv, dtype=torch.int32, device=dev)
    if not _launchable(vertices, 'vertices'):
        return vertices_out, colors_out, faces_out, vertex_map
    scratch = torch.empty(_size('atvs_mesh_select_scratch_size', nv, nf), dtype=torch.uint8, device=dev)
    info = torch.empty(3, dtype=torch.int32, device=dev)
    _call('atvs_mesh_select', _p(vertices), _p(colors), nv, _p(faces), _p(keep), nf, _p(scratch), scratch.numel(), _p(vertices_out),
          _p(colors_out), _p(faces_out), _p(vertex_map), _p(info), _stream())
    bad, kept_v, kept_f = (int(x) for x in info.cpu().tolist())
    if bad:
        raise _bad_faces('mesh_select', bad, nf, nv)
    return vertices_out[:kept_v], None if colors_out is None else colors_out[:kept_v], faces_out[:kept_f], vertex_map


def mesh_edge_census(faces, num_vertices):
    """faces (F,3) int32, num_vertices V -> a dict of ints over the distinct sorted pairs (lo, hi) among the faces' 3F pairs (f0,f1),
    (f1,f2), (f2,f0), pairs with lo == hi included: `edges` (the distinct pairs), `boundary` / `manifold` / `nonmanifold` (pairs
    that occur once / twice / more often), `misoriented` (pairs given twice or more in one direction), `max_faces_per_edge`,
    `self_edges` (pairs with lo == hi), `error` (0).  A face with an index outside 0..V-1 raises ValueError.  Synchronises once."""
    nv = _int_in(num_vertices, 'num_vertices', 0, CLOUD_MAX_POINTS)
    _mesh_arg(faces, 'faces', torch.int32, (3,), MESH_TOPOLOGY_MAX_FACES)
    nf, dev = int(faces.shape[0]), faces.device
    if not _launchable(faces, 'faces'):
        return dict.fromkeys(MESH_CENSUS_WORDS, 0)
    scratch = torch.empty(_size('atvs_mesh_edge_census_scratch_size', nf), dtype=torch.uint8, device=dev)
    words = torch.empty(len(MESH_CENSUS_WORDS), dtype=torch.int64, device=dev)
    _call('atvs_mesh_edge_census', _p(faces), nf, nv, _p(scratch), scratch.numel(), _p(words), _stream())
    census = dict(zip(MESH_CENSUS_WORDS, (int(x) for x in words.cpu().tolist())))
    if census['error']:
        raise _bad_faces('mesh_edge_census', census['error'], nf, nv)
    return census
