"""A triangle mesh simplified by vertex clustering with quadric placement, on the device (csrc/mesh_simplify.hip): `mesh_cluster`
sorts the vertices into the cells of a lattice and keeps each cluster's exact integer sums, `mesh_cluster_quadrics` accumulates the
clusters' quadrics as fixed-point integers, `mesh_cluster_place` places each cluster's representative (the mean, or the quadric's
minimiser inside the cell), `mesh_cluster_max_move` says how far a vertex moved, `mesh_cluster_faces` rewrites the faces and marks
the ones that stay.  The definitions are in include/atvsnet_hip.h and restated in tests/mesh_simplify_restated.py;
atvsnet/simplify_mesh.py is built on them and on `mesh_select`.  Integer atomics only: the same inputs give the same bits."""

import collections
import math

import numpy as np
import torch

from .. import _lib
from .base import _call, _p, _size, _stream
from .cloud import CLOUD_MAX_POINTS, _raise_cell_range, _same_device, _vec3
from .mesh import _launchable, _mesh_arg
from .mesh_topology import MESH_TOPOLOGY_MAX_FACES, _bad_faces

MESH_SIMPLIFY_MIN_SLOTS = _lib.header_macro('ATVS_MESH_SIMPLIFY_MIN_SLOTS')
MESH_SIMPLIFY_SOLVE_UNITS = _lib.header_macro('ATVS_MESH_SIMPLIFY_SOLVE_UNITS')     # units of 2^-53 / rank_epsilon, in cells
MESH_PLACEMENTS = collections.OrderedDict((('mean', _lib.header_macro('ATVS_MESH_PLACE_MEAN')),
                                           ('quadric', _lib.header_macro('ATVS_MESH_PLACE_QUADRIC'))))
MESH_RANK_EPSILON = 1e-3          # Lindstrom's value: a default, not a measurement

MeshClusters = collections.namedtuple('MeshClusters', 'vertex_cluster cells counts position_sums color_sums')


def _cell(cell):
    if isinstance(cell, (bool, str, bytes)):
        raise ValueError('cell must be a positive finite number, got %r' % (cell,))
    try:
        c = float(cell)
    except (TypeError, ValueError):
        raise ValueError('cell must be a positive finite number, got %r' % (cell,))
    if not (c > 0.0 and math.isfinite(c)):
        raise ValueError('cell must be a positive finite number, got %r' % (cell,))
    return c


def _placement(placement):
    if not isinstance(placement, str) or placement not in MESH_PLACEMENTS:
        raise ValueError('placement must be one of %s, got %r' % (', '.join(MESH_PLACEMENTS), placement))
    return MESH_PLACEMENTS[placement]


def _rank_epsilon(rank_epsilon):
    if isinstance(rank_epsilon, (bool, str, bytes)):
        raise ValueError('rank_epsilon must be a number in (0, 1), got %r' % (rank_epsilon,))
    try:
        e = float(rank_epsilon)
    except (TypeError, ValueError):
        raise ValueError('rank_epsilon must be a number in (0, 1), got %r' % (rank_epsilon,))
    if not 0.0 < e < 1.0:
        raise ValueError('rank_epsilon must be a number in (0, 1), got %r' % (rank_epsilon,))
    return e


def _origin(origin):
    if origin is None or isinstance(origin, (str, bytes)):
        raise ValueError('origin: expected 3 finite numbers, got %r' % (origin,))
    try:
        return _vec3(origin, 'origin')
    except TypeError:
        raise ValueError('origin: expected 3 finite numbers, got %r' % (origin,))


def _rows(t, name, dtype, trailing, n, ref):
    _mesh_arg(t, name, dtype, trailing)
    _same_device(t, name, ref, 'the first argument')
    if int(t.shape[0]) != n:
        raise ValueError('%s: %d rows, expected %d' % (name, int(t.shape[0]), n))


def mesh_cluster(vertices, colors, cell, origin):
    """vertices (V,3) float32, colors (V,3) uint8 or None, cell > 0, origin (3 host numbers: the corner of cell (0,0,0)) ->
    MeshClusters(vertex_cluster (V,) int32, cells (C,3) int32, counts (C,) int32, position_sums (C,3) int64 holding unsigned
    sums, color_sums (C,3) int64 or None).  The clusters are cloud_voxel_downsample's voxels; ids 0..C-1 in ascending order of the
    cluster's lowest vertex index; a vertex with a non-finite coordinate gets -1 and forms no cluster.  A finite vertex more than
    2^21 cells from the origin, or below it, raises ValueError.  Synchronises once, to read C."""
    cell, org = _cell(cell), _origin(origin)
    _mesh_arg(vertices, 'vertices', torch.float32, (3,), CLOUD_MAX_POINTS)
    nv, dev = int(vertices.shape[0]), vertices.device
    if colors is not None:
        _rows(colors, 'colors', torch.uint8, (3,), nv, vertices)
    vertex_cluster = torch.empty(nv, dtype=torch.int32, device=dev)
    cells = torch.empty((nv, 3), dtype=torch.int32, device=dev)
    counts = torch.empty(nv, dtype=torch.int32, device=dev)
    position_sums = torch.empty((nv, 3), dtype=torch.int64, device=dev)
    color_sums = None if colors is None else torch.empty((nv, 3), dtype=torch.int64, device=dev)
    if not _launchable(vertices, 'vertices') or nv == 0:
        return MeshClusters(vertex_cluster, cells[:0], counts[:0], position_sums[:0], None if color_sums is None else color_sums[:0])
    scratch = torch.empty(_size('atvs_mesh_cluster_scratch_size', nv), dtype=torch.uint8, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    _call('atvs_mesh_cluster', _p(vertices), _p(colors), nv, cell, org, _p(scratch), scratch.numel(), _p(vertex_cluster), _p(cells),
          _p(counts), _p(position_sums), _p(color_sums), _p(count), _stream())
    c = int(count.item())
    if c < 0:
        _raise_cell_range('mesh_cluster', vertices, org, cell)
    return MeshClusters(vertex_cluster, cells[:c], counts[:c], position_sums[:c], None if color_sums is None else color_sums[:c])


def mesh_cluster_quadrics(vertices, faces, vertex_cluster, num_clusters, cell, origin):
    """vertices (V,3) float32, faces (F,3) int32, vertex_cluster (V,) int32 of mesh_cluster, num_clusters C -> (quadrics (C,10)
    int64, incidences (C,) int32): per cluster the ten sums of its faces' plane quadrics, each term rounded to a multiple of 2^-30
    and summed exactly (include/atvsnet_hip.h), and the number of (face, cluster) incidences that added to it.  A face with an index
    outside 0..V-1 raises ValueError.  Synchronises once (the error word)."""
    cell, org = _cell(cell), _origin(origin)
    _mesh_arg(vertices, 'vertices', torch.float32, (3,), CLOUD_MAX_POINTS)
    nv, dev = int(vertices.shape[0]), vertices.device
    _mesh_arg(faces, 'faces', torch.int32, (3,), MESH_TOPOLOGY_MAX_FACES)
    _same_device(faces, 'faces', vertices, 'vertices')
    _rows(vertex_cluster, 'vertex_cluster', torch.int32, (), nv, vertices)
    nf = int(faces.shape[0])
    nc = int(num_clusters)
    if isinstance(num_clusters, bool) or nc != num_clusters or not 0 <= nc <= nv:
        raise ValueError('num_clusters: expected an integer in 0..%d, got %r' % (nv, num_clusters))
    quadrics = torch.empty((nc, 10), dtype=torch.int64, device=dev)
    incidences = torch.empty(nc, dtype=torch.int32, device=dev)
    if not _launchable(vertices, 'vertices'):
        return quadrics, incidences
    info = torch.empty(1, dtype=torch.int32, device=dev)
    _call('atvs_mesh_cluster_quadrics', _p(vertices), nv, _p(faces), nf, _p(vertex_cluster), nc, cell, org, _p(quadrics), _p(incidences),
          _p(info), _stream())
    bad = int(info.item())
    if bad:
        raise _bad_faces('mesh_cluster_quadrics', bad, nf, nv)
    return quadrics, incidences


def mesh_cluster_place(cells, counts, position_sums, color_sums, quadrics, cell, origin, placement='quadric', rank_epsilon=MESH_RANK_EPSILON):
    """The sums of mesh_cluster and mesh_cluster_quadrics -- INPUTS here: cells (C,3) int32, counts (C,) int32, position_sums (C,3)
    int64, color_sums (C,3) int64 or None, quadrics (C,10) int64 (None with placement 'mean') -> (positions (C,3) float32, colors
    (C,3) uint8 or None, placed (C,) uint8).  'mean': the exact mean of the cluster's vertices.  'quadric': the minimiser of the
    cluster's quadric on the eigenpairs with lambda_i > rank_epsilon lambda_max (the fixed Jacobi of cloud_normals), the mean where
    lambda_max <= 2^-20, a value is not finite or the minimiser leaves the cell; placed is 1 where the quadric's position was
    used.  Colours: (2 S + k) / (2 k) in integers.  No synchronisation."""
    cell, org, mode, eps = _cell(cell), _origin(origin), _placement(placement), _rank_epsilon(rank_epsilon)
    _mesh_arg(cells, 'cells', torch.int32, (3,), CLOUD_MAX_POINTS)
    nc, dev = int(cells.shape[0]), cells.device
    _rows(counts, 'counts', torch.int32, (), nc, cells)
    _rows(position_sums, 'position_sums', torch.int64, (3,), nc, cells)
    if color_sums is not None:
        _rows(color_sums, 'color_sums', torch.int64, (3,), nc, cells)
    if quadrics is not None:
        _rows(quadrics, 'quadrics', torch.int64, (10,), nc, cells)
    elif placement == 'quadric':
        raise ValueError('quadrics: placement \'quadric\' needs the clusters\' quadrics')
    positions = torch.empty((nc, 3), dtype=torch.float32, device=dev)
    colors = None if color_sums is None else torch.empty((nc, 3), dtype=torch.uint8, device=dev)
    placed = torch.empty(nc, dtype=torch.uint8, device=dev)
    if not _launchable(cells, 'cells') or nc == 0:
        return positions, colors, placed
    _call('atvs_mesh_cluster_place', _p(cells), _p(counts), _p(position_sums), _p(color_sums), _p(quadrics), nc, cell, org, mode, eps,
          _p(positions), _p(colors), _p(placed), _stream())
    return positions, colors, placed


def mesh_cluster_max_move(vertices, vertex_cluster, positions):
    """vertices (V,3) float32, vertex_cluster (V,) int32, positions (C,3) float32 -> the largest distance between a finite vertex
    and its cluster's position, a Python float: the square root of the largest float32 squared distance (an integer atomic max over
    its bits).  0.0 without a clustered vertex.  Synchronises once."""
    _mesh_arg(vertices, 'vertices', torch.float32, (3,), CLOUD_MAX_POINTS)
    nv, dev = int(vertices.shape[0]), vertices.device
    _rows(vertex_cluster, 'vertex_cluster', torch.int32, (), nv, vertices)
    _mesh_arg(positions, 'positions', torch.float32, (3,), nv)
    _same_device(positions, 'positions', vertices, 'vertices')
    if not _launchable(vertices, 'vertices') or nv == 0:
        return 0.0
    out = torch.empty(1, dtype=torch.int32, device=dev)
    _call('atvs_mesh_cluster_max_move', _p(vertices), nv, _p(vertex_cluster), _p(positions), int(positions.shape[0]), _p(out), _stream())
    return math.sqrt(float(out.cpu().numpy().view(np.float32)[0]))


def mesh_cluster_faces(faces, vertex_cluster):
    """faces (F,3) int32, vertex_cluster (V,) int32 -> (faces_out (F,3) int32, keep (F,) uint8, counts): each face rewritten to
    its three cluster ids, and keep = 0 for a face that names a non-finite vertex (counts['nonfinite_faces']), else has two equal ids
    ('degenerate_faces'), else has the same SET of ids as a face with a lower index that got this far ('duplicate_faces': the lowest
    index of each set stays, with its own winding).  A face with an index outside 0..V-1 raises ValueError.  ops.mesh_select then
    compacts.  Synchronises once (the four words)."""
    _mesh_arg(faces, 'faces', torch.int32, (3,), MESH_TOPOLOGY_MAX_FACES)
    _mesh_arg(vertex_cluster, 'vertex_cluster', torch.int32, (), CLOUD_MAX_POINTS)
    _same_device(vertex_cluster, 'vertex_cluster', faces, 'faces')
    nf, nv, dev = int(faces.shape[0]), int(vertex_cluster.shape[0]), faces.device
    faces_out = torch.empty_like(faces)
    keep = torch.empty(nf, dtype=torch.uint8, device=dev)
    counts = {'nonfinite_faces': 0, 'degenerate_faces': 0, 'duplicate_faces': 0}
    if not _launchable(faces, 'faces') or nf == 0:
        return faces_out, keep, counts
    scratch = torch.empty(_size('atvs_mesh_cluster_faces_scratch_size', nf), dtype=torch.uint8, device=dev)
    info = torch.empty(4, dtype=torch.int32, device=dev)
    _call('atvs_mesh_cluster_faces', _p(faces), nf, nv, _p(vertex_cluster), _p(scratch), scratch.numel(), _p(faces_out), _p(keep), _p(info),
          _stream())
    bad, counts['nonfinite_faces'], counts['degenerate_faces'], counts['duplicate_faces'] = (int(x) for x in info.cpu().tolist())
    if bad:
        raise _bad_faces('mesh_cluster_faces', bad, nf, nv)
    return faces_out, keep, counts
