"""Exact point-to-triangle distances from a cloud to a mesh's surface on the device (csrc/mesh_distance.hip): `mesh_grid` sorts a
mesh's usable faces into a uniform grid of face references, `mesh_nearest` gives every query the smallest squared distance to a face
within the grid's radius, the lowest face that attains it and, on request, the closest point on it.  The definition is in
include/atvsnet_hip.h and restated in tests/mesh_distance_restated.py; atvsnet/mesh_distance.py, eval_cloud's --exact_recon /
--exact_gt and the ETH3D driver's mesh=dict(score=dict(exact=True)) are built on them.  The result is a function of the mesh, the
queries and the radius alone: the grid's cell edge and reference budget cannot be seen in it, and the same inputs give the same bits."""

import struct

import torch

from .. import _lib
from .base import _call, _p, _size, _stream
from .cloud import CLOUD_MAX_POINTS, _radius
from .mesh import _launchable, _mesh_arg
from .mesh_sample import _same_device
from .mesh_topology import MESH_TOPOLOGY_MAX_FACES

MESH_GRID_MAX_REFS = _lib.header_macro('ATVS_MESH_GRID_MAX_REFS')
MESH_GRID_MIN_REFS_PER_FACE = 8              # a cell edge of the box's extent puts a face in at most 8 cells: the coarsening ends
MESH_GRID_DEFAULT_REFS_PER_FACE = 32         # the default budget, 32 references per face and at least 2^20: a default, not a measurement
MESH_GRID_MAX_ROUNDS = 128


class MeshGrid(object):
    """A mesh's usable faces sorted into a uniform grid of face references (atvs_mesh_grid_build).  Owns its device buffer, a copy of
    the faces' corners included; reusable for any number of mesh_nearest calls.  n_vertices, n_faces: the mesh's; radius: the float32
    search radius (as a Python float); max_refs: the reference budget; cell: the cell edge that was reached; refs: the references it
    needed; usable_faces: the faces with three indices in range and nine finite coordinates; rounds: builds it took."""
    __slots__ = ('buf', 'n_vertices', 'n_faces', 'radius', 'max_refs', 'cell', 'refs', 'usable_faces', 'rounds')

    def __init__(self, buf, n_vertices, n_faces, radius, max_refs, cell, refs, usable_faces, rounds):
        self.buf, self.n_vertices, self.n_faces, self.radius, self.max_refs = buf, n_vertices, n_faces, radius, max_refs
        self.cell, self.refs, self.usable_faces, self.rounds = cell, refs, usable_faces, rounds

    @property
    def nbytes(self):
        return self.buf.numel()


def _mesh_inputs(vertices, faces):
    try:
        _mesh_arg(vertices, 'vertices', torch.float32, (3,), CLOUD_MAX_POINTS)
        _mesh_arg(faces, 'faces', torch.int32, (3,), MESH_TOPOLOGY_MAX_FACES)
    except TypeError as e:
        raise ValueError(str(e))
    _same_device(faces, 'faces', vertices, 'vertices')


def _max_refs(max_refs, n_faces):
    least = MESH_GRID_MIN_REFS_PER_FACE * n_faces
    if max_refs is None:
        return min(max(MESH_GRID_DEFAULT_REFS_PER_FACE * n_faces, 1 << 20), MESH_GRID_MAX_REFS)
    if isinstance(max_refs, bool) or not isinstance(max_refs, int) or not least <= max_refs <= MESH_GRID_MAX_REFS:
        raise ValueError('max_refs must be an integer in %d (8 per face) .. %d, got %r' % (least, MESH_GRID_MAX_REFS, max_refs))
    return max_refs


def mesh_grid(vertices, faces, radius, max_refs=None):
    """vertices (V,3) float32, faces (F,3) int32, radius > 0 -> MeshGrid.  A face with an index outside 0..V-1 or a coordinate that
    is not finite is not usable and never a neighbour.  The cell edge starts at radius (1 + 2^-18), or what the cell cap needs, and
    is coarsened until the references fit max_refs (None: 32 per face, at least 2^20; never below 8 per face): after every build the
    host reads four words, and where the references do not fit it builds again with the cell edge doubled: it ends once the edge
    reaches the box's extent, where a face is in at most 8 cells, and since the first edge already keeps the box within the cell
    cap (no face in more cells than the cap), that is a handful of builds at the most.  Synchronises once per build: once where
    the first cell edge fits."""
    r = _radius(radius)
    _mesh_inputs(vertices, faces)
    nv, nf = int(vertices.shape[0]), int(faces.shape[0])
    budget = _max_refs(max_refs, nf)
    if not _launchable(vertices, 'vertices'):
        return MeshGrid(torch.empty(0, dtype=torch.uint8, device=vertices.device), nv, nf, r, budget, 0.0, 0, 0, 0)
    buf = torch.empty(_size('atvs_mesh_grid_scratch_size', nf, budget), dtype=torch.uint8, device=vertices.device)
    info = torch.empty(4, dtype=torch.int64, device=vertices.device)
    cell = 0.0
    for rounds in range(1, MESH_GRID_MAX_ROUNDS + 1):
        _call('atvs_mesh_grid_build', _p(vertices), nv, _p(faces), nf, r, cell, budget, _p(buf), buf.numel(), _p(info), _stream())
        refs, built, usable, bits = (int(x) for x in info.cpu().tolist())
        edge = struct.unpack('<d', struct.pack('<q', bits))[0]
        if built:
            return MeshGrid(buf, nv, nf, r, budget, edge, refs, usable, rounds)
        cell = 2.0 * edge
    raise RuntimeError('mesh_grid: %d references at a cell edge of %g after %d builds, the budget is %d' % (refs, edge, rounds, budget))


def mesh_nearest(grid, queries, closest=False):
    """queries (m,3) float32 -> (d2 (m,) float32, face (m,) int32), with closest=True also closest (m,3) float32: per query the
    smallest squared distance to a usable face of the grid's mesh (the closest point on the closed triangle found in double by the
    header's sequence, the squared distance rounded once), the lowest face attaining it and that closest point; (+inf, -1, NaN)
    where that is beyond the grid's radius, the query is not finite, or the mesh has no usable face."""
    if not isinstance(grid, MeshGrid):
        raise ValueError('grid: expected a MeshGrid (ops.mesh_grid), got %s' % type(grid).__name__)
    try:
        _mesh_arg(queries, 'queries', torch.float32, (3,), CLOUD_MAX_POINTS)
    except TypeError as e:
        raise ValueError(str(e))
    _same_device(queries, 'queries', grid.buf, 'the grid')
    m = int(queries.shape[0])
    d2 = torch.empty(m, dtype=torch.float32, device=queries.device)
    face = torch.empty(m, dtype=torch.int32, device=queries.device)
    points = torch.empty((m, 3), dtype=torch.float32, device=queries.device) if closest else None
    if m and _launchable(queries, 'queries'):
        scratch = torch.empty(_size('atvs_mesh_nearest_scratch_size', grid.n_faces, m), dtype=torch.uint8, device=queries.device)
        _call('atvs_mesh_nearest', _p(grid.buf), grid.buf.numel(), grid.n_faces, grid.max_refs, _p(queries), m,
              _p(scratch), scratch.numel(), _p(d2), _p(face), _p(points), _stream())
    return (d2, face, points) if closest else (d2, face)
