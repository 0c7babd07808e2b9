"""A triangle mesh smoothed by Taubin's filter, and its vertex normals, on the device (csrc/mesh_smooth.hip): `mesh_adjacency` builds
the distinct neighbours of every vertex once, `mesh_quantize` puts the positions on a power-of-two lattice of integers,
`mesh_smooth_pass` is one umbrella step as a per-vertex gather of exact integer sums, `mesh_dequantize` goes back to float32,
`mesh_smooth` does the four in sequence; `mesh_face_extent`, `mesh_vertex_normal_sums` and `mesh_normals_from_sums` give
`mesh_vertex_normals`, the area-weighted vertex normals.  The definitions are in include/atvsnet_hip.h and restated in
tests/mesh_smooth_restated.py; atvsnet/smooth_mesh.py is built on them.  Integer atomics only: the same inputs give the same bits,
in any order of the faces."""

import collections
import math

import numpy as np
import torch

from .. import _lib
from .base import _call, _p, _size, _stream
from .cloud import CLOUD_MAX_POINTS
from .mesh import _launchable, _mesh_arg
from .mesh_sample import _mesh_inputs, _same_device
from .mesh_topology import _bad_faces

MESH_ADJACENCY_MIN_SLOTS = _lib.header_macro('ATVS_MESH_ADJACENCY_MIN_SLOTS')
MESH_ADJACENCY_INFO = ('pairs', 'boundary_pairs', 'nonmanifold_pairs', 'skipped_index_faces', 'self_pairs', 'nonfinite_pairs',
                       'unplaced_pairs')
MESH_FLAG_FINITE, MESH_FLAG_BOUNDARY, MESH_FLAG_NONMANIFOLD = 1, 2, 4
MESH_FACE_EXTENT_INFO = ('max_extent', 'usable_faces', 'skipped_index_faces', 'nonfinite_faces')
MESH_SMOOTH_MAX_ITERATIONS = 1000
MESH_SMOOTH_LAMBDA, MESH_SMOOTH_MU = 0.5, -0.53          # Open3D's defaults: defaults, not measurements

MeshAdjacency = collections.namedtuple('MeshAdjacency', 'degree flags offsets neighbours info')


def _number(x, name, what, ok):
    if isinstance(x, (bool, str, bytes)):
        raise ValueError('%s must be %s, got %r' % (name, what, x))
    try:
        v = float(x)
    except (TypeError, ValueError):
        raise ValueError('%s must be %s, got %r' % (name, what, x))
    if not (math.isfinite(v) and ok(v)):
        raise ValueError('%s must be %s, got %r' % (name, what, x))
    return v


def _step(step):
    return _number(step, 'step', 'a positive power of two', lambda v: v > 0.0 and math.frexp(v)[0] == 0.5)


def _factor(factor):
    return _number(factor, 'factor', 'a finite number with |factor| <= 1', lambda v: abs(v) <= 1.0)


def _area_unit(area_unit):
    return _number(area_unit, 'area_unit', 'a positive finite number', lambda v: v > 0.0)


def _origin(origin):
    try:
        o = [float(x) for x in origin]
    except (TypeError, ValueError):
        raise ValueError('origin: expected 3 finite numbers, got %r' % (origin,))
    if len(o) != 3 or not all(math.isfinite(x) for x in o):
        raise ValueError('origin: expected 3 finite numbers, got %r' % (origin,))
    return np.asarray(o, np.float64)


def _rows(t, name, dtype, trailing, n, ref):
    try:
        _mesh_arg(t, name, dtype, trailing)
    except TypeError as e:
        raise ValueError(str(e))
    _same_device(t, name, ref, 'the first argument')
    if n is not None and int(t.shape[0]) != n:
        raise ValueError('%s: %d rows, expected %d' % (name, int(t.shape[0]), n))


def _adjacency(vertices, faces):
    """-> (degree, flags, offsets, the whole (6F,) neighbours buffer, the seven device words or None without a launch)."""
    nv, nf, dev = int(vertices.shape[0]), int(faces.shape[0]), vertices.device
    degree = torch.empty(nv, dtype=torch.int32, device=dev)
    flags = torch.empty(nv, dtype=torch.int32, device=dev)
    offsets = torch.empty(nv + 1, dtype=torch.int32, device=dev)
    neighbours = torch.empty(6 * nf, dtype=torch.int32, device=dev)
    if not _launchable(vertices, 'vertices') or nv == 0:
        return degree, flags, torch.zeros_like(offsets), neighbours, None
    scratch = torch.empty(_size('atvs_mesh_adjacency_scratch_size', nv, nf), dtype=torch.uint8, device=dev)
    words = torch.empty(len(MESH_ADJACENCY_INFO), dtype=torch.int64, device=dev)
    _call('atvs_mesh_adjacency', _p(vertices), nv, _p(faces), nf, _p(scratch), scratch.numel(), _p(degree), _p(flags), _p(offsets),
          _p(neighbours), _p(words), _stream())
    return degree, flags, offsets, neighbours, words


def mesh_adjacency(vertices, faces):
    """vertices (V,3) float32, faces (F,3) int32 -> MeshAdjacency(degree (V,) int32, flags (V,) int32, offsets (V+1,) int32,
    neighbours (2 P,) int32, info): the distinct neighbours of every vertex (include/atvsnet_hip.h).  flags: MESH_FLAG_FINITE,
    MESH_FLAG_BOUNDARY (endpoint of a pair with one face), MESH_FLAG_NONMANIFOLD (of a pair with more than two).  Row v of
    neighbours is offsets[v] .. offsets[v+1]-1, in an order that is NOT defined.  info: 'pairs' (P, the distinct pairs),
    'boundary_pairs', 'nonmanifold_pairs', 'skipped_index_faces' (faces with an index outside 0..V-1: skipped, not an error here),
    'self_pairs', 'nonfinite_pairs', 'unplaced_pairs'.  Synchronises once (the seven words)."""
    _mesh_inputs(vertices, None, faces)
    degree, flags, offsets, neighbours, words = _adjacency(vertices, faces)
    info = dict.fromkeys(MESH_ADJACENCY_INFO, 0)
    if words is None:
        return MeshAdjacency(degree, flags, offsets, neighbours[:0], info)
    info = dict(zip(MESH_ADJACENCY_INFO, (int(x) for x in words.cpu().tolist())))
    return MeshAdjacency(degree, flags, offsets, neighbours[:2 * info['pairs']], info)


def _quantize(vertices, org, step):
    nv, dev = int(vertices.shape[0]), vertices.device
    q = torch.empty((nv, 3), dtype=torch.int64, device=dev)
    if not _launchable(vertices, 'vertices') or nv == 0:
        return q, None
    words = torch.empty(2, dtype=torch.int64, device=dev)
    _call('atvs_mesh_quantize', _p(vertices), nv, org.ctypes.data, step, _p(q), _p(words), _stream())
    return q, words


def _out_of_lattice(op, n):
    return ValueError('%s: %d coordinates lie more than 2^31 steps from the origin' % (op, n))


def mesh_quantize(vertices, origin, step):
    """vertices (V,3) float32, origin (3 finite host numbers), step a positive power of two -> (q (V,3) int64, info): per
    coordinate llrint(((double)x - origin) / step); a vertex with a non-finite coordinate gets 0, 0, 0 ('nonfinite_vertices').  A
    coordinate with |q| > 2^31 raises ValueError.  Synchronises once (the two words)."""
    org, step = _origin(origin), _step(step)
    try:
        _mesh_arg(vertices, 'vertices', torch.float32, (3,), CLOUD_MAX_POINTS)
    except TypeError as e:
        raise ValueError(str(e))
    q, words = _quantize(vertices, org, step)
    info = {'nonfinite_vertices': 0}
    if words is not None:
        info['nonfinite_vertices'], far = (int(x) for x in words.cpu().tolist())
        if far:
            raise _out_of_lattice('mesh_quantize', far)
    return q, info


def mesh_smooth_pass(q_in, adjacency, factor, pin_mask=0, info=None):
    """q_in (V,3) int64, adjacency = (degree, flags, offsets, neighbours, ...) of mesh_adjacency, |factor| <= 1 -> (q_out (V,3)
    int64, info (2,) int32 on the device): one umbrella step q + llrint(factor (mean of the neighbours - q)), clamped to
    [-2^32, 2^32]; a vertex that is not finite, has no neighbour or has a flag of pin_mask keeps its q.  info is the caller's
    running pair of tallies (clamped coordinates, lanes with a row outside the arrays): None makes a zeroed one, a tensor from an
    earlier pass is added to.  No synchronisation."""
    factor = _factor(factor)
    if isinstance(pin_mask, bool) or not isinstance(pin_mask, int) or not 0 <= pin_mask < (1 << 31):
        raise ValueError('pin_mask must be an integer in 0..2^31-1, got %r' % (pin_mask,))
    try:
        _mesh_arg(q_in, 'q_in', torch.int64, (3,), CLOUD_MAX_POINTS)
    except TypeError as e:
        raise ValueError(str(e))
    degree, flags, offsets, neighbours = adjacency[:4]
    nv, dev = int(q_in.shape[0]), q_in.device
    _rows(degree, 'degree', torch.int32, (), nv, q_in)
    _rows(flags, 'flags', torch.int32, (), nv, q_in)
    _rows(offsets, 'offsets', torch.int32, (), nv + 1, q_in)
    _rows(neighbours, 'neighbours', torch.int32, (), None, q_in)
    if info is None:
        info = torch.zeros(2, dtype=torch.int32, device=dev)
    else:
        _rows(info, 'info', torch.int32, (), 2, q_in)
    q_out = torch.empty_like(q_in)
    if not _launchable(q_in, 'q_in') or nv == 0:
        return q_out, info
    _call('atvs_mesh_smooth_pass', _p(q_in), nv, _p(degree), _p(flags), _p(offsets), _p(neighbours), int(neighbours.shape[0]), factor,
          pin_mask, _p(q_out), _p(info), _stream())
    return q_out, info


def mesh_dequantize(q, q0, vertices, origin, step):
    """q, q0 (V,3) int64, vertices (V,3) float32 -> vertices_out (V,3) float32: a coordinate whose q equals its q0 keeps the bits
    of the input coordinate, any other is (float)(origin + step q).  No synchronisation."""
    org, step = _origin(origin), _step(step)
    try:
        _mesh_arg(vertices, 'vertices', torch.float32, (3,), CLOUD_MAX_POINTS)
    except TypeError as e:
        raise ValueError(str(e))
    nv = int(vertices.shape[0])
    _rows(q, 'q', torch.int64, (3,), nv, vertices)
    _rows(q0, 'q0', torch.int64, (3,), nv, vertices)
    vertices_out = torch.empty_like(vertices)
    if not _launchable(vertices, 'vertices') or nv == 0:
        return vertices_out
    _call('atvs_mesh_dequantize', _p(q), _p(q0), _p(vertices), nv, org.ctypes.data, step, _p(vertices_out), _stream())
    return vertices_out


def mesh_face_extent(vertices, faces):
    """-> info: 'max_extent' (a float: the largest s = |(b - a) x (c - a)|, twice the largest area, over the faces where it is
    finite), 'usable_faces', 'skipped_index_faces', 'nonfinite_faces'.  Synchronises once (the four words)."""
    _mesh_inputs(vertices, None, faces)
    nv, nf, dev = int(vertices.shape[0]), int(faces.shape[0]), vertices.device
    info = dict.fromkeys(MESH_FACE_EXTENT_INFO, 0)
    info['max_extent'] = 0.0
    if not _launchable(vertices, 'vertices') or nf == 0:
        return info
    words = torch.empty(4, dtype=torch.int64, device=dev)
    _call('atvs_mesh_face_extent', _p(vertices), nv, _p(faces), nf, _p(words), _stream())
    host = words.cpu().numpy()
    info.update(zip(MESH_FACE_EXTENT_INFO[1:], (int(x) for x in host[1:])))
    info['max_extent'] = float(host[:1].view(np.float64)[0])
    return info


def mesh_vertex_normal_sums(vertices, faces, area_unit):
    """-> (sums (V,3) int64, incidences (V,) int32): per vertex the sum over its faces of llrint(w n 2^30), n the face's unit
    normal and w = min(1, s / area_unit), and the number of faces that added to it (include/atvsnet_hip.h).  A face with an index
    outside 0..V-1 raises ValueError.  Synchronises once (the error word)."""
    area_unit = _area_unit(area_unit)
    _mesh_inputs(vertices, None, faces)
    nv, nf, dev = int(vertices.shape[0]), int(faces.shape[0]), vertices.device
    sums = torch.empty((nv, 3), dtype=torch.int64, device=dev)
    incidences = torch.empty(nv, dtype=torch.int32, device=dev)
    if not _launchable(vertices, 'vertices') or (nv == 0 and nf == 0):
        return sums, incidences
    info = torch.empty(1, dtype=torch.int32, device=dev)
    _call('atvs_mesh_vertex_normal_sums', _p(vertices), nv, _p(faces), nf, area_unit, _p(sums), _p(incidences), _p(info), _stream())
    bad = int(info.item())
    if bad:
        raise _bad_faces('mesh_vertex_normal_sums', bad, nf, nv)
    return sums, incidences


def mesh_normals_from_sums(sums):
    """sums (V,3) int64 -- an INPUT: mesh_vertex_normal_sums' or anybody's -> normals (V,3) float32: N / |N| in double, rounded
    once; 0, 0, 0 where the sum is.  No synchronisation."""
    try:
        _mesh_arg(sums, 'sums', torch.int64, (3,), CLOUD_MAX_POINTS)
    except TypeError as e:
        raise ValueError(str(e))
    nv = int(sums.shape[0])
    normals = torch.empty((nv, 3), dtype=torch.float32, device=sums.device)
    if not _launchable(sums, 'sums') or nv == 0:
        return normals
    _call('atvs_mesh_vertex_normals', _p(sums), nv, _p(normals), _stream())
    return normals


def mesh_vertex_normals(vertices, faces, area_unit=None):
    """-> normals (V,3) float32: the unit sum of the normals of a vertex's faces, each weighted by min(1, s / area_unit), s twice
    its area; 0, 0, 0 for a vertex no face with an area names.  area_unit None: the mesh's largest s (mesh_face_extent), which is
    plain area weighting.  They point the way the winding says.  Synchronises once, twice with area_unit None."""
    _mesh_inputs(vertices, None, faces)
    if area_unit is None:
        area_unit = mesh_face_extent(vertices, faces)['max_extent'] or 1.0          # no face with an area: nothing is weighted
    sums, _ = mesh_vertex_normal_sums(vertices, faces, area_unit)
    return mesh_normals_from_sums(sums)


def _smooth_options(iterations, lam, mu):
    if isinstance(iterations, bool) or not isinstance(iterations, int) or not 0 <= iterations <= MESH_SMOOTH_MAX_ITERATIONS:
        raise ValueError('iterations must be an integer in 0..%d, got %r' % (MESH_SMOOTH_MAX_ITERATIONS, iterations))
    lam = _number(lam, 'lam', 'a number with 0 < lam < 1', lambda v: 0.0 < v < 1.0)
    if mu is not None:
        mu = _number(mu, 'mu', 'None or a number with -1 <= mu < -lam (Taubin\'s condition), lam = %r' % lam, lambda v: -1.0 <= v < -lam)
    return iterations, lam, mu


def mesh_smooth_lattice(lo, hi):
    """(origin (3,) float64, step) of the lattice mesh_smooth quantises on, from the bounding box lo, hi of the finite vertices:
    origin = (lo + hi) / 2, step = 2^(e - 32) with 2^(e-1) <= the largest extent < 2^e (e = 0 for extent 0), so |q| <= 2^31 to begin
    with and a position is held to 2^-32 of the extent."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    extent = float((hi - lo).max())
    e = math.frexp(extent)[1] if extent > 0.0 else 0
    return (lo + hi) / 2.0, math.ldexp(1.0, e - 32)


def mesh_smooth(vertices, faces, iterations, lam=MESH_SMOOTH_LAMBDA, mu=MESH_SMOOTH_MU, pin_boundary=False, adjacency=None):
    """vertices (V,3) float32, faces (F,3) int32 -> (vertices_out (V,3) float32, info): `iterations` times a pass with `lam` then a
    pass with `mu` (Taubin's filter: 0 < lam < 1, -1 <= mu < -lam); mu None: a pass with lam only (Laplacian smoothing, which
    shrinks).  Umbrella weights: a vertex moves towards the plain mean of its distinct neighbours.  pin_boundary: the endpoints
    of edges with one face stay.  Vertices that are not finite or that no face names stay; a coordinate that did not move keeps
    its input bits.  adjacency: mesh_adjacency's result for this mesh, when the caller has it.  info: the adjacency's words,
    'origin', 'step', 'passes', 'nonfinite_vertices'.  A face with an index outside 0..V-1 raises ValueError; a coordinate that was
    clamped (the filter has diverged) raises RuntimeError.  Synchronises twice: the bounding box, and the info words at the end."""
    iterations, lam, mu = _smooth_options(iterations, lam, mu)
    _mesh_inputs(vertices, None, faces)
    nv, nf = int(vertices.shape[0]), int(faces.shape[0])
    factors = ([lam] if mu is None else [lam, mu]) * iterations
    info = dict.fromkeys(MESH_ADJACENCY_INFO, 0)
    info.update(origin=[0.0, 0.0, 0.0], step=math.ldexp(1.0, -32), passes=len(factors), nonfinite_vertices=0)
    if not _launchable(vertices, 'vertices') or nv == 0:
        return torch.empty_like(vertices), info
    finite = torch.isfinite(vertices).all(1, keepdim=True)
    box = torch.stack([torch.where(finite, vertices, float('inf')).amin(0), torch.where(finite, vertices, float('-inf')).amax(0)]).cpu()
    box = box.numpy().astype(np.float64)
    if not np.isfinite(box).all():                          # no finite vertex
        box[:] = 0.0
    org, step = mesh_smooth_lattice(box[0], box[1])
    if adjacency is None:
        degree, flags, offsets, neighbours, words = _adjacency(vertices, faces)
    else:
        degree, flags, offsets, neighbours = adjacency[:4]
        words = torch.tensor([adjacency.info[k] for k in MESH_ADJACENCY_INFO], dtype=torch.int64).to(vertices.device)
    q0, qwords = _quantize(vertices, org, step)
    tallies = torch.zeros(2, dtype=torch.int32, device=vertices.device)
    q = q0
    pin = MESH_FLAG_BOUNDARY if pin_boundary else 0
    for factor in factors:
        q, tallies = mesh_smooth_pass(q, (degree, flags, offsets, neighbours), factor, pin, tallies)
    out = mesh_dequantize(q, q0, vertices, org, step)
    host = [int(x) for x in torch.cat([words, qwords, tallies.to(torch.int64)]).cpu().tolist()]
    info.update(zip(MESH_ADJACENCY_INFO, host[:7]))
    info.update(origin=[float(x) for x in org], step=step, nonfinite_vertices=host[7])
    if info['skipped_index_faces']:
        raise _bad_faces('mesh_smooth', info['skipped_index_faces'], nf, nv)
    if host[8]:
        raise _out_of_lattice('mesh_smooth', host[8])
    if host[10]:
        raise RuntimeError('mesh_smooth: %d vertices have a row of neighbours outside the adjacency\'s arrays' % host[10])
    if host[9]:
        raise RuntimeError('mesh_smooth: the filter has diverged: %d coordinates left [-2^32, 2^32] steps and were clamped '
                           '(lam %r, mu %r, %d iterations)' % (host[9], lam, mu, iterations))
    return out, info
