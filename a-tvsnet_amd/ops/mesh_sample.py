"""A triangle mesh's surface sampled uniformly by area on the device (csrc/mesh_sample.hip): `mesh_sample_counts` gives every face
its number of samples (area times density, rounded stochastically by the face's own hashed number), `mesh_sample_points` places
the samples of given counts (points, faces, interpolated colours, face normals), `mesh_sample` does the two in sequence.  The
definitions are in include/atvsnet_hip.h and restated in tests/mesh_sample_restated.py; atvsnet/sample_mesh.py, eval_cloud's
--sample_recon / --sample_gt and the ETH3D driver's mesh=dict(score=...) are built on them.  Every random number is a hash of (seed,
face, sample within the face) and the only atomics are integer ones: the same inputs give the same bits."""

import collections
import math

import torch

from .. import _lib
from .base import _call, _p, _size, _stream
from .cloud import CLOUD_MAX_POINTS
from .mesh import _launchable, _mesh_arg
from .mesh_topology import MESH_TOPOLOGY_MAX_FACES

MESH_SAMPLE_MAX = _lib.header_macro('ATVS_MESH_SAMPLE_MAX')
MESH_SAMPLE_INFO = ('samples', 'skipped_index_faces', 'skipped_nonfinite_faces', 'max_per_face')

MeshSamples = collections.namedtuple('MeshSamples', 'points colors normals face')


def _density(density):
    if isinstance(density, (bool, str, bytes)):
        raise ValueError('density must be a positive finite number, got %r' % (density,))
    try:
        d = float(density)
    except (TypeError, ValueError):
        raise ValueError('density must be a positive finite number, got %r' % (density,))
    if not (d > 0.0 and math.isfinite(d)):
        raise ValueError('density must be a positive finite number, got %r' % (density,))
    return d


def _seed(seed):
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < (1 << 63):
        raise ValueError('seed must be an integer in 0..2^63-1, got %r' % (seed,))
    return seed


def _same_device(t, name, ref, ref_name):
    if t.device != ref.device:
        raise ValueError('%s on %s, %s on %s' % (name, t.device, ref_name, ref.device))


def _mesh_inputs(vertices, colors, faces):
    """Raises ValueError unless vertices (V,3) float32, colors (V,3) uint8 or None and faces (F,3) int32 are one mesh on one device."""
    try:
        _mesh_arg(vertices, 'vertices', torch.float32, (3,), CLOUD_MAX_POINTS)
        _mesh_arg(faces, 'faces', torch.int32, (3,), MESH_TOPOLOGY_MAX_FACES)
        if colors is not None:
            _mesh_arg(colors, 'colors', torch.uint8, (3,))
    except TypeError as e:
        raise ValueError(str(e))
    _same_device(faces, 'faces', vertices, 'vertices')
    if colors is not None:
        _same_device(colors, 'colors', vertices, 'vertices')
        if int(colors.shape[0]) != int(vertices.shape[0]):
            raise ValueError('colors: %d rows for %d vertices' % (int(colors.shape[0]), int(vertices.shape[0])))


def _too_many(op, needed, most):
    return ValueError('%s: the density needs %d samples (%d on one face), at most %d (MESH_SAMPLE_MAX) can be made' % (
        op, needed, most, MESH_SAMPLE_MAX))


def mesh_sample_counts(vertices, faces, density, seed=0):
    """vertices (V,3) float32, faces (F,3) int32, density > 0 in samples per unit area, seed in 0..2^63-1 -> (counts (F,) int32,
    areas (F,) float64, info): per face its area in double and floor(x) + (u_f < x - floor(x)) samples, x = area * density, u_f the
    face's hashed uniform number (include/atvsnet_hip.h).  A face with an index outside 0..V-1 or a non-finite area has count 0 and
    area 0.  info: 'samples' (the total), 'skipped_index_faces', 'skipped_nonfinite_faces', 'max_per_face'.  A total above
    MESH_SAMPLE_MAX, or a face that needs that many, raises ValueError with the total needed.  Synchronises once (the four words)."""
    density, seed = _density(density), _seed(seed)
    _mesh_inputs(vertices, None, faces)
    nv, nf, dev = int(vertices.shape[0]), int(faces.shape[0]), vertices.device
    counts = torch.empty(nf, dtype=torch.int32, device=dev)
    areas = torch.empty(nf, dtype=torch.float64, device=dev)
    info = dict.fromkeys(MESH_SAMPLE_INFO, 0)
    if not _launchable(vertices, 'vertices') or nf == 0:
        return counts, areas, info
    words = torch.empty(4, dtype=torch.int64, device=dev)
    _call('atvs_mesh_sample_counts', _p(vertices), nv, _p(faces), nf, density, seed, _p(counts), _p(areas), _p(words), _stream())
    info = dict(zip(MESH_SAMPLE_INFO, (int(x) for x in words.cpu().tolist())))
    if info['max_per_face'] >= MESH_SAMPLE_MAX or info['samples'] > MESH_SAMPLE_MAX:
        raise _too_many('mesh_sample_counts', info['samples'], info['max_per_face'])
    return counts, areas, info


def _place(vertices, colors, faces, counts, total, seed, normals):
    nv, nf, dev = int(vertices.shape[0]), int(faces.shape[0]), vertices.device
    points = torch.empty((total, 3), dtype=torch.float32, device=dev)
    face = torch.empty(total, dtype=torch.int32, device=dev)
    colors_out = None if colors is None else torch.empty((total, 3), dtype=torch.uint8, device=dev)
    normals_out = torch.empty((total, 3), dtype=torch.float32, device=dev) if normals else None
    if total == 0 or not _launchable(vertices, 'vertices'):
        return MeshSamples(points, colors_out, normals_out, face)
    scratch = torch.empty(_size('atvs_mesh_sample_scratch_size', nf), dtype=torch.uint8, device=dev)
    offsets = torch.empty(nf + 1, dtype=torch.int32, device=dev)
    _call('atvs_mesh_sample_offsets', _p(counts), nf, _p(scratch), scratch.numel(), _p(offsets), _stream())
    info = torch.empty(2, dtype=torch.int64, device=dev)
    _call('atvs_mesh_sample_place', _p(vertices), _p(colors), nv, _p(faces), nf, _p(offsets), total, seed, _p(points), _p(face),
          _p(colors_out), _p(normals_out), _p(info), _stream())
    mismatch, bad = (int(x) for x in info.cpu().tolist())
    if mismatch:
        raise RuntimeError('mesh_sample_points: the offsets do not end at the %d samples asked for' % total)
    if bad:
        raise ValueError('mesh_sample_points: %d of %d samples lie on faces with a vertex index outside 0..%d' % (bad, total, nv - 1))
    return MeshSamples(points, colors_out, normals_out, face)


def mesh_sample_points(vertices, colors, faces, counts, seed=0, normals=False):
    """vertices (V,3) float32, colors (V,3) uint8 or None, faces (F,3) int32, counts (F,) int32 >= 0 -- an INPUT: mesh_sample_counts'
    or anybody's -> MeshSamples(points (S,3) float32, colors (S,3) uint8 or None, normals (S,3) float32 or None, face (S,) int32), S
    the counts' total.  The samples of face f are rows offset[f] .. offset[f] + counts[f] - 1; sample j of it is the point
    (a + u (b - a)) + v (c - a) of the hashed pair (u, v) of (seed, f, j), folded into the triangle; colours are the barycentric
    mix, rounded to nearest even; normals the face's unit normal (include/atvsnet_hip.h).  A total above MESH_SAMPLE_MAX, a negative
    count or samples on a face with an index outside 0..V-1 raise ValueError.  Synchronises twice (the total; the error words)."""
    seed = _seed(seed)
    _mesh_inputs(vertices, colors, faces)
    nf = int(faces.shape[0])
    try:
        _mesh_arg(counts, 'counts', torch.int32, (), MESH_TOPOLOGY_MAX_FACES)
    except TypeError as e:
        raise ValueError(str(e))
    _same_device(counts, 'counts', vertices, 'vertices')
    if int(counts.shape[0]) != nf:
        raise ValueError('counts: %d rows for %d faces' % (int(counts.shape[0]), nf))
    total = 0
    if nf and _launchable(vertices, 'vertices'):
        if int(counts.min().item()) < 0:
            raise ValueError('counts: a negative count')
        total = int(counts.sum(dtype=torch.int64).item())
        if total > MESH_SAMPLE_MAX:
            raise _too_many('mesh_sample_points', total, int(counts.max().item()))
    return _place(vertices, colors, faces, counts, total, seed, bool(normals))


def mesh_sample(vertices, colors, faces, density, seed=0, normals=False):
    """mesh_sample_counts then mesh_sample_points of its counts -> (MeshSamples, info); info gains 'area', the float64 sum of the
    faces' areas on the device.  About area * density samples: the expected count of every face is exactly its x."""
    seed = _seed(seed)
    _mesh_inputs(vertices, colors, faces)
    counts, areas, info = mesh_sample_counts(vertices, faces, density, seed)
    launch = _launchable(vertices, 'vertices') and int(faces.shape[0]) > 0
    info['area'] = float(areas.sum().item()) if launch else 0.0
    return _place(vertices, colors, faces, counts, info['samples'], seed, bool(normals)), info
