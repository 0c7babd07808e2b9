"""A triangle mesh rendered into cameras on the device (csrc/mesh_render.hip): `mesh_render` gives, per pixel, the nearest depth of
the mesh along the ray through the pixel's centre and the face that gives it; `depth_occlude` takes the pixels of a depth map that
lie behind such a rendering out.  The definitions the kernels are held to are in include/atvsnet_hip.h and restated in
tests/mesh_render_restated.py; atvsnet/eval_depth.py (occlusion meshes, mesh ground truth) and atvsnet/mesh_fusion.py (a mesh seen
from its own cameras) are built on them."""

import math

import torch

from .. import _lib
from .base import _call, _p, _size, _stream
from .cloud import CLOUD_MAX_POINTS, SCAN_RENDER_MAX_CAMS, _int_in, _same_device

MESH_RENDER_SMALL_PIXELS = _lib.header_macro('ATVS_MESH_RENDER_SMALL_PIXELS')     # the largest box one lane rasterises
MESH_RENDER_MAX_FACES = (1 << 31) - 1


def _mesh_arg(t, name, dtype, trailing, limit=None):
    """Raises unless `t` is a contiguous (n,) + trailing tensor of that dtype with at most `limit` rows."""
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s: expected a tensor, got %s' % (name, type(t).__name__))
    if t.dtype != dtype:
        raise TypeError('%s: expected %s, got %s' % (name, dtype, t.dtype))
    if t.dim() != 1 + len(trailing) or tuple(int(s) for s in t.shape[1:]) != tuple(trailing):
        raise ValueError('%s: expected shape (n,%s), got %s' % (name, ','.join(str(s) for s in trailing), tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError('%s: must be contiguous' % name)
    if limit is not None and int(t.shape[0]) > limit:
        raise ValueError('%s: %d rows, at most %d' % (name, int(t.shape[0]), limit))


def _launchable(t, name):
    """True for a tensor on the current device, False on `meta` (the host checks alone run); anything else raises."""
    if t.device.type == 'meta':
        return False
    if t.device.type != 'cuda':
        raise RuntimeError('%s: the mesh kernels run on the MI355X only (no CPU fallback), got a tensor on %s' % (name, t.device))
    if t.device.index != torch.cuda.current_device():
        raise RuntimeError('%s: on %s, the launch goes to the current device cuda:%d' % (name, t.device, torch.cuda.current_device()))
    return True


def mesh_render(vertices, faces, cams, rows, cols, pixel_centre=0.0):
    """vertices (V,3) float32 in the cameras' frame, faces (F,3) int32, cams (n,16) float64 in scan_render's layout ->
    (depth (n,rows,cols) float32, face (n,rows,cols) int32): per pixel the nearest camera depth at which the ray through the
    pixel's centre (image coordinate u + pixel_centre) meets a face, and the lowest face that gives it; (0, -1) where none does.

    Float64 edge functions, both windings, both sides of every edge inclusive (a closed mesh has no cracks), no near-plane
    clipping (a face that crosses the camera plane renders where it is in front).  Zero-area, edge-on, NaN and infinite faces
    cover nothing.  A face with an index outside 0..V-1 raises ValueError.  include/atvsnet_hip.h has the definition in full; the
    same inputs give the same bits (a 64-bit integer atomic min).  Synchronises once (the error word)."""
    rows, cols = _int_in(rows, 'rows', 1), _int_in(cols, 'cols', 1)
    centre = float(pixel_centre)
    if not math.isfinite(centre):
        raise ValueError('pixel_centre must be finite, got %r' % (pixel_centre,))
    _mesh_arg(vertices, 'vertices', torch.float32, (3,), CLOUD_MAX_POINTS)
    _mesh_arg(faces, 'faces', torch.int32, (3,), MESH_RENDER_MAX_FACES)
    _mesh_arg(cams, 'cams', torch.float64, (16,))
    _same_device(faces, 'faces', vertices, 'vertices')
    _same_device(cams, 'cams', vertices, 'vertices')
    nv, nf, n_cams = int(vertices.shape[0]), int(faces.shape[0]), int(cams.shape[0])
    if not 1 <= n_cams <= SCAN_RENDER_MAX_CAMS:
        raise ValueError('cams: 1 to %d cameras, got %d' % (SCAN_RENDER_MAX_CAMS, n_cams))
    if n_cams * rows * cols >= 1 << 31:
        raise ValueError('%d maps of %d x %d: 2^31 pixels or more' % (n_cams, rows, cols))
    dev = vertices.device
    depth = torch.empty((n_cams, rows, cols), dtype=torch.float32, device=dev)
    face = torch.empty((n_cams, rows, cols), dtype=torch.int32, device=dev)
    if not _launchable(vertices, 'vertices'):
        return depth, face
    scratch = torch.empty(_size('atvs_mesh_render_scratch_size', n_cams, rows, cols, nf), dtype=torch.uint8, device=dev)
    err = torch.empty(1, dtype=torch.int32, device=dev)
    _call('atvs_mesh_render', _p(vertices), nv, _p(faces), nf, _p(cams), n_cams, rows, cols, centre, _p(scratch), scratch.numel(),
          _p(depth), _p(face), _p(err), _stream())
    bad = int(err.item())
    if bad:
        raise ValueError('mesh_render: %d of %d faces have a vertex index outside 0..%d' % (bad, nf, nv - 1))
    return depth, face


def depth_occlude(depth, occluder, tol=0.0, out=None):
    """depth, occluder: float32 tensors of one shape (0 = empty pixel) -> out (a new tensor, or `out`, which may be `depth`):
    0 where occluder > 0 and depth > 0 and depth is further than occluder * (1 + tol), compared in float64; depth elsewhere (a
    NaN in either keeps depth).  The occluder is a mesh rendered by mesh_render into the cameras of `depth`."""
    tol = float(tol)
    if not (tol >= 0.0 and math.isfinite(tol)):
        raise ValueError('tol must be >= 0 and finite, got %r' % (tol,))
    for t, name in ((depth, 'depth'), (occluder, 'occluder')) + (() if out is None else ((out, 'out'),)):
        if not isinstance(t, torch.Tensor):
            raise TypeError('%s: expected a tensor, got %s' % (name, type(t).__name__))
        if t.dtype != torch.float32:
            raise TypeError('%s: expected %s, got %s' % (name, torch.float32, t.dtype))
        if not t.is_contiguous():
            raise ValueError('%s: must be contiguous' % name)
        if tuple(t.shape) != tuple(depth.shape):
            raise ValueError('%s: shape %s, depth has %s' % (name, tuple(t.shape), tuple(depth.shape)))
        if t is not depth:
            _same_device(t, name, depth, 'depth')
    if depth.numel() >= 1 << 31:
        raise ValueError('depth: %d pixels, 2^31 or more' % depth.numel())
    if out is None:
        out = torch.empty_like(depth)
    if _launchable(depth, 'depth'):
        _call('atvs_depth_occlude', _p(depth), _p(occluder), depth.numel(), tol, _p(out), _stream())
    return out
