"""COLMAP model import on the device (csrc/colmap.hip): the per-image depth range by exact rank selection and the co-visibility
matrix of shared 3-D points.  The host side (model reader, CSR build, scene writer) is atvsnet/colmap.py.
"""

import ctypes

import torch

from .. import _lib
from .base import _ERR, _call, _p, _stream

COVIS_MAX_IMAGES = 16384            # atvs_colmap_covisibility: an (images x images) int32 matrix of at most 1 GiB


def _colmap_args(*specs):
    """(tensor, name, dtype, trailing shape) -> raises unless each is a contiguous tensor of that dtype on the current device."""
    for t, name, dtype, trailing in specs:
        if not isinstance(t, torch.Tensor):
            raise TypeError('%s: expected a tensor, got %s' % (name, type(t).__name__))
        if t.dtype != dtype:
            raise TypeError('%s: expected %s, got %s' % (name, dtype, t.dtype))
        if t.dim() != 1 + len(trailing) or tuple(int(s) for s in t.shape[1:]) != tuple(trailing):
            raise ValueError('%s: expected shape (n,%s), got %s' % (name, ','.join(str(s) for s in trailing), tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError('%s: must be contiguous' % name)
        if t.device.type != 'cuda':
            raise RuntimeError('%s: the COLMAP kernels run on the MI355X only (no CPU fallback), got a tensor on %s' % (name, t.device))
        if t.device.index != torch.cuda.current_device():
            raise RuntimeError('%s: on %s, the launch goes to the current device cuda:%d' % (name, t.device, torch.cuda.current_device()))


def colmap_depth_range(points, cams, percentile):
    """points (P,3) float64 X, Y, Z; cams (N,18) float64 per image = R row-major, t, fx, fy, cx, cy, width, height ->
    (n (N,) int32 points in view, d_lo (N,), d_hi (N,) float64): the in-view disparities' order statistics of rank
    int(n * (1 - percentile)) and int(n * percentile) (atvs_colmap_depth_range; 0.0 where n is 0), on the device."""
    _colmap_args((points, 'points', torch.float64, (3,)), (cams, 'cams', torch.float64, (18,)))
    if not 0.0 < float(percentile) < 1.0:
        raise ValueError('percentile must lie in (0, 1), got %r' % percentile)
    n_images, dev = int(cams.shape[0]), cams.device
    nbytes = ctypes.c_long(0)
    rc = _lib.lib().atvs_colmap_depth_range_scratch_size(n_images, ctypes.byref(nbytes))
    if rc != 0:
        raise RuntimeError('atvs_colmap_depth_range_scratch_size failed: %s (%d) for %d images' % (_ERR.get(rc, 'unknown'), rc, n_images))
    scratch = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
    n = torch.empty(n_images, dtype=torch.int32, device=dev)
    d_lo = torch.empty(n_images, dtype=torch.float64, device=dev)
    d_hi = torch.empty(n_images, dtype=torch.float64, device=dev)
    _call('atvs_colmap_depth_range', _p(points), ctypes.c_long(int(points.shape[0])), _p(cams), n_images,
          ctypes.c_double(float(percentile)), _p(scratch), ctypes.c_long(scratch.numel()), _p(n), _p(d_lo), _p(d_hi), _stream())
    return n, d_lo, d_hi


def colmap_covisibility(offsets, observers, n_images):
    """Tracks in CSR form -- offsets (T+1,) int32, observers (offsets[-1],) int32 distinct image indices per track -> the
    (n_images, n_images) int32 matrix of shared tracks, zero diagonal (atvs_colmap_covisibility), on the device."""
    offsets, observers = offsets.reshape(-1, 1), observers.reshape(-1, 1)
    _colmap_args((offsets, 'offsets', torch.int32, (1,)), (observers, 'observers', torch.int32, (1,)))
    if not 0 < int(n_images) <= COVIS_MAX_IMAGES:
        raise ValueError('co-visibility of %d images: the (images x images) matrix holds 1 to %d images (1 GiB)' %
                         (n_images, COVIS_MAX_IMAGES))
    if offsets.shape[0] < 1:
        raise ValueError('offsets: at least one entry (the start of the first track)')
    covis = torch.empty((int(n_images), int(n_images)), dtype=torch.int32, device=offsets.device)
    _call('atvs_colmap_covisibility', _p(offsets), _p(observers), int(offsets.shape[0]) - 1, int(observers.shape[0]), int(n_images),
          _p(covis), _stream())
    return covis
