"""Point-cloud scoring on the device (csrc/cloud.hip): a uniform grid over a reference cloud, the exact nearest reference point
within a radius for every query, and tolerance counts.  The definition the kernels are held to is in include/atvsnet_hip.h; the
evaluator built on them is atvsnet/eval_cloud.py.
"""

import ctypes
import math

import numpy as np
import torch

from .. import _lib
from .base import _ERR, _call, _p, _stream

CLOUD_MAX_POINTS = 1 << 30
CLOUD_MAX_TOLERANCES = 16


def _cloud_arg(t, name, dtype, trailing):
    """Raises unless `t` is a contiguous (n,) + trailing tensor of that dtype on the current device."""
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s: expected a tensor, got %s' % (name, type(t).__name__))
    if t.dtype != dtype:
        raise TypeError('%s: expected %s, got %s' % (name, dtype, t.dtype))
    if t.dim() != 1 + len(trailing) or tuple(int(s) for s in t.shape[1:]) != tuple(trailing):
        raise ValueError('%s: expected shape (n,%s), got %s' % (name, ','.join(str(s) for s in trailing), tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError('%s: must be contiguous' % name)
    if int(t.shape[0]) > CLOUD_MAX_POINTS:
        raise ValueError('%s: %d rows, at most 2^30' % (name, int(t.shape[0])))
    if t.device.type != 'cuda':
        raise RuntimeError('%s: the point-cloud kernels run on the MI355X only (no CPU fallback), got a tensor on %s' % (name, t.device))
    if t.device.index != torch.cuda.current_device():
        raise RuntimeError('%s: on %s, the launch goes to the current device cuda:%d' % (name, t.device, torch.cuda.current_device()))


def _radius(radius):
    with np.errstate(over='ignore'):
        r = float(np.float32(radius))
    if not (r > 0.0 and math.isfinite(r)):
        raise ValueError('radius must be a positive finite float32, got %r' % (radius,))
    return r


def _size(name, *args):
    nbytes = ctypes.c_long(0)
    rc = getattr(_lib.lib(), name)(*(ctypes.c_long(int(a)) for a in args), ctypes.byref(nbytes))
    if rc != 0:
        raise RuntimeError('%s failed: %s (%d) for %s' % (name, _ERR.get(rc, 'unknown'), rc, args))
    return int(nbytes.value)


class CloudGrid(object):
    """A reference cloud sorted into a uniform grid (atvs_cloud_grid_build).  Owns its device buffer; reusable for any number of
    cloud_nearest calls.  n: reference points, radius: the float32 search radius (as a Python float), nbytes: the buffer's size."""
    __slots__ = ('buf', 'n', 'radius')

    def __init__(self, buf, n, radius):
        self.buf, self.n, self.radius = buf, n, radius

    @property
    def nbytes(self):
        return self.buf.numel()


def cloud_grid(points, radius):
    """points (n,3) float32 on the device (n >= 0; non-finite rows are never neighbours), radius > 0 -> CloudGrid."""
    r = _radius(radius)
    _cloud_arg(points, 'points', torch.float32, (3,))
    n = int(points.shape[0])
    buf = torch.empty(_size('atvs_cloud_grid_scratch_size', n), dtype=torch.uint8, device=points.device)
    _call('atvs_cloud_grid_build', _p(points), ctypes.c_long(n), ctypes.c_float(r), _p(buf), ctypes.c_long(buf.numel()), _stream())
    return CloudGrid(buf, n, r)


def cloud_nearest(grid, queries):
    """queries (m,3) float32 -> (d2 (m,) float32, idx (m,) int32): per query the smallest float32 squared distance
    (dx*dx + dy*dy) + dz*dz to a finite point of the grid's cloud and the lowest index attaining it; (+inf, -1) where that is
    beyond the grid's radius, the query is not finite, or the cloud has no finite point."""
    if not isinstance(grid, CloudGrid):
        raise TypeError('grid: expected a CloudGrid (ops.cloud_grid), got %s' % type(grid).__name__)
    _cloud_arg(queries, 'queries', torch.float32, (3,))
    if queries.device != grid.buf.device:
        raise RuntimeError('queries on %s, the grid on %s' % (queries.device, grid.buf.device))
    m = int(queries.shape[0])
    d2 = torch.empty(m, dtype=torch.float32, device=queries.device)
    idx = torch.empty(m, dtype=torch.int32, device=queries.device)
    if m == 0:
        return d2, idx
    scratch = torch.empty(_size('atvs_cloud_nearest_scratch_size', grid.n, m), dtype=torch.uint8, device=queries.device)
    _call('atvs_cloud_nearest', _p(grid.buf), ctypes.c_long(grid.buf.numel()), ctypes.c_long(grid.n), _p(queries), ctypes.c_long(m),
          _p(scratch), ctypes.c_long(scratch.numel()), _p(d2), _p(idx), _stream())
    return d2, idx


def cloud_counts(d2, tolerances, radius=None):
    """d2 (m,) float32 of cloud_nearest, up to 16 tolerances -> (len(tolerances),) int64 on the device: how many entries have
    double(d2) <= tau * tau.  radius: the radius d2 was computed with; a tolerance above it raises (distances beyond the radius
    are not known).  None: the caller vouches for that."""
    tol = [float(t) for t in tolerances]
    if not 1 <= len(tol) <= CLOUD_MAX_TOLERANCES:
        raise ValueError('1 to %d tolerances, got %d' % (CLOUD_MAX_TOLERANCES, len(tol)))
    r = float(np.finfo(np.float32).max) if radius is None else _radius(radius)
    for t in tol:
        if not 0.0 <= t <= r:
            raise ValueError('tolerance %r outside [0, radius = %r]' % (t, r))
    _cloud_arg(d2, 'd2', torch.float32, ())
    counts = torch.empty(CLOUD_MAX_TOLERANCES, dtype=torch.int64, device=d2.device)
    arr = (ctypes.c_double * len(tol))(*tol)
    _call('atvs_cloud_counts', _p(d2), ctypes.c_long(int(d2.shape[0])), arr, len(tol), ctypes.c_float(r), _p(counts), _stream())
    return counts[:len(tol)]
