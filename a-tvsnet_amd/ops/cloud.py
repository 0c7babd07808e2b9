"""Point-cloud scoring on the device (csrc/cloud.hip): a uniform grid over a reference cloud, the exact nearest reference point
within a radius for every query, and tolerance counts.  The definition the kernels are held to is in include/atvsnet_hip.h; the
evaluator built on them is atvsnet/eval_cloud.py.

Registration (csrc/cloud_register.hip; atvsnet/register_cloud.py is built on it): cloud_transform moves a cloud through a matrix,
cloud_pair_moments reduces matched pairs to the 18 sums of a closed-form similarity fit, cloud_plane_moments to the 37 sums of a
point-to-plane step over the source's normals, cloud_voxel_downsample keeps one mean point per occupied voxel.

Neighbourhoods (csrc/cloud_knn.hip; atvsnet/clean_cloud.py is built on it): cloud_knn finds the k nearest reference points within
the grid's radius, cloud_radius_count counts the reference points inside it, cloud_knn_mean and cloud_sor_stats reduce the k-NN
distances to the three numbers of statistical outlier removal, cloud_bounds is the bounding box of the finite rows.

Normals (csrc/cloud_normals.hip): cloud_normals turns cloud_knn's neighbours into one PCA normal per query;
cloud_plane_moments_target is the point-to-plane step over such normals of the TARGET (atvsnet/register_cloud.py
normal_side='target', atvsnet/cloud_normals.py).

Global registration (csrc/cloud_features.hip, csrc/cloud_ransac.hip; register_cloud.global_init is built on it): cloud_fpfh turns
cloud_knn's neighbours and cloud_normals' normals into one 33-bin descriptor per point, cloud_feature_nearest matches descriptors
exactly, cloud_ransac scores three-point hypotheses over the matches and returns the best few.

Rendering (csrc/scan_render.hip; atvsnet/eval_depth.py is built on it): scan_render splats a scan into a set of cameras and keeps
the nearest depth per pixel, the ground-truth depth maps the network's maps are scored against.

ETH3D-style scoring (csrc/cloud_visibility.hip, csrc/cloud_register.hip; atvsnet/eval_cloud.py's `scans=` is built on it):
cloud_scan_excess is a point's signed distance to what a scanner saw along its ray (cube maps rendered by scan_render),
cloud_voxel_shares the per-voxel hit shares summed over voxels as integers.
"""

import ctypes
import math

import numpy as np
import torch

from .. import _lib
from .base import _call, _p, _size, _stream

CLOUD_MAX_POINTS = 1 << 30
# include/atvsnet_hip.h defines these limits; the kernels take them from there too
CLOUD_MAX_TOLERANCES = _lib.header_macro('ATVS_CLOUD_MAX_TOLERANCES')
CLOUD_MAX_K = _lib.header_macro('ATVS_CLOUD_MAX_K')
SCAN_RENDER_MAX_SPLAT = _lib.header_macro('ATVS_SCAN_RENDER_MAX_SPLAT')
SCAN_RENDER_MAX_CAMS = _lib.header_macro('ATVS_SCAN_RENDER_MAX_CAMS')
CLOUD_SCAN_MAX_WINDOW = _lib.header_macro('ATVS_CLOUD_SCAN_MAX_WINDOW')


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


def _int_in(v, name, lo, hi=None):
    """int(v) for an integer (not a bool) in lo..hi; hi None: 1 or more."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < lo or (hi is not None and int(v) > hi):
        raise ValueError('%s: expected %s, got %r' % (name, 'a positive integer' if hi is None else 'an integer in %d..%d' % (lo, hi), v))
    return int(v)


def _same_device(t, name, ref, ref_name):
    if t.device != ref.device:
        raise RuntimeError('%s on %s, %s on %s' % (name, t.device, ref_name, ref.device))


def _tolerances(tolerances, bounded=False, radius=None):
    """-> (tolerances as floats, r): each >= 0 and r None, or `bounded` by r = radius (None: the largest float32)."""
    tol = [float(t) for t in tolerances]
    if not 1 <= len(tol) <= CLOUD_MAX_TOLERANCES:
        raise ValueError('1 to %d tolerances, got %d' % (CLOUD_MAX_TOLERANCES, len(tol)))
    if not bounded:
        if any(not t >= 0.0 for t in tol):
            raise ValueError('tolerances must be >= 0, got %r' % (tol,))
        return tol, None
    r = float(np.finfo(np.float32).max) if radius is None else _radius(radius)
    for t in tol:
        if not 0.0 <= t <= r:
            raise ValueError('tolerance %r outside [0, radius = %r]' % (t, r))
    return tol, r


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
    _call('atvs_cloud_grid_build', _p(points), n, r, _p(buf), buf.numel(), _stream())
    return CloudGrid(buf, n, r)


def cloud_nearest(grid, queries):
    """queries (m,3) float32 -> (d2 (m,) float32, idx (m,) int32): per query the smallest float32 squared distance
    (dx*dx + dy*dy) + dz*dz to a finite point of the grid's cloud and the lowest index attaining it; (+inf, -1) where that is
    beyond the grid's radius, the query is not finite, or the cloud has no finite point."""
    m = _search_args(grid, queries, False)
    d2 = torch.empty(m, dtype=torch.float32, device=queries.device)
    idx = torch.empty(m, dtype=torch.int32, device=queries.device)
    if m == 0:
        return d2, idx
    scratch = torch.empty(_size('atvs_cloud_nearest_scratch_size', grid.n, m), dtype=torch.uint8, device=queries.device)
    _call('atvs_cloud_nearest', _p(grid.buf), grid.buf.numel(), grid.n, _p(queries), m,
          _p(scratch), scratch.numel(), _p(d2), _p(idx), _stream())
    return d2, idx


def cloud_counts(d2, tolerances, radius=None):
    """d2 (m,) float32 of cloud_nearest, up to 16 tolerances -> (len(tolerances),) int64 on the device: how many entries have
    double(d2) <= tau * tau.  radius: the radius d2 was computed with; a tolerance above it raises (distances beyond the radius
    are not known).  None: the caller vouches for that."""
    tol, r = _tolerances(tolerances, True, radius)
    _cloud_arg(d2, 'd2', torch.float32, ())
    counts = torch.empty(CLOUD_MAX_TOLERANCES, dtype=torch.int64, device=d2.device)
    arr = (ctypes.c_double * len(tol))(*tol)
    _call('atvs_cloud_counts', _p(d2), int(d2.shape[0]), arr, len(tol), r, _p(counts), _stream())
    return counts[:len(tol)]


def _vec3(v, name):
    a = np.zeros(3, np.float64) if v is None else np.asarray(v, np.float64).reshape(-1)
    if a.shape != (3,) or not np.isfinite(a).all():
        raise ValueError('%s: expected 3 finite numbers, got %r' % (name, v))
    return (ctypes.c_double * 3)(*a.tolist())


def cloud_transform(points, matrix, out=None):
    """points (n,3) float32 through `matrix` (4x4, or its rows 0-2 as 3x4; host numbers) -> (n,3) float32: per coordinate k, in
    double, ((T[k][0] x + T[k][1] y) + T[k][2] z) + T[k][3], rounded once to float32.  out: None (a new tensor) or a tensor to
    write, which may be `points` itself."""
    T = np.asarray(matrix, np.float64)
    if T.shape not in ((4, 4), (3, 4)):
        raise ValueError('matrix: expected a 4x4 (or 3x4) matrix, got shape %s' % (T.shape,))
    _cloud_arg(points, 'points', torch.float32, (3,))
    if out is None:
        out = torch.empty_like(points)
    else:
        _cloud_arg(out, 'out', torch.float32, (3,))
        if out.shape != points.shape or out.device != points.device:
            raise ValueError('out: expected %s on %s, got %s on %s' % (tuple(points.shape), points.device, tuple(out.shape), out.device))
    arr = (ctypes.c_double * 12)(*T[:3].reshape(-1).tolist())
    _call('atvs_cloud_transform', _p(points), int(points.shape[0]), arr, _p(out), _stream())
    return out


def cloud_pair_moments(src, dst, idx, d2, trim=float('inf'), pivot_src=None, pivot_dst=None):
    """src (m,3) float32: the queries as ops.cloud_nearest searched them; dst (n,3) float32: the grid's cloud in its original
    order; idx (m,) int32, d2 (m,) float32: what cloud_nearest returned.  Pair i takes part when idx[i] >= 0 and
    double(d2[i]) <= trim * trim.  With a = double(src[i]) - pivot_src, b = double(dst[idx[i]]) - pivot_dst (pivots: 3 host
    numbers, default 0) -> (count, moments): the number of pairs as a Python int and a HOST numpy float64 (18,): sum a (3),
    sum b (3), sum a_r b_c (9, row r of a), sum |a|^2, sum |b|^2, sum double(d2).  The 19 words are what crosses to the host
    (one synchronising copy of 152 bytes); the same input gives the same words bit for bit."""
    trim = float(trim)
    if not trim >= 0.0:
        raise ValueError('trim must be >= 0 (inf allowed), got %r' % (trim,))
    ps, pd = _vec3(pivot_src, 'pivot_src'), _vec3(pivot_dst, 'pivot_dst')
    _cloud_arg(src, 'src', torch.float32, (3,))
    _cloud_arg(dst, 'dst', torch.float32, (3,))
    _cloud_arg(idx, 'idx', torch.int32, ())
    _cloud_arg(d2, 'd2', torch.float32, ())
    m, n = int(src.shape[0]), int(dst.shape[0])
    if int(idx.shape[0]) != m or int(d2.shape[0]) != m:
        raise ValueError('idx %s and d2 %s must have one entry per row of src %s' % (tuple(idx.shape), tuple(d2.shape), tuple(src.shape)))
    for t, name in ((dst, 'dst'), (idx, 'idx'), (d2, 'd2')):
        _same_device(t, name, src, 'src')
    out = torch.empty(19, dtype=torch.int64, device=src.device)
    scratch = torch.empty(_size('atvs_cloud_pair_moments_scratch_size', m), dtype=torch.uint8, device=src.device)
    _call('atvs_cloud_pair_moments', _p(src), _p(dst), n, _p(idx), _p(d2), m, trim, ps, pd,
          _p(scratch), scratch.numel(), _p(out), _stream())
    words = out.cpu().numpy()
    return int(words[0]), words[1:].view(np.float64).copy()


def cloud_plane_moments(src, normals, T, dst, idx, d2, trim=float('inf'), pivot=None):
    """The sums of one Gauss-Newton step of point-to-plane ICP over the source's normals (atvs_cloud_plane_moments; the header
    states every term).  src (m,3) float32: the ORIGINAL source; normals (m,3) float32: its normals in its own frame; T: the
    current 4x4 (or 3x4) similarity as host numbers; dst (n,3) float32, idx (m,) int32, d2 (m,) float32: the searched cloud and
    what cloud_nearest returned for cloud_transform(src, T); pivot: 3 host numbers in dst's frame (default 0).  A pair takes part
    under cloud_pair_moments' rule when its normal is finite and not zero.  The rotation the normals turn by is T's 3x3 block
    divided by the cube root of its determinant.  -> (count, moments): a Python int and a HOST numpy float64 (37,): sum J_a J_b
    for a <= b (28, row-major), sum J_a r (7), sum r^2, sum double(d2), with J = [g x n' (3), n' (3), q . n'].  The 38 words are
    what crosses to the host (one synchronising copy of 304 bytes); the same input gives the same words bit for bit."""
    trim = float(trim)
    if not trim >= 0.0:
        raise ValueError('trim must be >= 0 (inf allowed), got %r' % (trim,))
    p = _vec3(pivot, 'pivot')
    M = np.asarray(T, np.float64)
    if M.shape not in ((4, 4), (3, 4)) or not np.isfinite(M).all():
        raise ValueError('T: expected a finite 4x4 (or 3x4) matrix, got %r' % (T,))
    det = float(np.linalg.det(M[:3, :3]))
    if not det > 0.0:
        raise ValueError('T: the 3x3 block must have a positive determinant (a similarity), got %r' % det)
    _cloud_arg(src, 'src', torch.float32, (3,))
    _cloud_arg(normals, 'normals', torch.float32, (3,))
    _cloud_arg(dst, 'dst', torch.float32, (3,))
    _cloud_arg(idx, 'idx', torch.int32, ())
    _cloud_arg(d2, 'd2', torch.float32, ())
    m, n = int(src.shape[0]), int(dst.shape[0])
    if int(normals.shape[0]) != m or int(idx.shape[0]) != m or int(d2.shape[0]) != m:
        raise ValueError('normals %s, idx %s and d2 %s must have one entry per row of src %s' % (
            tuple(normals.shape), tuple(idx.shape), tuple(d2.shape), tuple(src.shape)))
    for t, name in ((normals, 'normals'), (dst, 'dst'), (idx, 'idx'), (d2, 'd2')):
        _same_device(t, name, src, 'src')
    m12 = (ctypes.c_double * 12)(*M[:3].reshape(-1).tolist())
    rot = (ctypes.c_double * 9)(*(M[:3, :3] / np.cbrt(det)).reshape(-1).tolist())
    out = torch.empty(38, dtype=torch.int64, device=src.device)
    scratch = torch.empty(_size('atvs_cloud_plane_moments_scratch_size', m), dtype=torch.uint8, device=src.device)
    _call('atvs_cloud_plane_moments', _p(src), _p(normals), m12, rot, _p(dst), n, _p(idx), _p(d2), m, trim, p,
          _p(scratch), scratch.numel(), _p(out), _stream())
    words = out.cpu().numpy()
    return int(words[0]), words[1:].view(np.float64).copy()


def cloud_plane_moments_target(src, T, dst, dst_normals, idx, d2, trim=float('inf'), pivot=None):
    """The sums of one Gauss-Newton step of point-to-plane ICP over the TARGET's normals (atvs_cloud_plane_moments_target; the
    header states every term).  src (m,3) float32: the ORIGINAL source; T: the current 4x4 (or 3x4) matrix as host numbers; dst
    (n,3) float32 and dst_normals (n,3) float32: the searched cloud and one normal per row of it, in its frame (used as they are:
    nothing is rotated); idx (m,) int32, d2 (m,) float32: what cloud_nearest returned for cloud_transform(src, T); pivot: 3 host
    numbers in dst's frame (default 0).  A pair takes part under cloud_pair_moments' rule when dst_normals[idx] is finite and not
    zero.  -> (count, moments) in cloud_plane_moments' layout, with J = [q x n (3), n (3), q . n]; motion_from_plane_moments takes
    them as they are.  Negating normals changes no bit of the result."""
    trim = float(trim)
    if not trim >= 0.0:
        raise ValueError('trim must be >= 0 (inf allowed), got %r' % (trim,))
    p = _vec3(pivot, 'pivot')
    M = np.asarray(T, np.float64)
    if M.shape not in ((4, 4), (3, 4)) or not np.isfinite(M).all():
        raise ValueError('T: expected a finite 4x4 (or 3x4) matrix, got %r' % (T,))
    _cloud_arg(src, 'src', torch.float32, (3,))
    _cloud_arg(dst, 'dst', torch.float32, (3,))
    _cloud_arg(dst_normals, 'dst_normals', torch.float32, (3,))
    _cloud_arg(idx, 'idx', torch.int32, ())
    _cloud_arg(d2, 'd2', torch.float32, ())
    m, n = int(src.shape[0]), int(dst.shape[0])
    if int(dst_normals.shape[0]) != n:
        raise ValueError('dst_normals %s must have one row per row of dst %s' % (tuple(dst_normals.shape), tuple(dst.shape)))
    if int(idx.shape[0]) != m or int(d2.shape[0]) != m:
        raise ValueError('idx %s and d2 %s must have one entry per row of src %s' % (tuple(idx.shape), tuple(d2.shape), tuple(src.shape)))
    for t, name in ((dst, 'dst'), (dst_normals, 'dst_normals'), (idx, 'idx'), (d2, 'd2')):
        _same_device(t, name, src, 'src')
    m12 = (ctypes.c_double * 12)(*M[:3].reshape(-1).tolist())
    out = torch.empty(38, dtype=torch.int64, device=src.device)
    scratch = torch.empty(_size('atvs_cloud_plane_moments_target_scratch_size', m), dtype=torch.uint8, device=src.device)
    _call('atvs_cloud_plane_moments_target', _p(src), m12, _p(dst), _p(dst_normals), n, _p(idx), _p(d2), m, trim, p,
          _p(scratch), scratch.numel(), _p(out), _stream())
    words = out.cpu().numpy()
    return int(words[0]), words[1:].view(np.float64).copy()


def _voxel(voxel):
    voxel = float(voxel)
    if not (voxel > 0.0 and math.isfinite(voxel)):
        raise ValueError('voxel must be positive and finite, got %r' % (voxel,))
    return voxel


def _default_origin(points):
    """The floor of the finite points' minimum (0 when there is none) as _vec3 gives it."""
    lo = cloud_bounds(points)[0] if int(points.shape[0]) else None
    return _vec3(None if lo is None else np.floor(lo), 'origin')


def _raise_cell_range(fn, points, org, voxel):
    """What the device could only flag: a finite point whose cell leaves [0, 2^21) on an axis."""
    lo, hi = cloud_bounds(points)
    o = np.array(list(org))
    if (lo < o).any():
        raise ValueError('%s: a point lies below the origin %s (the finite minimum is %s)' % (fn, o.tolist(), lo.tolist()))
    fit = float((hi - o).max()) / float(1 << 21) * (1.0 + 1e-5)          # a little above the limit, so that the printed digits fit too
    raise ValueError('%s: voxel %r puts a point more than 2^21 voxels from the origin (bad shape); the '
                     'smallest voxel that fits this cloud is %.8g' % (fn, voxel, fit))


def cloud_voxel_downsample(points, voxel, origin=None):
    """points (n,3) float32, voxel > 0 -> (means (k,3) float32, first (k,) int32): one point per occupied cubic voxel of edge
    `voxel`, the exact mean of the voxel's finite points (integer sums of 32-bit fractions; include/atvsnet_hip.h), in ascending
    order of the voxel's lowest original index, which is `first`.  Non-finite points are dropped.  origin: 3 host numbers, the
    corner of voxel (0,0,0); None: the floor of the finite points' minimum (one small reduction and copy).  A point more than
    2^21 voxels from the origin, or below it, raises with the voxel size that would fit.  Synchronises once, to read k."""
    voxel = _voxel(voxel)
    org = origin if origin is None else _vec3(origin, 'origin')
    _cloud_arg(points, 'points', torch.float32, (3,))
    n = int(points.shape[0])
    if org is None:
        org = _default_origin(points)
    means = torch.empty((n, 3), dtype=torch.float32, device=points.device)
    first = torch.empty(n, dtype=torch.int32, device=points.device)
    count = torch.empty(1, dtype=torch.int64, device=points.device)
    scratch = torch.empty(_size('atvs_cloud_voxel_downsample_scratch_size', n), dtype=torch.uint8, device=points.device)
    _call('atvs_cloud_voxel_downsample', _p(points), n, voxel, org, _p(scratch), scratch.numel(),
          _p(means), _p(count), _p(first), _stream())
    k = int(count.item())
    if k < 0:
        _raise_cell_range('cloud_voxel_downsample', points, org, voxel)
    return means[:k], first[:k]


def cloud_bounds(points):
    """(min, max) host numpy float64 (3,) over the finite rows of a device cloud (n,3) float32, or (None, None) when there is
    none.  One reduction kernel (atvs_cloud_bounds, the bounding-box pass of the grid build) and one copy of 32 bytes: the default
    origin of cloud_voxel_downsample, the pivots and the box corners of register_cloud.register."""
    _cloud_arg(points, 'points', torch.float32, (3,))
    out = torch.empty(8, dtype=torch.int32, device=points.device)
    _call('atvs_cloud_bounds', _p(points), int(points.shape[0]), _p(out), _stream())
    words = out.cpu().numpy()
    if not words[6]:
        return None, None
    box = words[:6].view(np.float32).astype(np.float64)
    return box[:3].copy(), box[3:].copy()


def _search_args(grid, queries, exclude_same_index):
    """The checks cloud_nearest, cloud_knn and cloud_radius_count share -> m."""
    if not isinstance(grid, CloudGrid):
        raise TypeError('grid: expected a CloudGrid (ops.cloud_grid), got %s' % type(grid).__name__)
    if exclude_same_index and isinstance(queries, torch.Tensor) and queries.dim() == 2 and int(queries.shape[0]) != grid.n:
        raise ValueError('exclude_same_index: the queries must be the grid\'s own cloud, row for row (%d queries, %d reference '
                         'points)' % (int(queries.shape[0]), grid.n))
    _cloud_arg(queries, 'queries', torch.float32, (3,))
    _same_device(queries, 'queries', grid.buf, 'the grid')
    return int(queries.shape[0])


def cloud_knn(grid, queries, k, exclude_same_index=False):
    """queries (m,3) float32, 1 <= k <= 32 -> (d2 (m,k) float32, idx (m,k) int32): per query its k nearest finite points of the
    grid's cloud within the grid's radius (double(d2) <= double(R)^2, d2 the float32 (dx*dx + dy*dy) + dz*dz), in ascending order
    of (d2, index), padded with (+inf, -1); a non-finite query has none.  exclude_same_index: the queries are the grid's own cloud
    and row j is no neighbour of itself (index j alone: a duplicate at another index is a neighbour at distance 0).  With k = 1
    and the flag clear it is cloud_nearest bit for bit."""
    k = _int_in(k, 'k', 1, CLOUD_MAX_K)
    m = _search_args(grid, queries, exclude_same_index)
    d2 = torch.empty((m, k), dtype=torch.float32, device=queries.device)
    idx = torch.empty((m, k), dtype=torch.int32, device=queries.device)
    if m == 0:
        return d2, idx
    scratch = torch.empty(_size('atvs_cloud_knn_scratch_size', grid.n, m), dtype=torch.uint8, device=queries.device)
    _call('atvs_cloud_knn', _p(grid.buf), grid.buf.numel(), grid.n, _p(queries), m, k, 1 if exclude_same_index else 0,
          _p(scratch), scratch.numel(), _p(d2), _p(idx), _stream())
    return d2, idx


def cloud_radius_count(grid, queries, exclude_same_index=False):
    """queries (m,3) float32 -> count (m,) int32: the number of finite points of the grid's cloud with double(d2) <= double(R)^2
    (cloud_knn's candidates and distance); 0 for a non-finite query.  exclude_same_index as for cloud_knn."""
    m = _search_args(grid, queries, exclude_same_index)
    count = torch.empty(m, dtype=torch.int32, device=queries.device)
    if m == 0:
        return count
    scratch = torch.empty(_size('atvs_cloud_knn_scratch_size', grid.n, m), dtype=torch.uint8, device=queries.device)
    _call('atvs_cloud_radius_count', _p(grid.buf), grid.buf.numel(), grid.n, _p(queries), m, 1 if exclude_same_index else 0,
          _p(scratch), scratch.numel(), _p(count), _stream())
    return count


def cloud_knn_mean(d2):
    """d2 (m,k) float32 of cloud_knn -> s (m,) float64: the mean distance to the k neighbours, (sum_t sqrt(double(d2[j,t]))) / k
    added in ascending t in double, or +inf where the row has fewer than k neighbours (a padded entry)."""
    if not isinstance(d2, torch.Tensor):
        raise TypeError('d2: expected a tensor, got %s' % type(d2).__name__)
    k = int(d2.shape[1]) if d2.dim() == 2 else 0
    if not 1 <= k <= CLOUD_MAX_K:
        raise ValueError('d2: expected shape (m,k) with k in 1..%d, got %s' % (CLOUD_MAX_K, tuple(d2.shape)))
    _cloud_arg(d2, 'd2', torch.float32, (k,))
    m = int(d2.shape[0])
    s = torch.empty(m, dtype=torch.float64, device=d2.device)
    if m:
        _call('atvs_cloud_knn_mean', _p(d2), m, k, _p(s), _stream())
    return s


def cloud_sor_stats(s):
    """s (m,) float64 of cloud_knn_mean -> (count, mean, std) as Python numbers: the number of finite entries, their mean, and
    the sample standard deviation sqrt(sum (s - mean)^2 / (count - 1)) (0 below two entries; the mean is 0 of none).  Two passes of
    a fixed-shape sum on the device: the same s gives the same three words bit for bit; they are all that crosses to the host."""
    _cloud_arg(s, 's', torch.float64, ())
    m = int(s.shape[0])
    out = torch.empty(3, dtype=torch.int64, device=s.device)
    scratch = torch.empty(_size('atvs_cloud_sor_stats_scratch_size', m), dtype=torch.uint8, device=s.device)
    _call('atvs_cloud_sor_stats', _p(s), m, _p(scratch), scratch.numel(), _p(out), _stream())
    words = out.cpu().numpy()
    mean, std = words[1:].view(np.float64).tolist()
    return int(words[0]), mean, std


def cloud_normals(points, queries, idx, self_counts=False, viewpoints=None, view_of=None, variation=False):
    """points (n,3) float32: the searched cloud; queries (m,3) float32; idx (m,k) int32 as cloud_knn returned it for `queries` in
    `points` (1 <= k <= 32, -1 padded) -> normals (m,3) float32: per row the unit eigenvector of the smallest eigenvalue of the
    covariance of the samples points[idx] - query (atvs_cloud_normals: float64 throughout, a fixed 18-rotation Jacobi solver; the
    header states every operation).  self_counts: the query is itself a sample (the self-search with exclude_same_index).  The
    zero normal where a row has fewer than 3 samples, a non-finite one, an index >= n, or samples along one line.  viewpoints:
    None, (v,3) host numbers, or a (v,3) float64 tensor on the device: row j's normal is turned towards viewpoint view_of[j]
    (view_of (m,) int32 on the device; None: viewpoint 0 for every row; -1: not oriented).  A row that is not oriented has the
    canonical sign: its component of largest magnitude is positive.  variation=True: -> (normals, variation (m,) float32 =
    lambda_0 / (lambda_0 + lambda_1 + lambda_2), NaN where the normal is zero)."""
    if not isinstance(self_counts, (bool, np.bool_)):
        raise TypeError('self_counts: expected a bool, got %r' % (self_counts,))
    if not isinstance(idx, torch.Tensor):
        raise TypeError('idx: expected a tensor, got %s' % type(idx).__name__)
    k = int(idx.shape[1]) if idx.dim() == 2 else 0
    if not 1 <= k <= CLOUD_MAX_K:
        raise ValueError('idx: expected shape (m,k) with k in 1..%d, got %s' % (CLOUD_MAX_K, tuple(idx.shape)))
    views = viewpoints
    if viewpoints is not None and not isinstance(viewpoints, torch.Tensor):
        views = np.asarray(viewpoints, np.float64)
        if views.shape == (3,):
            views = views.reshape(1, 3)
        if views.ndim != 2 or views.shape[1] != 3 or not len(views) or not np.isfinite(views).all():
            raise ValueError('viewpoints: expected (v,3) finite numbers, v >= 1, got %r' % (viewpoints,))
    if view_of is not None and views is None:
        raise ValueError('view_of needs viewpoints')
    _cloud_arg(points, 'points', torch.float32, (3,))
    _cloud_arg(queries, 'queries', torch.float32, (3,))
    _cloud_arg(idx, 'idx', torch.int32, (k,))
    n, m = int(points.shape[0]), int(queries.shape[0])
    if int(idx.shape[0]) != m:
        raise ValueError('idx %s must have one row per row of queries %s' % (tuple(idx.shape), tuple(queries.shape)))
    for t, name in ((queries, 'queries'), (idx, 'idx')):
        _same_device(t, name, points, 'points')
    n_views = 0
    if views is not None:
        if not isinstance(views, torch.Tensor):
            views = torch.from_numpy(np.ascontiguousarray(views)).to(points.device)
        _cloud_arg(views, 'viewpoints', torch.float64, (3,))
        _same_device(views, 'viewpoints', points, 'points')
        n_views = int(views.shape[0])
        if n_views < 1:
            raise ValueError('viewpoints: at least one row')
    if view_of is not None:
        _cloud_arg(view_of, 'view_of', torch.int32, ())
        if int(view_of.shape[0]) != m:
            raise ValueError('view_of %s must have one entry per row of queries %s' % (tuple(view_of.shape), tuple(queries.shape)))
        _same_device(view_of, 'view_of', points, 'points')
    normals = torch.empty((m, 3), dtype=torch.float32, device=points.device)
    var = torch.empty(m, dtype=torch.float32, device=points.device) if variation else None
    if m:
        _call('atvs_cloud_normals', _p(points), n, _p(queries), m, _p(idx), k, 1 if self_counts else 0, _p(views), n_views,
              _p(view_of), _p(normals), _p(var), _stream())
    return (normals, var) if variation else normals


CLOUD_FPFH_BINS = _lib.header_macro('ATVS_CLOUD_FPFH_BINS')
CLOUD_RANSAC_MAX_BEST = _lib.header_macro('ATVS_CLOUD_RANSAC_MAX_BEST')
CLOUD_RANSAC_MAX_HYPOTHESES = 1 << 24


def cloud_fpfh(points, idx, normals):
    """points (n,3) float32; idx (n,k) int32 as cloud_knn(grid, points, k, exclude_same_index=True) returned it for the cloud in
    itself (1 <= k <= 32, -1 padded); normals (n,3) float32 as cloud_normals returned them (unoriented, zero rows allowed) ->
    (n,33) float32: the FPFH descriptor of every point (atvs_cloud_fpfh: float64 throughout, no transcendental function; the
    header states every operation).  The normal's sign is made intrinsic first: a point's normal is turned towards the centroid
    of its neighbours, a neighbour's to the side of the point's.  Three features (alpha, phi, theta) of 11 bins each, every part
    scaled to sum 1, so that moving, turning or scaling the cloud and negating any normal leave the descriptor as it is.  The zero
    row where no pair counts (a zero or non-finite normal, no neighbour, duplicates only)."""
    if not isinstance(idx, torch.Tensor):
        raise TypeError('idx: expected a tensor, got %s' % type(idx).__name__)
    k = int(idx.shape[1]) if idx.dim() == 2 else 0
    if not 1 <= k <= CLOUD_MAX_K:
        raise ValueError('idx: expected shape (n,k) with k in 1..%d, got %s' % (CLOUD_MAX_K, tuple(idx.shape)))
    _cloud_arg(points, 'points', torch.float32, (3,))
    _cloud_arg(idx, 'idx', torch.int32, (k,))
    _cloud_arg(normals, 'normals', torch.float32, (3,))
    n = int(points.shape[0])
    if int(idx.shape[0]) != n or int(normals.shape[0]) != n:
        raise ValueError('idx %s and normals %s must have one row per row of points %s' % (
            tuple(idx.shape), tuple(normals.shape), tuple(points.shape)))
    for t, name in ((idx, 'idx'), (normals, 'normals')):
        _same_device(t, name, points, 'points')
    out = torch.empty((n, 3 * CLOUD_FPFH_BINS), dtype=torch.float32, device=points.device)
    if n:
        scratch = torch.empty(_size('atvs_cloud_fpfh_scratch_size', n), dtype=torch.uint8, device=points.device)
        _call('atvs_cloud_fpfh', _p(points), n, _p(idx), k, _p(normals), _p(scratch), scratch.numel(), _p(out), _stream())
    return out


def cloud_feature_nearest(feat_ref, feat_query):
    """feat_ref (n,33) float32, feat_query (m,33) float32 -> (d2 (m,) float32, idx (m,) int32): per query row the smallest
    float32 sum of the 33 squared differences (added in ascending bin order, nothing fused) over the reference rows that are not
    all zero, and the lowest index attaining it; (+inf, -1) for an all-zero query row or when no reference row qualifies.  Exact
    brute force (atvs_cloud_feature_nearest)."""
    width = 3 * CLOUD_FPFH_BINS
    _cloud_arg(feat_ref, 'feat_ref', torch.float32, (width,))
    _cloud_arg(feat_query, 'feat_query', torch.float32, (width,))
    _same_device(feat_query, 'feat_query', feat_ref, 'feat_ref')
    n, m = int(feat_ref.shape[0]), int(feat_query.shape[0])
    d2 = torch.empty(m, dtype=torch.float32, device=feat_ref.device)
    idx = torch.empty(m, dtype=torch.int32, device=feat_ref.device)
    if m:
        _call('atvs_cloud_feature_nearest', _p(feat_ref), n, _p(feat_query), m, _p(d2), _p(idx), _stream())
    return d2, idx


def cloud_ransac(src, dst, triples, tau, with_scale, edge_ratio=0.9, best=4, return_valid=False):
    """src, dst (c,3) float32: row i of one matches row i of the other; triples (h,3) int32: one hypothesis per row, the similarity
    (with_scale) or rigid motion through the three pairs it names (two orthonormal frames, the perimeters' ratio, the centroids;
    no SVD) -> a list of `best` (1..8) dicts in the order larger count, smaller sum, lower index: matrix (3x4 numpy float64: moves
    src onto dst), count (the pairs with |M a - b|^2 <= tau^2, of all c), sum (of those squared distances, float64, in ascending
    pair order), index (the row of `triples`).  A triple is invalid (never returned) when it repeats or leaves 0..c-1, has a
    degenerate triangle, or an edge whose lengths, after the scale, differ by more than the factor edge_ratio.  Slots beyond the
    valid hypotheses have count -1, index -1.  atvs_cloud_ransac_score: the same input gives the same words bit for bit; best x 15
    words cross to the host (one synchronising copy).  return_valid: -> (that list, the number of valid hypotheses), counted on the
    device from the scores the selection read (one more word crosses)."""
    tau, edge_ratio = float(tau), float(edge_ratio)
    if not (tau > 0.0 and math.isfinite(tau)):
        raise ValueError('tau must be positive and finite, got %r' % (tau,))
    if not 0.0 < edge_ratio <= 1.0:
        raise ValueError('edge_ratio must be in (0, 1], got %r' % (edge_ratio,))
    if not isinstance(with_scale, (bool, np.bool_)):
        raise TypeError('with_scale: expected a bool, got %r' % (with_scale,))
    best = _int_in(best, 'best', 1, CLOUD_RANSAC_MAX_BEST)
    _cloud_arg(src, 'src', torch.float32, (3,))
    _cloud_arg(dst, 'dst', torch.float32, (3,))
    _cloud_arg(triples, 'triples', torch.int32, (3,))
    c, h = int(src.shape[0]), int(triples.shape[0])
    if int(dst.shape[0]) != c:
        raise ValueError('dst %s must have one row per row of src %s' % (tuple(dst.shape), tuple(src.shape)))
    if c < 3:
        raise ValueError('%d pairs: a hypothesis needs 3' % c)
    if not 1 <= h <= CLOUD_RANSAC_MAX_HYPOTHESES:
        raise ValueError('triples: 1 to 2^24 rows, got %d' % h)
    for t, name in ((dst, 'dst'), (triples, 'triples')):
        _same_device(t, name, src, 'src')
    out = torch.empty(best * 15, dtype=torch.int64, device=src.device)
    scratch = torch.empty(_size('atvs_cloud_ransac_scratch_size', h), dtype=torch.uint8, device=src.device)
    _call('atvs_cloud_ransac_score', _p(src), _p(dst), c, _p(triples), h, tau, 1 if with_scale else 0, edge_ratio, best,
          _p(scratch), scratch.numel(), _p(out), _stream())
    words = out.cpu().numpy().reshape(best, 15)
    found = [{'matrix': w[:12].view(np.float64).reshape(3, 4).copy(), 'count': int(w[12]), 'sum': float(w[13:14].view(np.float64)[0]),
              'index': int(w[14])} for w in words]
    if not return_valid:
        return found
    return found, int((scratch[:4 * h].view(torch.int32) >= 0).sum().item())         # the scratch begins with the h counts


def scan_render(points, cams, rows, cols, pixel_centre=0.0, splat=0, occlusion_tol=0.0):
    """points (n,3) float32 in the cameras' frame, cams (n_cams,16) float64 = R (3x3 row-major, world to camera), t (3), fx, fy,
    cx, cy -> depth (n_cams, rows, cols) float32: per pixel the nearest float32 depth c_2 of the points that project into it, in
    float64, by u = floor((x - pixel_centre) + 0.5); 0 where none does, and 0 where that depth is further than (1 + occlusion_tol)
    times the nearest depth landing within `splat` pixels (a background point seen through a hole).  splat 0..4; splat = 0 keeps
    every pixel.  include/atvsnet_hip.h has the definition in full; the same inputs give the same bits (integer atomics)."""
    rows, cols = _int_in(rows, 'rows', 1), _int_in(cols, 'cols', 1)
    splat = _int_in(splat, 'splat', 0, SCAN_RENDER_MAX_SPLAT)
    tol, centre = float(occlusion_tol), float(pixel_centre)
    if not (tol >= 0.0 and math.isfinite(tol)):
        raise ValueError('occlusion_tol must be >= 0 and finite, got %r' % (occlusion_tol,))
    if not math.isfinite(centre):
        raise ValueError('pixel_centre must be finite, got %r' % (pixel_centre,))
    _cloud_arg(points, 'points', torch.float32, (3,))
    _cloud_arg(cams, 'cams', torch.float64, (16,))
    _same_device(cams, 'cams', points, 'points')
    n, n_cams = int(points.shape[0]), int(cams.shape[0])
    if not 1 <= n_cams <= SCAN_RENDER_MAX_CAMS:
        raise ValueError('cams: 1 to %d cameras, got %d' % (SCAN_RENDER_MAX_CAMS, n_cams))
    if n_cams * rows * cols >= 1 << 31:
        raise ValueError('%d maps of %d x %d: 2^31 pixels or more' % (n_cams, rows, cols))
    depth = torch.empty((n_cams, rows, cols), dtype=torch.float32, device=points.device)
    scratch = torch.empty(_size('atvs_scan_render_scratch_size', n_cams, rows, cols), dtype=torch.uint8, device=points.device)
    _call('atvs_scan_render', _p(points), n, _p(cams), n_cams, rows, cols, centre, splat, tol,
          _p(scratch), scratch.numel(), _p(depth), _stream())
    return depth


def cloud_scan_excess(points, cams, maps, pixel_centre=0.5, window=1):
    """points (m,3) float32, cams (6 S,16) float64 and maps (6 S,N,N) float32: S scanners' cube maps, six faces each, as
    ops.scan_render rendered them (0 = empty) -> (excess (m,) float32, scanner (m,) int32): the signed distance along the point's
    ray to the nearest scan sample of the (2 window + 1)^2 pixels around where it projects, r (1 - z_scan / c_2) -- negative in
    front of it (free space), positive behind -- minimised over the scanners that observe the point, and the lowest scanner
    attaining it; (+inf, -1) where none does or the point is not finite.  The face is the first of the six in view; a window stays
    inside its face.  window 0..2.  include/atvsnet_hip.h has the definition in full; the output is a function of the inputs."""
    window = _int_in(window, 'window', 0, CLOUD_SCAN_MAX_WINDOW)
    centre = float(pixel_centre)
    if not math.isfinite(centre):
        raise ValueError('pixel_centre must be finite, got %r' % (pixel_centre,))
    _cloud_arg(points, 'points', torch.float32, (3,))
    _cloud_arg(cams, 'cams', torch.float64, (16,))
    n_cams = int(cams.shape[0])
    if n_cams < 6 or n_cams % 6 or n_cams > SCAN_RENDER_MAX_CAMS:
        raise ValueError('cams: six faces per scanner, 6 to %d rows, got %d' % (SCAN_RENDER_MAX_CAMS // 6 * 6, n_cams))
    if not isinstance(maps, torch.Tensor) or maps.dim() != 3 or int(maps.shape[1]) != int(maps.shape[2]) or int(maps.shape[1]) < 1:
        raise ValueError('maps: expected a tensor of shape (%d,N,N), got %s' % (n_cams, tuple(getattr(maps, 'shape', ()))))
    size = int(maps.shape[1])
    _cloud_arg(maps, 'maps', torch.float32, (size, size))
    if int(maps.shape[0]) != n_cams:
        raise ValueError('maps: %d maps for %d cameras' % (int(maps.shape[0]), n_cams))
    if n_cams * size * size >= 1 << 31:
        raise ValueError('%d maps of %d x %d: 2^31 pixels or more' % (n_cams, size, size))
    for t, name in ((cams, 'cams'), (maps, 'maps')):
        _same_device(t, name, points, 'points')
    m = int(points.shape[0])
    excess = torch.empty(m, dtype=torch.float32, device=points.device)
    scanner = torch.empty(m, dtype=torch.int32, device=points.device)
    if m:
        _call('atvs_cloud_scan_excess', _p(points), m, _p(cams), _p(maps), n_cams // 6, size, centre, window,
              _p(excess), _p(scanner), _stream())
    return excess, scanner


def cloud_voxel_shares(points, d2, excess, voxel, origin, tolerances, margin=0.0):
    """points (n,3) float32, d2 (n,) float32 of cloud_nearest, excess (n,) float32 of cloud_scan_excess or None, voxel > 0 and
    origin (3 host numbers; None: the floor of the finite minimum) as for cloud_voxel_downsample, up to 16 tolerances -> (T,4) int64
    on the device, per tolerance tau: sum over voxels of q = (hit * 2^32) // den, the number of voxels with den > 0, sum of hit, sum
    of den.  hit: the voxel's points with double(d2) <= tau * tau; den: all its points when excess is None, else hit + the points
    that are not hit and have double(excess) <= margin (the rest are unobserved).  The voxel-averaged share is
    sum q / (voxels * 2^32).  Integer atomics only: the same inputs give the same words.  A point more than 2^21 voxels from the
    origin, or below it, raises as cloud_voxel_downsample does.  Synchronises once, to read the error word."""
    voxel, margin = float(voxel), float(margin)
    voxel = _voxel(voxel)
    if math.isnan(margin):
        raise ValueError('margin must be a number, got %r' % (margin,))
    tol, _ = _tolerances(tolerances)
    org = origin if origin is None else _vec3(origin, 'origin')
    _cloud_arg(points, 'points', torch.float32, (3,))
    _cloud_arg(d2, 'd2', torch.float32, ())
    n = int(points.shape[0])
    for t, name in ((d2, 'd2'), (excess, 'excess')):
        if t is None:
            continue
        if name == 'excess':
            _cloud_arg(excess, 'excess', torch.float32, ())
        if int(t.shape[0]) != n:
            raise ValueError('%s %s must have one entry per row of points %s' % (name, tuple(t.shape), tuple(points.shape)))
        _same_device(t, name, points, 'points')
    if org is None:
        org = _default_origin(points)
    out = torch.empty((len(tol), 4), dtype=torch.int64, device=points.device)
    scratch = torch.empty(_size('atvs_cloud_voxel_shares_scratch_size', n), dtype=torch.uint8, device=points.device)
    arr = (ctypes.c_double * len(tol))(*tol)
    _call('atvs_cloud_voxel_shares', _p(points), _p(d2), _p(excess), n, voxel, org, arr, len(tol), margin,
          _p(scratch), scratch.numel(), _p(out), _stream())
    if int(out[0, 0].item()) < 0:
        _raise_cell_range('cloud_voxel_shares', points, org, voxel)
    return out
