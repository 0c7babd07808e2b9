"""A surface from depth maps on the device (csrc/tsdf.hip): `tsdf_integrate` fuses depth maps (and their images) into a block-sparse
truncated-signed-distance volume, `tsdf_mesh` extracts an indexed, coloured triangle mesh from one by marching tetrahedra.  The
definitions the kernels are held to are in include/atvsnet_hip.h and restated in tests/tsdf_restated.py; atvsnet/mesh_fusion.py is
built on them.

`TsdfVolume` is the volume: a box of `dims` = (bx, by, bz) blocks of 8^3 voxels at `origin`, and exactly the blocks that have a
voxel of weight > 0.  `TsdfVolume.from_dense` / `.to_dense` are plain torch / numpy helpers (no kernel) to build or inspect one.
"""

import math

import numpy as np
import torch

from .. import _lib
from .base import _call, _p, _size, _stream
from .cloud import _int_in, _same_device, _vec3, _voxel, SCAN_RENDER_MAX_CAMS

TSDF_BLOCK = 8
TSDF_MAX_DIRECTORY = _lib.header_macro('ATVS_TSDF_MAX_DIRECTORY')
TSDF_MAX_MESH_BLOCKS = _lib.header_macro('ATVS_TSDF_MAX_MESH_BLOCKS')
TSDF_MAX_PIXEL_BLOCKS = _lib.header_macro('ATVS_TSDF_MAX_PIXEL_BLOCKS')


def _dims(dims):
    d = tuple(dims)
    if len(d) != 3:
        raise ValueError('dims: expected (bx, by, bz), got %r' % (dims,))
    d = tuple(_int_in(v, 'dims', 1) for v in d)
    if d[0] * d[1] * d[2] > TSDF_MAX_DIRECTORY:
        raise ValueError('dims %r: %d blocks, at most 2^26' % (d, d[0] * d[1] * d[2]))
    return d


def _trunc(trunc):
    trunc = float(trunc)
    if not (trunc > 0.0 and math.isfinite(trunc)):
        raise ValueError('trunc must be positive and finite, got %r' % (trunc,))
    return trunc


class TsdfVolume(object):
    """A block-sparse TSDF volume.  origin: 3 host float64 (the corner of voxel (0,0,0); its centre is origin + 0.5 voxel), voxel,
    trunc: floats, dims: (bx, by, bz) blocks of 8^3 voxels; blocks (nb,3) int32 block coordinates (x, y, z), ascending in the linear
    index (z by + y) bx + x; tsdf, weight (nb,8,8,8) float32 indexed [z][y][x]; color (nb,8,8,8,3) float32 (b, g, r) or None; free
    (nb,8,8,8) float32, the views that saw past each voxel, or None (only tsdf_integrate with carve_weight gives one; from_dense,
    to_dense and tsdf_mesh ignore it)."""
    __slots__ = ('origin', 'voxel', 'trunc', 'dims', 'blocks', 'tsdf', 'weight', 'color', 'free')

    def __init__(self, origin, voxel, trunc, dims, blocks, tsdf, weight, color=None, free=None):
        self.origin = np.array(list(_vec3(origin, 'origin')), np.float64)
        self.voxel, self.trunc, self.dims = _voxel(voxel), _trunc(trunc), _dims(dims)
        nb = int(blocks.shape[0])
        for t, name, dtype, shape in ((blocks, 'blocks', torch.int32, (nb, 3)), (tsdf, 'tsdf', torch.float32, (nb, 8, 8, 8)),
                                      (weight, 'weight', torch.float32, (nb, 8, 8, 8)), (color, 'color', torch.float32, (nb, 8, 8, 8, 3)),
                                      (free, 'free', torch.float32, (nb, 8, 8, 8))):
            if t is None and name in ('color', 'free'):
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape:
                raise ValueError('%s: expected a %s tensor of shape %s, got %s %s' % (
                    name, dtype, shape, getattr(t, 'dtype', type(t).__name__), tuple(getattr(t, 'shape', ()))))
            if t.device != blocks.device:
                raise RuntimeError('%s on %s, blocks on %s' % (name, t.device, blocks.device))
        self.blocks, self.tsdf, self.weight, self.color, self.free = blocks, tsdf, weight, color, free

    @property
    def device(self):
        return self.blocks.device

    @property
    def num_blocks(self):
        return int(self.blocks.shape[0])

    @classmethod
    def from_dense(cls, tsdf, weight, color, origin, voxel, trunc, device=None):
        """Dense arrays indexed [z][y][x] (numpy or torch; color (...,3) b, g, r or None) -> the volume of the blocks that have a
        voxel of weight > 0, on `device` (None: the CPU).  The arrays are padded to whole blocks with weight 0."""
        def host(a, tail):
            a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
            if a.ndim != 3 + len(tail) or tuple(a.shape[3:]) != tail:
                raise ValueError('expected a dense [z][y][x]%s array, got shape %s' % (''.join('[%d]' % t for t in tail), a.shape))
            return a.astype(np.float32)
        f, w = host(tsdf, ()), host(weight, ())
        c = None if color is None else host(color, (3,))
        if f.shape != w.shape or (c is not None and c.shape[:3] != f.shape):
            raise ValueError('tsdf, weight and color differ in shape')
        nz, ny, nx = f.shape
        bz, by, bx = (-(-s // TSDF_BLOCK) for s in (nz, ny, nx))
        dims = _dims((bx, by, bz))

        def blocked(a):
            pad = [(0, bz * 8 - nz), (0, by * 8 - ny), (0, bx * 8 - nx)] + [(0, 0)] * (a.ndim - 3)
            a = np.pad(a, pad)
            a = a.reshape((bz, 8, by, 8, bx, 8) + a.shape[3:])
            return a.transpose((0, 2, 4, 1, 3, 5) + tuple(range(6, a.ndim))).reshape((bz * by * bx, 8, 8, 8) + a.shape[6:])
        fb, wb = blocked(f), blocked(w)
        keep = np.flatnonzero((wb > 0).reshape(len(wb), -1).any(axis=1))
        blocks = np.stack([keep % bx, (keep // bx) % by, keep // (bx * by)], axis=1).astype(np.int32).reshape(-1, 3)
        dev = torch.device('cpu') if device is None else torch.device(device)

        def put(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return cls(origin, voxel, trunc, dims, put(blocks), put(fb[keep]), put(wb[keep]), None if c is None else put(blocked(c)[keep]))

    def to_dense(self):
        """-> (tsdf, weight, color or None): host numpy arrays over the whole box, indexed [z][y][x]; weight 0 where no block is."""
        bx, by, bz = self.dims
        blocks = self.blocks.detach().cpu().numpy().astype(np.int64)
        lin = (blocks[:, 2] * by + blocks[:, 1]) * bx + blocks[:, 0]

        def dense(t, tail):
            full = np.zeros((bz * by * bx, 8, 8, 8) + tail, np.float32)
            full[lin] = t.detach().cpu().numpy()
            full = full.reshape((bz, by, bx, 8, 8, 8) + tail)
            return np.ascontiguousarray(full.transpose((0, 3, 1, 4, 2, 5) + tuple(range(6, 6 + len(tail)))).reshape(
                (bz * 8, by * 8, bx * 8) + tail))
        return dense(self.tsdf, ()), dense(self.weight, ()), None if self.color is None else dense(self.color, (3,))


def _scan(counters, count, total=None):
    """Exclusive prefix sum of `count` uint32 words (held in an int32 tensor) in place -> `total`, a 1-element int64 device tensor
    (None: a new one): their sum."""
    if total is None:
        total = torch.empty(1, dtype=torch.int64, device=counters.device)
    scratch = torch.empty(_size('atvs_tsdf_scan_scratch_size', count), dtype=torch.uint8, device=counters.device)
    _call('atvs_tsdf_scan', _p(counters), count, _p(scratch), scratch.numel(), _p(total), _stream())
    return total


def _map_arg(t, name, dtype, dim, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s: expected a tensor, got %s' % (name, type(t).__name__))
    if t.dtype != dtype:
        raise TypeError('%s: expected %s, got %s' % (name, dtype, t.dtype))
    if t.dim() != dim:
        raise ValueError('%s: expected %s, got shape %s' % (name, what, tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError('%s: must be contiguous' % name)


def _launchable(t, name):
    """True for a tensor on the current device, False on `meta` (the host checks alone run); anything else raises."""
    if t.device.type == 'meta':
        return False
    if t.device.type != 'cuda':
        raise RuntimeError('%s: the TSDF kernels run on the MI355X only (no CPU fallback), got a tensor on %s' % (name, t.device))
    if t.device.index != torch.cuda.current_device():
        raise RuntimeError('%s: on %s, the launch goes to the current device cuda:%d' % (name, t.device, torch.cuda.current_device()))
    return True


def _empty_volume(origin, voxel, trunc, dims, device, with_color, with_free=False):
    return TsdfVolume(origin, voxel, trunc, dims, torch.empty((0, 3), dtype=torch.int32, device=device),
                      torch.empty((0, 8, 8, 8), dtype=torch.float32, device=device),
                      torch.empty((0, 8, 8, 8), dtype=torch.float32, device=device),
                      torch.empty((0, 8, 8, 8, 3), dtype=torch.float32, device=device) if with_color else None,
                      torch.empty((0, 8, 8, 8), dtype=torch.float32, device=device) if with_free else None)


def _carve_weight(carve_weight):
    """None, or the weight of a free vote as a float: finite and > 0; anything else raises ValueError."""
    if carve_weight is None:
        return None
    if isinstance(carve_weight, bool) or not isinstance(carve_weight, (int, float, np.integer, np.floating)):
        raise ValueError('carve_weight must be None or a finite number > 0, got %r' % (carve_weight,))
    cw = float(carve_weight)
    if not (cw > 0.0 and math.isfinite(cw)):
        raise ValueError('carve_weight must be None or a finite number > 0, got %r' % (carve_weight,))
    return cw


def tsdf_free_views(blocks, cams, rows, cols, voxel, origin, dims, pixel_centre=0.0):
    """blocks (count,3) int32 block coordinates of the box (origin, voxel, dims), cams (n,16) float64 -> (count, ceil(n/64)) int64:
    bit v of a block's words is set unless view v provably sees no voxel centre of the block (include/atvsnet_hip.h has the rule:
    the eight corners of the block's cube projected, their bounding box padded by a pixel against the image; depths are not
    consulted).  A superset of the views that contribute to or carve a voxel of the block: what tsdf_integrate's carving loops over."""
    voxel, dims = _voxel(voxel), _dims(dims)
    org = _vec3(origin, 'origin')
    centre = float(pixel_centre)
    if not math.isfinite(centre):
        raise ValueError('pixel_centre must be finite, got %r' % (pixel_centre,))
    rows, cols = _int_in(rows, 'rows', 1), _int_in(cols, 'cols', 1)
    _map_arg(blocks, 'blocks', torch.int32, 2, '(count,3)')
    _map_arg(cams, 'cams', torch.float64, 2, '(n,16)')
    count, n = int(blocks.shape[0]), int(cams.shape[0])
    if int(blocks.shape[1]) != 3:
        raise ValueError('blocks: expected shape (count,3), got %s' % (tuple(blocks.shape),))
    if int(cams.shape[1]) != 16 or not 1 <= n <= SCAN_RENDER_MAX_CAMS:
        raise ValueError('cams: expected shape (n,16) with 1 <= n <= %d, got %s' % (SCAN_RENDER_MAX_CAMS, tuple(cams.shape)))
    if n * rows * cols >= 1 << 31:
        raise ValueError('%d maps of %d x %d: 2^31 pixels or more' % (n, rows, cols))
    if count > dims[0] * dims[1] * dims[2]:
        raise ValueError('blocks: %d blocks in a box of %d' % (count, dims[0] * dims[1] * dims[2]))
    _same_device(cams, 'cams', blocks, 'blocks')
    masks = torch.empty((count, (n + 63) // 64), dtype=torch.int64, device=blocks.device)
    if _launchable(blocks, 'blocks') and count:
        _call('atvs_tsdf_free_views', _p(blocks), count, _p(cams), n, rows, cols, voxel, org, *dims, centre, _p(masks), _stream())
    return masks


def tsdf_integrate(depths, cams, voxel, trunc, origin, dims, images=None, pixel_centre=0.0, max_blocks=131072, carve_weight=None,
                   weights=None):
    """depths (n,rows,cols) float32 z-depth (0 or non-finite: no sample), cams (n,16) float64 in scan_render's layout, images
    (n,rows,cols,C>=3) float32 with b, g, r in channels 0..2 or None -> TsdfVolume over the box (origin, voxel, dims).

    Per voxel and view, in float64: the voxel's centre is projected as scan_render projects a point; the view contributes when the
    pixel's depth d is > 0 and finite and sdf = d - c_2 lies in [-trunc, trunc]; tsdf is the mean of sdf / trunc, weight the number
    of contributing views, color the mean of the pixels' b, g, r.  A view outside that band adds nothing (no free-space carving).
    The volume holds exactly the blocks with a voxel of weight > 0; the same inputs give the same bits.  Blocks are first marked
    conservatively from the maps; more than `max_blocks` marked blocks raise a ValueError that names the count, and a voxel so small
    that one pixel's depth segment meets more than 4096 blocks raises too.  Synchronises twice (the two counts).

    carve_weight: None (the above, with the launches it always made), or a finite number > 0: free-space carving.  A view whose
    depth lies beyond a voxel's band (sdf > trunc) has seen past the voxel: it adds 1 to the voxel's `free` count Wf and no colour,
    and tsdf = (S + cw Wf) / (W + cw Wf) over the in-band sums S, W.  weight stays the in-band count, a voxel no view has in band
    is not carved, so blocks, weight and color keep their bits, and tsdf does wherever free == 0; the volume's `free` holds Wf.
    One more launch (tsdf_free_views: the views that can see into each marked block) and a second form of the integrate kernel.

    weights: None (the above, with the launches it always made), or (n,rows,cols) float32 on the depths' device: the weight w of
    every pixel of every view (ops.fusion_support's `weight`, a probability map, ...).  A view is a sample at the pixel it lands on
    only when also w > 0 and w is finite -- a weight that is 0, negative, NaN or infinite neither contributes nor carves -- and it
    then adds w where it added 1: S += w (sdf / trunc), W += w, C += w image, with carving Wf += w.  weight is the sum of the
    weights (tsdf_mesh's min_weight is compared with it as before), free the sum of the free views' weights.  Blocks are marked
    from the depths alone; the volume still holds exactly the blocks with a voxel of weight > 0.  All-ones weights give the bits of
    the call without weights; a third form of the integrate kernel (atvs_tsdf_integrate_weighted), with or without carve_weight."""
    cw = _carve_weight(carve_weight)
    voxel, trunc, dims = _voxel(voxel), _trunc(trunc), _dims(dims)
    org = _vec3(origin, 'origin')
    centre = float(pixel_centre)
    if not math.isfinite(centre):
        raise ValueError('pixel_centre must be finite, got %r' % (pixel_centre,))
    max_blocks = _int_in(max_blocks, 'max_blocks', 1)
    _map_arg(depths, 'depths', torch.float32, 3, '(n,rows,cols)')
    _map_arg(cams, 'cams', torch.float64, 2, '(n,16)')
    n, rows, cols = (int(s) for s in depths.shape)
    if tuple(cams.shape) != (n, 16):
        raise ValueError('cams: expected shape (%d,16), got %s' % (n, tuple(cams.shape)))
    if not 1 <= n <= SCAN_RENDER_MAX_CAMS or rows < 1 or cols < 1:
        raise ValueError('depths: 1 to %d maps of at least one pixel, got shape %s' % (SCAN_RENDER_MAX_CAMS, tuple(depths.shape)))
    if n * rows * cols >= 1 << 31:
        raise ValueError('%d maps of %d x %d: 2^31 pixels or more' % (n, rows, cols))
    _same_device(cams, 'cams', depths, 'depths')
    channels = 0
    if images is not None:
        _map_arg(images, 'images', torch.float32, 4, '(n,rows,cols,C)')
        if tuple(images.shape[:3]) != (n, rows, cols) or int(images.shape[3]) < 3:
            raise ValueError('images: expected shape (%d,%d,%d,C>=3), got %s' % (n, rows, cols, tuple(images.shape)))
        _same_device(images, 'images', depths, 'depths')
        channels = int(images.shape[3])
    if weights is not None:
        _map_arg(weights, 'weights', torch.float32, 3, '(n,rows,cols)')
        if tuple(weights.shape) != (n, rows, cols):
            raise ValueError('weights: expected shape (%d,%d,%d), got %s' % (n, rows, cols, tuple(weights.shape)))
        _same_device(weights, 'weights', depths, 'depths')
    dev = depths.device
    if not _launchable(depths, 'depths'):
        return _empty_volume(origin, voxel, trunc, dims, dev, images is not None, cw is not None)
    bx, by, bz = dims
    nbk = bx * by * bz
    box = (voxel, trunc, org, bx, by, bz, centre)
    directory = torch.empty(nbk, dtype=torch.int32, device=dev)
    err = torch.empty(1, dtype=torch.int32, device=dev)
    _call('atvs_tsdf_mark', _p(depths), _p(cams), n, rows, cols, *box, _p(directory), _p(err), _stream())
    total = _scan(directory, nbk)
    count, bad = int(total.item()), int(err.item())
    if bad:
        raise ValueError('tsdf_integrate: voxel too small for these maps: one pixel\'s depth segment of +-%g meets more than %d blocks '
                         'of %g' % (trunc, TSDF_MAX_PIXEL_BLOCKS, 8 * voxel))
    if count > max_blocks:
        raise ValueError('tsdf_integrate: the maps mark %d blocks of %d, max_blocks is %d: raise it, or the voxel' % (count, nbk, max_blocks))
    if count == 0:
        return _empty_volume(origin, voxel, trunc, dims, dev, images is not None, cw is not None)
    words = (n + 63) // 64
    coords = torch.empty((count, 3), dtype=torch.int32, device=dev)
    masks = torch.empty((count, words), dtype=torch.int64, device=dev)
    _call('atvs_tsdf_assign', _p(depths), _p(cams), n, rows, cols, *box, _p(directory), count, _p(coords), _p(masks), _p(err), _stream())
    tsdf = torch.empty((count, 8, 8, 8), dtype=torch.float32, device=dev)
    weight = torch.empty((count, 8, 8, 8), dtype=torch.float32, device=dev)
    color = torch.empty((count, 8, 8, 8, 3), dtype=torch.float32, device=dev) if images is not None else None
    keep = torch.empty(count, dtype=torch.int32, device=dev)
    free = None
    if weights is not None:
        free_masks = None if cw is None else tsdf_free_views(coords, cams, rows, cols, voxel, origin, dims, centre)
        free = None if cw is None else torch.empty((count, 8, 8, 8), dtype=torch.float32, device=dev)
        _call('atvs_tsdf_integrate_weighted', _p(depths), _p(weights), _p(images), channels, _p(cams), n, rows, cols, *box, _p(coords),
              _p(masks), _p(free_masks), 0.0 if cw is None else cw, count, _p(tsdf), _p(weight), _p(color), _p(free), _p(keep), _stream())
    elif cw is None:
        _call('atvs_tsdf_integrate', _p(depths), _p(images), channels, _p(cams), n, rows, cols, *box, _p(coords), _p(masks), count,
              _p(tsdf), _p(weight), _p(color), _p(keep), _stream())
    else:
        free_masks = tsdf_free_views(coords, cams, rows, cols, voxel, origin, dims, centre)
        free = torch.empty((count, 8, 8, 8), dtype=torch.float32, device=dev)
        _call('atvs_tsdf_integrate_carve', _p(depths), _p(images), channels, _p(cams), n, rows, cols, *box, _p(coords), _p(masks),
              _p(free_masks), cw, count, _p(tsdf), _p(weight), _p(color), _p(free), _p(keep), _stream())
    kept = int(_scan(keep, count).item())
    if kept == count:
        return TsdfVolume(origin, voxel, trunc, dims, coords, tsdf, weight, color, free)
    out = _empty_volume(origin, voxel, trunc, dims, dev, images is not None, cw is not None)
    if kept == 0:
        return out
    out.blocks = torch.empty((kept, 3), dtype=torch.int32, device=dev)
    out.tsdf = torch.empty((kept, 8, 8, 8), dtype=torch.float32, device=dev)
    out.weight = torch.empty((kept, 8, 8, 8), dtype=torch.float32, device=dev)
    out.color = torch.empty((kept, 8, 8, 8, 3), dtype=torch.float32, device=dev) if images is not None else None
    out.free = torch.empty((kept, 8, 8, 8), dtype=torch.float32, device=dev) if cw is not None else None
    _call('atvs_tsdf_gather', _p(coords), _p(tsdf), _p(weight), _p(color), _p(keep), count, kept,
          _p(out.blocks), _p(out.tsdf), _p(out.weight), _p(out.color), _p(free), _p(out.free), _stream())
    return out


def tsdf_mesh(volume, min_weight=1.0):
    """TsdfVolume -> (vertices (V,3) float32, colors (V,3) uint8 r, g, b or None, faces (F,3) int32) by marching tetrahedra.

    A voxel is valid when weight >= min_weight and inside when tsdf < 0.  The cube of 8 neighbouring voxel centres is meshed when
    all 8 are valid, as six Kuhn tetrahedra; a vertex lies on an edge whose endpoints differ in `inside`, at t = fa / (fa - fb),
    with the colour interpolated alike.  Normals point from the surface into free space.  Vertices are ordered by owning voxel
    (blocks ascending, x fastest) and edge type, faces by cube, tetrahedron and triangle; no vertex is unreferenced; zero-area
    triangles (tsdf == 0 at a corner) are kept.  include/atvsnet_hip.h has the definition in full.  The volume's blocks must be
    ascending in the linear index and distinct, as tsdf_integrate and from_dense make them (neighbours are found by binary search;
    this is not checked).  At most 2^18 blocks.  Synchronises once (V and F)."""
    if not isinstance(volume, TsdfVolume):
        raise TypeError('volume: expected a TsdfVolume, got %s' % type(volume).__name__)
    mw = float(min_weight)
    if math.isnan(mw):
        raise ValueError('min_weight must be a number, got %r' % (min_weight,))
    mw = float(np.float32(mw))
    nb = volume.num_blocks
    if nb > TSDF_MAX_MESH_BLOCKS:
        raise ValueError('tsdf_mesh: %d blocks, at most %d' % (nb, TSDF_MAX_MESH_BLOCKS))
    dev = volume.device
    for t, name in ((volume.blocks, 'blocks'), (volume.tsdf, 'tsdf'), (volume.weight, 'weight'), (volume.color, 'color')):
        if t is not None and not t.is_contiguous():
            raise ValueError('volume.%s: must be contiguous' % name)
    launch = _launchable(volume.blocks, 'volume')

    def empty():
        return (torch.empty((0, 3), dtype=torch.float32, device=dev),
                None if volume.color is None else torch.empty((0, 3), dtype=torch.uint8, device=dev),
                torch.empty((0, 3), dtype=torch.int32, device=dev))
    if not launch or nb == 0:
        return empty()
    bx, by, bz = volume.dims
    org = _vec3(volume.origin, 'origin')
    cube_ok = torch.empty(nb * 512, dtype=torch.uint8, device=dev)
    emask = torch.empty(nb * 512, dtype=torch.uint8, device=dev)
    counts = torch.empty((2, nb * 512), dtype=torch.int32, device=dev)
    _call('atvs_tsdf_mesh_count', _p(volume.blocks), nb, bx, by, bz, _p(volume.tsdf), _p(volume.weight), mw,
          _p(cube_ok), _p(emask), _p(counts[0]), _p(counts[1]), _stream())
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    _scan(counts[0], nb * 512, totals[0:1])
    _scan(counts[1], nb * 512, totals[1:2])
    totals = totals.cpu()
    nv, nf = int(totals[0]), int(totals[1])
    if nv == 0 and nf == 0:
        return empty()
    vertices = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    colors = None if volume.color is None else torch.empty((nv, 3), dtype=torch.uint8, device=dev)
    faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    _call('atvs_tsdf_mesh_emit', _p(volume.blocks), nb, bx, by, bz, volume.voxel, org, _p(volume.tsdf), _p(volume.color),
          _p(emask), _p(counts[0]), _p(counts[1]), nv, nf, _p(vertices), _p(colors), _p(faces), _stream())
    return vertices, colors, faces
