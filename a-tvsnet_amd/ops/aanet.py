"""AANet aggregation (one launch per module, or score convolution + combine, or the view-sharded partial forms) and the depth-map
fusion entry points (after the hot path: per reference camera, and the whole scene with its staging).
"""

import torch

from .. import _lib
from .base import _Timed, _call, _dev_ok, _new, _p, _ptr_array, _size, _stream, cfg
from .packing import _abi_pack, split_on


def aanet_combine(srs, xs, out=None):
    """srs: list of (V..,16) [S|R] tensors, xs: list of (V..,8) -> sum_n softmax_n(U) X_n, shape of xs[0]
    (written into `out` when given)."""
    out = _new(xs[0], xs[0].shape) if out is None else out
    if _dev_ok(*(list(srs) + list(xs))):
        _call('atvs_aanet_combine', _ptr_array(srs), _ptr_array(xs), len(xs), _p(out), out.numel() // 8, _stream())
    return out


def aanet_fused_ok(xs):
    """Does the whole AANet module over these views run as ONE launch (atvs_aanet_b_f32)?"""
    return (cfg.aanet_fused and cfg.conv_c16 and cfg.force_impl is None and split_on('c16b') and xs[0].dim() == 4
            and xs[0].shape[-1] == 8 and xs[0].shape[2] >= 12 and all(t.is_contiguous() and tuple(t.shape) == tuple(xs[0].shape) for t in xs)
            and bool(_lib.lib().atvs_aanet_b_supported(8, len(xs))))


def aanet_fused(xs, key, w_shared, w_unique):
    """AANet over the views xs (list of (D,H,W,8)): score convolutions + cross-view softmax + weighted sum in one launch ->
    (D,H,W,8).  w_shared / w_unique: host TF kernels [3,3,3,8,8]; key: pack-cache key."""
    pk = _abi_pack('aanet_b', key, (w_shared, w_unique), xs[0].device, 'aanet_b_pack', (), True)
    D, H, W, _ = xs[0].shape
    out = _new(xs[0], xs[0].shape)
    if _dev_ok(out, *xs):
        with _Timed(key, (D, H, W, 8), 16, len(xs)):
            _call('atvs_aanet_b_f32', _ptr_array(xs), len(xs), _p(pk.wp), _p(out), D, H, W, _stream())
    return out


def aanet_partial(srs, xs, stage, ssum=None, umax=None):
    V8 = tuple(xs[0].shape)
    out = _new(xs[0], ((2,) + V8) if stage == 2 else V8)
    if _dev_ok(*(list(srs) + list(xs))):
        _call('atvs_aanet_partial', _ptr_array(srs), _ptr_array(xs), len(srs), int(stage), _p(ssum), _p(umax), _p(out),
              xs[0].numel() // 8, _stream())
    return out


def divide(num, den):
    out = _new(num, num.shape)
    if _dev_ok(num, den):
        _call('atvs_divide', _p(num), _p(den), _p(out), num.numel(), _stream())
    return out


def fusibile(cams, normals_depths, images, ref, disp_thresh, normal_thresh, num_consistent):
    """The consistency-voting kernel of the reference's fusibile for reference camera `ref` (atvs_fusibile).
    cams (N,28), normals_depths / images (N,rows,cols,4) -> coord, normal, texture (rows,cols,4), created (rows,cols)."""
    if not isinstance(normals_depths, torch.Tensor) or normals_depths.dim() != 4:
        raise ValueError('fusibile: normals_depths must be a (N, rows, cols, 4) tensor')
    N, rows, cols, _ = (int(s) for s in normals_depths.shape)
    if not 0 <= int(ref) < N:
        raise ValueError('fusibile: ref must be in 0 .. %d, got %d' % (N - 1, int(ref)))
    launch = _fusion_args((cams, 'cams', torch.float32, (N, 28)), (normals_depths, 'normals_depths', torch.float32, (N, rows, cols, 4)),
                          (images, 'images', torch.float32, (N, rows, cols, 4)))
    coord, normal, tex = (_new(images, (rows, cols, 4)) for _ in range(3))
    created = _new(images, (rows, cols))
    if launch:
        _call('atvs_fusibile', _p(cams), _p(normals_depths), _p(images), N, int(ref), rows, cols, disp_thresh, normal_thresh,
              int(num_consistent), _p(coord), _p(normal), _p(tex), _p(created), _stream())
    return coord, normal, tex, created


def _fusion_args(*specs):
    """Validation of a fusion entry point's tensor arguments before any launch, specs = (tensor, name, dtype, shape): first every
    dtype, shape and layout, then the devices -- the current device, or `meta` for all of them (shape checks only, no launch).
    -> True when the kernel is to be launched."""
    for t, name, dtype, shape in specs:
        if not isinstance(t, torch.Tensor):
            raise TypeError('%s: expected a tensor, got %s' % (name, type(t).__name__))
        if t.dtype != dtype:
            raise TypeError('%s: expected %s, got %s' % (name, dtype, t.dtype))
        if t.dim() != len(shape) or any(int(d) != s for d, s in zip(t.shape, shape)):
            raise ValueError('%s: expected shape %s, got %s' % (name, tuple(shape), tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError('%s: must be contiguous' % name)
    kinds = set(t.device.type for t, _, _, _ in specs)
    if kinds == {'meta'}:
        return False
    if 'meta' in kinds:
        raise RuntimeError('mixing meta and device tensors')
    for t, name, _, _ in specs:
        if t.device.type != 'cuda':
            raise RuntimeError('%s: the fusion kernels run on the MI355X only (no CPU fallback), got a tensor on %s' % (name, t.device))
        if t.device.index != torch.cuda.current_device():
            raise RuntimeError('%s: on %s, the launch goes to the current device cuda:%d' % (name, t.device,
                                                                                              torch.cuda.current_device()))
    return True


def fusion_stage(depth, prob, bgr, inverse_depth, prob_thresh, nd_out, img_out):
    """One finished depth map into its slot of a scene's fusion slab (atvs_fusion_stage_f32): depth, prob (rows, cols) float32,
    bgr (rows, cols, 3) uint8 -> nd_out (rows, cols, 4) = (normal, filtered depth), img_out (rows, cols, 4) = (b, g, r, 0), both
    float32 and written in place (typically rows of a (N, rows, cols, 4) slab).  On the current stream."""
    if not isinstance(depth, torch.Tensor) or depth.dim() != 2:
        raise ValueError('fusion_stage: depth must be a (rows, cols) tensor')
    rows, cols = (int(s) for s in depth.shape)
    if _fusion_args((depth, 'depth', torch.float32, (rows, cols)), (prob, 'prob', torch.float32, (rows, cols)),
                    (bgr, 'bgr', torch.uint8, (rows, cols, 3)), (nd_out, 'nd_out', torch.float32, (rows, cols, 4)),
                    (img_out, 'img_out', torch.float32, (rows, cols, 4))):
        _call('atvs_fusion_stage_f32', _p(depth), _p(prob), _p(bgr), rows, cols, int(bool(inverse_depth)), prob_thresh,
              _p(nd_out), _p(img_out), _stream())
    return nd_out, img_out


def depth_normals(cams, normals_depths, step=1, depth_gate=0.02):
    """Normals of a scene's depth maps from the maps themselves (atvs_depth_normals_f32): cams (N,28), normals_depths
    (N,rows,cols,4) float32 = (nx, ny, nz, depth), whose three normal floats are rewritten IN PLACE from its depth plane (which is
    left as it is): the float64 cross products of the four neighbour quadrants at `step` pixels, a neighbour counting when its
    depth is within depth_gate * depth, oriented towards the camera; (0,0,0) where there is no depth or no usable quadrant.
    On the current stream.  -> normals_depths."""
    if not isinstance(normals_depths, torch.Tensor) or normals_depths.dim() != 4:
        raise ValueError('depth_normals: normals_depths must be a (N, rows, cols, 4) tensor')
    if int(step) != step or int(step) < 1:
        raise ValueError('depth_normals: step must be an integer >= 1, got %r' % (step,))
    depth_gate = float(depth_gate)
    if not (0.0 <= depth_gate < float('inf')):
        raise ValueError('depth_normals: depth_gate must be >= 0 and finite, got %r' % (depth_gate,))
    N, rows, cols, _ = (int(s) for s in normals_depths.shape)
    if _fusion_args((cams, 'cams', torch.float32, (N, 28)), (normals_depths, 'normals_depths', torch.float32, (N, rows, cols, 4))):
        _call('atvs_depth_normals_f32', _p(cams), _p(normals_depths), N, rows, cols, int(step), depth_gate, _stream())
    return normals_depths


def fusibile_scene(cams, normals_depths, images, disp_thresh, normal_thresh, num_consistent, with_normals=False):
    """Every reference camera of the slab fused in one pass, the host filter of fuse_views applied and the kept points compacted on
    the device (atvs_fusibile_scene).  cams (N,28), normals_depths / images (N,rows,cols,4) float32 -> (points (M,3) float32,
    colors (M,3) uint8 r,g,b) on the device, camera-major and row-major as fuse_views concatenates them.  Reads the count back
    (one synchronisation of the current stream).
    with_normals: -> (points, colors, normals (M,3) float32), the normal averaged over the reference and the agreeing views of
    every point, not normalised (atvs_fusibile_scene_normals; points and colours are the same bits)."""
    if not isinstance(normals_depths, torch.Tensor) or normals_depths.dim() != 4:
        raise ValueError('fusibile_scene: normals_depths must be a (N, rows, cols, 4) tensor')
    N, rows, cols, _ = (int(s) for s in normals_depths.shape)
    if not _fusion_args((cams, 'cams', torch.float32, (N, 28)), (normals_depths, 'normals_depths', torch.float32, (N, rows, cols, 4)),
                        (images, 'images', torch.float32, (N, rows, cols, 4))):
        raise RuntimeError('fusibile_scene: the number of points is only known after a launch (got meta tensors)')
    dev = normals_depths.device
    capacity = N * rows * cols
    name = 'atvs_fusibile_scene_normals' if with_normals else 'atvs_fusibile_scene'
    scratch = torch.empty(_size(name + '_scratch_size', N, rows, cols), dtype=torch.uint8, device=dev)
    points = torch.empty((capacity, 3), dtype=torch.float32, device=dev)
    colors = torch.empty((capacity, 3), dtype=torch.uint8, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    outputs = [points, colors] + ([torch.empty((capacity, 3), dtype=torch.float32, device=dev)] if with_normals else [])
    _call(name, _p(cams), _p(normals_depths), _p(images), N, rows, cols, disp_thresh, normal_thresh, int(num_consistent),
          _p(scratch), scratch.numel(), *([_p(t) for t in outputs] + [capacity, _p(count), _stream()]))
    m = int(count.item())
    return tuple(t[:m] for t in outputs)


FUSION_SUPPORT_OUTPUTS = ('count', 'depth', 'weight')


def fusion_support(cams, normals_depths, disp_thresh, normal_thresh, num_consistent, want=FUSION_SUPPORT_OUTPUTS):
    """The fusion's agreement count of every pixel of the slab, from the fusion's own loop without the images (atvs_fusion_support,
    one launch, no synchronisation).  cams (N,28), normals_depths (N,rows,cols,4) float32 -> a dict of what `want` names, each
    (N,rows,cols) on the slab's device:
        count   int32: fusibile's count of the pixel -- the other views, ascending, that pass the in-image, disparity and normal test;
        depth   float32: the pixel's own depth, bit for bit, where count >= num_consistent, +0 elsewhere (the consistency-masked plane);
        weight  float32: float32(1 + count) / float32(1 + num_consistent), for every pixel whatever the mask says: 1 for a sample that
                just passes the mask, more for a better supported one (a default, not a measurement).
    `meta` tensors run the host checks alone (the outputs come back on `meta`)."""
    if not isinstance(normals_depths, torch.Tensor) or normals_depths.dim() != 4:
        raise ValueError('fusion_support: normals_depths must be a (N, rows, cols, 4) tensor')
    if isinstance(num_consistent, bool) or int(num_consistent) != num_consistent or int(num_consistent) < 0:
        raise ValueError('fusion_support: num_consistent must be an integer >= 0, got %r' % (num_consistent,))
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or len(set(want)) != len(want) or any(w not in FUSION_SUPPORT_OUTPUTS for w in want):
        raise ValueError('fusion_support: want must name at least one of %s, each once, got %r' % (FUSION_SUPPORT_OUTPUTS, want))
    N, rows, cols, _ = (int(s) for s in normals_depths.shape)
    launch = _fusion_args((cams, 'cams', torch.float32, (N, 28)), (normals_depths, 'normals_depths', torch.float32, (N, rows, cols, 4)))
    if N < 1 or rows < 1 or cols < 1 or -(-rows * cols // 256) * 256 * N > 0x7fffffff:
        raise ValueError('fusion_support: %d maps of %d x %d: at least one pixel, and fewer than 2^31 with every map rounded up to '
                         '256 pixels' % (N, rows, cols))
    out = {w: torch.empty((N, rows, cols), dtype=torch.int32 if w == 'count' else torch.float32, device=normals_depths.device)
           for w in want}
    if launch:
        _call('atvs_fusion_support', _p(cams), _p(normals_depths), N, rows, cols, disp_thresh, normal_thresh, int(num_consistent),
              _p(out.get('count')), _p(out.get('depth')), _p(out.get('weight')), _stream())
    return out
