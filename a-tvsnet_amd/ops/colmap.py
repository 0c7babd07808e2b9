"""COLMAP model import on the device (csrc/colmap.hip): the per-image depth range by exact rank selection and the co-visibility
matrix of shared 3-D points; and the undistortion of distorted camera models (csrc/undistort.hip): the per-camera sampling map
and the image gather.  The host side (model reader, CSR build, scene writer) is atvsnet/colmap.py, that of the undistortion
(forward models, their inverse, the output camera) atvsnet/undistort.py.
"""

import ctypes

import torch

from .base import _call, _p, _size, _stream

COVIS_MAX_IMAGES = 16384            # atvs_colmap_covisibility: an (images x images) int32 matrix of at most 1 GiB
# atvs_undistort_map: COLMAP's camera model ids of the models it undistorts, and their parameter counts
UNDISTORT_MODELS = {'SIMPLE_RADIAL': (2, 4), 'RADIAL': (3, 5), 'OPENCV': (4, 8), 'OPENCV_FISHEYE': (5, 8), 'FULL_OPENCV': (6, 12),
                    'SIMPLE_RADIAL_FISHEYE': (8, 4), 'RADIAL_FISHEYE': (9, 5), 'THIN_PRISM_FISHEYE': (10, 12)}
UNDISTORT_MAX_SIDE = 1 << 21        # (side - 1) * 1024 stays an int32


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
    scratch = torch.empty(_size('atvs_colmap_depth_range_scratch_size', n_images), dtype=torch.uint8, device=dev)
    n = torch.empty(n_images, dtype=torch.int32, device=dev)
    d_lo = torch.empty(n_images, dtype=torch.float64, device=dev)
    d_hi = torch.empty(n_images, dtype=torch.float64, device=dev)
    _call('atvs_colmap_depth_range', _p(points), int(points.shape[0]), _p(cams), n_images,
          float(percentile), _p(scratch), scratch.numel(), _p(n), _p(d_lo), _p(d_hi), _stream())
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


def _image_size(width, height, what):
    width, height = int(width), int(height)
    if not (1 <= width <= UNDISTORT_MAX_SIDE and 1 <= height <= UNDISTORT_MAX_SIDE and width * height <= 0x7fffffff):
        raise ValueError('%s of %d x %d pixels: sides of 1 to %d and at most 2^31 - 1 pixels (the int32 pixel index)' %
                         (what, width, height, UNDISTORT_MAX_SIDE))
    return width, height


def undistort_map(model, params, width, height, camera):
    """The sampling map of one camera (atvs_undistort_map).  model: a name of UNDISTORT_MODELS, params: its parameters in COLMAP's
    order, width x height: the distorted camera's size; camera = ((fx, fy, cx, cy), (W', H')) the undistorted pinhole camera
    (atvsnet.undistort.undistorted_camera) -> (H', W', 2) int32 on the current device: per output pixel the source coordinate
    in 22.10 fixed point, (INT32_MIN, 0) where it falls outside the source."""
    if model not in UNDISTORT_MODELS:
        raise ValueError('model %r: the undistortion knows %s' % (model, ', '.join(sorted(UNDISTORT_MODELS))))
    model_id, npar = UNDISTORT_MODELS[model]
    p = [float(v) for v in params]
    if len(p) != npar:
        raise ValueError('%s takes %d parameters, got %d' % (model, npar, len(p)))
    (fx, fy, cx, cy), (wo, ho) = camera
    k = [float(fx), float(fy), float(cx), float(cy)]
    if not all(abs(v) < float('inf') for v in p + k):               # NaN fails the comparison too
        raise ValueError('%s: parameters %r and camera %r must be finite' % (model, tuple(p), tuple(k)))
    if k[0] == 0.0 or k[1] == 0.0:
        raise ValueError('camera: a focal length of 0')
    width, height = _image_size(width, height, 'a distorted camera')
    wo, ho = _image_size(wo, ho, 'an undistorted camera')
    if not torch.cuda.is_available():
        raise RuntimeError('undistort_map: the COLMAP kernels run on the MI355X only (no CPU fallback)')
    out = torch.empty((ho, wo, 2), dtype=torch.int32, device=torch.device('cuda', torch.cuda.current_device()))
    _call('atvs_undistort_map', model_id, (ctypes.c_double * 12)(*(p + [0.0] * (12 - npar))), width, height,
          (ctypes.c_double * 4)(*k), wo, ho, _p(out), _stream())
    return out


def undistort_remap(image_u8, map):
    """image_u8 (H, W, 3) uint8, map (H', W', 2) int32 of undistort_map -> (H', W', 3) uint8 on the device: the integer bilinear
    gather of atvs_undistort_remap, black where the map holds INT32_MIN."""
    for t, name, dtype, last in ((image_u8, 'image_u8', torch.uint8, 3), (map, 'map', torch.int32, 2)):
        if not isinstance(t, torch.Tensor):
            raise TypeError('%s: expected a tensor, got %s' % (name, type(t).__name__))
        if t.dim() != 3 or int(t.shape[2]) != last:
            raise ValueError('%s: expected shape (rows, cols, %d), got %s' % (name, last, tuple(t.shape)))
    height, width = (int(v) for v in image_u8.shape[:2])
    ho, wo = (int(v) for v in map.shape[:2])
    _colmap_args((image_u8, 'image_u8', torch.uint8, (width, 3)), (map, 'map', torch.int32, (wo, 2)))
    _image_size(width, height, 'image_u8')
    _image_size(wo, ho, 'map')
    out = torch.empty((ho, wo, 3), dtype=torch.uint8, device=map.device)
    _call('atvs_undistort_remap', _p(image_u8), width, height, _p(map), wo, ho, _p(out), _stream())
    return out
