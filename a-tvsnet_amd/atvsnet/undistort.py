"""Undistortion of COLMAP's distorted camera models: what `colmap image_undistorter` does, restated.

    distort             the forward models (u, v) -> (u_d, v_d) in normalised coordinates, float64 numpy, in the operation order
                        csrc/undistort.hip follows
    undistort_points    their inverse by Newton's method (host only: at most 2 (W + H) border points per camera)
    undistorted_camera  COLMAP's UndistortCamera: the pinhole camera (same focal lengths) scaled so that, for blank_pixels = 0, no
                        pixel of the output lies outside the source, for 1 every source pixel is kept
    undistort_image     one image through its camera's sampling map on the GPU (ops.undistort_map, cached per camera, and
                        ops.undistort_remap): one upload, one launch, one download

No COLMAP run pins this: it is written from COLMAP's published definition, with one deliberate difference in the resampling (the
map is 22.10 fixed point and the bilinear blend is exact integer arithmetic; COLMAP blends in double and rejects the last row and
column).  FOV, max_image_size and the ROI options are not built.
"""
import collections

import numpy as np

# parameters per model: COLMAP's order (src/colmap/sensor/models.h)
PARAM_COUNT = {'SIMPLE_PINHOLE': 3, 'PINHOLE': 4, 'SIMPLE_RADIAL': 4, 'RADIAL': 5, 'OPENCV': 8, 'OPENCV_FISHEYE': 8, 'FULL_OPENCV': 12,
               'SIMPLE_RADIAL_FISHEYE': 4, 'RADIAL_FISHEYE': 5, 'THIN_PRISM_FISHEYE': 12}
ONE_FOCAL = ('SIMPLE_PINHOLE', 'SIMPLE_RADIAL', 'RADIAL', 'SIMPLE_RADIAL_FISHEYE', 'RADIAL_FISHEYE')
FISHEYE = ('OPENCV_FISHEYE', 'SIMPLE_RADIAL_FISHEYE', 'RADIAL_FISHEYE', 'THIN_PRISM_FISHEYE')
PINHOLE = ('SIMPLE_PINHOLE', 'PINHOLE')


def split_params(model, params):
    """-> (fx, fy, cx, cy), [distortion coefficients] of a model's parameter tuple."""
    if model not in PARAM_COUNT:
        raise ValueError('the %s model is not undistorted (known: %s)' % (model, ', '.join(sorted(PARAM_COUNT))))
    p = [float(v) for v in params]
    if len(p) != PARAM_COUNT[model]:
        raise ValueError('%s takes %d parameters, got %d' % (model, PARAM_COUNT[model], len(p)))
    if model in ONE_FOCAL:
        return (p[0], p[0], p[1], p[2]), p[3:]
    return tuple(p[:4]), p[4:]


def distort(model, params, u, v):
    """Normalised ray coordinates (u, v) -> distorted (u_d, v_d), float64 arrays of one shape.  Products and sums run left to
    right; r4 = r2 r2, r6 = r4 r2, r8 = r6 r2."""
    _, c = split_params(model, params)
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    if model in PINHOLE:
        return u.copy(), v.copy()
    r2 = u * u + v * v
    if model in FISHEYE:
        r = np.sqrt(r2)
        theta = np.arctan(r)
        off_axis = r > 1e-8
        with np.errstate(divide='ignore', invalid='ignore'):
            uu = np.where(off_axis, u * theta / r, u)
            vv = np.where(off_axis, v * theta / r, v)
        t2 = uu * uu + vv * vv
        t4 = t2 * t2
        t6 = t4 * t2
        t8 = t6 * t2
        if model == 'SIMPLE_RADIAL_FISHEYE':
            rad = c[0] * t2
        elif model == 'RADIAL_FISHEYE':
            rad = c[0] * t2 + c[1] * t4
        elif model == 'OPENCV_FISHEYE':
            rad = c[0] * t2 + c[1] * t4 + c[2] * t6 + c[3] * t8
        else:
            k1, k2, p1, p2, k3, k4, sx1, sy1 = c
            rad = k1 * t2 + k2 * t4 + k3 * t6 + k4 * t8
            return (uu + uu * rad + 2.0 * p1 * uu * vv + p2 * (t2 + 2.0 * uu * uu) + sx1 * t2,
                    vv + vv * rad + 2.0 * p2 * uu * vv + p1 * (t2 + 2.0 * vv * vv) + sy1 * t2)
        return uu + uu * rad, vv + vv * rad
    r4 = r2 * r2
    if model == 'SIMPLE_RADIAL':
        rad = c[0] * r2
    elif model == 'RADIAL':
        rad = c[0] * r2 + c[1] * r4
    elif model == 'OPENCV':
        k1, k2, p1, p2 = c
        rad = k1 * r2 + k2 * r4
        return (u + u * rad + 2.0 * p1 * u * v + p2 * (r2 + 2.0 * u * u),
                v + v * rad + 2.0 * p2 * u * v + p1 * (r2 + 2.0 * v * v))
    else:                                                    # FULL_OPENCV
        k1, k2, p1, p2, k3, k4, k5, k6 = c
        r6 = r4 * r2
        with np.errstate(divide='ignore', invalid='ignore'):
            rad = (1.0 + k1 * r2 + k2 * r4 + k3 * r6) / (1.0 + k4 * r2 + k5 * r4 + k6 * r6)
            return (u * rad + 2.0 * p1 * u * v + p2 * (r2 + 2.0 * u * u),
                    v * rad + 2.0 * p2 * u * v + p1 * (r2 + 2.0 * v * v))
    return u + u * rad, v + v * rad


def undistort_points(model, params, u_d, v_d, camera='the camera', tol=1e-12, max_iterations=100):
    """The inverse of distort: (u, v) with distort(u, v) = (u_d, v_d).  Newton's method on the forward model, its Jacobian by
    central differences, started at the target (the fisheye models: at the target scaled by tan(rho) / rho, rho its norm), until
    the forward residual max(|du|, |dv|) is <= tol in normalised units.  ValueError naming `camera` when a point has not
    converged after max_iterations: a fisheye that reaches past what a pinhole camera can hold."""
    u_d, v_d = np.asarray(u_d, np.float64), np.asarray(v_d, np.float64)
    shape = u_d.shape
    tu, tv = u_d.reshape(-1).copy(), v_d.reshape(-1).copy()
    u, v = tu.copy(), tv.copy()
    if model in FISHEYE:
        rho = np.sqrt(tu * tu + tv * tv)
        with np.errstate(divide='ignore', invalid='ignore'):
            s = np.where(rho > 1e-8, np.tan(rho) / rho, 1.0)
        u, v = u * s, v * s
    todo = np.arange(len(u))
    with np.errstate(all='ignore'):
        for it in range(max_iterations + 1):
            fu, fv = distort(model, params, u[todo], v[todo])
            ru, rv = fu - tu[todo], fv - tv[todo]
            bad = ~(np.maximum(np.abs(ru), np.abs(rv)) <= tol)             # NaN stays bad
            todo, ru, rv = todo[bad], ru[bad], rv[bad]
            if len(todo) == 0 or it == max_iterations:
                break
            x, y = u[todo], v[todo]
            hx, hy = 1e-6 * np.maximum(np.abs(x), 1.0), 1e-6 * np.maximum(np.abs(y), 1.0)
            ax, bx = distort(model, params, x + hx, y), distort(model, params, x - hx, y)
            ay, by = distort(model, params, x, y + hy), distort(model, params, x, y - hy)
            j00, j10 = (ax[0] - bx[0]) / (2.0 * hx), (ax[1] - bx[1]) / (2.0 * hx)
            j01, j11 = (ay[0] - by[0]) / (2.0 * hy), (ay[1] - by[1]) / (2.0 * hy)
            det = j00 * j11 - j01 * j10
            u[todo] = x - (j11 * ru - j01 * rv) / det
            v[todo] = y - (j00 * rv - j10 * ru) / det
    if len(todo):
        k = int(todo[0])
        raise ValueError('%s (%s): Newton\'s inverse of the distortion did not converge for %d of %d points, e.g. the distorted '
                         'ray (%.6g, %.6g): the lens reaches past what a pinhole camera can hold' %
                         (camera, model, len(todo), len(u), tu[k], tv[k]))
    return u.reshape(shape), v.reshape(shape)


def undistorted_camera(model, params, width, height, blank_pixels=0.0, min_scale=0.2, max_scale=2.0, camera='the camera'):
    """COLMAP's UndistortCamera without max_image_size and ROI -> (fx, fy, cx', cy'), (W', H') of the pinhole camera the images
    are resampled into: the source's focal lengths, its size scaled per axis by 1 / (min_scale b + max_scale (1 - b)) with b =
    blank_pixels and the two scales those at which the undistorted border just fills, respectively just fits, the frame."""
    (fx, fy, cx, cy), coef = split_params(model, params)
    W, H = int(width), int(height)
    if W < 1 or H < 1:
        raise ValueError('%s: a size of %d x %d' % (camera, W, H))
    if not 0.0 <= blank_pixels <= 1.0 or not 0.0 < min_scale <= max_scale:
        raise ValueError('blank_pixels must lie in [0, 1] and 0 < min_scale <= max_scale, got %r, %r, %r' %
                         (blank_pixels, min_scale, max_scale))
    # no distortion: the camera as it is.  (The border rule alone would not say so: the left and top border sit at 0.5, which
    # enters c / (c - lo) but not (n - 0.5 - c) / (hi - c), and would shave a pixel.)
    if model in PINHOLE or not any(coef):
        return (fx, fy, cx, cy), (W, H)

    def pinhole_of(px, py):                                  # distorted pixel coordinates -> the pinhole's pixel coordinates
        u, v = undistort_points(model, params, (px - cx) / fx, (py - cy) / fy, camera)
        return fx * u + cx, fy * v + cy

    ys, xs = np.arange(H, dtype=np.float64) + 0.5, np.arange(W, dtype=np.float64) + 0.5
    left = pinhole_of(np.full(H, 0.5), ys)[0]
    right = pinhole_of(np.full(H, W - 0.5), ys)[0]
    top = pinhole_of(xs, np.full(W, 0.5))[1]
    bottom = pinhole_of(xs, np.full(W, H - 0.5))[1]

    def scale(lo, hi, c, n):
        s_min = min(c / (c - lo.min()), (n - 0.5 - c) / (hi.max() - c))
        s_max = max(c / (c - lo.max()), (n - 0.5 - c) / (hi.min() - c))
        s = 1.0 / (s_min * blank_pixels + s_max * (1.0 - blank_pixels))
        if not np.isfinite(s):
            raise ValueError('%s (%s): the undistorted border gives no finite scale' % (camera, model))
        return float(min(max(s, min_scale), max_scale))

    Wo = int(max(1, scale(left, right, cx, W) * W))
    Ho = int(max(1, scale(top, bottom, cy, H) * H))
    return (fx, fy, cx * Wo / W, cy * Ho / H), (Wo, Ho)


class MapCache(object):
    """The sampling maps of the last `capacity` cameras on the device (a 24-megapixel map is 190 MB), least recently used out."""

    def __init__(self, capacity=2):
        self.capacity, self.maps = int(capacity), collections.OrderedDict()

    def get(self, model, params, width, height, camera):
        import torch
        from .. import ops
        (fx, fy, cx, cy), (wo, ho) = camera
        key = (model, tuple(float(v) for v in params), int(width), int(height), (float(fx), float(fy), float(cx), float(cy)),
               (int(wo), int(ho)), torch.cuda.current_device())
        m = self.maps.pop(key, None)
        if m is None:
            m = ops.undistort_map(model, params, width, height, camera)
        self.maps[key] = m
        while len(self.maps) > self.capacity:
            self.maps.popitem(last=False)
        return m


_maps = MapCache()


def undistort_image(image, model, params, width, height, camera=None, cache=None):
    """image (height, width, 3) uint8 numpy, as decoded -> (H', W', 3) uint8 numpy of `camera` (default: undistorted_camera's).
    ValueError when the image's size is not its camera's.  One upload, one launch (two for a camera's first image), one download."""
    import torch
    from .. import ops
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError('image: expected (rows, cols, 3) uint8, got %s %s' % (image.shape, image.dtype))
    if image.shape[:2] != (int(height), int(width)):
        raise ValueError('the image is %d x %d pixels, its %s camera %d x %d' % (image.shape[1], image.shape[0], model, width, height))
    if camera is None:
        camera = undistorted_camera(model, params, width, height)
    m = (_maps if cache is None else cache).get(model, params, width, height, camera)
    src = torch.from_numpy(np.ascontiguousarray(image)).to(m.device)
    return ops.undistort_remap(src, m).cpu().numpy()
