"""Test-side restatement of the undistortion (float64 numpy), written from its definition -- the forward models of COLMAP's
camera models, the Newton inverse, COLMAP's UndistortCamera, the 22.10 fixed-point map with its validity rule and the integer
bilinear sample -- not from the product's code.  Sums and products run left to right; r4 = r2 r2, r6 = r4 r2, r8 = r6 r2."""
import numpy as np

INT32_MIN = -2 ** 31
NPARAMS = {'SIMPLE_RADIAL': 4, 'RADIAL': 5, 'OPENCV': 8, 'FULL_OPENCV': 12, 'SIMPLE_RADIAL_FISHEYE': 4, 'RADIAL_FISHEYE': 5,
           'OPENCV_FISHEYE': 8, 'THIN_PRISM_FISHEYE': 12}
POLYNOMIAL = ('SIMPLE_RADIAL', 'RADIAL', 'OPENCV', 'FULL_OPENCV')
FISHEYE = ('SIMPLE_RADIAL_FISHEYE', 'RADIAL_FISHEYE', 'OPENCV_FISHEYE', 'THIN_PRISM_FISHEYE')
MODEL_IDS = {'SIMPLE_PINHOLE': 0, 'PINHOLE': 1, 'SIMPLE_RADIAL': 2, 'RADIAL': 3, 'OPENCV': 4, 'OPENCV_FISHEYE': 5, 'FULL_OPENCV': 6,
             'FOV': 7, 'SIMPLE_RADIAL_FISHEYE': 8, 'RADIAL_FISHEYE': 9, 'THIN_PRISM_FISHEYE': 10}


def intrinsics(model, p):
    """-> fx, fy, cx, cy, coefficients."""
    assert len(p) == NPARAMS[model]
    if NPARAMS[model] in (4, 5):
        return p[0], p[0], p[1], p[2], list(p[3:])
    return p[0], p[1], p[2], p[3], list(p[4:])


def forward(model, p, u, v):
    k = intrinsics(model, p)[4]
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    with np.errstate(all='ignore'):
        r2 = u * u + v * v
        if model in FISHEYE:
            r = np.sqrt(r2)
            theta = np.arctan(r)
            uu = np.where(r > 1e-8, u * theta / r, u)
            vv = np.where(r > 1e-8, v * theta / r, v)
            t2 = uu * uu + vv * vv
            t4 = t2 * t2
            t6 = t4 * t2
            t8 = t6 * t2
            if model == 'SIMPLE_RADIAL_FISHEYE':
                rad = k[0] * t2
            elif model == 'RADIAL_FISHEYE':
                rad = k[0] * t2 + k[1] * t4
            elif model == 'OPENCV_FISHEYE':
                rad = k[0] * t2 + k[1] * t4 + k[2] * t6 + k[3] * t8
            else:
                k1, k2, p1, p2, k3, k4, sx1, sy1 = k
                rad = k1 * t2 + k2 * t4 + k3 * t6 + k4 * t8
                ud = uu + uu * rad + 2 * p1 * uu * vv + p2 * (t2 + 2 * uu * uu) + sx1 * t2
                vd = vv + vv * rad + 2 * p2 * uu * vv + p1 * (t2 + 2 * vv * vv) + sy1 * t2
                return ud, vd
            return uu + uu * rad, vv + vv * rad
        r4 = r2 * r2
        r6 = r4 * r2
        if model == 'SIMPLE_RADIAL':
            rad = k[0] * r2
            return u + u * rad, v + v * rad
        if model == 'RADIAL':
            rad = k[0] * r2 + k[1] * r4
            return u + u * rad, v + v * rad
        if model == 'OPENCV':
            k1, k2, p1, p2 = k
            rad = k1 * r2 + k2 * r4
            return (u + u * rad + 2 * p1 * u * v + p2 * (r2 + 2 * u * u),
                    v + v * rad + 2 * p2 * u * v + p1 * (r2 + 2 * v * v))
        assert model == 'FULL_OPENCV'
        k1, k2, p1, p2, k3, k4, k5, k6 = k
        rad = (1 + k1 * r2 + k2 * r4 + k3 * r6) / (1 + k4 * r2 + k5 * r4 + k6 * r6)
        return (u * rad + 2 * p1 * u * v + p2 * (r2 + 2 * u * u),
                v * rad + 2 * p2 * u * v + p1 * (r2 + 2 * v * v))


def inverse(model, p, ud, vd):
    """Newton on `forward` from the target (fisheye: the target scaled by tan(rho) / rho), a forward-difference Jacobian of its own,
    until the residual is <= 1e-12 or 100 iterations; asserts convergence.  Pinned by its residual, not its path."""
    ud, vd = np.asarray(ud, np.float64).ravel(), np.asarray(vd, np.float64).ravel()
    x = np.stack([ud, vd])
    if model in FISHEYE:
        rho = np.sqrt((x * x).sum(0))
        x = x * np.where(rho > 1e-8, np.tan(rho) / np.where(rho > 1e-8, rho, 1.0), 1.0)
    for _ in range(100):
        f = np.stack(forward(model, p, x[0], x[1])) - np.stack([ud, vd])
        if np.abs(f).max() <= 1e-12:
            break
        h = 1e-7
        fa = np.stack(forward(model, p, x[0] + h, x[1])) - np.stack([ud, vd])
        fb = np.stack(forward(model, p, x[0], x[1] + h)) - np.stack([ud, vd])
        a, c = (fa - f) / h                                  # d/du of (f0, f1)
        b, d = (fb - f) / h                                  # d/dv
        det = a * d - b * c
        x = x - np.stack([d * f[0] - b * f[1], a * f[1] - c * f[0]]) / det
    f = np.stack(forward(model, p, x[0], x[1])) - np.stack([ud, vd])
    assert np.abs(f).max() <= 1e-12, 'the restatement\'s inverse did not converge'
    return x[0], x[1]


def output_camera(model, p, W, H, b=0.0, min_scale=0.2, max_scale=2.0, margin=1e-6):
    """UndistortCamera -> (fx, fy, cx', cy'), (W', H').  Asserts that scale W and scale H are more than `margin` from an integer
    (else truncation could differ between two correct implementations).  All-zero coefficients: the camera as it is."""
    fx, fy, cx, cy, k = intrinsics(model, p)
    if not any(k):
        return (fx, fy, cx, cy), (W, H)

    def to_pinhole(px, py):
        u, v = inverse(model, p, (np.asarray(px, np.float64) - cx) / fx, (np.asarray(py, np.float64) - cy) / fy)
        return fx * u + cx, fy * v + cy

    ys, xs = np.arange(H) + 0.5, np.arange(W) + 0.5
    left_x = to_pinhole(np.full(H, 0.5), ys)[0]
    right_x = to_pinhole(np.full(H, W - 0.5), ys)[0]
    top_y = to_pinhole(xs, np.full(W, 0.5))[1]
    bottom_y = to_pinhole(xs, np.full(W, H - 0.5))[1]
    min_sx = min(cx / (cx - left_x.min()), (W - 0.5 - cx) / (right_x.max() - cx))
    max_sx = max(cx / (cx - left_x.max()), (W - 0.5 - cx) / (right_x.min() - cx))
    min_sy = min(cy / (cy - top_y.min()), (H - 0.5 - cy) / (bottom_y.max() - cy))
    max_sy = max(cy / (cy - top_y.max()), (H - 0.5 - cy) / (bottom_y.min() - cy))
    sx = min(max(1.0 / (min_sx * b + max_sx * (1.0 - b)), min_scale), max_scale)
    sy = min(max(1.0 / (min_sy * b + max_sy * (1.0 - b)), min_scale), max_scale)
    for s, n in ((sx, W), (sy, H)):
        assert abs(s * n - round(s * n)) > margin, 'scale * size %r is within %g of an integer: choose other parameters' % (s * n, margin)
    Wo, Ho = int(max(1, sx * W)), int(max(1, sy * H))
    return (fx, fy, cx * Wo / W, cy * Ho / H), (Wo, Ho)


def sampling_map(model, p, W, H, camera):
    """-> q (H', W', 2) int32 and tie (H', W', 2) float64: the distance of s 1024 + 0.5 from the nearest integer per coordinate
    (inf where it is not finite)."""
    (fxo, fyo, cxo, cyo), (Wo, Ho) = camera
    fx, fy, cx, cy, _ = intrinsics(model, p)
    Y, X = np.meshgrid(np.arange(Ho, dtype=np.float64), np.arange(Wo, dtype=np.float64), indexing='ij')
    u = (X + 0.5 - cxo) / fxo
    v = (Y + 0.5 - cyo) / fyo
    ud, vd = forward(model, p, u, v)
    with np.errstate(all='ignore'):
        s = np.stack([fx * ud + cx - 0.5, fy * vd + cy - 0.5], -1)
        t = s * 1024 + 0.5
        qf = np.floor(t)
        tie = np.where(np.isfinite(t), np.abs(t - np.round(t)), np.inf)
        hi = np.array([(W - 1) * 1024, (H - 1) * 1024], np.float64)
        valid = (np.isfinite(s) & (qf >= 0) & (qf <= hi)).all(-1)
    q = np.where(valid[..., None], qf, 0.0).astype(np.int64)
    q[~valid] = (INT32_MIN, 0)
    return q.astype(np.int32), tie


def sample(src, q):
    """src (H, W, 3) uint8, q (H', W', 2) int32 of a VALID map -> (H', W', 3) uint8: the integer bilinear blend."""
    H, W = src.shape[:2]
    q = q.astype(np.int64)
    valid = q[..., 0] != INT32_MIN
    qx, qy = np.where(valid, q[..., 0], 0), np.where(valid, q[..., 1], 0)
    assert (qx >= 0).all() and (qx <= (W - 1) * 1024).all() and (qy >= 0).all() and (qy <= (H - 1) * 1024).all()
    ix, fx, iy, fy = qx >> 10, (qx & 1023)[..., None], qy >> 10, (qy & 1023)[..., None]
    ix1, iy1 = np.minimum(ix + 1, W - 1), np.minimum(iy + 1, H - 1)
    s = src.astype(np.int64)
    top = s[iy, ix] * (1024 - fx) + s[iy, ix1] * fx
    bot = s[iy1, ix] * (1024 - fx) + s[iy1, ix1] * fx
    out = (top * (1024 - fy) + bot * fy + 2 ** 19) >> 20
    out[~valid] = 0
    return out.astype(np.uint8)


def undistort(src, model, p, camera):
    return sample(src, sampling_map(model, p, src.shape[1], src.shape[0], camera)[0])


def write_cameras_binary(path, cameras):
    """cameras.bin for every model id ([(id, model, width, height, params)]); tests/colmap_model.write_binary knows five."""
    import struct
    with open(path, 'wb') as f:
        f.write(struct.pack('<Q', len(cameras)))
        for cid, model, w, h, params in cameras:
            f.write(struct.pack('<iiQQ', cid, MODEL_IDS[model], w, h) + struct.pack('<%dd' % len(params), *params))


def test_camera(model, W, H, strength=1.0):
    """A plausible camera of `model` for a W x H image: focal length 0.8 W, principal point off centre, barrel distortion of
    `strength` (1: about 6 % at the corner) with small higher-order, tangential and thin-prism terms -> its parameter tuple."""
    f, cx, cy = 0.8 * W, 0.5 * W + 0.37, 0.5 * H - 0.61
    k1, k2, k3, k4 = -0.12 * strength, 0.02 * strength, -0.003 * strength, 0.0004 * strength
    p1, p2 = 0.002 * strength, -0.0015 * strength
    return {'SIMPLE_RADIAL': (f, cx, cy, k1), 'RADIAL': (f, cx, cy, k1, k2),
            'OPENCV': (f, 1.01 * f, cx, cy, k1, k2, p1, p2),
            'FULL_OPENCV': (f, 1.01 * f, cx, cy, k1, k2, p1, p2, k3, 0.01 * strength, -0.002 * strength, 0.0003 * strength),
            'SIMPLE_RADIAL_FISHEYE': (f, cx, cy, k1), 'RADIAL_FISHEYE': (f, cx, cy, k1, k2),
            'OPENCV_FISHEYE': (f, 1.01 * f, cx, cy, k1, k2, k3, k4),
            'THIN_PRISM_FISHEYE': (f, 1.01 * f, cx, cy, k1, k2, p1, p2, k3, k4, 0.001 * strength, -0.0008 * strength)}[model]


test_camera.__test__ = False
