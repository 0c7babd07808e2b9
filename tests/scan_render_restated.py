"""The definition of atvs_scan_render (include/atvsnet_hip.h) restated in numpy, and once more as a literal Python loop.

scan_render: float64 in the stated order, np.minimum.at on uint32 bit patterns, one camera at a time.  scan_render_loop: the same
words one (camera, point) pair at a time with Python floats (IEEE doubles, nothing contracted) -- slow, for tiny cases: it is what
the vectorised form is checked against."""
import math

import numpy as np

EMPTY = np.uint32(0xFFFFFFFF)


def project(points, cam, pixel_centre):
    """-> (c2, xs, ys) float64 (n,) of one camera's 16 doubles."""
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    c = np.asarray(cam, np.float64).reshape(16)
    X, Y, Z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all='ignore'):
        c0 = ((c[0] * X + c[1] * Y) + c[2] * Z) + c[9]
        c1 = ((c[3] * X + c[4] * Y) + c[5] * Z) + c[10]
        c2 = ((c[6] * X + c[7] * Y) + c[8] * Z) + c[11]
        x = (c0 / c2) * c[12] + c[14]
        y = (c1 / c2) * c[13] + c[15]
        xs = (x - float(pixel_centre)) + 0.5
        ys = (y - float(pixel_centre)) + 0.5
    return c2, xs, ys


def planes(points, cam, rows, cols, pixel_centre=0.0, splat=0):
    """-> (near, front) uint32 (rows, cols) of one camera."""
    c2, xs, ys = project(points, cam, pixel_centre)
    near = np.full((rows, cols), EMPTY, np.uint32)
    front = np.full((rows, cols), EMPTY, np.uint32)
    with np.errstate(all='ignore'):
        z = c2.astype(np.float32)
        ok = (c2 > 0.0) & np.isfinite(z) & (z > 0)
        ok &= (xs >= -float(splat)) & (xs < float(cols) + float(splat)) & (ys >= -float(splat)) & (ys < float(rows) + float(splat))
    u = np.floor(xs[ok]).astype(np.int64)
    v = np.floor(ys[ok]).astype(np.int64)
    bits = z[ok].view(np.uint32)
    inside = (u >= 0) & (u < cols) & (v >= 0) & (v < rows)
    np.minimum.at(near, (v[inside], u[inside]), bits[inside])
    for dv in range(-splat, splat + 1):
        for du in range(-splat, splat + 1):
            uu, vv = u + du, v + dv
            inside = (uu >= 0) & (uu < cols) & (vv >= 0) & (vv < rows)
            np.minimum.at(front, (vv[inside], uu[inside]), bits[inside])
    return near, front


def resolve(near, front, occlusion_tol=0.0):
    z = near.view(np.float32)
    zf = front.view(np.float32)
    with np.errstate(all='ignore'):          # all-ones is a NaN pattern: masked below
        keep = (near != EMPTY) & (z.astype(np.float64) <= zf.astype(np.float64) * (1.0 + float(occlusion_tol)))
    return np.where(keep, z, np.float32(0)).astype(np.float32)


def scan_render(points, cams, rows, cols, pixel_centre=0.0, splat=0, occlusion_tol=0.0):
    """-> (n_cams, rows, cols) float32."""
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    out = np.zeros((len(cams), rows, cols), np.float32)
    for k, cam in enumerate(cams):
        near, front = planes(points, cam, rows, cols, pixel_centre, splat)
        out[k] = resolve(near, front, occlusion_tol)
    return out


def _div(a, b):
    """IEEE float64 division of Python floats (Python raises where IEEE gives inf / NaN)."""
    return float(np.float64(a) / np.float64(b))


def scan_render_loop(points, cams, rows, cols, pixel_centre=0.0, splat=0, occlusion_tol=0.0):
    """The definition one pair at a time."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    out = np.zeros((len(cams), rows, cols), np.float32)
    pc = float(pixel_centre)
    for k in range(len(cams)):
        c = [float(v) for v in cams[k]]
        near = [[0xFFFFFFFF] * cols for _ in range(rows)]
        front = [[0xFFFFFFFF] * cols for _ in range(rows)]
        for p in pts:
            X, Y, Z = float(p[0]), float(p[1]), float(p[2])
            with np.errstate(all='ignore'):
                c0 = ((c[0] * X + c[1] * Y) + c[2] * Z) + c[9]
                c1 = ((c[3] * X + c[4] * Y) + c[5] * Z) + c[10]
                c2 = ((c[6] * X + c[7] * Y) + c[8] * Z) + c[11]
                if not c2 > 0.0:
                    continue
                z = np.float32(c2)
                if not (np.isfinite(z) and z > 0):
                    continue
                x = _div(c0, c2) * c[12] + c[14]
                y = _div(c1, c2) * c[13] + c[15]
            xs = (x - pc) + 0.5
            ys = (y - pc) + 0.5
            if not (xs >= -splat and xs < cols + splat and ys >= -splat and ys < rows + splat):
                continue
            u, v = int(math.floor(xs)), int(math.floor(ys))
            bits = int(np.array([z], np.float32).view(np.uint32)[0])
            if 0 <= u < cols and 0 <= v < rows:
                near[v][u] = min(near[v][u], bits)
            for dv in range(-splat, splat + 1):
                for du in range(-splat, splat + 1):
                    if 0 <= u + du < cols and 0 <= v + dv < rows:
                        front[v + dv][u + du] = min(front[v + dv][u + du], bits)
        for v in range(rows):
            for u in range(cols):
                if near[v][u] == 0xFFFFFFFF:
                    continue
                z = np.array([near[v][u]], np.uint32).view(np.float32)[0]
                zf = np.array([front[v][u]], np.uint32).view(np.float32)[0]
                if float(z) <= float(zf) * (1.0 + float(occlusion_tol)):
                    out[k, v, u] = z
    return out


def ring_cameras(n_cams, rows, cols, radius=3.0, focal=None, height=0.3):
    """n_cams cameras on a circle of `radius` around the origin, looking at it -> (n_cams,16) float64 rows."""
    focal = 0.9 * cols if focal is None else float(focal)
    out = np.zeros((n_cams, 16), np.float64)
    for k in range(n_cams):
        a = 2.0 * np.pi * k / n_cams + 0.1
        C = np.array([radius * np.cos(a), height * np.sin(3 * a), radius * np.sin(a)])
        fwd = -C / np.linalg.norm(C)
        right = np.cross(np.array([0.0, 1.0, 0.0]), fwd)
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        R = np.stack([right, down, fwd])
        out[k, :9] = R.reshape(-1)
        out[k, 9:12] = -R @ C
        out[k, 12:] = (focal, focal * 1.03, cols / 2.0 - 0.25, rows / 2.0 + 0.4)
    return out
