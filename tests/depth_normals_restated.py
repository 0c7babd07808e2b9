"""TEST INFRASTRUCTURE: numpy float64 restatement of atvs_depth_normals_f32 (csrc/depth_normals.hip), and the
scenes the depth-normal tests share.

Per pixel (x, y) of camera c with depth d (float32 inputs, every operation in float64):
    d > 0 false -> (0,0,0)
    X(x, y, d) = M_inv (d x - p0, d y - p1, d - p2)
    neighbours R = (x+step, y), D = (x, y+step), L = (x-step, y), U = (x, y-step), valid when inside the image, dn > 0 and
    |dn - d| <= float64(float32(depth_gate)) * d
    quadrants (R,D), (D,L), (L,U), (U,R) in this order: both valid -> c = (Xa - X) x (Xb - X); |c| > 0 -> sum += c / |c|
    |sum| = 0 -> (0,0,0); else n = sum / |sum|, negated when n . (C - X) < 0; float32(n) per component.
"""
import numpy as np

import fusion_scene


def _back_project(cam, xs, ys, d):
    Mi, pc = cam[12:21], cam[24:27]
    ptx, pty, ptz = d * xs - pc[0], d * ys - pc[1], d - pc[2]
    return np.stack([Mi[0] * ptx + Mi[1] * pty + Mi[2] * ptz,
                     Mi[3] * ptx + Mi[4] * pty + Mi[5] * ptz,
                     Mi[6] * ptx + Mi[7] * pty + Mi[8] * ptz], -1)


def _shift(a, dx, dy):
    """a[y + dy, x + dx] where that pixel exists (-> the values, the mask of pixels that have one)."""
    rows, cols = a.shape[:2]
    ys, xs = np.meshgrid(np.arange(rows), np.arange(cols), indexing='ij')
    inside = (xs + dx >= 0) & (xs + dx < cols) & (ys + dy >= 0) & (ys + dy < rows)
    return a[np.clip(ys + dy, 0, rows - 1), np.clip(xs + dx, 0, cols - 1)], inside


def depth_normals(cams, depths, step=1, depth_gate=0.02):
    """cams (N,28) float32, depths (N,rows,cols) float32 -> (N,rows,cols,3) float32."""
    cams, depths = np.asarray(cams, np.float32), np.asarray(depths, np.float32)
    gate = np.float64(np.float32(depth_gate))
    N, rows, cols = depths.shape
    out = np.zeros((N, rows, cols, 3), np.float32)
    ys, xs = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing='ij')
    with np.errstate(all='ignore'):
        for v in range(N):
            cam, d = cams[v].astype(np.float64), depths[v].astype(np.float64)
            X = _back_project(cam, xs, ys, d)
            edges, valid = [], []
            for dx, dy in ((step, 0), (0, step), (-step, 0), (0, -step)):            # R, D, L, U
                dn, inside = _shift(d, dx, dy)
                ok = inside & (dn > 0) & (np.abs(dn - d) <= gate * d)
                edges.append(_back_project(cam, xs + dx, ys + dy, dn) - X)
                valid.append(ok)
            total = np.zeros((rows, cols, 3))
            for k in range(4):                                                       # (R,D), (D,L), (L,U), (U,R)
                k2 = (k + 1) % 4
                c = np.cross(edges[k], edges[k2])
                length = np.sqrt((c * c).sum(-1))
                use = valid[k] & valid[k2] & (length > 0)
                total = total + np.where(use[..., None], c / length[..., None], 0.0)
            length = np.sqrt((total * total).sum(-1))
            n = np.where((length > 0)[..., None], total / length[..., None], 0.0)
            flip = (n * (cam[21:24] - X)).sum(-1) < 0
            n = np.where(flip[..., None], -n, n)
            n = np.where((d > 0)[..., None], n, 0.0)
            out[v] = n.astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------------------- shared scenes

PATCH = (slice(16, 32), slice(24, 40))             # rows 16..31, cols 24..39 of view 1
_SCENES = {}


def plane_scene():
    """fusion_scene.make_scene(4, 48, 64), made once: (Ps, depths, normals, images, n, d0).  Shared: do not write into it."""
    if 'plane' not in _SCENES:
        _SCENES['plane'] = fusion_scene.make_scene(4, 48, 64)
        for a in _SCENES['plane'][:4]:
            a.setflags(write=False)
    return _SCENES['plane']


def sawtooth_depths():
    """The plane scene's depths with the patch of view 1 replaced by 45 degree sawtooth facets, depth + ((x % 4) - 1.5) * 5 / 60:
    up to 2.9 % of disparity change, so a disparity threshold of 0.05 cannot see it and one of 0.01 sees half of it."""
    if 'saw' not in _SCENES:
        depths = plane_scene()[1].copy()
        x = np.arange(24, 40, dtype=np.float64)
        depths[1][PATCH] = (depths[1][PATCH].astype(np.float64) + ((x % 4) - 1.5)[None, :] * 5.0 / 60.0).astype(np.float32)
        depths.setflags(write=False)
        _SCENES['saw'] = depths
    return _SCENES['saw']


def planted_depths(n, rows, cols, seed=0):
    """Smooth positive depth maps of any size with a zero-depth block, isolated holes, a depth step far across every gate the
    tests use and one pixel whose four neighbours are all cut.  The smooth part varies by < 0.2 % between neighbours at step 1
    and 2 and the planted step is 30 %, so no gate comparison at 0.02 or 0.05 is near an equality."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing='ij')
    maps = []
    for v in range(n):
        d = 5.0 + 0.004 * xs - 0.003 * ys + 0.02 * np.sin(0.3 * xs + v) * np.cos(0.2 * ys)
        d = d * (1.0 + 1e-4 * rng.normal(size=d.shape))
        if rows >= 12 and cols >= 12:
            d[rows // 2:, cols // 2:] *= 1.3                        # a depth step across the gate
            d[2:5, 5:9] = 0.0                                       # a zero-depth block
            d[rows - 3, 1] = 0.0                                    # an isolated hole
            y0, x0 = rows // 4 + 3, cols // 4 + 3                   # a pixel alone at its depth: no valid neighbour at any step
            d[y0, x0] *= 1.5
        else:
            d[1, 2] = 0.0
            d[rows - 2, cols - 2] *= 1.5
        maps.append(d.astype(np.float32))
    return np.stack(maps)


def cameras(n, rows, cols):
    """n full 3x4 projection matrices (fusion_scene's rig) for maps of rows x cols."""
    return fusion_scene.make_scene(n, rows, cols)[0]
