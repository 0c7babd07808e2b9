"""Free-space carving (include/atvsnet_hip.h) restated in numpy on the DENSE grid, independent of the
kernels' blocks and view masks: `integrate` visits every voxel of the box for every view and keeps a free count beside the sums of
tests/tsdf_restated.py; `free_views` restates the rule of atvs_tsdf_free_views as tests/tsdf_cases.marked_blocks restates marking;
`exact_views` is what that rule must be a superset of: the (block, view) pairs with a band or free contribution, from the dense grid.
With them the scenes the carving tests share: the floater (a blob two views agree on, in front of the sphere), the exact band edge,
the narrow field."""
import functools

import numpy as np

import tsdf_restated as R
from scan_render_restated import ring_cameras

RADIUS, VOXEL, TRUNC = 0.9, 0.05, 0.2                    # the constants of tests/test_gpu_tsdf.py
ORIGIN = (-1.237, -1.181, -1.213)
DIMS = (6, 6, 6)


def _project(c, X, Y, Z, pixel_centre):
    """scan_project's operations in its order -> (c2, xs, ys)."""
    with np.errstate(all='ignore'):
        c2 = ((c[6] * X + c[7] * Y) + c[8] * Z) + c[11]
        c0 = ((c[0] * X + c[1] * Y) + c[2] * Z) + c[9]
        c1 = ((c[3] * X + c[4] * Y) + c[5] * Z) + c[10]
        x = (c0 / c2) * c[12] + c[14]
        y = (c1 / c2) * c[13] + c[15]
        xs = (x - float(pixel_centre)) + 0.5
        ys = (y - float(pixel_centre)) + 0.5
    return c2, xs, ys


def _views(depths, cams, voxel, trunc, origin, dims, pixel_centre):
    """Per view, over the dense grid: (band, free (nz,ny,nx) bool, sdf float64, v, u the pixel)."""
    depths = np.asarray(depths, np.float32)
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    n, rows, cols = depths.shape
    bx, by, bz = dims
    Z, Y, X = np.meshgrid(R.centres(origin, voxel, bz * 8, 2), R.centres(origin, voxel, by * 8, 1), R.centres(origin, voxel, bx * 8, 0),
                          indexing='ij')
    trunc = float(trunc)
    for k in range(n):
        c2, xs, ys = _project(cams[k], X, Y, Z, pixel_centre)
        with np.errstate(all='ignore'):
            z = c2.astype(np.float32)
            ok = (c2 > 0.0) & np.isfinite(z) & (z > 0) & (xs >= 0.0) & (xs < float(cols)) & (ys >= 0.0) & (ys < float(rows))
        u = np.where(ok, np.floor(np.where(ok, xs, 0.0)), 0).astype(np.int64)
        v = np.where(ok, np.floor(np.where(ok, ys, 0.0)), 0).astype(np.int64)
        d = depths[k][v, u]
        with np.errstate(all='ignore'):
            sdf = d.astype(np.float64) - c2
            ok &= (d > 0) & np.isfinite(d)
            band = ok & (sdf >= -trunc) & (sdf <= trunc)
            free = ok & (sdf > trunc)
        yield k, band, free, sdf, v, u


def integrate(depths, cams, voxel, trunc, origin, dims, images=None, pixel_centre=0.0, carve_weight=1.0):
    """tests/tsdf_restated.integrate with carving -> its dict plus free (nz,ny,nx) float32."""
    bx, by, bz = dims
    shape = (bz * 8, by * 8, bx * 8)
    S, W, Wf = np.zeros(shape, np.float64), np.zeros(shape, np.float64), np.zeros(shape, np.float64)
    C = np.zeros(shape + (3,), np.float64)
    for k, band, free, sdf, v, u in _views(depths, cams, voxel, trunc, origin, dims, pixel_centre):
        S[band] += sdf[band] / float(trunc)
        W[band] += 1.0
        Wf[free] += 1.0
        if images is not None:
            C[band] += np.asarray(images[k], np.float32)[v[band], u[band], :3].astype(np.float64)
    has = W > 0
    f = float(carve_weight) * Wf                          # formed once
    with np.errstate(all='ignore'):
        tsdf = np.where(has, (S + f) / (W + f), 0.0).astype(np.float32)
        color = None if images is None else np.where(has[..., None], C / W[..., None], 0.0).astype(np.float32)
    occupied = has.reshape(bz, 8, by, 8, bx, 8).any(axis=(1, 3, 5))
    zz, yy, xx = np.nonzero(occupied)
    return dict(tsdf=tsdf, weight=W.astype(np.float32), color=color, free=np.where(has, Wf, 0.0).astype(np.float32),
                blocks=np.stack([xx, yy, zz], axis=1).astype(np.int32).reshape(-1, 3))


def all_blocks(dims):
    """(bx by bz,3) int32: every block of the box, ascending in the linear index."""
    bx, by, bz = dims
    z, y, x = np.meshgrid(np.arange(bz), np.arange(by), np.arange(bx), indexing='ij')
    return np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(np.int32)


def free_views(blocks, cams, rows, cols, voxel, origin, pixel_centre=0.0, padding=1.0):
    """The rule of atvs_tsdf_free_views -> (count, ceil(n/64)) uint64.  padding=0: the rule without its pixel of padding."""
    blocks = np.asarray(blocks, np.int64).reshape(-1, 3)
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    n = len(cams)
    masks = np.zeros((len(blocks), (n + 63) // 64), np.uint64)
    corner = []
    for k in range(8):
        delta = np.array([k & 1, (k >> 1) & 1, k >> 2])
        corner.append([float(origin[a]) + (8 * (blocks[:, a] + delta[a])).astype(np.float64) * float(voxel) for a in range(3)])
    for view, c in enumerate(cams):
        pos = np.zeros(len(blocks), np.int64)
        nan = np.zeros(len(blocks), bool)
        lox, loy = np.full(len(blocks), np.inf), np.full(len(blocks), np.inf)
        hix, hiy = np.full(len(blocks), -np.inf), np.full(len(blocks), -np.inf)
        for X, Y, Z in corner:
            c2, xs, ys = _project(c, X, Y, Z, pixel_centre)
            with np.errstate(invalid='ignore'):
                front = c2 > 0.0
            pos += front
            nan |= front & (np.isnan(xs) | np.isnan(ys))
            use = front & ~np.isnan(xs) & ~np.isnan(ys)
            lox, hix = np.where(use, np.minimum(lox, xs), lox), np.where(use, np.maximum(hix, xs), hix)
            loy, hiy = np.where(use, np.minimum(loy, ys), loy), np.where(use, np.maximum(hiy, ys), hiy)
        inside = (hix >= -padding) & (lox < float(cols) + padding) & (hiy >= -padding) & (loy < float(rows) + padding)
        bit = np.where((pos == 8) & ~nan, inside, pos > 0)
        masks[bit, view >> 6] |= np.uint64(1) << np.uint64(view & 63)
    return masks


def exact_views(depths, cams, voxel, trunc, origin, dims, pixel_centre=0.0):
    """(bx by bz, ceil(n/64)) uint64 over all_blocks(dims): bit v where a voxel of the block has a band or a free contribution from
    view v, found on the dense grid."""
    bx, by, bz = dims
    n = len(depths)
    masks = np.zeros((bx * by * bz, (n + 63) // 64), np.uint64)
    for k, band, free, _, _, _ in _views(depths, cams, voxel, trunc, origin, dims, pixel_centre):
        hit = (band | free).reshape(bz, 8, by, 8, bx, 8).any(axis=(1, 3, 5)).reshape(-1)
        masks[hit, k >> 6] |= np.uint64(1) << np.uint64(k & 63)
    return masks


def bits_set(masks):
    return int(sum(bin(int(w)).count('1') for w in np.asarray(masks).reshape(-1)))


def largest_component_faces(faces, num_vertices):
    """The face count of the largest connected component (faces joined by a shared vertex) and the number of components."""
    parent = np.arange(num_vertices)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b, c in np.asarray(faces).tolist():
        ra, rb, rc = find(a), find(b), find(c)
        parent[rb] = ra
        parent[find(rc)] = ra
    roots = np.array([find(a) for a in np.asarray(faces)[:, 0].tolist()])
    _, counts = np.unique(roots, return_counts=True)
    return int(counts.max()), int(len(counts))


# ----------------------------------------------------------------------------------------------------------------------------------
# the scenes
# ----------------------------------------------------------------------------------------------------------------------------------
class Scene(object):
    """Inputs of an integration; `.want(cw)` is the dense restatement with carving, `.plain` the one without, each once."""
    def __init__(self, depths, cams, images, trunc=TRUNC, origin=ORIGIN, dims=DIMS, pixel_centre=0.0, voxel=VOXEL):
        self.depths = np.ascontiguousarray(depths, np.float32)
        self.cams = np.ascontiguousarray(cams, np.float64)
        self.images = None if images is None else np.ascontiguousarray(images, np.float32)
        self.trunc, self.origin, self.dims, self.pixel_centre, self.voxel = trunc, origin, dims, pixel_centre, voxel
        self._want, self._plain = {}, None

    @classmethod
    def of(cls, case):
        """A tests/tsdf_cases.Integration as a Scene."""
        return cls(case.depths, case.cams, case.images, case.trunc, case.origin, case.dims, case.pixel_centre, case.voxel)

    def args(self):
        return self.voxel, self.trunc, self.origin, self.dims

    def want(self, cw=1.0):
        if cw not in self._want:
            self._want[cw] = integrate(self.depths, self.cams, *self.args(), images=self.images, pixel_centre=self.pixel_centre,
                                       carve_weight=cw)
        return self._want[cw]

    @property
    def plain(self):
        if self._plain is None:
            self._plain = R.integrate(self.depths, self.cams, *self.args(), images=self.images, pixel_centre=self.pixel_centre)
        return self._plain

    def mesh(self, cw=None, min_weight=1.0):
        w = self.plain if cw is None else self.want(cw)
        return R.mesh(w['tsdf'], w['weight'], w['color'], self.origin, self.voxel, min_weight)

    def exact(self):
        return exact_views(self.depths, self.cams, *self.args(), pixel_centre=self.pixel_centre)

    def rule(self, padding=1.0):
        return free_views(all_blocks(self.dims), self.cams, self.depths.shape[1], self.depths.shape[2], self.voxel, self.origin,
                          self.pixel_centre, padding)


@functools.lru_cache(maxsize=None)
def ring(n=9, rows=37, cols=53):
    """The clean sphere of tests/test_gpu_tsdf.py in n ring cameras."""
    cams = ring_cameras(n, rows, cols)
    depths, images = R.sphere_depths(cams, rows, cols, RADIUS)
    return Scene(depths, cams, images)


def ball_depths(cams, rows, cols, centre, radius, pixel_centre=0.0):
    """Analytic z-depth maps of a ball at `centre` (tests/tsdf_restated.sphere_depths, off the origin) -> (n,rows,cols) float32, 0
    where the ray misses."""
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    out = np.zeros((len(cams), rows, cols), np.float32)
    v, u = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing='ij')
    for k, c in enumerate(cams):
        Rm, t = c[:9].reshape(3, 3), c[9:12]
        eye = -Rm.T @ t - np.asarray(centre, np.float64)
        ray = np.stack([(u + pixel_centre - c[14]) / c[12], (v + pixel_centre - c[15]) / c[13], np.ones_like(u)], axis=-1)
        dirs = ray @ Rm
        A, B, Cc = (dirs * dirs).sum(-1), 2.0 * (dirs @ eye), eye @ eye - radius * radius
        disc = B * B - 4.0 * A * Cc
        hit = disc > 0
        s = np.where(hit, (-B - np.sqrt(np.where(hit, disc, 0.0))) / (2.0 * A), 0.0)
        out[k] = np.where(hit & (s > 0), s, 0.0).astype(np.float32)
    return out


FLOATER_RADIUS, FLOATER_AT = 0.09, 1.12


@functools.lru_cache(maxsize=None)
def floater():
    """The sphere in 24 ring cameras of 37 x 53, and a blob of radius 0.09 at radius 1.12, midway between the directions of cameras 0
    and 1, rendered into the depth maps of views 0 and 1 only: two views agree on a too-near depth, 22 look through it."""
    n, rows, cols = 24, 37, 53
    cams = ring_cameras(n, rows, cols)
    depths, images = R.sphere_depths(cams, rows, cols, RADIUS)
    a = 0.5 * ((2.0 * np.pi * 0 / n + 0.1) + (2.0 * np.pi * 1 / n + 0.1))               # ring_cameras' angles
    blob = ball_depths(cams[:2], rows, cols, FLOATER_AT * np.array([np.cos(a), 0.0, np.sin(a)]), FLOATER_RADIUS)
    assert (blob > 0).sum(axis=(1, 2)).min() >= 4
    depths[:2] = np.where(blob > 0, blob, depths[:2])
    return Scene(depths, cams, images)


@functools.lru_cache(maxsize=None)
def band_edge():
    """R = I, t = 0, dyadic voxel, origin, trunc and depth: a voxel's c2 is its z centre exactly, so sdf = d - c2 meets +trunc and
    -trunc exactly at some voxels.  Two views (the same camera twice) so that weights reach 2; the second depth is farther by four
    voxels: its +trunc edge falls inside the first one's band."""
    rows, cols = 16, 16
    cam = np.zeros(16)
    cam[[0, 4, 8]] = 1.0
    cam[12:] = (16.0, 16.0, 8.0, 8.0)
    voxel, trunc = 0.125, 0.5
    origin = (-1.0, -1.0, 1.0)                            # z centres at 1.0625 + 0.125 k
    depths = np.stack([np.full((rows, cols), 2.0625, np.float32), np.full((rows, cols), 2.5625, np.float32)])
    rng = np.random.RandomState(5)
    images = rng.uniform(0, 255, (2, rows, cols, 3)).astype(np.float32)
    return Scene(depths, np.stack([cam, cam]), images, trunc=trunc, origin=origin, dims=(2, 2, 2), voxel=voxel)


def band_edge_counts(scene):
    """How many (voxel, view) pairs in view have sdf == +trunc and sdf == -trunc exactly."""
    plus = minus = 0
    for _, band, free, sdf, _, _ in _views(scene.depths, scene.cams, *scene.args(), scene.pixel_centre):
        plus += int((band & (sdf == scene.trunc)).sum())
        minus += int((band & (sdf == -scene.trunc)).sum())
        assert not (free & (sdf == scene.trunc)).any()
    return plus, minus


@functools.lru_cache(maxsize=None)
def narrow_field():
    """12 ring cameras of 23 x 31 with three times the focal length: each view sees only part of the box."""
    n, rows, cols = 12, 23, 31
    cams = ring_cameras(n, rows, cols, focal=3 * cols)
    depths, images = R.sphere_depths(cams, rows, cols, RADIUS)
    return Scene(depths, cams, images)


@functools.lru_cache(maxsize=None)
def views65():
    """65 ring cameras of 5 x 7: a second mask word."""
    cams = ring_cameras(65, 5, 7)
    depths, images = R.sphere_depths(cams, 5, 7, RADIUS)
    return Scene(depths, cams, images)
