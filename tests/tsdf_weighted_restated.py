"""Per-pixel view weights in the TSDF integration and the fusion's agreement count per pixel (include/atvsnet_hip.h, DESIGN.md
section 10.3c) restated in numpy, independent of the kernels: `integrate` is tests/tsdf_carve_restated.integrate on the DENSE grid
with a weight per pixel (every voxel of the box against every view, with or without carving); `support` is the oracle's
fuse_reference run for every reference camera, its trace's count turned into the masked depth plane and the weight plane.  With them
the scenes and the derived inputs the weighted tests share, each made once: do not write into what these functions return."""
import functools

import numpy as np

import tsdf_restated as R
from tsdf_carve_restated import _views, Scene, ring, floater, ball_depths, largest_component_faces      # noqa: F401
from tsdf_carve_restated import FLOATER_AT, FLOATER_RADIUS, RADIUS, TRUNC

from oracle import fusibile as F

FAKE_NORMAL = np.float32(1.0) / np.float32(1.732050808)          # depth_fusion.fake_colmap_normal's (nv, nv, nv)
FAKE_NORMAL_THRESHOLD = 360 * np.pi / 180.0                      # depth_fusion.NORMAL_THRESHOLD: rejects nothing
DISP_THRESHOLD = 0.01


def integrate(depths, cams, voxel, trunc, origin, dims, weights, images=None, pixel_centre=0.0, carve_weight=None):
    """-> dict(tsdf, weight (nz,ny,nx) float32, color (nz,ny,nx,3) float32 or None, free (nz,ny,nx) float32 or None without
    carve_weight, blocks (nb,3) int32).  weights (n,rows,cols) float32: a view is a sample at the pixel it lands on only when the
    pixel's weight is > 0 and finite; it then adds w where tests/tsdf_restated.py adds 1, each product rounded before its sum."""
    weights = np.asarray(weights, np.float32)
    assert weights.shape == np.asarray(depths).shape
    bx, by, bz = dims
    shape = (bz * 8, by * 8, bx * 8)
    S, W, Wf = np.zeros(shape, np.float64), np.zeros(shape, np.float64), np.zeros(shape, np.float64)
    C = np.zeros(shape + (3,), np.float64)
    for k, band, free, sdf, v, u in _views(depths, cams, voxel, trunc, origin, dims, pixel_centre):
        w32 = weights[k][v, u]
        with np.errstate(invalid='ignore'):
            sample = (w32 > 0) & np.isfinite(w32)
        w = w32.astype(np.float64)
        band, free = band & sample, free & sample
        S[band] += w[band] * (sdf[band] / float(trunc))
        W[band] += w[band]
        Wf[free] += w[free]
        if images is not None:
            C[band] += w[band][:, None] * np.asarray(images[k], np.float32)[v[band], u[band], :3].astype(np.float64)
    has = W > 0
    with np.errstate(all='ignore'):
        if carve_weight is None:
            tsdf = np.where(has, S / W, 0.0).astype(np.float32)
        else:
            f = float(carve_weight) * Wf                      # formed once
            tsdf = np.where(has, (S + f) / (W + f), 0.0).astype(np.float32)
        color = None if images is None else np.where(has[..., None], C / W[..., None], 0.0).astype(np.float32)
        weight = W.astype(np.float32)
    occupied = has.reshape(bz, 8, by, 8, bx, 8).any(axis=(1, 3, 5))
    zz, yy, xx = np.nonzero(occupied)
    return dict(tsdf=tsdf, weight=weight, color=color, free=None if carve_weight is None else np.where(has, Wf, 0.0).astype(np.float32),
                blocks=np.stack([xx, yy, zz], axis=1).astype(np.int32).reshape(-1, 3))


def integrate_scene(scene, weights, carve_weight=None, depths=None):
    """`integrate` on a Scene (or a tests/tsdf_cases.Integration), optionally with other depths."""
    return integrate(scene.depths if depths is None else depths, scene.cams, scene.voxel, scene.trunc, scene.origin, scene.dims,
                     weights, images=scene.images, pixel_centre=scene.pixel_centre, carve_weight=carve_weight)


def mesh_of(scene, want, min_weight=1.0):
    return R.mesh(want['tsdf'], want['weight'], want['color'], scene.origin, scene.voxel, min_weight)


# ----------------------------------------------------------------------------------------------------------------------------------
# the agreement count
# ----------------------------------------------------------------------------------------------------------------------------------
def projections(cams16):
    """The (n,3,4) projection matrices K [R | t] of cameras in scan_render's layout (R row-major, t, fx, fy, cx, cy)."""
    cams16 = np.asarray(cams16, np.float64).reshape(-1, 16)
    Ps = []
    for c in cams16:
        K = np.array([[c[12], 0.0, c[14]], [0.0, c[13], c[15]], [0.0, 0.0, 1.0]])
        Ps.append(K @ np.concatenate([c[:9].reshape(3, 3), c[9:12].reshape(3, 1)], axis=1))
    return np.stack(Ps)


def fusion_cameras(cams16):
    """(n,28) float32, the fusion's camera rows of the same cameras."""
    return F.pack_cameras(projections(cams16))


def fake_slab(depths):
    """(n,rows,cols,4) float32 = (nv, nv, nv, depth) where depth > 0, (0, 0, 0, depth) elsewhere: what atvs_fusion_stage_f32 stages."""
    depths = np.asarray(depths, np.float32)
    with np.errstate(invalid='ignore'):
        nv = np.where(depths > 0, FAKE_NORMAL, np.float32(0.0)).astype(np.float32)
    return np.ascontiguousarray(np.stack([nv, nv, nv, depths], axis=-1))


def support(cams28, nd, disp_thresh, normal_thresh, num_consistent):
    """-> dict(count (n,rows,cols) int32, depth, weight (n,rows,cols) float32): the oracle's count of every reference camera, the
    pixel's own depth (its bits) where count >= num_consistent and +0 elsewhere, float32(1 + count) / float32(1 + num_consistent)."""
    nd = np.asarray(nd, np.float32)
    n = len(nd)
    count = np.zeros(nd.shape[:3], np.int32)
    blank = np.zeros(nd.shape, np.float32)
    for ref in range(n):
        trace = {}
        F.fuse_reference(cams28, nd, blank, ref, disp_thresh, normal_thresh, num_consistent, trace=trace)
        count[ref] = trace['count']
    return dict(count=count, **planes(count, nd[..., 3], num_consistent))


def planes(count, depth, num_consistent):
    """The masked depth plane and the weight plane of a count."""
    masked = np.where(count >= int(num_consistent), depth, np.float32(0.0)).astype(np.float32)
    weight = ((1 + count).astype(np.float32) / np.float32(1 + int(num_consistent))).astype(np.float32)
    return dict(depth=np.ascontiguousarray(masked), weight=np.ascontiguousarray(weight))


@functools.lru_cache(maxsize=None)
def scene_count(name):
    """('ring' | 'floater') -> (cams28, slab, count) under the fake normal and DISP_THRESHOLD; the count does not depend on
    num_consistent, so one oracle run serves every value of it."""
    scene = {'ring': ring, 'floater': floater}[name]()
    cams28, nd = fusion_cameras(scene.cams), fake_slab(scene.depths)
    return cams28, nd, support(cams28, nd, DISP_THRESHOLD, FAKE_NORMAL_THRESHOLD, 0)['count']


def scene_support(name, num_consistent):
    cams28, nd, count = scene_count(name)
    return dict(count=count, **planes(count, nd[..., 3], num_consistent))


def blob_pixels():
    """(2,rows,cols) bool: where the floater's blob was rendered into views 0 and 1."""
    scene = floater()
    n, rows, cols = scene.depths.shape
    a = 0.5 * ((2.0 * np.pi * 0 / n + 0.1) + (2.0 * np.pi * 1 / n + 0.1))
    return ball_depths(scene.cams[:2], rows, cols, FLOATER_AT * np.array([np.cos(a), 0.0, np.sin(a)]), FLOATER_RADIUS) > 0


@functools.lru_cache(maxsize=None)
def floater_masked(num_consistent=2):
    """The floater integrated from its consistency-masked depths, unweighted -> (masked depths, the dense restatement)."""
    scene = floater()
    depths = scene_support('floater', num_consistent)['depth']
    return depths, R.integrate(depths, scene.cams, *scene.args(), images=scene.images, pixel_centre=scene.pixel_centre)


@functools.lru_cache(maxsize=None)
def floater_masked_mesh(num_consistent=2, min_weight=1.0):
    return mesh_of(floater(), floater_masked(num_consistent)[1], min_weight)


@functools.lru_cache(maxsize=None)
def floater_plain_mesh(min_weight=1.0):
    return floater().mesh(None, min_weight)


def farthest(vertices):
    return float(np.linalg.norm(np.asarray(vertices, np.float64), axis=1).max())


def random_weights(shape, seed, lo=0.0, hi=2.0):
    """float32 weights in (lo, hi] from a fixed seed: almost none is dyadic, so w * x rounds."""
    rng = np.random.RandomState(seed)
    return (hi - rng.uniform(0.0, hi - lo, shape)).astype(np.float32)


def special_weights(shape, seed):
    """Random weights with 0, -0, -1, NaN, +inf, -inf and a denormal planted at a seventh of the pixels each way."""
    w = random_weights(shape, seed).reshape(-1)
    rng = np.random.RandomState(seed + 1)
    kind = rng.randint(0, 14, w.shape)
    for k, v in enumerate((0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 1e-40)):
        w[kind == k] = np.float32(v)
    return w.reshape(shape)


@functools.lru_cache(maxsize=None)
def biased_ring():
    """ring() with view 0's depths farther by half the truncation -> (scene, weights with 0.05 on view 0 and 1 elsewhere)."""
    base = ring()
    depths = base.depths.copy()
    depths[0] = np.where(depths[0] > 0, depths[0] + np.float32(0.5 * TRUNC), 0).astype(np.float32)
    weights = np.ones(depths.shape, np.float32)
    weights[0] = np.float32(0.05)
    return Scene(depths, base.cams, base.images), weights


def mean_radius_error(vertices):
    return float(np.abs(np.linalg.norm(np.asarray(vertices, np.float64), axis=1) - RADIUS).mean())
