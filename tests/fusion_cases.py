"""Shared inputs of the depth-map fusion tests (tests/test_fusion_cases_host.py pins their properties on the CPU oracle,
tests/test_gpu_fusion.py and tests/test_gpu_fusion_scene.py run the HIP kernels on them).  Plain helpers, no fixtures.

fusion_scene.make_scene is a tilted plane seen by cameras rotated about y only, K diagonal with fx = fy, P unscaled, one constant
normal per view and nothing occluded: half of every P and M_inv is exact zeros and ones and several branches of fuse_pixel
(csrc/fusion_pixel.h) never run.  general_scene is a sphere in front of a tilted wall seen by full cameras (every entry of P and
M_inv filled, every P scaled by its own factor, K with skew and fx != fy), optionally far from the origin; hard_maps plants the
special depths and normals; the four small pairs put exact values into the projective divide, the disparity test and tex_fetch.

The cases are chosen so that the oracle's answer does not hang on a last bit the device may round otherwise: at the finite normal
thresholds the angle of every in-bounds (pixel, view) pair stays 1e-4 rad away from the threshold (test (d) of the host file).
Bilinear blends of unit normals are shorter than 1, so on the sphere acos(dot) runs continuously from 0 up to over 0.1 rad towards
the limb, and on a large map some sample always lands next to 0.08: that threshold is used on the small maps and view counts only,
and a case's `seed` picks noise and planted patches that keep the distance.  The reversed normals have length 0.999.

Measured on the CPU by tests/test_fusion_cases_host.py (it prints these; cases named as case_id names them):
* ray casting against the oracle's `created`, 5 views at 67x131, every ordered pair, both offsets alike: 86.8 % of 175,540 (pixel,
  view) pairs compared, 0 mismatches, 115,964 visible, 2,063 occluded, 34,297 outside;
* `created` of the float64 evaluation against the float32 oracle: 0 pixels differ in every case except
  2x67x131-o1-n0.004-hard-d0.01-a6.28-c1, 1 of 17,554 (0.006 %), and 5x240x320-o1-n0.004-hard-d0.01-a6.28-c2, 66 of 384,000
  (0.017 %); the small pairs 0;
* the least distance of an in-bounds angle from its finite threshold: 1.8e-4 rad (5x67x131-o1-n0-plain-d0.02-a0.30-c5 and
  3x67x131-o0-n0-hard-d0.02-a0.30-c2), 1.9e-4 rad (5x67x131-o1-n0.004-hard-d0.02-a0.30-c2-s1), 2.7e-4 rad
  (2x56x72-o0-n0.004-plain-d0.005-a0.08-c0-s4), 4.8e-4 rad (3x9x33-o1-n0.004-hard-d0.005-a0.08-c2);
* 64,634 in-bounds samples of the plain cases have dot > 1 and pass the disparity test (the `ang != ang` branch decides them);
* a contracted get3Dpoint_cu changes coord at 86-89 % of the pixels at the origin and 58 % at the far offset.
"""
import collections

import numpy as np

from fusion_scene import make_scene

OFFSETS = ((0.0, 0.0, 0.0), (1000.0, -1000.0, 300.0))
SPHERE_RADIUS = 1.2
SPHERE_DEPTH = 8.0          # z of the sphere's centre before the offset
WALL_BEHIND = 3.0           # the wall passes this far behind the sphere's centre
TWO_PI = 2.0 * np.pi

# The sizes the GPU files may use; they refuse a shape that is not listed.
FUSION_SHAPES = {
    'kernel': ((1, 1), (1, 300), (300, 1), (9, 33), (56, 72), (67, 131)),
    'scene': ((240, 320), (67, 131), (48, 64), (37, 53), (41, 45), (33, 70), (30, 40)),
}


# ------------------------------------------------------------------------------------------------------------ the world

def _rot(axis, rad):
    c, s = np.cos(rad), np.sin(rad)
    if axis == 'x':
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    if axis == 'y':
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def world(offset):
    """(sphere centre, wall normal, a point of the wall) in float64."""
    o = np.asarray(offset, np.float64)
    centre = o + np.array([0.1, -0.05, SPHERE_DEPTH])
    nw = np.array([0.15, -0.1, -1.0])
    nw /= np.linalg.norm(nw)
    return centre, nw, centre + np.array([0.0, 0.0, WALL_BEHIND])


def cast(C, dirs, offset):
    """First hit of the rays C + t dirs (t > 0) with the sphere or the wall, float64: -> (t, label) with label 1 = sphere,
    0 = wall, t = inf where a ray hits neither."""
    centre, nw, w0 = world(offset)
    dirs = np.asarray(dirs, np.float64)
    oc = np.asarray(C, np.float64) - centre
    a = (dirs * dirs).sum(-1)
    b = 2.0 * (dirs @ oc)
    c = oc @ oc - SPHERE_RADIUS ** 2
    disc = b * b - 4.0 * a * c
    with np.errstate(all='ignore'):
        ts = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0.0))) / (2.0 * a), np.inf)
        ts = np.where(ts > 0, ts, np.inf)
        tw = ((w0 - np.asarray(C, np.float64)) @ nw) / (dirs @ nw)
        tw = np.where(tw > 0, tw, np.inf)
    return np.minimum(ts, tw), (ts < tw).astype(np.int8)


def general_views(n, rows, cols, offset):
    """[(R, C, K, scale)] float64 of the n cameras: rotation about all three axes (up to about +-18 degrees about y), centres
    spread over about +-1.6 units, every view its own K with skew and fx != fy, P = scale K [R | -R C] with scale = 1 + 0.25 i."""
    o = np.asarray(offset, np.float64)
    m = float(max(rows, cols))
    views = []
    for i in range(n):
        k = (i + 1) // 2
        s = (-1.0) ** i
        R = _rot('z', np.deg2rad(0.6 - 2.0 * k * s)) @ _rot('y', np.deg2rad(-0.7 + 8.5 * k * s)) @ \
            _rot('x', np.deg2rad(1.1 + 1.5 * k * s))
        C = o + np.array([0.05 + 0.8 * k * s, 0.03 - 0.25 * k * s, -0.04 + 0.1 * k])
        K = np.array([[0.89 * m + 0.4 * i, 0.35 + 0.1 * i, cols / 2.0 + 1.3 - 0.6 * i],
                      [0, 0.86 * m - 0.3 * i, rows / 2.0 - 0.8 + 0.5 * i],
                      [0, 0, 1]])
        views.append((R, C, K, 1.0 + 0.25 * i))
    return views


def general_scene(n, rows, cols, offset, noise=0.0, seed=0):
    """A sphere in front of a tilted wall (the gap stays above 15 % in depth), seen by general_views.
    -> (Ps (n,3,4) float64, depths (n,rows,cols) float32 -- scaled like P --, normals (n,rows,cols,3) float32 per pixel, in the
    world frame, images (n,rows,cols,3) uint8 b,g,r, truth) with truth = {'R', 'C', 'K', 'scale' (lists), 'hit' (n,rows,cols,3) and
    'label' (n,rows,cols), 'offset'} in float64.  offset moves the whole world, scene and cameras; noise multiplies every depth
    by 1 + noise * N(0, 1)."""
    rng = np.random.default_rng(seed)
    o = np.asarray(offset, np.float64)
    centre, nw, _ = world(offset)
    ys, xs = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing='ij')
    pix = np.stack([xs, ys, np.ones_like(xs)], -1)
    Ps, depths, normals, images, hits, labels = [], [], [], [], [], []
    views = general_views(n, rows, cols, offset)
    for R, C, K, scale in views:
        Ps.append(scale * (K @ np.concatenate([R, (-R @ C)[:, None]], 1)))
        dirs = pix @ np.linalg.inv(K).T @ R            # camera z of a direction is 1: t is the depth
        t, label = cast(C, dirs, offset)
        assert np.isfinite(t).all()
        hit = C + t[..., None] * dirs
        nrm = np.where(label[..., None] == 1, (hit - centre) / SPHERE_RADIUS, nw)
        depths.append((scale * t).astype(np.float32))
        normals.append(nrm.astype(np.float32))
        Xl = hit - o
        img = 127.0 + 100.0 * np.stack([np.sin(Xl[..., 0] * 2.0), np.cos(Xl[..., 1] * 3.0), np.sin(Xl[..., 0] + Xl[..., 2])], -1)
        images.append(np.clip(img, 0, 255).astype(np.uint8))
        hits.append(hit)
        labels.append(label)
    depths = np.stack(depths)
    if noise:
        depths = depths * (1.0 + noise * rng.normal(size=depths.shape)).astype(np.float32)
    truth = {'R': [v[0] for v in views], 'C': [v[1] for v in views], 'K': [v[2] for v in views], 'scale': [v[3] for v in views],
             'hit': np.stack(hits), 'label': np.stack(labels), 'offset': tuple(float(v) for v in offset)}
    return np.stack(Ps), depths, np.stack(normals), np.stack(images), truth


def textures(depths, normals, images):
    """(normals_depths, images) (n,rows,cols,4) float32 as the kernels take them."""
    nd = np.ascontiguousarray(np.concatenate([normals, depths[..., None]], -1).astype(np.float32))
    img = np.asarray(images)
    img4 = np.ascontiguousarray(np.concatenate([img.astype(np.float32), np.zeros(img.shape[:3] + (1,), np.float32)], -1))
    return nd, img4


# ---------------------------------------------------------------------------------------------------------- special values

SPECIAL_DEPTHS = (0.0, -0.0, -2.5, np.inf, np.nan, 1e-39, 3e38)
FAKE_NORMAL = np.float32(1.0) / np.float32(1.732050808)          # depth_fusion.fake_colmap_normal's (nv, nv, nv)


def is_special(depth):
    """Where a depth is one of SPECIAL_DEPTHS' kind: not a finite value of ordinary magnitude above 0."""
    with np.errstate(invalid='ignore'):
        return ~(np.isfinite(depth) & (depth > 1e-3) & (depth < 1e6))


def hard_maps(nd, seed):
    """A copy of nd (n,rows,cols,4) with special values planted, in every view at its own places.  Depths: each of SPECIAL_DEPTHS
    singly and as a small patch (2x2 on maps under 20 pixels in a dimension, else 3x3), so that bilinear footprints mix them with
    valid texels; the zero depths get zero normals, as fusion_stage_kernel writes them.  Normals, depth untouched: a patch of
    (nv, nv, nv), one of normals of length 1.001 (the dot product with an agreeing unit normal exceeds 1, acosf gives NaN, which
    the kernel turns into 0), one of reversed normals of length 0.999 (the angle is pi - 0.045 whatever the rounding of the dot
    product; at length 1 float32 puts it on either side of -1, that is at pi or at NaN -> 0) and one of reversed normals of length
    1.001 (dot < -1: NaN -> 0, so the view passes the normal test)."""
    nd = np.array(nd, np.float32, copy=True)
    n, rows, cols = nd.shape[:3]
    small = min(rows, cols) < 20
    p = 2 if small else 3
    mr, mc = (0, 0) if small else (rows // 5, cols // 5)
    cells = [(r, c) for r in range(mr, rows - mr - p + 1, p + 1) for c in range(mc, cols - mc - p + 1, p + 1)]
    need = 2 * len(SPECIAL_DEPTHS) + 4
    assert len(cells) >= need, 'map too small for hard_maps'
    rng = np.random.default_rng(seed)
    for v in range(n):
        pick = [cells[j] for j in rng.choice(len(cells), need, replace=False)]
        for j, d in enumerate(SPECIAL_DEPTHS):
            for (r, c), size in ((pick[2 * j], 1), (pick[2 * j + 1], p)):
                nd[v, r:r + size, c:c + size, 3] = np.float32(d)
                if d == 0:
                    nd[v, r:r + size, c:c + size, :3] = 0
        base = 2 * len(SPECIAL_DEPTHS)
        (r, c) = pick[base]
        nd[v, r:r + p, c:c + p, :3] = FAKE_NORMAL
        for (r, c), factor in ((pick[base + 1], 1.001), (pick[base + 2], -0.999), (pick[base + 3], -1.001)):
            nd[v, r:r + p, c:c + p, :3] *= np.float32(factor)
    return nd


# ------------------------------------------------------------------------------------------------------------- small pairs

PAIR_SHAPE = (56, 72)


def _plane_views(K, Rs, Cs, rows, cols, seed=0):
    """The tilted plane of fusion_scene.make_scene seen by cameras (K, R, C): -> Ps, depths, normals (world), images."""
    rng = np.random.default_rng(seed)
    nrm = np.array([0.1, -0.05, -1.0])
    nrm /= np.linalg.norm(nrm)
    d0 = 5.0
    ys, xs = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing='ij')
    Ps, depths, normals, images = [], [], [], []
    for R, C in zip(Rs, Cs):
        C = np.asarray(C, np.float64)
        Ps.append(K @ np.concatenate([R, (-R @ C)[:, None]], 1))
        rays = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K).T @ R
        s = -(nrm @ C + d0) / (rays @ nrm)
        depths.append(s.astype(np.float32))
        normals.append(np.broadcast_to(nrm.astype(np.float32), (rows, cols, 3)).copy())
        X = C + s[..., None] * rays
        img = 127.0 + 100.0 * np.stack([np.sin(X[..., 0] * 2.0), np.cos(X[..., 1] * 3.0), np.sin(X[..., 0] + X[..., 1])], -1)
        images.append(np.clip(img + rng.uniform(0, 4, img.shape), 0, 255).astype(np.uint8))
    return np.stack(Ps), np.stack(depths), np.stack(normals), np.stack(images)


def facing_away_pair():
    """View 0 of make_scene(2, 56, 72) and the same camera turned 180 degrees about its own y axis, its centre moved by 0.05
    along x; both carry view 0's maps.  Every point of one view lies behind the other: tz < 0, the relative disparity difference
    |d - o| / d is negative and passes (the reference's quirk, fusibile.cu:211), so with the normal threshold at 2 pi the created
    pixels are exactly the ones that project inside the image.  -> Ps, depths, normals, images."""
    from oracle.fusibile import decompose_projection
    Ps, depths, normals, images, _, _ = make_scene(2, *PAIR_SHAPE)
    K, R, C = decompose_projection(Ps[0])
    K = K / K[2, 2]
    R1 = np.diag([-1.0, 1.0, -1.0]) @ R
    C1 = C + np.array([0.05, 0.0, 0.0])
    P1 = K @ np.concatenate([R1, (-R1 @ C1)[:, None]], 1)
    two = lambda a: np.stack([a[0], a[0]])          # noqa: E731
    return np.stack([Ps[0], P1]), two(depths), two(normals), two(images)


_K64 = np.array([[64.0, 0, 32.0], [0, 64.0, 32.0], [0, 0, 1]])


def side_by_side_holes():
    """Two cameras of identical orientation (the identity) whose centres differ along x only, (0, 0, 0) and (0.5, 0, 0), K of
    powers of two, the tilted plane with holes of depth 0 (a block and single pixels).  A hole back-projects to its own camera's
    centre exactly, which lies in the other camera's principal plane: tz == 0 exactly, px = -+inf, py = 0 / 0.
    -> Ps, depths, normals, images."""
    rows, cols = PAIR_SHAPE
    Ps, depths, normals, images = _plane_views(_K64, [np.eye(3)] * 2, [(0, 0, 0), (0.5, 0, 0)], rows, cols, seed=3)
    depths[:, 3:9, 40:50] = 0
    depths[:, 20::7, 5::11] = 0
    normals[depths == 0] = 0
    return Ps, depths, normals, images


def zero_baseline_pair():
    """Two views with one centre, the origin, the second turned by 2 degrees about y: base = 0, both disparities are 0 and
    0 / 0 is NaN, so nothing agrees.  -> Ps, depths, normals, images."""
    rows, cols = PAIR_SHAPE
    return _plane_views(_K64, [np.eye(3), _rot('y', np.deg2rad(2.0))], [(0, 0, 0), (0, 0, 0)], rows, cols, seed=4)


# (sx, sy) of exact_projections: px = x + sx, py = y + sy
EXACT_SHIFTS = (
    (0.0, 0.0),                                         # 0 and cols - 1, weight 0
    (-2.0 ** -10, -2.0 ** -10),                         # just below 0: column 0 / row 0 are out; elsewhere the weight rounds to 1.0
    (1.0 - 2.0 ** -10, 1.0 - 2.0 ** -10),               # cols - 2^-10: the second texel clamps and has weight 1.0
    (1.0, 1.0),                                         # exactly cols: out of bounds
    (77.0 / 256, 3.0 / 256),                            # fractions k / 256
    (77.0 / 256 + 1.0 / 512, 200.0 / 256 + 1.0 / 512),  # rounding ties
    (255.5 / 256, 255.5 / 256),                         # the tie that rounds up to weight 1.0
    (255.75 / 256, 0.5),                                # above it
    (-3.25, -2.5),                                      # several columns and rows out on the low side
    (2.0 + 130.0 / 256, 3.0 + 1.0 / 512),               # several out on the high side
)


# (rows, cols, sx, sy) of exact_projections on one-row, one-column and one-pixel maps, where both texels of a footprint clamp to
# the same row or column: ties, weight 1.0, an out-of-bounds side each, and a shift that leaves nothing in bounds
THIN_EXACT = (
    (1, 300, 77.0 / 256 + 1.0 / 512, 0.5),
    (1, 300, 1.0 - 2.0 ** -10, 255.5 / 256),
    (1, 300, -3.25, 0.0),
    (1, 300, 0.0, 1.0),
    (300, 1, 0.5, 77.0 / 256 + 1.0 / 512),
    (300, 1, 255.5 / 256, 1.0 - 2.0 ** -10),
    (300, 1, 0.0, -3.25),
    (300, 1, 1.0, 0.0),
    (1, 1, 0.0, 0.0),
    (1, 1, 0.5, 0.25 + 1.0 / 512),
    (1, 1, 1.0 - 2.0 ** -10, 1.0 - 2.0 ** -10),
    (1, 1, -2.0 ** -10, 0.0),
)
# every (rows, cols, sx, sy) the GPU file runs
EXACT_CASES = tuple(PAIR_SHAPE + s for s in EXACT_SHIFTS) + THIN_EXACT


def exact_projections(sx, sy, shape=PAIR_SHAPE):
    """A fronto-parallel plane at depth 4 seen by two cameras with f = 64 and a baseline of 0.5 along x: the disparity is exactly
    8.  The second camera's principal point is (32 + 8 + sx, 32 + sy), so a pixel (x, y) of view 0 projects to
    (x + sx, y + sy) in view 1 with every intermediate exact in float32 (sx, sy: binary fractions).  Depths are 4, normals
    (0, 0, -1), colours small integers.  -> Ps, depths, normals, images (float32 colours)."""
    rows, cols = shape
    K1 = np.array([[64.0, 0, 40.0 + sx], [0, 64.0, 32.0 + sy], [0, 0, 1]])
    Ps = np.stack([_K64 @ np.concatenate([np.eye(3), np.zeros((3, 1))], 1),
                   K1 @ np.concatenate([np.eye(3), -np.array([[0.5], [0.0], [0.0]])], 1)])
    depths = np.full((2, rows, cols), 4.0, np.float32)
    normals = np.zeros((2, rows, cols, 3), np.float32)
    normals[..., 2] = -1.0
    ys, xs = np.meshgrid(np.arange(rows), np.arange(cols), indexing='ij')
    images = np.stack([np.stack([(3 * xs + ys + 5 * v) % 13, (xs + 5 * ys + v) % 11, (xs * ys + 3 * v) % 7], -1) for v in range(2)])
    return Ps, depths, normals, images.astype(np.float32)


def exact_blend(img, sx, sy):
    """By hand, in float64 (every product is exact: 8-bit weights, 4-bit colours): the blend tex_fetch must return at
    (x + sx, y + sy) for every pixel (x, y) of the (rows, cols, 3) image, and whether that position is inside the image."""
    rows, cols = img.shape[:2]
    img = np.asarray(img, np.float64)
    out = np.zeros((rows, cols, 3))
    inside = np.zeros((rows, cols), bool)
    for y in range(rows):
        py = y + sy
        for x in range(cols):
            px = x + sx
            if not (0 <= px < cols and 0 <= py < rows):
                continue
            inside[y, x] = True
            x0, y0 = int(np.floor(px)), int(np.floor(py))
            wx = np.floor((px - x0) * 256 + 0.5) / 256           # 8 fractional bits, ties up
            wy = np.floor((py - y0) * 256 + 0.5) / 256
            x1, y1 = min(x0 + 1, cols - 1), min(y0 + 1, rows - 1)
            out[y, x] = (1 - wy) * ((1 - wx) * img[y0, x0] + wx * img[y0, x1]) + wy * ((1 - wx) * img[y1, x0] + wx * img[y1, x1])
    return out, inside


def expected_exact(images, sx, sy):
    """(texture (rows,cols,3) float64, created) of reference camera 0 of exact_projections at num_consistent = 1, by hand: the mean
    of the pixel's own colour and the blend where the projection is inside the image, else the pixel's own colour."""
    blend, inside = exact_blend(images[1], sx, sy)
    img0 = np.asarray(images[0], np.float64)
    return np.where(inside[..., None], (img0 + blend) / 2.0, img0), inside


# ------------------------------------------------------------------------------------------------------------ the GPU cases

T_WIDE, T_MID, T_TIGHT = (0.01, TWO_PI), (0.02, 0.3), (0.005, 0.08)      # (disparity threshold, normal threshold)
FINITE_NORMAL_THRESHOLDS = (0.3, 0.08)

Case = collections.namedtuple('Case', 'n rows cols offset noise hard thresholds ncons seed', defaults=(0,))

# what tests/test_gpu_fusion.py runs through the per-camera kernel, every reference camera of each
KERNEL_CASES = (
    Case(2, 9, 33, 0, 0.0, False, T_TIGHT, 1),
    Case(3, 9, 33, 1, 0.004, True, T_TIGHT, 2),
    Case(2, 56, 72, 0, 0.004, False, T_TIGHT, 0, seed=4),
    Case(5, 56, 72, 1, 0.0, True, T_WIDE, 4),
    Case(3, 56, 72, 0, 0.004, True, T_MID, 3, seed=2),
    Case(5, 67, 131, 0, 0.0, False, T_WIDE, 1),
    Case(5, 67, 131, 1, 0.004, True, T_MID, 2, seed=1),
    Case(5, 67, 131, 1, 0.0, False, T_MID, 5),
    Case(5, 67, 131, 0, 0.004, True, T_WIDE, 0),
    Case(2, 67, 131, 1, 0.004, True, T_WIDE, 1),
    Case(3, 67, 131, 0, 0.0, True, T_MID, 2),
    Case(2, 1, 1, 0, 0.0, False, T_WIDE, 1),
    Case(3, 1, 300, 1, 0.0, False, T_WIDE, 1),
    Case(3, 300, 1, 0, 0.004, False, T_MID, 2),
)
# what tests/test_gpu_fusion_scene.py runs through the whole-scene kernel: every 67x131 case above, and 5 views of 240x320
SCENE_CASES = tuple(c for c in KERNEL_CASES if (c.rows, c.cols) == (67, 131)) + (Case(5, 240, 320, 1, 0.004, True, T_WIDE, 2),)


def case_id(case):
    """views x rows x cols - offset - noise - plain / hard - disparity threshold - normal threshold - num_consistent [- seed]"""
    return '%dx%dx%d-o%d-n%g-%s-d%g-a%.2f-c%d%s' % (case.n, case.rows, case.cols, case.offset, case.noise,
                                                     'hard' if case.hard else 'plain', case.thresholds[0], case.thresholds[1],
                                                     case.ncons, '-s%d' % case.seed if case.seed else '')


_cache = {}


def case_inputs(case):
    """(Ps, depths, normals, images, truth) of a Case, built once and shared (read-only)."""
    if case not in _cache:
        Ps, depths, normals, images, truth = general_scene(case.n, case.rows, case.cols, OFFSETS[case.offset], case.noise,
                                                           seed=case.n + case.rows + case.seed)
        if case.hard:
            nd = hard_maps(np.concatenate([normals, depths[..., None]], -1), seed=case.cols + case.ncons + case.seed)
            depths, normals = np.ascontiguousarray(nd[..., 3]), np.ascontiguousarray(nd[..., :3])
        for a in (Ps, depths, normals, images):
            a.setflags(write=False)
        _cache[case] = (Ps, depths, normals, images, truth)
    return _cache[case]
