"""Shared inputs of the geometry tests (tests/test_geometry_cases_host.py pins their properties on the CPU oracle,
tests/test_gpu_geometry.py runs the HIP kernels on them).  Plain helpers, no fixtures.

synthetic.make_cams gives an identity reference camera, sources rotated about y and shifted along x only, and K without skew and
with fx = fy: half of every homography and relative pose is exact zeros and ones, and c_l = 0.  general_cams fills every entry;
metric_range / metric_map restate the same scene in metric depth (FLAGS.inverse_depth = False); degenerate_homographies puts
exact zeros, sign changes and an overflow into the projective divide; backwards_cam looks away from the scene (negative z).
"""
import numpy as np
import torch


def _rot(axis, rad):
    c, s = np.cos(rad), np.sin(rad)
    if axis == 'x':
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    if axis == 'y':
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def general_cams(n, h, w, D, d_min=0.05, d_max=0.36):
    """(1, n, 2, 4, 4) float32 cameras for an (h, w) map: no identity, no axis-aligned rotation or shift, K with skew and
    fx != fy, every view its own K.  cam[1,3,0:2] = (inverse-depth start, interval) of the range d_min .. d_max in D planes."""
    cams = np.zeros((n, 2, 4, 4), np.float64)
    for i in range(n):
        k = (i + 1) // 2
        s = (-1.0) ** i
        R = _rot('z', np.deg2rad(0.6 - 1.3 * k * s)) @ _rot('y', np.deg2rad(-0.7 + 2.0 * k * s)) @ \
            _rot('x', np.deg2rad(1.1 + 0.9 * k * s))
        E = np.eye(4)
        E[:3, :3] = R
        E[:3, 3] = (0.03 - 0.25 * k * s, 0.02 + 0.11 * k * s, -0.04 + 0.07 * k)
        cams[i, 0] = E
        cams[i, 1, :3, :3] = [[0.89 * w + 0.4 * i, 0.35 + 0.1 * i, w / 2.0 + 1.3 - 0.6 * i],
                              [0, 0.93 * w - 0.3 * i, h / 2.0 - 0.8 + 0.5 * i],
                              [0, 0, 1]]
        cams[i, 1, 3, 0] = d_min
        cams[i, 1, 3, 1] = (d_max - d_min) / D
    return torch.from_numpy(cams.astype(np.float32))[None]


def metric_range(ds, di, D):
    """The metric depth sweep over the scene range of the inverse sweep (ds, di, D): it starts at the nearest plane's depth
    1 / (ds + D di) and reaches the farthest one's, 1 / ds, after D intervals."""
    ds_m = 1.0 / (ds + float(D) * di)
    di_m = (1.0 / ds - ds_m) / float(D)
    return ds_m, di_m


def inverse_map(h, w, seed, zero_patch=False, lo=0.05, hi=0.35):
    """(h, w) inverse depths inside the sweep's range; zero_patch: d[:3, :5] = 0, the invalid depths of the 1e-10 clip / mask
    (at least one pixel stays valid at every size)."""
    g = torch.Generator().manual_seed(seed)
    d = lo + (hi - lo) * torch.rand(h, w, generator=g)
    if zero_patch:
        d[:3, :5] = 0.0
        if not bool((d > 0).any()):
            d[-1, -1] = 0.5 * (lo + hi)
    return d


def metric_map(inv):
    """The metric depth map of an all-valid inverse one (metric mode has no validity handling: reference
    homography_warping.py:301-305,321-324 are skipped)."""
    assert bool((inv > 0).all())
    return 1.0 / inv


def degenerate_homographies():
    """(1, 4, 3, 3) float32 of exact binary fractions for a 17 x 23 map (x + 0.5, y + 0.5 are exact, so are the products):
    plane 0: dv == 0 exactly on the column x = 10, dv < 0 left of it    (the +1e-7 guard, a sign change inside the image)
    plane 1: dv == 0 exactly on the row y = 8, dv < 0 below it
    plane 2: xa overflows to inf: every pixel invalid; the bilinear output is NaN (inf * 0), the nearest one pixel (0,0)
    plane 3: ordinary."""
    r0, r1 = [1.03125, -0.03125, -1.25], [0.046875, 0.984375, 0.171875]
    ordinary = [0.0009765625, -0.00048828125, 0.984375]
    H = torch.tensor([[r0, r1, [0.125, 0.0, -1.3125]],
                      [r0, r1, [0.0, -0.25, 2.125]],
                      [[3e38, 0.0, 3e38], r1, ordinary],
                      [r0, r1, ordinary]], dtype=torch.float32)
    return H[None]


DEGENERATE_HW = (17, 23)

# Every (h, w, D) at which tests/test_gpu_geometry.py builds general_cams for a warp: tests/test_geometry_cases_host.py pins, on
# the CPU oracle alone, that no entry of the homographies and relative poses is a structural 0 or 1 and that the masks hold both
# valid and invalid samples there.  The GPU tests refuse a shape that is not listed.
WARP_SHAPES = ((32, 40, 32), (30, 36, 8), (17, 23, 5), (32, 40, 16), (9, 11, 4), (32, 40, 8), (32, 40, 1), (32, 40, 192),
               (24, 40, 12), (48, 64, 3), (48, 64, 2), (24, 40, 1), (24, 40, 8), (24, 40, 6))
# metric-depth sweeps (metric_range) among them
METRIC_SHAPES = ((24, 40, 1), (24, 40, 8), (24, 40, 6))
# (h, w) of the transform_depth tests: the one-workgroup kernel up to 32,768 pixels, the general path above
TRANSFORM_SIZES = ((128, 256), (37, 883), (3, 1500), (300, 7), (4099, 1), (1, 1), (129, 256), (181, 182), (24, 40), (32, 40))
# sizes at which a map is also transformed into backwards_cam
BACKWARDS_SIZES = ((129, 256), (128, 256))


def transform_map(h, w, seed):
    """The inverse depth map of the transform_depth tests: a zero patch wherever the map is large enough to keep valid pixels."""
    return inverse_map(h, w, seed, zero_patch=h * w > 15)


def backwards_cam(cam):
    """cam (..., 2, 4, 4) with its rotation replaced by Rz(0.01) Ry(pi - 0.03) Rx(0.02) (radians): it looks away from what the
    general cameras see, so a depth map transformed into it has only negative z."""
    out = cam.clone()
    R = _rot('z', 0.01) @ _rot('y', np.pi - 0.03) @ _rot('x', 0.02)
    out[..., 0, :3, :3] = torch.from_numpy(R.astype(np.float32))
    return out
