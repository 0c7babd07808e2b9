"""The ETH3D-style part of eval_cloud: voxel-averaged shares and the scanners' free space.

ETH3D's published protocol (Schoeps et al., CVPR 2017) differs from plain precision / recall in two ways, both restated
here.  (1) The shares are formed per occupied voxel and averaged over voxels, so that a surface seen by eight cameras does not weigh
eight times.  (2) A reconstruction point without a ground-truth point within tau is INACCURATE only where a scanner could have seen
it -- in front of what the scanner measured along that ray (free space), or no further behind it than a margin; a point behind
everything the scanners saw, or seen by none, is UNOBSERVED and counts nowhere.

A scanner's view of its own scan is a cube map: six 90-degree pinhole cameras at the scanner's origin (cube_cameras), rendered by
ops.scan_render with splat = 0 -- a laser scanner sees every point it recorded.  ops.cloud_scan_excess looks every reconstruction
point up in them, ops.cloud_voxel_shares forms the per-voxel shares as integers; include/atvsnet_hip.h has both definitions.

This is the protocol as published, restated -- not ETH3D's evaluation program, which was never run beside it.  What still differs
by construction: the official program models each laser beam's radius and divergence, where this takes the nearest sample of a
(2 vis_window + 1)^2 pixel window; a window stops at a cube edge instead of continuing on the neighbouring face.  cube_size,
vis_window and free_space_margin are DEFAULTS chosen here, not measurements of that program.
"""
import os
import xml.etree.ElementTree as ET

import numpy as np

# world axes of (right, down, forward) per face: forward = +x, -x, +y, -y, +z, -z; right = down x forward, so each is a rotation
_FACES = np.array([
    [[0, -1, 0], [0, 0, -1], [1, 0, 0]],
    [[0, 1, 0], [0, 0, -1], [-1, 0, 0]],
    [[1, 0, 0], [0, 0, -1], [0, 1, 0]],
    [[-1, 0, 0], [0, 0, -1], [0, -1, 0]],
    [[1, 0, 0], [0, 1, 0], [0, 0, 1]],
    [[1, 0, 0], [0, -1, 0], [0, 0, -1]],
], np.float64)

PIXEL_CENTRE = 0.5          # what cube_cameras' maps are rendered and queried with


def cube_cameras(origin, size):
    """The six faces of a cube map at `origin` (3 numbers), size x size pixels each -> (6,16) float64 rows of ops.scan_render:
    R (row-major), t = -R origin, fx = fy = cx = cy = size / 2.  With pixel_centre = 0.5 a face covers |c_0|, |c_1| <= c_2."""
    o = np.asarray(origin, np.float64).reshape(-1)
    if o.shape != (3,) or not np.isfinite(o).all():
        raise ValueError('origin: expected 3 finite numbers, got %r' % (origin,))
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or int(size) < 1:
        raise ValueError('size: expected a positive integer, got %r' % (size,))
    out = np.zeros((6, 16), np.float64)
    out[:, :9] = _FACES.reshape(6, 9)
    out[:, 9:12] = -(_FACES @ o)
    out[:, 12:] = int(size) / 2.0
    return out


def read_mlp(path):
    """A MeshLab project (ETH3D's scan_alignment.mlp) -> [(PLY path resolved against the file's folder, 4x4 float64)] in file
    order: every MLMesh's `filename` and the 16 numbers of its MLMatrix44 child (identity when it has none)."""
    root = ET.parse(path).getroot()
    folder = os.path.dirname(os.path.abspath(path))
    out = []
    for mesh in root.iter('MLMesh'):
        name = mesh.get('filename')
        if not name:
            raise ValueError('%s: an MLMesh without a filename' % path)
        node = mesh.find('MLMatrix44')
        if node is None:
            T = np.eye(4)
        else:
            try:
                T = np.array([float(w) for w in (node.text or '').split()], np.float64)
            except ValueError:
                T = np.zeros(0)
            if T.size != 16 or not np.isfinite(T).all():
                raise ValueError('%s: the MLMatrix44 of %s is not 16 finite numbers' % (path, name))
            T = T.reshape(4, 4)
        out.append((os.path.normpath(os.path.join(folder, name)), T))
    if not out:
        raise ValueError('%s: no MLMesh in the project' % path)
    return out


def load_origins(path):
    """A text file with one `x y z` per scan -> (S,3) float64."""
    o = np.loadtxt(path, dtype=np.float64, ndmin=2)
    if o.ndim != 2 or o.shape[1] != 3 or not np.isfinite(o).all():
        raise ValueError('%s: expected one finite `x y z` per line' % path)
    return o


def check_options(eth3d_voxel, cube_size, vis_window, free_space_margin):
    v, m = float(eth3d_voxel), float(free_space_margin)
    if not (v > 0.0 and np.isfinite(v)):
        raise ValueError('eth3d_voxel must be positive and finite, got %r' % (eth3d_voxel,))
    if isinstance(cube_size, bool) or not isinstance(cube_size, (int, np.integer)) or int(cube_size) < 1:
        raise ValueError('cube_size: expected a positive integer, got %r' % (cube_size,))
    if isinstance(vis_window, bool) or not isinstance(vis_window, (int, np.integer)) or not 0 <= int(vis_window) <= 2:
        raise ValueError('vis_window: expected an integer in 0..2, got %r' % (vis_window,))
    if not np.isfinite(m):
        raise ValueError('free_space_margin must be finite, got %r' % (free_space_margin,))
    return v, int(cube_size), int(vis_window), m


def check_scans(scans, scanner_origins):
    """-> (S,3) float64 origins; raises unless there is one finite origin per scan."""
    scans = list(scans)
    if not scans:
        raise ValueError('scans: at least one scan')
    if scanner_origins is None:
        raise ValueError('scans need scanner_origins: one `x y z` per scan')
    o = np.asarray(scanner_origins, np.float64)
    if o.ndim != 2 or o.shape[1:] != (3,) or not np.isfinite(o).all():
        raise ValueError('scanner_origins: expected (S,3) finite numbers, got shape %s' % (o.shape,))
    if o.shape[0] != len(scans):
        raise ValueError('%d scans but %d scanner origins: one origin per scan' % (len(scans), o.shape[0]))
    return o


def metrics(words_recon, words_gt, n_recon, tolerances, params):
    """The `eth3d` dict from the (T,4) integer words of ops.cloud_voxel_shares for the reconstruction (with excess) and the
    ground truth (without): plain Python numbers; a share without voxels is 0."""
    def share(w):
        return int(w[0]) / (int(w[1]) * 4294967296) if int(w[1]) else 0.0
    out = dict(params)
    out['tolerances'] = []
    for t, wr, wg in zip(tolerances, words_recon, words_gt):
        a, c = share(wr), share(wg)
        out['tolerances'].append({'tolerance': float(t), 'accuracy': a, 'completeness': c,
                                  'f1': 2.0 * a * c / (a + c) if a + c > 0.0 else 0.0,
                                  'n_accurate': int(wr[2]), 'n_inaccurate': int(wr[3]) - int(wr[2]),
                                  'n_unobserved': int(n_recon) - int(wr[3]),
                                  'voxels_recon': int(wr[1]), 'voxels_gt': int(wg[1])})
    return out


def voxel_origin(*boxes):
    """The corner of voxel (0,0,0) both clouds share: the floor of the minimum over the (lo, hi) pairs of ops.cloud_bounds."""
    lows = [lo for lo, _ in boxes if lo is not None]
    return np.floor(np.min(lows, axis=0)) if lows else np.zeros(3)


def score(recon, gt, sizes, origins, d2_recon, d2_gt, tolerances, eth3d_voxel, cube_size, vis_window, free_space_margin):
    """recon (m,3) and gt (n,3): device tensors in one frame; gt is the scans one after the other, sizes their point counts, origins
    (S,3) host numbers; d2_recon (m,) / d2_gt (n,) of ops.cloud_nearest in both directions -> the `eth3d` dict."""
    import torch
    from .. import ops
    cams = np.concatenate([cube_cameras(o, cube_size) for o in origins], 0)
    cams_d = torch.from_numpy(cams).to(recon.device)
    ends = np.cumsum([0] + [int(k) for k in sizes])
    maps = torch.cat([ops.scan_render(gt[ends[k]:ends[k + 1]], cams_d[6 * k:6 * k + 6], cube_size, cube_size, PIXEL_CENTRE, 0)
                      for k in range(len(sizes))], 0)
    excess, _ = ops.cloud_scan_excess(recon, cams_d, maps, PIXEL_CENTRE, vis_window)
    org = voxel_origin(ops.cloud_bounds(recon), ops.cloud_bounds(gt))
    wr = ops.cloud_voxel_shares(recon, d2_recon, excess, eth3d_voxel, org, tolerances, free_space_margin).cpu().tolist()
    wg = ops.cloud_voxel_shares(gt, d2_gt, None, eth3d_voxel, org, tolerances, free_space_margin).cpu().tolist()
    params = {'voxel': eth3d_voxel, 'cube_size': cube_size, 'vis_window': vis_window, 'free_space_margin': free_space_margin,
              'n_scanners': len(sizes), 'scanner_origins': np.asarray(origins, np.float64).tolist()}
    return metrics(wr, wg, int(recon.shape[0]), tolerances, params)
