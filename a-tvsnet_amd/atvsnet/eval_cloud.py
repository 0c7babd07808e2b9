"""Score a reconstructed point cloud against a ground-truth cloud on the MI355X: accuracy, completeness and F-score at a set of
distance tolerances.

    python -m atvsnet_amd.atvsnet.eval_cloud --recon final3d_model.ply --gt scan1.ply [scan2.ply ...]
           [--tolerances 0.01,0.02,0.05,0.1,0.2,0.5] [--radius R] [--gt_transform T.txt] [--out cloud_eval.json] [--distances PREFIX]
           [--register [--with_scale] [--register_distances a,b,c] [--register_voxel v]
            [--register_icp plane [--register_normals target [--register_normal_k K] [--register_normal_radius R]]]
            [--register_global [--global_voxel V] [--global_hypotheses H] [--global_seed S] [--global_tau T] [--global_no_mutual]]]
           [--init_transform T.txt | --init_cameras RECON_SPARSE GT_SPARSE] [--save_transform T.txt] [--voxel v]
           [--eth3d (--gt_mlp scan_alignment.mlp | --scanner_origins origins.txt) [--eth3d_voxel 0.01] [--cube_size 1024]
            [--vis_window 1] [--free_space_margin 0]]
           [--sample_recon S [--exact_recon]] [--sample_gt S [--exact_gt]] [--sample_seed K]

The top-level keys are the PLAIN precision / recall definition (the one Tanks and Temples uses): per tolerance tau, `accuracy` is
the share of reconstruction points with a ground-truth point within tau, `completeness` the share of ground-truth points with a
reconstruction point within tau, `f1` their harmonic mean.

--eth3d adds the key `eth3d`: the same shares by ETH3D's published protocol, restated (atvsnet/eval_eth3d.py): formed per occupied
voxel of --eth3d_voxel and averaged over voxels, with a reconstruction point that has no ground truth within tau counted
inaccurate only where a laser scanner could have seen it (in front of what the scanner measured along that ray, or at most
--free_space_margin behind it) and left out as unobserved otherwise.  It needs each scan on its own and its scanner's position:
--gt_mlp (ETH3D's scan_alignment.mlp: the PLY files and their matrices, whose translation is the scanner's origin) replaces --gt,
or --gt a.ply b.ply with --scanner_origins (a text file, one `x y z` per scan, in the ground truth's frame after --gt_transform).
This is NOT ETH3D's official evaluation program and no run of that program pins it: it restates the published protocol.  What
still differs by construction: the beams' radius and divergence (a pixel window of a cube map stands in for them), windows that
stop at cube edges, and --cube_size, --vis_window, --free_space_margin, which are defaults chosen here, not measurements.  Compare
its numbers between runs of this tool; against the leaderboard they are an approximation of unknown size.

Both directions of the nearest-neighbour search run on the device (ops.cloud_grid / cloud_nearest / cloud_counts, csrc/cloud.hip),
exactly: per point the smallest float32 squared distance (dx*dx + dy*dy) + dz*dz to the other cloud, unknown (+inf) beyond
`radius`; a point counts at tau when double(d2) <= tau * tau.  There is no CPU fallback.  `metrics` is the pure-host part.

A reconstruction in another frame than the ground truth's (a COLMAP model: rotation, translation and scale are free) scores 0 as
it stands.  --register aligns it first (atvsnet/register_cloud.py: voxel down-sampling, trimmed point-to-point ICP in stages, on the
device), starting from --init_transform (a 4x4 matrix applied to the RECONSTRUCTION) or --init_cameras (the similarity between
the camera centres of two COLMAP models of the same images), or, with --register_global, from a start found from the clouds alone
(register_cloud.global_init: FPFH descriptors, exact matching in feature space and RANSAC over triples of matches, on the device --
for a cloud that comes without cameras in the ground truth's frame); --save_transform keeps the matrix found.  --register_icp plane
registers by point-to-plane ICP over the normals the reconstruction's PLY carries (depth_fusion --normals depth), or, with
--register_normals target, over the ground truth's, estimated on the GPU (the reconstruction then needs none).  --voxel scores the
voxel-down-sampled clouds (both sides), so that point density does not weight the shares.  Without these options the result is
what it was before they existed.

A triangle mesh given as --recon scores by its VERTICES: a simplified mesh then loses completeness by construction.  --sample_recon S
samples its surface uniformly by area at spacing S on the device first (atvsnet/sample_mesh.py: one sample per S x S, every number a
hash of --sample_seed, the face and the sample, so the same run gives the same score) and the samples are the reconstruction for
everything above; with --register_icp plane over the source's normals the samples' face normals serve.  --sample_gt S does the same
for every --gt file that is a mesh (a dataset whose ground truth is a surface).  The result gains `recon_mesh` (sample_mesh's report
without `seconds`) and / or `gt_mesh` (a list of such reports, one per sampled file, each with its `file`).  Samples turn a surface
back into points, and the half of the score measured AGAINST them inherits their spacing: a spacing of at most half the smallest
tolerance is what DESIGN.md section 10.3e supports for it.  --exact_recon (with --sample_recon) measures completeness against the
mesh itself instead: the exact point-to-triangle distance of every ground-truth point to the surface of --recon, on the device
(ops.mesh_grid / mesh_nearest, csrc/mesh_distance.hip), which no spacing enters; --exact_gt (with
--sample_gt, every --gt file a mesh) does the same for accuracy against the ground-truth surface.  The samples remain the points of
the other direction and of the registration.  The result gains `exact`.
"""
from __future__ import print_function

import argparse
import json
import os

import numpy as np

from ..tools import ply
from ..tools.common import write_json  # noqa: F401

DEFAULT_TOLERANCES = (0.01, 0.02, 0.05, 0.1, 0.2, 0.5)
NO_NORMALS = ('%s carries no normals (nx ny nz): point-to-plane registration needs the reconstruction\'s own; fuse it with '
              '`depth_fusion --normals depth`, or use --register_icp point, or --register_normals target (the planes of the ground '
              'truth, whose normals are estimated on the GPU)')


def _check_tolerances(tolerances, radius):
    tol = [float(t) for t in tolerances]
    if not 1 <= len(tol) <= 16:
        raise ValueError('1 to 16 tolerances, got %d' % len(tol))
    want = max(tol) if radius is None else float(radius)
    r32 = np.float32(want)
    if float(r32) < want:          # the kernels take a float32 radius: rounded UP, so that a tolerance equal to the radius stays inside
        r32 = np.nextafter(r32, np.float32(np.inf))
    radius = float(r32)
    if not (radius > 0.0 and np.isfinite(radius)):
        raise ValueError('radius must be positive and finite, got %r' % radius)
    for t in tol:
        if not 0.0 <= t <= radius:
            raise ValueError('tolerance %r outside [0, radius = %r]: distances beyond the radius are not known' % (t, radius))
    return tol, radius


def _f1(a, c):
    return 2.0 * a * c / (a + c) if a + c > 0.0 else 0.0


def _direction(d2, radius):
    """(not found within the radius, mean, median of min(d, radius)) of one direction's float32 d2, in float64 on the host."""
    d2 = np.asarray(d2, np.float32)
    if d2.size == 0:
        return 0, None, None
    d = np.minimum(np.sqrt(d2.astype(np.float64)), radius)
    return int(np.isinf(d2).sum()), float(d.mean()), float(np.median(d))


def metrics(d2_recon, d2_gt, tolerances, radius, counts=None):
    """The score from the two directions' float32 squared distances (+inf = nothing within `radius`): d2_recon per reconstruction
    point (to the ground truth), d2_gt per ground-truth point (to the reconstruction).  counts: None (counted here, in float64:
    double(d2) <= tau * tau) or (counts_recon, counts_gt) per tolerance as ops.cloud_counts returns them.  -> a dict of plain
    Python numbers (JSON as it stands); shares of an empty cloud are 0, its mean / median None."""
    tol, radius = _check_tolerances(tolerances, radius)
    d2_recon, d2_gt = np.asarray(d2_recon, np.float32).reshape(-1), np.asarray(d2_gt, np.float32).reshape(-1)
    if counts is None:
        counts = [[int((d2.astype(np.float64) <= t * t).sum()) for t in tol] for d2 in (d2_recon, d2_gt)]
    out = {'n_recon': int(d2_recon.size), 'n_gt': int(d2_gt.size), 'radius': radius, 'tolerances': []}
    for name, d2 in (('recon', d2_recon), ('gt', d2_gt)):
        out['not_found_' + name], out['mean_' + name], out['median_' + name] = _direction(d2, radius)
    for k, t in enumerate(tol):
        a = int(counts[0][k]) / float(d2_recon.size) if d2_recon.size else 0.0
        c = int(counts[1][k]) / float(d2_gt.size) if d2_gt.size else 0.0
        out['tolerances'].append({'tolerance': t, 'accuracy': a, 'completeness': c, 'f1': _f1(a, c),
                                  'n_recon_within': int(counts[0][k]), 'n_gt_within': int(counts[1][k])})
    return out


def transform_points(points, matrix):
    """points (M,3) through a 4x4 matrix (rotation / scale / translation rows 0-2; row 3 ignored) in float64, rounded once."""
    T = np.asarray(matrix, np.float64).reshape(4, 4)
    p = np.asarray(points).astype(np.float64)
    return (p @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


def _matrix(T, name):
    T = np.asarray(T, np.float64)
    if T.size != 16 or not np.isfinite(T).all():
        raise ValueError('%s: expected the 16 finite numbers of a 4x4 matrix' % name)
    return T.reshape(4, 4)


def _surface(surface, name):
    """None, or the (vertices (V,3), faces (F,3)) of evaluate's recon_surface / gt_surface; anything else raises ValueError."""
    if surface is None:
        return None
    if not isinstance(surface, (tuple, list)) or len(surface) != 2:
        raise ValueError('%s: expected (vertices (V,3), faces (F,3)), got %s' % (name, type(surface).__name__))
    for part, what in zip(surface, ('vertices', 'faces')):
        shape = tuple(getattr(part, 'shape', ()))
        if len(shape) != 2 or shape[1] != 3:
            raise ValueError('%s: %s: expected shape (n,3), got %s' % (name, what, shape))
    return tuple(surface)


def evaluate(recon, gt, tolerances=DEFAULT_TOLERANCES, radius=None, gt_transform=None, device=None, distances=None,
             register=False, with_scale=False, register_distances=None, register_voxel=None, init_transform=None, voxel=None,
             scans=None, scanner_origins=None, eth3d_voxel=0.01, cube_size=1024, vis_window=1, free_space_margin=0.0,
             register_icp='point', recon_normals=None, register_normals='source', register_normal_k=None,
             register_normal_radius=None, register_global=False, global_options=None, recon_surface=None, gt_surface=None):
    """recon (M,3), gt (N,3): host arrays (or device tensors) of float32 points -> the dict of `metrics`.  radius: the search
    radius, default the largest tolerance.  gt_transform: a 4x4 matrix applied to `gt` on the host (float64, rounded once).
    distances: a dict that receives d2_recon, idx_recon, d2_gt, idx_gt as numpy arrays.

    The rest changes nothing when left at its default.  init_transform: a 4x4 matrix applied to `recon` (on the device,
    ops.cloud_transform).  register: align `recon` to `gt` by register_cloud.register before scoring, starting from
    init_transform; with_scale, register_distances (default 4x, 2x, 1x the largest tolerance), register_voxel are its arguments;
    the result gains `registration` (its dict; `matrix` includes init_transform).  register_icp = 'plane' registers by
    point-to-plane ICP over recon_normals (M,3), the reconstruction's own normals, one per row of `recon`; with
    register_normals = 'target' over the ground truth's instead, estimated on the device from register_normal_k neighbours
    within register_normal_radius (register_cloud.register's normal_side, normal_k, normal_radius and their defaults), and
    recon_normals is not used.  register_global: the start is found from the clouds alone (register_cloud.global_init: FPFH
    matching and RANSAC on the device; global_options: its keyword arguments) instead of init_transform, which is then an argument
    error; `registration` gains `global`.  Without register,
    init_transform is recorded as `init_transform`.  voxel: both clouds are scored after ops.cloud_voxel_downsample with this edge (after the alignment); the
    result gains `voxel`, `n_recon_full`, `n_gt_full`, and the distances refer to the down-sampled clouds.

    scans: the ground truth as a list of (n_i,3) arrays, one per laser scan, with scanner_origins (S,3), each scanner's position
    in the scans' frame (after gt_transform); `gt` must then be None and is their concatenation.  The result gains `eth3d`
    (atvsnet/eval_eth3d.py): the parameters and per tolerance accuracy, completeness, f1 averaged over voxels of eth3d_voxel,
    n_accurate, n_inaccurate, n_unobserved (reconstruction points by class) and voxels_recon, voxels_gt (voxels counted).  Every
    scanner's own points are rendered into a cube map of 6 x cube_size^2 pixels; a reconstruction point is looked up in a
    (2 vis_window + 1)^2 window and is unobserved when it lies more than free_space_margin behind the nearest sample there.
    eth3d_voxel = 0.01 and the default tolerances are ETH3D's published ones; cube_size, vis_window and free_space_margin are
    defaults, not measurements of ETH3D's program.  With `voxel` it is an argument error: down-sampling loses which scanner saw a
    point.  Every other key is what it is without scans.

    recon_surface, gt_surface: None, or (vertices (V,3) float32, faces (F,3) int32) as host arrays or device tensors: the triangle
    mesh that `recon` / `gt` are points of.  With gt_surface the reconstruction's distances (d2_recon, accuracy) are the EXACT
    point-to-triangle distances to that surface (ops.mesh_grid / mesh_nearest, csrc/mesh_distance.hip) instead of the distances
    to the nearest point of `gt`; with recon_surface the ground truth's distances (d2_gt, completeness) are those to the
    reconstruction's surface.  recon_surface's vertices are moved by the matrix `recon` is moved by (init_transform or the
    registration's, ops.cloud_transform), gt_surface's by gt_transform; voxel down-samples the points and leaves the surfaces
    alone; `eth3d` receives the new distances in the form of the old.  The distances' idx_* then hold face indices.  The result
    gains `exact`: accuracy and completeness (whether that direction ran against a surface) and gt_surface_faces,
    recon_surface_faces (the usable faces, None without the surface)."""
    import torch
    from .. import ops
    tol, radius = _check_tolerances(tolerances, radius)
    recon_surface, gt_surface = _surface(recon_surface, 'recon_surface'), _surface(gt_surface, 'gt_surface')
    if gt_surface is not None and gt_transform is not None:
        moved = gt_surface[0].cpu().numpy() if isinstance(gt_surface[0], torch.Tensor) else gt_surface[0]
        gt_surface = (transform_points(moved, gt_transform), gt_surface[1])
    if register_icp not in ('point', 'plane'):
        raise ValueError("register_icp must be 'point' or 'plane', got %r" % (register_icp,))
    if register_icp == 'plane' and not register:
        raise ValueError("register_icp='plane' needs register=True")
    if register_normals not in ('source', 'target'):
        raise ValueError("register_normals must be 'source' or 'target', got %r" % (register_normals,))
    target = register_normals == 'target'
    if target and register_icp != 'plane':
        raise ValueError("register_normals='target' needs register_icp='plane'")
    if not target and (register_normal_k is not None or register_normal_radius is not None):
        raise ValueError("register_normal_k and register_normal_radius need register_normals='target'")
    if target and recon_normals is not None:
        raise ValueError("register_normals='target' runs over the ground truth's normals: recon_normals is not used")
    if (register_icp == 'plane' and not target) != (recon_normals is not None):
        raise ValueError("register_icp='plane' and recon_normals go together: the reconstruction's normals, one per point")
    if (register_global or global_options is not None) and not register:
        raise ValueError('register_global and global_options need register=True')
    if global_options is not None and not register_global:
        raise ValueError('global_options need register_global=True')
    if register_global and init_transform is not None:
        raise ValueError('register_global finds the starting matrix itself: init_transform is not used')
    plane = {'icp': 'plane', 'normals': recon_normals} if register_icp == 'plane' else {}
    if target:
        plane = {'icp': 'plane', 'normal_side': 'target'}
        if register_normal_k is not None:
            plane['normal_k'] = register_normal_k
        if register_normal_radius is not None:
            plane['normal_radius'] = register_normal_radius
    origins = None
    if scans is not None:
        from . import eval_eth3d
        if gt is not None:
            raise ValueError('scans is the ground truth, one array per scan: gt must be None')
        if voxel is not None:
            raise ValueError('scans with voxel: the down-sampling loses which scanner saw a point (eth3d_voxel is the grid of the '
                             'voxel-averaged shares)')
        scans = [s.cpu().numpy() if isinstance(s, torch.Tensor) else s for s in scans]
        scans = [np.ascontiguousarray(np.asarray(s, np.float32).reshape(-1, 3)) for s in scans]
        origins = eval_eth3d.check_scans(scans, scanner_origins)
        eth3d_args = eval_eth3d.check_options(eth3d_voxel, cube_size, vis_window, free_space_margin)
        if gt_transform is not None:
            scans = [transform_points(s, gt_transform) for s in scans]
            gt_transform = None
        gt = np.concatenate(scans, 0)
    elif scanner_origins is not None:
        raise ValueError('scanner_origins needs scans')
    elif gt is None:
        raise ValueError('gt: the ground truth is missing (or give scans)')
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)

    def upload(x):
        if isinstance(x, torch.Tensor):
            return x.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1, 3))).to(dev)

    def upload_faces(x):
        if isinstance(x, torch.Tensor):
            return x.to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous()
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.int32).reshape(-1, 3))).to(dev)

    if gt_transform is not None:
        gt = transform_points(gt.cpu().numpy() if isinstance(gt, torch.Tensor) else gt, gt_transform)
    if not register and (with_scale or register_distances is not None or register_voxel is not None):
        raise ValueError('with_scale, register_distances and register_voxel need register=True')
    if voxel is not None and not (float(voxel) > 0.0 and np.isfinite(float(voxel))):
        raise ValueError('voxel must be positive and finite, got %r' % (voxel,))
    init = None if init_transform is None else _matrix(init_transform, 'init_transform')
    extra = {}
    with torch.cuda.device(dev):
        r, g = upload(recon), upload(gt)
        surface_r, surface_g = (None if m is None else (upload(m[0]), upload_faces(m[1])) for m in (recon_surface, gt_surface))
        if register:
            from . import register_cloud
            dist = [4.0 * max(tol), 2.0 * max(tol), max(tol)] if register_distances is None else list(register_distances)
            if register_global:
                plane = dict(plane, global_options=global_options)
            extra['registration'] = register_cloud.register(r, g, init='global' if register_global else init, with_scale=with_scale,
                                                            distances=dist, voxel=register_voxel, device=dev, **plane)
            r = ops.cloud_transform(r, extra['registration']['matrix'])
            if surface_r is not None:
                surface_r = (ops.cloud_transform(surface_r[0], extra['registration']['matrix']), surface_r[1])
        elif init is not None:
            extra['init_transform'] = init.tolist()
            r = ops.cloud_transform(r, init)
            if surface_r is not None:
                surface_r = (ops.cloud_transform(surface_r[0], init), surface_r[1])
        if voxel is not None:
            extra.update(voxel=float(voxel), n_recon_full=int(r.shape[0]), n_gt_full=int(g.shape[0]))
            r, g = ops.cloud_voxel_downsample(r, voxel)[0], ops.cloud_voxel_downsample(g, voxel)[0]
        if surface_g is None:
            d2_r, idx_r = ops.cloud_nearest(ops.cloud_grid(g, radius), r)
        else:
            grid_g = ops.mesh_grid(surface_g[0], surface_g[1], radius)
            d2_r, idx_r = ops.mesh_nearest(grid_g, r)
        if surface_r is None:
            d2_g, idx_g = ops.cloud_nearest(ops.cloud_grid(r, radius), g)
        else:
            grid_r = ops.mesh_grid(surface_r[0], surface_r[1], radius)
            d2_g, idx_g = ops.mesh_nearest(grid_r, g)
        if surface_r is not None or surface_g is not None:
            extra['exact'] = {'accuracy': surface_g is not None, 'completeness': surface_r is not None,
                              'gt_surface_faces': None if surface_g is None else grid_g.usable_faces,
                              'recon_surface_faces': None if surface_r is None else grid_r.usable_faces}
        counts = [ops.cloud_counts(d2, tol, radius).cpu().tolist() for d2 in (d2_r, d2_g)]
        if origins is not None:
            extra['eth3d'] = eval_eth3d.score(r, g, [len(s) for s in scans], origins, d2_r, d2_g, tol, *eth3d_args)
        d2_r, d2_g = d2_r.cpu().numpy(), d2_g.cpu().numpy()
        if distances is not None:
            distances.update(d2_recon=d2_r, idx_recon=idx_r.cpu().numpy(), d2_gt=d2_g, idx_gt=idx_g.cpu().numpy())
    result = metrics(d2_r, d2_g, tol, radius, counts=counts)
    result.update(extra)
    return result


def load_matrix(path):
    """A text file of 16 numbers -> the 4x4 matrix, row-major."""
    T = np.loadtxt(path, dtype=np.float64)
    if T.size != 16:
        raise ValueError('%s: expected the 16 numbers of a 4x4 matrix, got %d' % (path, T.size))
    return T.reshape(4, 4)


def save_matrix(path, T):
    """The 4x4 matrix as text that load_matrix reads back exactly (17 significant digits)."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savetxt(path, np.asarray(T, np.float64).reshape(4, 4), fmt='%.17g')


def mesh_faces(path):
    """The number of faces the header of a PLY file declares (0 without a `face` element); a file without a PLY header raises
    ValueError.  Only the header is read."""
    with open(path, 'rb') as f:
        if f.readline().strip() != b'ply':
            raise ValueError('%s: not a PLY file (no "ply" magic)' % path)
        for _ in range(4096):
            raw = f.readline()
            if not raw:
                break
            words = raw.decode('ascii', 'replace').split()
            if words[:1] == ['end_header']:
                return 0
            if words[:2] == ['element', 'face'] and len(words) == 3 and words[2].isdigit():
                return int(words[2])
    raise ValueError('%s: the header has no end_header' % path)


def _spacing(value, name):
    if isinstance(value, (bool, str, bytes)) or not (float(value) > 0.0 and np.isfinite(float(value))):
        raise ValueError('%s must be a positive finite spacing, got %r' % (name, value))
    return float(value)


def sample_file(path, spacing, seed=0, normals=False, name='sample_recon'):
    """The triangle mesh in `path` sampled at `spacing` on the current device -> (ops.MeshSamples on the device, sample_mesh's report
    without `seconds`).  A file without faces, or with other polygons than triangles, raises ValueError."""
    from . import sample_mesh
    from .clean_mesh import read_mesh
    import torch
    if not mesh_faces(path):
        raise ValueError('%s: %s has no faces: the option needs a triangle mesh' % (name, path))
    vertices, colors, faces = read_mesh(path)
    dev = torch.device('cuda', torch.cuda.current_device())
    v = torch.from_numpy(np.ascontiguousarray(vertices, np.float32)).to(dev)
    f = torch.from_numpy(np.ascontiguousarray(faces, np.int32)).to(dev)
    samples, report = sample_mesh.sample_device(v, None, f, spacing=spacing, seed=seed, normals=normals)
    report = {k: report[k] for k in sample_mesh.REPORT_KEYS if k != 'seconds'}
    return samples, report


def read_surfaces(paths):
    """The triangle meshes of `paths` as one (vertices (V,3) float32, faces (F,3) int32): concatenated, the indices offset."""
    from .clean_mesh import read_mesh
    vertices, faces, first = [], [], 0
    for path in paths:
        v, _, f = read_mesh(path)
        vertices.append(np.asarray(v, np.float32).reshape(-1, 3))
        faces.append(np.asarray(f, np.int64).reshape(-1, 3) + first)
        first += len(vertices[-1])
    return np.ascontiguousarray(np.concatenate(vertices)), np.ascontiguousarray(np.concatenate(faces).astype(np.int32))


def evaluate_files(recon_path, gt_paths, tolerances=DEFAULT_TOLERANCES, radius=None, gt_transform_path=None, distances=None,
                   init_transform_path=None, init_cameras=None, save_transform_path=None, gt_mlp_path=None,
                   scanner_origins_path=None, sample_recon=None, sample_gt=None, sample_seed=None, exact_recon=False, exact_gt=False,
                   **options):
    """`evaluate` of PLY files (tools/ply.read_ply_points): several ground-truth files are concatenated; gt_transform_path: a text
    file of 16 numbers, the 4x4 matrix row-major.  init_transform_path: the same for evaluate's init_transform; init_cameras:
    (recon_sparse_dir, gt_sparse_dir), two COLMAP models whose camera centres give it (register_cloud.init_from_cameras; the
    result's `registration` / top level gains `init_cameras`: matched images and their rms).  save_transform_path: the matrix that
    was applied to the reconstruction is written there.  options: evaluate's other keyword arguments; with register_icp='plane'
    the reconstruction's normals are read from its PLY (tools/ply.read_ply_normals; a file without them raises), unless
    register_normals='target': then the plain reader is used and no normals are needed.

    The ETH3D-style score (evaluate's `scans`): gt_mlp_path, a MeshLab project (eval_eth3d.read_mlp) that replaces gt_paths -- each
    scan is moved by gt_transform times its own matrix (float64, rounded once) and that product's translation is its scanner's
    origin -- or gt_paths with scanner_origins_path, a text file of one `x y z` per scan in the frame after gt_transform.

    sample_recon: recon_path is a triangle mesh whose surface is sampled at this spacing on the device first (sample_file), with
    sample_seed (default 0); the samples are the reconstruction for everything else, their face normals the recon_normals of
    register_icp='plane'; the result gains `recon_mesh`.  sample_gt: the same for every file of gt_paths that has faces (at least one
    must); the result gains `gt_mesh`, a list.  A file that is no triangle mesh, or sample_seed without either, raises ValueError.

    exact_recon (needs sample_recon): the samples stay the reconstruction's points for accuracy and registration, and the mesh of
    recon_path itself answers completeness: it is evaluate's recon_surface.  exact_gt (needs sample_gt, every file of gt_paths a
    triangle mesh, no gt_mlp_path): the ground-truth meshes, concatenated with offset indices, are evaluate's gt_surface, which
    answers accuracy.  The result gains `exact`."""
    if sample_seed is not None and sample_recon is None and sample_gt is None:
        raise ValueError('sample_seed needs sample_recon or sample_gt')
    if exact_recon and sample_recon is None:
        raise ValueError('exact_recon needs sample_recon: the samples remain the reconstruction\'s points for accuracy and registration')
    if exact_gt:
        if gt_mlp_path is not None:
            raise ValueError('exact_gt with gt_mlp_path: a MeshLab project names laser scans, not meshes')
        if sample_gt is None:
            raise ValueError('exact_gt needs sample_gt: the samples remain the ground truth\'s points for completeness')
        without = [str(p) for p in gt_paths if not mesh_faces(p)]
        if without or not gt_paths:
            raise ValueError('exact_gt: every ground-truth file must be a triangle mesh, %s' % (
                '%s has no faces' % without[0] if without else 'none is given'))
    seed = 0 if sample_seed is None else sample_seed
    sampled = {}
    plane_source = options.get('register_icp') == 'plane' and options.get('register_normals', 'source') != 'target'
    if sample_gt is not None:
        sample_gt = _spacing(sample_gt, 'sample_gt')
        if gt_mlp_path is not None:
            raise ValueError('sample_gt with gt_mlp_path: a MeshLab project names laser scans, not meshes')
        if not any(mesh_faces(p) for p in gt_paths):
            raise ValueError('sample_gt: none of the ground-truth files is a triangle mesh')
        sampled['gt_mesh'] = []

    def read_gt(path):
        if sample_gt is None or not mesh_faces(path):
            return ply.read_ply_points(path)
        samples, report = sample_file(path, sample_gt, seed, name='sample_gt')
        sampled['gt_mesh'].append(dict(report, file=str(path)))
        return samples.points.cpu().numpy()

    if exact_gt:
        options['gt_surface'] = read_surfaces(gt_paths)
    if sample_recon is not None:
        samples, sampled['recon_mesh'] = sample_file(recon_path, _spacing(sample_recon, 'sample_recon'), seed, normals=plane_source)
        recon = samples.points
        if exact_recon:
            options['recon_surface'] = read_surfaces([recon_path])
        if plane_source:
            options['recon_normals'] = samples.normals.cpu().numpy()
    elif plane_source:
        if not ply.has_normals(recon_path):
            raise ValueError(NO_NORMALS % recon_path)
        recon, _, options['recon_normals'] = ply.read_ply_normals(recon_path)
    else:
        recon = ply.read_ply_points(recon_path)
    T = None
    if gt_transform_path is not None:
        T = np.loadtxt(gt_transform_path, dtype=np.float64)
        if T.size != 16:
            raise ValueError('%s: expected the 16 numbers of a 4x4 matrix, got %d' % (gt_transform_path, T.size))
    if gt_mlp_path is not None or scanner_origins_path is not None:
        from . import eval_eth3d
        if gt_mlp_path is not None and (gt_paths or scanner_origins_path is not None):
            raise ValueError('gt_mlp_path names the scans and their scanners: give neither gt_paths nor scanner_origins_path with it')
        if gt_mlp_path is not None:
            G = np.eye(4) if T is None else _matrix(T, gt_transform_path)
            moves = [(p, G @ M) for p, M in eval_eth3d.read_mlp(gt_mlp_path)]
            options['scans'] = [transform_points(ply.read_ply_points(p), M) for p, M in moves]
            options['scanner_origins'] = np.array([M[:3, 3] for _, M in moves])
            T = None
        else:
            options['scans'] = [read_gt(p) for p in gt_paths]
            options['scanner_origins'] = eval_eth3d.load_origins(scanner_origins_path)
        gt = None
    else:
        gt = [read_gt(p) for p in gt_paths]
        gt = np.concatenate(gt, 0) if gt else np.zeros((0, 3), np.float32)
    init, cams = None, None
    if init_transform_path is not None and init_cameras is not None:
        raise ValueError('init_transform_path and init_cameras both give the starting matrix: choose one')
    if init_transform_path is not None:
        init = load_matrix(init_transform_path)
    elif init_cameras is not None:
        from . import register_cloud
        init, matched, rms = register_cloud.init_from_cameras(*init_cameras)
        cams = {'recon_sparse': str(init_cameras[0]), 'gt_sparse': str(init_cameras[1]), 'matched_images': matched, 'rms': rms}
    if init is None and not options and save_transform_path is None:
        result = evaluate(recon, gt, tolerances, radius, gt_transform=T, distances=distances)
        result.update(sampled)
        return result
    result = evaluate(recon, gt, tolerances, radius, gt_transform=T, distances=distances, init_transform=init, **options)
    result.update(sampled)
    if cams is not None:
        result['init_cameras'] = cams
    if save_transform_path is not None:
        applied = result['registration']['matrix'] if 'registration' in result else init
        if applied is None:
            raise ValueError('save_transform_path: no matrix was applied to the reconstruction (give register or an initial matrix)')
        save_matrix(save_transform_path, applied)
    return result


GLOBAL_FLAGS = {'global_voxel': 'feature_voxel', 'global_hypotheses': 'hypotheses', 'global_seed': 'seed', 'global_tau': 'tau',
                'global_no_mutual': 'mutual'}                      # command-line option -> register_cloud.global_init's argument


def add_register_arguments(parser):
    """--register and the registration options this command line and eval_pointcloud's share."""
    parser.add_argument('--register', action='store_true',
                        help='align the reconstruction to the ground truth before scoring (voxel down-sampling + ICP in stages)')
    parser.add_argument('--with_scale', action='store_true', help='--register: fit a similarity (scale too), not a rigid motion')
    parser.add_argument('--register_icp', default=None, choices=('point', 'plane'),
                        help='--register: point-to-point ICP (the default) or point-to-plane over the normals the reconstruction carries (nx ny nz '
                             'in its PLY, as `depth_fusion --normals depth` writes them; eval_pointcloud: --fuse_normals depth): far fewer iterations')
    parser.add_argument('--register_normals', default=None, choices=('source', 'target'),
                        help='--register_icp plane: whose planes -- source (the default: the reconstruction\'s own normals) or '
                             'target (the ground truth\'s, estimated on the GPU: the reconstruction needs none)')
    parser.add_argument('--register_normal_k', type=int, default=None, metavar='K',
                        help='--register_normals target: neighbours per estimated normal, 2..32 (default 16; a default, not a measurement)')
    parser.add_argument('--register_normal_radius', type=float, default=None, metavar='R',
                        help='--register_normals target: their search radius (default: 4 edges of the registration\'s voxel, or twice '
                             'the last distance without one; a default, not a measurement)')
    parser.add_argument('--init_cameras', default=None, nargs=2, metavar=('RECON_SPARSE', 'GT_SPARSE'),
                        help='two COLMAP sparse model folders of the same images, in the reconstruction\'s and the ground truth\'s '
                             'frame: the similarity between their camera centres (matched by image name) is the initial matrix')
    parser.add_argument('--register_global', action='store_true',
                        help='--register: find the starting matrix from the clouds alone (FPFH descriptors matched in feature space, '
                             'RANSAC over triples of matches, on the GPU) instead of --init_transform / --init_cameras')
    parser.add_argument('--global_voxel', type=float, default=None, metavar='V',
                        help='--register_global: voxel edge of the clouds the descriptors are computed on (default: twice the '
                             'registration\'s voxel; with --with_scale 1/64 of each cloud\'s bounding-box diagonal; defaults, not '
                             'measurements)')
    parser.add_argument('--global_hypotheses', type=int, default=None, metavar='H',
                        help='--register_global: triples of matches tried (default 65536; a default, not a measurement)')
    parser.add_argument('--global_seed', type=int, default=None, metavar='S',
                        help='--register_global: seed of the triples (default 0): the same seed gives the same matrix')
    parser.add_argument('--global_tau', type=float, default=None, metavar='T',
                        help='--register_global: a match agrees with a hypothesis within this distance, in the ground truth\'s units '
                             '(default: 1.5 feature voxels; a default, not a measurement)')
    parser.add_argument('--global_no_mutual', action='store_true',
                        help='--register_global: keep every source-to-target match, not only those the target matches back')


def check_register_values(parser, args, need_register=('register_global',)):
    """The argument errors this command line and eval_pointcloud's share: an option of `need_register` or of --register_global's without
    its switch; --global_hypotheses, --global_seed, --register_normal_k or --register_normal_radius out of range."""
    for name in need_register:
        if getattr(args, name) not in (None, False) and not args.register:
            parser.error('--%s needs --register' % name)
    for name in GLOBAL_FLAGS:
        if getattr(args, name) not in (None, False) and not args.register_global:
            parser.error('--%s needs --register_global' % name)
    if args.global_hypotheses is not None and not 1 <= args.global_hypotheses <= 1 << 24:
        parser.error('--global_hypotheses must be in 1..2^24')
    if args.global_seed is not None and args.global_seed < 0:
        parser.error('--global_seed must be >= 0')
    if args.register_normal_k is not None and not 2 <= args.register_normal_k <= 32:
        parser.error('--register_normal_k must be in 2..32')
    if args.register_normal_radius is not None and not (args.register_normal_radius > 0.0 and np.isfinite(args.register_normal_radius)):
        parser.error('--register_normal_radius must be positive and finite')


def global_options(args):
    """register_cloud.global_init's keyword arguments that a command line gives ({}: its defaults); None without --register_global.
    An option `args` lacks is not given."""
    if not getattr(args, 'register_global', False):
        return None
    chosen = {key: getattr(args, name) for name, key in GLOBAL_FLAGS.items() if getattr(args, name, None) not in (None, False)}
    if 'mutual' in chosen:
        chosen['mutual'] = False
    return chosen


def register_arguments(with_scale=False, icp=None, normal_side=None, normal_k=None, normal_radius=None, global_=None, **_others):
    """evaluate's keyword arguments of a registration: register, with_scale, register_icp ('plane' only), register_normals ('target'
    only, with register_normal_k and register_normal_radius when given), register_global and global_options (global_: None, or
    global_options' dict).  The arguments are the keys of the ETH3D driver's register dict (with gt_ply only), which is None, or
    dict(with_scale=, init_cameras=(recon_sparse, gt_sparse) or None): the cloud is aligned to the ground truth before it is scored
    (--register [--init_cameras]); cloud_eval.json carries `registration`.  With icp='plane' (fuse_normals normals='depth' only) the
    registration is point-to-plane over the normals the fusion returns; with normal_side='target' too (optionally normal_k,
    normal_radius) over the ground truth's planes instead, its normals estimated on the device: no fuse_normals needed.  With global=
    ({} or register_cloud.global_init's keyword arguments) the start is found from the clouds alone; init_cameras is then refused."""
    out = dict(register=True, with_scale=bool(with_scale))
    if icp == 'plane':
        out['register_icp'] = 'plane'
    if normal_side == 'target':
        out['register_normals'] = 'target'
        out.update({'register_' + key: v for key, v in (('normal_k', normal_k), ('normal_radius', normal_radius)) if v is not None})
    if global_ is not None:
        out['register_global'] = True
        out.update({'global_options': dict(global_)} if global_ else {})
    return out


def register_rules(register, fused_normals):
    """The ETH3D driver's rules for its register dict, as (broken, message) rows: those of the target normals, of point-to-plane over
    the fused cloud's own normals (fused_normals: whether the fusion estimates them) and of global=, each only when the dict asks."""
    register = register or {}
    target = register.get('normal_side') == 'target'
    plane_row = [] if not register.get('icp') == 'plane' or target else [
        (not fused_normals, '--register_icp plane needs --fuse_normals depth (register icp=plane needs fuse_normals normals=depth): '
                            'point-to-plane registration runs over the fused cloud\'s own normals; or give --register_normals target '
                            '(register normal_side=target): the ground truth\'s planes, its normals estimated on the GPU')]
    target_row = [] if not any(k in register for k in ('normal_side', 'normal_k', 'normal_radius')) else [
        (target and not register.get('icp') == 'plane', '--register_normals target needs --register_icp plane (register '
                                                        'normal_side=target needs icp=plane)'),
        (not target and ('normal_k' in register or 'normal_radius' in register),
         '--register_normal_k and --register_normal_radius need --register_normals target (normal_k and normal_radius need '
         'normal_side=target)')]
    global_row = [] if register.get('global') is None else [
        (bool(register.get('init_cameras')), '--register_global finds the initial matrix from the clouds alone: give it or '
                                             '--init_cameras (register global= or init_cameras=)')]
    return target_row + plane_row + global_row


def register_options(parser, args):
    """The registration options of a parsed command line as evaluate_files' keyword arguments ({} when none is given);
    contradictory ones are argument errors."""
    if args.init_transform and args.init_cameras:
        parser.error('--init_transform and --init_cameras both give the initial matrix: choose one')
    check_register_values(parser, args, ('with_scale', 'register_distances', 'register_voxel', 'register_icp', 'register_normals',
                                         'register_normal_k', 'register_normal_radius', 'register_global'))
    if args.register_global and (args.init_transform or args.init_cameras):
        parser.error('--register_global finds the initial matrix from the clouds alone: give it, --init_transform or --init_cameras')
    if args.global_voxel is not None and not (args.global_voxel > 0.0 and np.isfinite(args.global_voxel)):
        parser.error('--global_voxel must be positive and finite')
    if args.global_tau is not None and not (args.global_tau > 0.0 and np.isfinite(args.global_tau)):
        parser.error('--global_tau must be positive and finite')
    if args.save_transform and not (args.register or args.init_transform or args.init_cameras):
        parser.error('--save_transform needs --register, --init_transform or --init_cameras: no matrix is applied otherwise')
    if args.voxel is not None and not args.voxel > 0.0:
        parser.error('--voxel must be positive')
    target = args.register_normals == 'target'
    if target and args.register_icp != 'plane':
        parser.error('--register_normals target needs --register_icp plane')
    if not target and (args.register_normal_k is not None or args.register_normal_radius is not None):
        parser.error('--register_normal_k and --register_normal_radius need --register_normals target')
    options = {}
    if args.register:
        if args.register_distances is not None:
            try:
                options['register_distances'] = [float(t) for t in args.register_distances.split(',') if t.strip()]
            except ValueError:
                parser.error('--register_distances: expected comma-separated numbers, got %r' % args.register_distances)
            d = options['register_distances']
            if not d or any(not v > 0.0 for v in d) or any(b >= a for a, b in zip(d, d[1:])):
                parser.error('--register_distances must be positive and decreasing')
        if args.register_voxel is not None:
            if not args.register_voxel >= 0.0:
                parser.error('--register_voxel must be >= 0')
            options['register_voxel'] = args.register_voxel
        if args.register_icp == 'plane' and not target and getattr(args, 'sample_recon', None) is None:
            try:
                with_normals = ply.has_normals(args.recon)
            except (OSError, ValueError) as e:
                parser.error('--register_icp plane: cannot read %s: %s' % (args.recon, e))
            if not with_normals:
                parser.error('--register_icp plane: ' + NO_NORMALS % args.recon)
        options.update(register_arguments(args.with_scale, args.register_icp, args.register_normals, args.register_normal_k,
                                          args.register_normal_radius, global_options(args)))
    if args.init_transform:
        options['init_transform_path'] = args.init_transform
    if args.init_cameras:
        options['init_cameras'] = tuple(args.init_cameras)
    if args.save_transform:
        options['save_transform_path'] = args.save_transform
    if args.voxel is not None:
        options['voxel'] = args.voxel
    return options


def eth3d_options(parser, args):
    """The --eth3d options of a parsed command line as evaluate_files' keyword arguments ({} without --eth3d)."""
    given = [n for n in ('eth3d_voxel', 'cube_size', 'vis_window', 'free_space_margin') if getattr(args, n) is not None]
    if not args.eth3d:
        for name in given + [n for n in ('gt_mlp', 'scanner_origins') if getattr(args, n)]:
            parser.error('--%s needs --eth3d' % name)
        if not args.gt:
            parser.error('--gt is required (or --eth3d --gt_mlp)')
        return {}
    if not args.gt_mlp and not args.scanner_origins:
        parser.error('--eth3d needs the scanners\' positions: --gt_mlp FILE (a MeshLab project, replaces --gt) or '
                     '--gt a.ply b.ply with --scanner_origins FILE')
    if args.gt_mlp and (args.gt or args.scanner_origins):
        parser.error('--gt_mlp replaces --gt and --scanner_origins: give it alone')
    if args.scanner_origins and not args.gt:
        parser.error('--scanner_origins needs --gt: one PLY file per scan')
    if args.voxel is not None:
        parser.error('--eth3d with --voxel: the down-sampling loses which scanner saw a point (--eth3d_voxel is the grid of the '
                     'voxel-averaged shares)')
    options = {name: getattr(args, name) for name in given}
    if args.gt_mlp:
        options['gt_mlp_path'] = args.gt_mlp
    else:
        options['scanner_origins_path'] = args.scanner_origins
    from . import eval_eth3d
    try:
        eval_eth3d.check_options(options.get('eth3d_voxel', 0.01), options.get('cube_size', 1024), options.get('vis_window', 1),
                                 options.get('free_space_margin', 0.0))
    except ValueError as e:
        parser.error(str(e))
    return options


def make_parser():
    parser = argparse.ArgumentParser(description='accuracy / completeness / F-score of a point cloud against ground truth '
                                                 '(plain precision / recall; --eth3d adds ETH3D\'s published protocol restated: '
                                                 'voxel-averaged shares and scanner free space -- not the official ETH3D program)')
    parser.add_argument('--recon', required=True, help='the reconstruction (PLY)')
    parser.add_argument('--gt', default=None, nargs='+', help='ground-truth PLY file(s), concatenated (required unless --gt_mlp)')
    parser.add_argument('--tolerances', default=','.join(str(t) for t in DEFAULT_TOLERANCES), help='comma-separated distances')
    parser.add_argument('--radius', type=float, default=None, help='search radius (default: the largest tolerance)')
    parser.add_argument('--gt_transform', default=None, help='text file with a 4x4 row-major matrix applied to the ground truth')
    parser.add_argument('--out', default=None, help='write the result as JSON here (default: print it)')
    parser.add_argument('--distances', default=None, metavar='PREFIX',
                        help='write PREFIX_d2_recon.npy, PREFIX_idx_recon.npy, PREFIX_d2_gt.npy, PREFIX_idx_gt.npy')
    parser.add_argument('--gpu_id', type=int, default=0)
    add_register_arguments(parser)
    parser.add_argument('--register_distances', default=None, metavar='a,b,c',
                        help='--register: the stages\' search distances, decreasing (default: 4, 2, 1 x the largest tolerance)')
    parser.add_argument('--register_voxel', type=float, default=None, metavar='V',
                        help='--register: voxel edge of the down-sampling before the fit (default: half the last distance; 0: none)')
    parser.add_argument('--init_transform', default=None, metavar='FILE',
                        help='text file with a 4x4 row-major matrix applied to the RECONSTRUCTION (the start of --register)')
    parser.add_argument('--save_transform', default=None, metavar='FILE', help='write the matrix applied to the reconstruction here')
    parser.add_argument('--voxel', type=float, default=None, metavar='V',
                        help='score the clouds after a voxel down-sampling of edge V (both sides)')
    parser.add_argument('--eth3d', action='store_true',
                        help='add the key `eth3d`: shares averaged over voxels, and points the laser scanners could not have seen '
                             'left out (the published protocol restated, not the official program); needs --gt_mlp or '
                             '--scanner_origins')
    parser.add_argument('--gt_mlp', default=None, metavar='FILE',
                        help='--eth3d: a MeshLab project (ETH3D\'s scan_alignment.mlp) naming the scans and their matrices; a '
                             'matrix\'s translation is the scanner\'s origin; replaces --gt')
    parser.add_argument('--scanner_origins', default=None, metavar='FILE',
                        help='--eth3d: text file, one `x y z` per --gt file, in the ground truth\'s frame after --gt_transform')
    parser.add_argument('--eth3d_voxel', type=float, default=None, metavar='V',
                        help='--eth3d: voxel edge of the averaged shares (default 0.01, ETH3D\'s)')
    parser.add_argument('--cube_size', type=int, default=None, metavar='N',
                        help='--eth3d: pixels per edge of a scanner\'s cube-map face (default 1024: a default, not a measurement)')
    parser.add_argument('--vis_window', type=int, default=None, metavar='W',
                        help='--eth3d: the nearest scan sample within W pixels decides, 0..2 (default 1: a default, not a measurement)')
    parser.add_argument('--free_space_margin', type=float, default=None, metavar='M',
                        help='--eth3d: a point up to M behind the scan still counts as observed (default 0: a default, not a '
                             'measurement)')
    return parser


def add_sample_arguments(parser):
    """--sample_recon, --sample_gt and --sample_seed: added by `cli` to what make_parser declares (the surface make_parser shares
    with the ETH3D driver's option groups stays as it is)."""
    parser.add_argument('--sample_recon', type=float, default=None, metavar='S',
                        help='--recon is a triangle mesh: score samples of its surface, one per S x S, drawn on the GPU (no default; at '
                             'most half the smallest tolerance), instead of its vertices')
    parser.add_argument('--sample_gt', type=float, default=None, metavar='S',
                        help='the same for every --gt file that is a triangle mesh (ground truth given as a surface)')
    parser.add_argument('--sample_seed', type=int, default=None, metavar='K',
                        help='--sample_recon / --sample_gt: the seed of the samples, 0..2^63-1 (default 0)')
    return parser


def sample_options(parser, args):
    """--sample_recon, --sample_gt and --sample_seed of a parsed command line as evaluate_files' keyword arguments ({} without
    them); an option without its mesh is an argument error, as is a file that is not a triangle mesh (the headers are read here)."""
    if args.sample_seed is not None and args.sample_recon is None and args.sample_gt is None:
        parser.error('--sample_seed needs --sample_recon or --sample_gt')
    if args.sample_seed is not None and not 0 <= args.sample_seed < (1 << 63):
        parser.error('--sample_seed must be in 0..2^63-1')
    options = {}
    for name, paths in (('sample_recon', [args.recon]), ('sample_gt', args.gt or [])):
        value = getattr(args, name)
        if value is None:
            continue
        if not (value > 0.0 and np.isfinite(value)):
            parser.error('--%s must be a positive finite spacing' % name)
        if name == 'sample_gt' and args.gt_mlp:
            parser.error('--sample_gt with --gt_mlp: a MeshLab project names laser scans, not meshes')
        try:
            faces = [mesh_faces(p) for p in paths]
        except (OSError, ValueError) as e:
            parser.error('--%s: %s' % (name, e))
        if not any(faces):
            parser.error('--%s: %s: the option needs a triangle mesh' % (name, ('%s has no faces' % paths[0]) if len(paths) == 1 else
                                                                         'none of the --gt files has faces'))
        options[name] = value
    if options and args.sample_seed is not None:
        options['sample_seed'] = args.sample_seed
    return options


def add_exact_arguments(parser):
    """--exact_recon and --exact_gt: added by `cli` to what make_parser and add_sample_arguments declare."""
    parser.add_argument('--exact_recon', action='store_true',
                        help='--sample_recon: completeness from the exact point-to-triangle distance of every ground-truth point to '
                             'the mesh of --recon (it no longer depends on the spacing); the samples still answer accuracy')
    parser.add_argument('--exact_gt', action='store_true',
                        help='--sample_gt, every --gt file a triangle mesh: accuracy from the exact distance of every reconstruction '
                             'point to the ground-truth surface; the samples still answer completeness')
    return parser


def exact_options(parser, args):
    """--exact_recon and --exact_gt of a parsed command line as evaluate_files' keyword arguments ({} without them); a flag without
    its --sample_* option, --exact_gt with --gt_mlp or with a --gt file that has no faces are argument errors."""
    options = {}
    if args.exact_recon:
        if args.sample_recon is None:
            parser.error('--exact_recon needs --sample_recon: the samples remain the reconstruction\'s points for accuracy and registration')
        options['exact_recon'] = True
    if args.exact_gt:
        if args.gt_mlp:
            parser.error('--exact_gt with --gt_mlp: a MeshLab project names laser scans, not meshes')
        if args.sample_gt is None:
            parser.error('--exact_gt needs --sample_gt: the samples remain the ground truth\'s points for completeness')
        try:
            without = [p for p in args.gt or [] if not mesh_faces(p)]
        except (OSError, ValueError) as e:
            parser.error('--exact_gt: %s' % e)
        if without:
            parser.error('--exact_gt: every --gt file must be a triangle mesh, %s has no faces' % without[0])
        options['exact_gt'] = True
    return options


def cli(argv=None):
    parser = add_exact_arguments(add_sample_arguments(make_parser()))
    args = parser.parse_args(argv)
    try:
        tol = [float(t) for t in args.tolerances.split(',') if t.strip()]
        tol, _ = _check_tolerances(tol, args.radius)
    except ValueError as e:
        parser.error(str(e))
    options = register_options(parser, args)
    options.update(eth3d_options(parser, args))
    options.update(sample_options(parser, args))
    options.update(exact_options(parser, args))
    import torch
    torch.cuda.set_device(args.gpu_id)
    dist = {} if args.distances else None
    try:
        result = evaluate_files(args.recon, args.gt or [], tol, args.radius, args.gt_transform, distances=dist, **options)
    except ValueError as e:
        if not any(k in options for k in ('sample_recon', 'sample_gt')):
            raise
        parser.error(str(e))             # a mesh of other polygons than triangles is only seen when its body is read
    if dist is not None:
        for k, v in dist.items():
            np.save('%s_%s.npy' % (args.distances, k), v)
    if args.out:
        write_json(args.out, result)
    else:
        print(json.dumps(result, indent=1, sort_keys=True))
    return result


if __name__ == '__main__':
    cli()
