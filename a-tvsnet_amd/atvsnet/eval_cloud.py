"""Score a reconstructed point cloud against a ground-truth cloud on the MI355X: accuracy, completeness and F-score at a set of
distance tolerances.

    python -m atvsnet_amd.atvsnet.eval_cloud --recon final3d_model.ply --gt scan1.ply [scan2.ply ...]
           [--tolerances 0.01,0.02,0.05,0.1,0.2,0.5] [--radius R] [--gt_transform T.txt] [--out cloud_eval.json] [--distances PREFIX]

This is the PLAIN precision / recall definition (the one Tanks and Temples uses): per tolerance tau, `accuracy` is the share of
reconstruction points with a ground-truth point within tau, `completeness` the share of ground-truth points with a reconstruction
point within tau, `f1` their harmonic mean.  It is NOT ETH3D's official evaluator, which also voxelises the clouds and uses the
scans' visibility (free space): the numbers are comparable between runs of this tool, not with the ETH3D leaderboard.

Both directions of the nearest-neighbour search run on the device (ops.cloud_grid / cloud_nearest / cloud_counts, csrc/cloud.hip),
exactly: per point the smallest float32 squared distance (dx*dx + dy*dy) + dz*dz to the other cloud, unknown (+inf) beyond
`radius`; a point counts at tau when double(d2) <= tau * tau.  There is no CPU fallback.  `metrics` is the pure-host part.
"""
from __future__ import print_function

import argparse
import json
import os

import numpy as np

from ..tools import ply

DEFAULT_TOLERANCES = (0.01, 0.02, 0.05, 0.1, 0.2, 0.5)


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


def evaluate(recon, gt, tolerances=DEFAULT_TOLERANCES, radius=None, gt_transform=None, device=None, distances=None):
    """recon (M,3), gt (N,3): host arrays (or device tensors) of float32 points -> the dict of `metrics`.  radius: the search
    radius, default the largest tolerance.  gt_transform: a 4x4 matrix applied to `gt` on the host (float64, rounded once).
    distances: a dict that receives d2_recon, idx_recon, d2_gt, idx_gt as numpy arrays."""
    import torch
    from .. import ops
    tol, radius = _check_tolerances(tolerances, radius)
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)

    def upload(x):
        if isinstance(x, torch.Tensor):
            return x.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1, 3))).to(dev)

    if gt_transform is not None:
        gt = transform_points(gt.cpu().numpy() if isinstance(gt, torch.Tensor) else gt, gt_transform)
    with torch.cuda.device(dev):
        r, g = upload(recon), upload(gt)
        d2_r, idx_r = ops.cloud_nearest(ops.cloud_grid(g, radius), r)
        d2_g, idx_g = ops.cloud_nearest(ops.cloud_grid(r, radius), g)
        counts = [ops.cloud_counts(d2, tol, radius).cpu().tolist() for d2 in (d2_r, d2_g)]
        d2_r, d2_g = d2_r.cpu().numpy(), d2_g.cpu().numpy()
        if distances is not None:
            distances.update(d2_recon=d2_r, idx_recon=idx_r.cpu().numpy(), d2_gt=d2_g, idx_gt=idx_g.cpu().numpy())
    return metrics(d2_r, d2_g, tol, radius, counts=counts)


def evaluate_files(recon_path, gt_paths, tolerances=DEFAULT_TOLERANCES, radius=None, gt_transform_path=None, distances=None):
    """`evaluate` of PLY files (tools/ply.read_ply_points): several ground-truth files are concatenated; gt_transform_path: a text
    file of 16 numbers, the 4x4 matrix row-major."""
    recon = ply.read_ply_points(recon_path)
    gt = [ply.read_ply_points(p) for p in gt_paths]
    gt = np.concatenate(gt, 0) if gt else np.zeros((0, 3), np.float32)
    T = None
    if gt_transform_path is not None:
        T = np.loadtxt(gt_transform_path, dtype=np.float64)
        if T.size != 16:
            raise ValueError('%s: expected the 16 numbers of a 4x4 matrix, got %d' % (gt_transform_path, T.size))
    return evaluate(recon, gt, tolerances, radius, gt_transform=T, distances=distances)


def write_json(path, result):
    with open(path, 'w') as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write('\n')


def cli(argv=None):
    parser = argparse.ArgumentParser(description='accuracy / completeness / F-score of a point cloud against ground truth '
                                                 '(plain precision / recall; not the official ETH3D evaluator)')
    parser.add_argument('--recon', required=True, help='the reconstruction (PLY)')
    parser.add_argument('--gt', required=True, nargs='+', help='ground-truth PLY file(s), concatenated')
    parser.add_argument('--tolerances', default=','.join(str(t) for t in DEFAULT_TOLERANCES), help='comma-separated distances')
    parser.add_argument('--radius', type=float, default=None, help='search radius (default: the largest tolerance)')
    parser.add_argument('--gt_transform', default=None, help='text file with a 4x4 row-major matrix applied to the ground truth')
    parser.add_argument('--out', default=None, help='write the result as JSON here (default: print it)')
    parser.add_argument('--distances', default=None, metavar='PREFIX',
                        help='write PREFIX_d2_recon.npy, PREFIX_idx_recon.npy, PREFIX_d2_gt.npy, PREFIX_idx_gt.npy')
    parser.add_argument('--gpu_id', type=int, default=0)
    args = parser.parse_args(argv)
    try:
        tol = [float(t) for t in args.tolerances.split(',') if t.strip()]
        tol, _ = _check_tolerances(tol, args.radius)
    except ValueError as e:
        parser.error(str(e))
    import torch
    torch.cuda.set_device(args.gpu_id)
    dist = {} if args.distances else None
    result = evaluate_files(args.recon, args.gt, tol, args.radius, args.gt_transform, distances=dist)
    if dist is not None:
        for k, v in dist.items():
            np.save('%s_%s.npy' % (args.distances, k), v)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        write_json(args.out, result)
    else:
        print(json.dumps(result, indent=1, sort_keys=True))
    return result


if __name__ == '__main__':
    cli()
