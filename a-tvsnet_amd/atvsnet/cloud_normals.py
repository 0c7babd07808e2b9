"""Give a point cloud normals on the MI355X: per point the direction of least variance of its k nearest neighbours.

    python -m atvsnet_amd.atvsnet.cloud_normals --in cloud.ply --out cloud_n.ply [--k 16] --radius R [--viewpoint x,y,z]
           [--variation_json FILE] [--gpu_id 0]

Three launches' worth of kernels: ops.cloud_grid over the cloud with the search radius, ops.cloud_knn of the cloud in itself
(exclude_same_index: a point is no neighbour of itself) and ops.cloud_normals with self_counts (the point is a sample of its own
neighbourhood, as in PCL and Open3D).  include/atvsnet_hip.h states what a normal is, bit for bit.  A point with fewer than two
neighbours within the radius, or whose samples lie along one line, gets the zero normal -- the normal that point-to-plane
registration skips.  --viewpoint turns every normal towards that position (a scanner's, a camera's); without it a normal has the
canonical sign (its component of largest magnitude is positive).  Signs are NOT propagated across the cloud.  k and the radius are
the caller's: 16 is a common default, not a measurement, and the radius must reach k neighbours at the cloud's density.

--out is written by tools/ply.write_ply as x y z nx ny nz red green blue, the layout tools/ply.read_ply_normals reads and
eval_cloud --register_icp plane takes; colours are the input's when the input has write_ply's own vertex layout.  Any other PLY --
without colours, or with them under other names or in another order -- is read for x y z alone and written white, and the tool
says so when it does.  --variation_json receives the
count of zero normals and the quartiles of the surface variation lambda_0 / (lambda_0 + lambda_1 + lambda_2).  There is no CPU
fallback.
"""
from __future__ import print_function

import argparse
import json
import os

import numpy as np

from ..tools import ply


def estimate(points, k=16, radius=None, viewpoint=None, device=None, variation=False):
    """points (n,3) float32 (host array or device tensor) -> normals (n,3) float32 as a numpy array, or (normals, variation
    (n,) float32) with variation=True.  k 2..32 neighbours within `radius` (required), the point itself counted; viewpoint: None or
    3 numbers every normal is turned towards."""
    import torch
    from .. import ops
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 2 <= int(k) <= ops.CLOUD_MAX_K:
        raise ValueError('k: expected an integer in 2..%d, got %r' % (ops.CLOUD_MAX_K, k))
    if radius is None or not (float(radius) > 0.0 and np.isfinite(float(radius))):
        raise ValueError('radius must be positive and finite, got %r' % (radius,))
    view = None
    if viewpoint is not None:
        view = np.asarray(viewpoint, np.float64).reshape(-1)
        if view.shape != (3,) or not np.isfinite(view).all():
            raise ValueError('viewpoint: expected 3 finite numbers, got %r' % (viewpoint,))
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        if isinstance(points, torch.Tensor):
            cloud = points.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
        else:
            cloud = torch.from_numpy(np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))).to(dev)
        idx = ops.cloud_knn(ops.cloud_grid(cloud, float(radius)), cloud, int(k), exclude_same_index=True)[1]
        out = ops.cloud_normals(cloud, cloud, idx, self_counts=True, viewpoints=None if view is None else view.reshape(1, 3),
                                variation=variation)
        if variation:
            return out[0].cpu().numpy(), out[1].cpu().numpy()
        return out.cpu().numpy()


def report(normals, variation, k, radius, viewpoint):
    """The numbers of --variation_json."""
    zero = ~(normals != 0).any(axis=1)
    v = variation[~zero].astype(np.float64)
    q = np.percentile(v, [0, 25, 50, 75, 100]).tolist() if len(v) else [None] * 5
    return {'n_points': int(len(normals)), 'n_zero_normals': int(zero.sum()), 'k': int(k), 'radius': float(radius),
            'viewpoint': None if viewpoint is None else [float(x) for x in viewpoint],
            'variation': dict(zip(('min', 'q1', 'median', 'q3', 'max'), q))}


def make_parser():
    parser = argparse.ArgumentParser(description='normals of a point cloud by PCA over the k nearest neighbours, on the GPU')
    parser.add_argument('--in', dest='input', required=True, help='the cloud: a PLY')
    parser.add_argument('--out', required=True, help='the PLY to write: x y z nx ny nz red green blue')
    parser.add_argument('--k', type=int, default=16, help='neighbours per normal, 2..32 (default 16: a default, not a measurement)')
    parser.add_argument('--radius', type=float, required=True, help='the search radius: neighbours further away are not used')
    parser.add_argument('--viewpoint', default=None, metavar='x,y,z', help='turn every normal towards this position')
    parser.add_argument('--variation_json', default=None, metavar='FILE',
                        help='write the number of zero normals and the quartiles of the surface variation here')
    parser.add_argument('--gpu_id', type=int, default=0)
    return parser


def options(parser, args):
    """The parsed command line as `estimate`'s keyword arguments; a bad value is an argument error."""
    if not 2 <= args.k <= 32:
        parser.error('--k must be in 2..32')
    if not (args.radius > 0.0 and np.isfinite(args.radius)):
        parser.error('--radius must be positive and finite')
    view = None
    if args.viewpoint is not None:
        try:
            view = [float(t) for t in args.viewpoint.split(',')]
        except ValueError:
            view = []
        if len(view) != 3 or not np.isfinite(view).all():
            parser.error('--viewpoint: expected x,y,z, three finite numbers, got %r' % args.viewpoint)
    return dict(k=args.k, radius=args.radius, viewpoint=view)


def cli(argv=None):
    parser = make_parser()
    args = parser.parse_args(argv)
    opts = options(parser, args)
    try:
        try:
            points, colors = ply.read_ply(args.input)
        except ValueError:                                                   # not write_ply's layout: any PLY with x y z
            points = ply.read_ply_points(args.input)
            colors = np.full((len(points), 3), 255, np.uint8)
            print('%s is not in the vertex layout tools/ply.write_ply writes: only x y z are read, and %s is written white (colours '
                  'and any other properties of the input are dropped)' % (args.input, args.out))
    except (OSError, ValueError) as e:
        parser.error('cannot read %s: %s' % (args.input, e))
    import torch
    torch.cuda.set_device(args.gpu_id)
    normals, variation = estimate(points, variation=True, **opts)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    ply.write_ply(args.out, points, colors, normals)
    rep = report(normals, variation, **opts)
    if args.variation_json:
        with open(args.variation_json, 'w') as f:
            json.dump(rep, f, indent=1, sort_keys=True)
            f.write('\n')
    else:
        print(json.dumps(rep, indent=1, sort_keys=True))
    return rep


if __name__ == '__main__':
    cli()
