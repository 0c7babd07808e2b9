"""Clean a fused point cloud on the MI355X before it is scored: thin it to one point per voxel, remove statistical outliers,
remove points with too few neighbours.

    python -m atvsnet_amd.atvsnet.clean_cloud --in final3d_model.ply --out clean.ply [--voxel V] [--sor K,RATIO [--sor_radius R]]
           [--radius_filter R,N] [--keep_normals] [--report clean.json] [--gpu_id 0]

The cloud depth_fusion writes has one point per consistent pixel of every reference camera (a surface patch appears once per
camera that saw it) and the isolated floaters that pass the consistency vote.  The steps run in this order, each optional:

    voxel V                one point per occupied voxel of edge V, the mean of its points (ops.cloud_voxel_downsample); its colour
                           is the colour of the voxel's lowest row (and with --keep_normals its normal that row's);
                           non-finite rows drop out
    sor (k, ratio, radius) statistical outlier removal as PCL and Open3D define it: s[j] = the mean distance of row j to its k
                           nearest other rows (ops.cloud_knn with exclude_same_index, ops.cloud_knn_mean), mu and sigma = the mean
                           and sample standard deviation of the finite s (ops.cloud_sor_stats); row j stays when
                           s[j] <= mu + ratio * sigma, compared in double.  The search has a horizon: a row with fewer than k
                           neighbours within `radius` has s = +inf, takes no part in mu and sigma, and is removed
    radius_filter (radius, min_neighbours)
                           a row stays when at least min_neighbours other rows lie within `radius` (ops.cloud_radius_count)

The inputs and outputs are host arrays; everything between the upload and the download stays on the device (the searches, the
reductions; the comparison with the threshold and the order-preserving compaction are torch indexing).  Rows keep their order.
There is no CPU fallback.  This module imports without a GPU; only `clean` needs one.
"""
from __future__ import print_function

import argparse
import json
import math
import os

import numpy as np

from ..tools import ply
from ..tools.common import write_json  # noqa: F401

SOR_RADIUS_VOXELS = 8.0          # --sor without --sor_radius: the horizon is this many voxel edges.  A default, not a measurement.


def _check(voxel, sor, radius_filter):
    """The steps' arguments as plain numbers; ValueError names the argument."""
    if voxel is None and sor is None and radius_filter is None:
        raise ValueError('clean: at least one of voxel, sor, radius_filter is needed')
    if voxel is not None:
        voxel = float(voxel)
        if not (voxel > 0.0 and math.isfinite(voxel)):
            raise ValueError('voxel must be positive and finite, got %r' % (voxel,))
    if sor is not None:
        if len(sor) != 3:
            raise ValueError('sor: expected (k, ratio, radius), got %r' % (sor,))
        k, ratio, radius = sor
        if int(k) != k or not 1 <= int(k) <= 32:
            raise ValueError('sor: k must be an integer in 1..32, got %r' % (k,))
        ratio, radius = float(ratio), float(radius)
        if not math.isfinite(ratio):
            raise ValueError('sor: ratio must be finite, got %r' % (ratio,))
        if not (radius > 0.0 and math.isfinite(radius)):
            raise ValueError('sor: radius must be positive and finite, got %r' % (radius,))
        sor = (int(k), ratio, radius)
    if radius_filter is not None:
        if len(radius_filter) != 2:
            raise ValueError('radius_filter: expected (radius, min_neighbours), got %r' % (radius_filter,))
        radius, least = radius_filter
        radius = float(radius)
        if not (radius > 0.0 and math.isfinite(radius)):
            raise ValueError('radius_filter: radius must be positive and finite, got %r' % (radius,))
        if int(least) != least or int(least) < 0:
            raise ValueError('radius_filter: min_neighbours must be an integer >= 0, got %r' % (least,))
        radius_filter = (radius, int(least))
    return voxel, sor, radius_filter


def clean(points, colors=None, voxel=None, sor=None, radius_filter=None, device=None, normals=None):
    """points (n,3) float32, colors (n,3) uint8 or None: host arrays -> (points, colors, report): the rows that stay, in their
    order, as host arrays (colors None when none were given), and what every step did.  normals (n,3) float32 (a fused cloud's
    nx ny nz): -> (points, colors, normals, report) instead; the normals follow their rows as the colours do (a voxel's normal is
    its lowest row's, not an average; a filter keeps rows).  voxel, sor=(k, ratio, radius),
    radius_filter=(radius, min_neighbours): the module's steps, None = skipped; at least one is needed.
    report: {'n_in', 'n_out', 'steps': [{'step', its arguments, 'rows_in', 'rows_out'}, ...]}; the sor step also carries `count`,
    `mean`, `std` (ops.cloud_sor_stats) and `threshold` = mean + ratio * std."""
    voxel, sor, radius_filter = _check(voxel, sor, radius_filter)
    import torch
    from .. import ops
    pts = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
    if colors is not None:
        colors = np.ascontiguousarray(np.asarray(colors, np.uint8).reshape(-1, 3))
        if len(colors) != len(pts):
            raise ValueError('colors: %d rows for %d points' % (len(colors), len(pts)))
    if normals is not None:
        normals = np.ascontiguousarray(np.asarray(normals, np.float32).reshape(-1, 3))
        if len(normals) != len(pts):
            raise ValueError('normals: %d rows for %d points' % (len(normals), len(pts)))
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    report = {'n_in': int(len(pts)), 'steps': []}
    with torch.cuda.device(dev):
        p = torch.from_numpy(pts).to(dev)
        c = None if colors is None else torch.from_numpy(colors).to(dev)
        nrm = None if normals is None else torch.from_numpy(normals).to(dev)

        def keep_rows(mask):
            return tuple(None if t is None else t[mask].contiguous() for t in (p, c, nrm))

        if voxel is not None:
            rows_in = int(p.shape[0])
            p, first = ops.cloud_voxel_downsample(p, voxel)
            p = p.contiguous()
            if c is not None:
                c = c[first.long()].contiguous()
            if nrm is not None:
                nrm = nrm[first.long()].contiguous()
            report['steps'].append({'step': 'voxel', 'voxel': voxel, 'rows_in': rows_in, 'rows_out': int(p.shape[0])})
        if sor is not None:
            k, ratio, radius = sor
            rows_in = int(p.shape[0])
            d2, _ = ops.cloud_knn(ops.cloud_grid(p, radius), p, k, exclude_same_index=True)
            s = ops.cloud_knn_mean(d2)
            count, mean, std = ops.cloud_sor_stats(s)
            threshold = mean + ratio * std
            p, c, nrm = keep_rows(s <= threshold)
            report['steps'].append({'step': 'sor', 'k': k, 'ratio': ratio, 'radius': radius, 'rows_in': rows_in,
                                    'rows_out': int(p.shape[0]), 'count': count, 'mean': mean, 'std': std, 'threshold': threshold})
        if radius_filter is not None:
            radius, least = radius_filter
            rows_in = int(p.shape[0])
            found = ops.cloud_radius_count(ops.cloud_grid(p, radius), p, exclude_same_index=True)
            p, c, nrm = keep_rows(found >= least)
            report['steps'].append({'step': 'radius_filter', 'radius': radius, 'min_neighbours': least, 'rows_in': rows_in,
                                    'rows_out': int(p.shape[0])})
        out_p = p.cpu().numpy()
        out_c = None if c is None else c.cpu().numpy()
        out_n = None if nrm is None else nrm.cpu().numpy()
    report['n_out'] = int(len(out_p))
    if normals is not None:
        return out_p, out_c, out_n, report
    return out_p, out_c, report


def add_options(parser, prefix=''):
    """The three steps' options --<prefix>voxel, --<prefix>sor, --<prefix>sor_radius, --<prefix>radius_filter, and --<prefix>keep_normals."""
    parser.add_argument('--%svoxel' % prefix, type=float, default=None, metavar='V',
                        help='keep one point per occupied voxel of edge V: the mean of its points, the colour of its first')
    parser.add_argument('--%ssor' % prefix, default=None, metavar='K,RATIO',
                        help='statistical outlier removal: remove a point whose mean distance to its K nearest neighbours (K <= 32) '
                             'exceeds the mean of that figure over the cloud by more than RATIO standard deviations')
    parser.add_argument('--%ssor_radius' % prefix, type=float, default=None, metavar='R',
                        help='the horizon of the --%ssor search: a point with fewer than K neighbours within R is removed.  Default '
                             'with --%svoxel V: %g V (a default, not a measurement); required without' % (prefix, prefix, SOR_RADIUS_VOXELS))
    parser.add_argument('--%sradius_filter' % prefix, default=None, metavar='R,N',
                        help='remove a point with fewer than N other points within the distance R')
    parser.add_argument('--%skeep_normals' % prefix, action='store_true',
                        help='the cloud carries normals (nx ny nz, as `depth_fusion --normals depth` writes them; the ETH3D driver: --fuse_normals '
                             'depth): write those of the rows that stay into the cleaned cloud (a voxel keeps the normal of its first row)')


def keep_normals_rules(clean, keep_normals, fused_normals):
    """The ETH3D driver's rules for its clean_keep_normals, as (broken, message) rows: none unless it is asked for.  clean: the
    driver's cleaning steps or None; fused_normals: whether its fusion estimates normals (fuse_normals normals='depth')."""
    return [] if not keep_normals else [
        (not clean, '--clean_keep_normals needs --clean_voxel, --clean_sor or --clean_radius_filter (clean_keep_normals needs clean)'),
        (not fused_normals, '--clean_keep_normals needs --fuse_normals depth (clean_keep_normals needs fuse_normals normals=depth): '
                            'there are no normals to keep')]


def options(parser, args, prefix=''):
    """The parsed options of add_options as clean's keyword arguments ({} when none is given); a bad one is an argument error."""
    get = lambda name: getattr(args, prefix + name)          # noqa: E731
    out = {}
    if get('voxel') is not None:
        out['voxel'] = get('voxel')
    if get('sor_radius') is not None and get('sor') is None:
        parser.error('--%ssor_radius needs --%ssor' % (prefix, prefix))
    if get('sor') is not None:
        try:
            k, ratio = get('sor').split(',')
            k, ratio = int(k), float(ratio)
        except ValueError:
            parser.error('--%ssor: expected K,RATIO (an integer and a number), got %r' % (prefix, get('sor')))
        radius = get('sor_radius')
        if radius is None:
            if get('voxel') is None:
                parser.error('--%ssor needs a horizon: give --%ssor_radius R, or --%svoxel V (the horizon is then %g V)'
                             % (prefix, prefix, prefix, SOR_RADIUS_VOXELS))
            radius = SOR_RADIUS_VOXELS * get('voxel')
        out['sor'] = (k, ratio, radius)
    if get('radius_filter') is not None:
        try:
            radius, least = get('radius_filter').split(',')
            radius, least = float(radius), int(least)
        except ValueError:
            parser.error('--%sradius_filter: expected R,N (a number and an integer), got %r' % (prefix, get('radius_filter')))
        out['radius_filter'] = (radius, least)
    if out:
        try:
            _check(out.get('voxel'), out.get('sor'), out.get('radius_filter'))
        except ValueError as e:
            parser.error('--%s%s' % (prefix, e))
    return out


def make_parser():
    parser = argparse.ArgumentParser(description='clean a point cloud on the GPU: voxel down-sampling, statistical outlier '
                                                 'removal, radius outlier removal (in this order)')
    parser.add_argument('--in', dest='input', required=True, help='the cloud (a PLY as depth_fusion writes it)')
    parser.add_argument('--out', required=True, help='the cleaned cloud (PLY)')
    add_options(parser)
    parser.add_argument('--report', default=None, metavar='FILE.json', help='write what every step did here (default: print it)')
    parser.add_argument('--gpu_id', type=int, default=0)
    return parser


def cli(argv=None):
    parser = make_parser()
    args = parser.parse_args(argv)
    steps = options(parser, args)
    if not steps:
        parser.error('nothing to do: give at least one of --voxel, --sor, --radius_filter')
    if args.keep_normals:
        try:
            with_normals = ply.has_normals(args.input)
        except (OSError, ValueError) as e:
            parser.error('--keep_normals: cannot read %s: %s' % (args.input, e))
        if not with_normals:
            parser.error('--keep_normals: %s carries no normals (nx ny nz); `depth_fusion --normals depth` writes them' % args.input)
    import torch
    torch.cuda.set_device(args.gpu_id)
    normals = None
    if args.keep_normals:
        points, colors, normals = ply.read_ply_normals(args.input)
        points, colors, normals, report = clean(points, colors, normals=normals, **steps)
    else:
        points, colors = ply.read_ply(args.input)
        points, colors, report = clean(points, colors, **steps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    ply.write_ply(args.out, points, colors, normals)
    if args.report:
        write_json(args.report, report)
    else:
        print(json.dumps(report, indent=1, sort_keys=True))
    return report


if __name__ == '__main__':
    cli()
