"""Smooth a triangle mesh on the MI355X by Taubin's filter, and give it vertex normals: DESIGN.md section 10.3g.  A TSDF averaged over
a handful of depth maps and cut by marching tetrahedra is a staircase of slivers; this moves the vertices, and nothing else.

    python -m atvsnet_amd.atvsnet.smooth_mesh --in mesh.ply --out smooth.ply --iterations 10 [--lam 0.5 --mu -0.53 | --laplacian]
           [--pin_boundary] [--normals [--normal_area_unit A]] [--report smooth.json] [--gpu_id 0]

The distinct neighbours of every vertex are built once (ops.mesh_adjacency: the edge census' hash table, a scan, a scatter), the
positions are put on a lattice of 2^-32 of the bounding box (ops.mesh_quantize), and every pass moves a vertex by a factor of the
way to the plain mean of its neighbours (ops.mesh_smooth_pass: one lane per vertex gathers an exact integer sum, so no result depends
on an order and the same file gives the same bytes).  An iteration is a pass with lam and a pass with mu < -lam (Taubin: the second
pass undoes the shrinkage of the first); --laplacian leaves the second out and shrinks.  --pin_boundary keeps the endpoints of edges
with one face where they are.  Vertices that are not finite or that no face names stay; a coordinate that does not move keeps its
bits.  --normals writes area-weighted vertex normals of the smoothed mesh into the PLY (ops.mesh_vertex_normals); a face larger
than --normal_area_unit (twice an area; default the mesh's largest, which is plain area weighting) votes 1.  --iterations 0 --normals
only adds normals.

`--iterations` has no default: how much noise a scene has was not measured.  lam 0.5 and mu -0.53 are Open3D's defaults: defaults,
not measurements.

What this is not: umbrella weights only -- no cotangent weights, no feature preservation (edges and corners round off); colours do
not move; no hole filling; topology does not change.  There is no CPU fallback.  This module imports without a GPU; only `smooth`
and `smooth_device` need one.
"""
from __future__ import print_function

import argparse
import json
import math
import os
import time

import numpy as np

from ..tools import ply
from ..tools.common import write_json  # noqa: F401

DEFAULT_LAMBDA, DEFAULT_MU = 0.5, -0.53        # Open3D's defaults: defaults, not measurements
MAX_ITERATIONS = 1000
REPORT_KEYS = ('iterations', 'lam', 'mu', 'pin_boundary', 'normals', 'area_unit', 'step', 'origin', 'vertices', 'faces', 'pairs',
               'boundary_pairs', 'nonmanifold_pairs', 'skipped_index_faces', 'self_pairs', 'nonfinite_pairs', 'unplaced_pairs',
               'boundary_vertices', 'pinned', 'isolated_vertices', 'nonfinite_vertices', 'moved', 'max_move', 'seconds')


def _real(x, name, what, ok):
    if isinstance(x, (bool, str, bytes)) or x is None:
        raise ValueError('%s must be %s, got %r' % (name, what, x))
    try:
        v = float(x)
    except (TypeError, ValueError):
        raise ValueError('%s must be %s, got %r' % (name, what, x))
    if not (math.isfinite(v) and ok(v)):
        raise ValueError('%s must be %s, got %r' % (name, what, x))
    return v


def check_options(iterations, lam=DEFAULT_LAMBDA, mu=DEFAULT_MU, pin_boundary=False, normals=False, area_unit=None):
    """-> (iterations int, lam float, mu float or None, pin_boundary bool, normals bool, area_unit float or None); ValueError names
    a bad one.  0 < lam < 1; mu None (Laplacian) or -1 <= mu < -lam (Taubin's condition); iterations an integer in 0..1000;
    area_unit None or a finite number > 0, with normals only."""
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or not 0 <= int(iterations) <= MAX_ITERATIONS:
        raise ValueError('iterations must be an integer in 0..%d, got %r' % (MAX_ITERATIONS, iterations))
    lam = _real(lam, 'lam', 'a number with 0 < lam < 1', lambda v: 0.0 < v < 1.0)
    if mu is not None:
        mu = _real(mu, 'mu', 'None or a number with -1 <= mu < -lam (Taubin\'s condition; lam is %r)' % lam, lambda v: -1.0 <= v < -lam)
    for name, value in (('pin_boundary', pin_boundary), ('normals', normals)):
        if not isinstance(value, (bool, np.bool_)):
            raise ValueError('%s must be True or False, got %r' % (name, value))
    if area_unit is not None:
        area_unit = _real(area_unit, 'area_unit', 'None or a finite number > 0', lambda v: v > 0.0)
        if not normals:
            raise ValueError('area_unit weights the normals: it needs normals=True')
    return int(iterations), lam, mu, bool(pin_boundary), bool(normals), area_unit


def smooth_device(vertices, colors, faces, iterations, lam=DEFAULT_LAMBDA, mu=DEFAULT_MU, pin_boundary=False, normals=False,
                  area_unit=None):
    """vertices (V,3) float32, colors (V,3) uint8 or None, faces (F,3) int32 on the current device -> (vertices, colors, faces,
    normals or None, report) with the smoothed vertices still on the device.  Colours and faces are returned as they came: topology
    does not change.  normals: the smoothed mesh's vertex normals (V,3) float32, weighted by min(1, s / area_unit), area_unit None:
    the largest s.  report: REPORT_KEYS."""
    import torch
    from .. import ops
    iterations, lam, mu, pin_boundary, normals, area_unit = check_options(iterations, lam, mu, pin_boundary, normals, area_unit)
    dev = vertices.device
    nv, nf = int(vertices.shape[0]), int(faces.shape[0])
    seconds = {}

    def timed(name, fn):
        torch.cuda.synchronize(dev)
        t0 = time.time()
        out = fn()
        torch.cuda.synchronize(dev)
        seconds[name] = time.time() - t0
        return out

    adjacency = timed('adjacency', lambda: ops.mesh_adjacency(vertices, faces))
    out, info = timed('smooth', lambda: ops.mesh_smooth(vertices, faces, iterations, lam, mu, pin_boundary, adjacency=adjacency))

    def measure():
        if nv == 0:
            return 0, 0, 0, 0, 0.0
        finite = (adjacency.flags & ops.MESH_FLAG_FINITE) != 0
        counts = torch.stack([((adjacency.flags & ops.MESH_FLAG_BOUNDARY) != 0).sum(), (finite & (adjacency.degree == 0)).sum(), (~finite).sum(),
                              (out.view(torch.int32) != vertices.view(torch.int32)).any(1).sum()]).cpu().tolist()
        move = ops.mesh_cluster_max_move(vertices, torch.arange(nv, dtype=torch.int32, device=dev), out)
        return tuple(int(c) for c in counts) + (move,)
    boundary, isolated, nonfinite, moved, max_move = timed('measure', measure)
    out_normals = timed('normals', lambda: ops.mesh_vertex_normals(out, faces, area_unit)) if normals else None
    report = {'iterations': iterations, 'lam': lam, 'mu': mu, 'pin_boundary': pin_boundary, 'normals': normals, 'area_unit': area_unit,
              'step': info['step'], 'origin': info['origin'], 'vertices': nv, 'faces': nf, 'boundary_vertices': boundary,
              'pinned': boundary if pin_boundary else 0, 'isolated_vertices': isolated, 'nonfinite_vertices': nonfinite, 'moved': moved,
              'max_move': max_move, 'seconds': seconds}
    report.update({k: adjacency.info[k] for k in ops.MESH_ADJACENCY_INFO})
    return out, colors, faces, out_normals, report


def smooth(vertices, colors, faces, iterations, lam=DEFAULT_LAMBDA, mu=DEFAULT_MU, pin_boundary=False, normals=False, area_unit=None,
           device=None):
    """Host arrays -> (vertices, colors, faces, normals or None, report), host arrays (colors None when none were given)."""
    check_options(iterations, lam, mu, pin_boundary, normals, area_unit)
    import torch
    v = np.ascontiguousarray(np.asarray(vertices, np.float32).reshape(-1, 3))
    f = np.ascontiguousarray(np.asarray(faces, np.int32).reshape(-1, 3))
    if colors is not None:
        colors = np.ascontiguousarray(np.asarray(colors, np.uint8).reshape(-1, 3))
        if len(colors) != len(v):
            raise ValueError('colors: %d rows for %d vertices' % (len(colors), len(v)))
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        t0 = time.time()
        dv, df = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
        upload = time.time() - t0
        out_v, _, _, out_n, report = smooth_device(dv, None, df, iterations, lam, mu, pin_boundary, normals, area_unit)
        t0 = time.time()
        out_v, out_n = out_v.cpu().numpy(), None if out_n is None else out_n.cpu().numpy()
        report['seconds'].update(upload=upload, download=time.time() - t0)
    return out_v, colors, f, out_n, report


def read_mesh(path):
    """-> (vertices, colors or None, faces): ply.read_mesh where the file has write_mesh's layout (its colours are kept; normals it
    carries are dropped: they belong to the unsmoothed surface), else ply.read_mesh_any."""
    try:
        return ply.read_mesh(path)
    except (ValueError, UnicodeDecodeError):
        vertices, faces = ply.read_mesh_any(path)
        return vertices, None, faces


def make_parser():
    parser = argparse.ArgumentParser(description='smooth a triangle mesh on the GPU by Taubin\'s filter (umbrella weights: no cotangent '
                                                 'weights, no feature preservation; colours do not move; no hole filling) and write '
                                                 'vertex normals')
    parser.add_argument('--in', dest='input', required=True, help='the mesh: a PLY as mesh_fusion writes it (its colours are kept) or a '
                                                                  'third-party triangle-mesh PLY')
    parser.add_argument('--out', required=True, help='the smoothed mesh (a binary PLY)')
    parser.add_argument('--iterations', type=int, required=True, metavar='N', help='iterations of a lam pass and a mu pass (no default: '
                        'how much noise a scene has was not measured); 0 with --normals only adds normals')
    parser.add_argument('--lam', type=float, default=DEFAULT_LAMBDA, help='the shrinking pass\' factor, 0 < lam < 1 (default %g, Open3D\'s: '
                                                                         'a default, not a measurement)' % DEFAULT_LAMBDA)
    parser.add_argument('--mu', type=float, default=None, help='the inflating pass\' factor, -1 <= mu < -lam, written --mu=-0.53 '
                                                               '(default %g, Open3D\'s: a default, not a measurement)' % DEFAULT_MU)
    parser.add_argument('--laplacian', action='store_true', help='no mu pass: plain Laplacian smoothing, which shrinks the mesh')
    parser.add_argument('--pin_boundary', action='store_true', help='the endpoints of edges with one face do not move')
    parser.add_argument('--normals', action='store_true', help='write area-weighted vertex normals of the smoothed mesh (nx ny nz)')
    parser.add_argument('--normal_area_unit', type=float, default=None, metavar='A',
                        help='--normals: a face with |(b-a) x (c-a)| above A votes 1, a smaller one in proportion (default: the '
                             'mesh\'s largest, plain area weighting)')
    parser.add_argument('--report', default=None, metavar='FILE.json', help='write what moved and how far here (default: print it)')
    parser.add_argument('--gpu_id', type=int, default=0)
    return parser


def options(parser, args):
    """The parsed arguments as smooth's keyword arguments; a bad one is an argument error."""
    if args.laplacian and args.mu is not None:
        parser.error('--laplacian has no mu pass: it cannot be combined with --mu')
    if args.normal_area_unit is not None and not args.normals:
        parser.error('--normal_area_unit needs --normals')
    out = dict(iterations=args.iterations, lam=args.lam, mu=None if args.laplacian else (DEFAULT_MU if args.mu is None else args.mu),
               pin_boundary=args.pin_boundary, normals=args.normals, area_unit=args.normal_area_unit)
    try:
        check_options(**out)
    except ValueError as e:
        parser.error('--%s' % str(e).replace('area_unit', 'normal_area_unit'))
    return out


def cli(argv=None):
    parser = make_parser()
    args = parser.parse_args(argv)
    chosen = options(parser, args)
    if not os.path.isfile(args.input):
        parser.error('--in %s: no such file' % args.input)
    try:
        vertices, colors, faces = read_mesh(args.input)
    except ValueError as e:
        parser.error('--in: %s' % e)
    import torch
    torch.cuda.set_device(args.gpu_id)
    vertices, colors, faces, normals, report = smooth(vertices, colors, faces, **chosen)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    ply.write_mesh(args.out, vertices, colors, faces, normals)
    if args.report:
        write_json(args.report, report)
    else:
        print(json.dumps(report, indent=1, sort_keys=True))
    return report


if __name__ == '__main__':
    cli()
