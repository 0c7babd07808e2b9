"""Simplify a triangle mesh on the MI355X by vertex clustering (Rossignac and Borrel) with each cluster's representative placed by
its quadric (Lindstrom): DESIGN.md section 10.3d.  Marching tetrahedra emit several triangles per surface voxel, so a scene meshed at
a pixel's footprint has tens of millions of faces for what is mostly walls and floors; this gives one vertex per occupied cell of a
coarser lattice.

    python -m atvsnet_amd.atvsnet.simplify_mesh --in mesh.ply --out simple.ply --cell C [--placement quadric|mean] [--origin x,y,z]
           [--rank_epsilon 1e-3] [--report simple.json] [--gpu_id 0]

The vertices are sorted into the cubic cells of edge `cell` whose corner (0,0,0) is `origin` (ops.mesh_cluster: the voxels of
ops.cloud_voxel_downsample, exact integer sums).  Every cell that holds a vertex becomes one vertex:

    mean       the exact mean of the cell's vertices
    quadric    the point of the cell that minimises the summed squared distance to the planes of the faces that touch the cell
               (ops.mesh_cluster_quadrics: fixed-point integer sums; ops.mesh_cluster_place: the fixed Jacobi of ops.cloud_normals on
               the eigenpairs above rank_epsilon), the mean where the faces are slivers only or the minimiser leaves the cell

and its colour is the rounded mean.  A face is rewritten to its three cells and dropped when it names a non-finite vertex, when two
of the three are the same cell, or when a face before it has the same set of three (ops.mesh_cluster_faces); ops.mesh_select
compacts what is left, so surviving faces and cells keep their order.  One pass over the vertices, one over the faces, one lane
per cell, nothing iterative; integer atomics only, so the output is a function of the input alone.  Both placements keep a vertex
inside its cell: nothing moves farther than cell * sqrt(3), and the report says how far something did.

`--cell` has no default: which cell suits depends on the scene.  `quadric` is the default placement as Lindstrom's choice, not as a
measured winner: it keeps edges and corners, and on smooth or noisy surfaces it is no better than the mean (section 10.3d has the
restatement's numbers).  rank_epsilon = 1e-3 is Lindstrom's value, a default and not a measurement.

What this is not: edge-collapse decimation to a target face count, topology preservation (two sheets closer than a cell merge, a
thin handle closes; the report's two edge censuses say what happened instead of hiding it), boundary or colour-seam constraints.
atvsnet/eval_cloud.py --recon scores a mesh by its VERTICES, so a simplified mesh loses completeness there by construction: give
it --sample_recon, which scores samples of the surface instead (atvsnet/sample_mesh.py).  There is no CPU fallback.  This module imports without
a GPU; only `simplify` and `simplify_device` need one.
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
from .clean_mesh import read_mesh

PLACEMENTS = ('quadric', 'mean')
DEFAULT_PLACEMENT = 'quadric'      # Lindstrom's choice, not a measured winner
DEFAULT_RANK_EPSILON = 1e-3        # Lindstrom's value: a default, not a measurement


def check_options(cell, placement=DEFAULT_PLACEMENT, origin=None, rank_epsilon=DEFAULT_RANK_EPSILON):
    """-> (cell float, placement, origin as a tuple of 3 floats or None, rank_epsilon float); ValueError names a bad one."""
    if isinstance(cell, (bool, str, bytes)) or cell is None:
        raise ValueError('cell must be a positive finite number, got %r' % (cell,))
    try:
        c = float(cell)
    except (TypeError, ValueError):
        raise ValueError('cell must be a positive finite number, got %r' % (cell,))
    if not (c > 0.0 and math.isfinite(c)):
        raise ValueError('cell must be a positive finite number, got %r' % (cell,))
    if not isinstance(placement, str) or placement not in PLACEMENTS:
        raise ValueError('placement must be one of %s, got %r' % (', '.join(PLACEMENTS), placement))
    if isinstance(rank_epsilon, (bool, str, bytes)) or rank_epsilon is None:
        raise ValueError('rank_epsilon must be a number in (0, 1), got %r' % (rank_epsilon,))
    try:
        e = float(rank_epsilon)
    except (TypeError, ValueError):
        raise ValueError('rank_epsilon must be a number in (0, 1), got %r' % (rank_epsilon,))
    if not 0.0 < e < 1.0:
        raise ValueError('rank_epsilon must be a number in (0, 1), got %r' % (rank_epsilon,))
    if origin is not None:
        try:
            o = np.asarray(origin, np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError('origin must be 3 finite numbers, got %r' % (origin,))
        if o.shape != (3,) or not np.isfinite(o).all():
            raise ValueError('origin must be 3 finite numbers, got %r' % (origin,))
        origin = tuple(float(x) for x in o)
    return c, placement, origin, e


def simplify_device(vertices, colors, faces, cell, placement=DEFAULT_PLACEMENT, origin=None, rank_epsilon=DEFAULT_RANK_EPSILON):
    """vertices (V,3) float32, colors (V,3) uint8 or None, faces (F,3) int32 on the current device -> (vertices, colors, faces,
    report) with the simplified mesh still on the device.  origin None: the lower bound of the finite vertices (ops.cloud_bounds)."""
    import torch
    from .. import ops
    cell, placement, origin, rank_epsilon = check_options(cell, placement, origin, rank_epsilon)
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

    census_in = timed('census_before', lambda: ops.mesh_edge_census(faces, nv))
    if origin is None:
        lo = timed('bounds', lambda: ops.cloud_bounds(vertices)[0] if nv else None)
        origin = (0.0, 0.0, 0.0) if lo is None else tuple(float(x) for x in lo)
    clusters = timed('cluster', lambda: ops.mesh_cluster(vertices, colors, cell, origin))
    nc = int(clusters.counts.shape[0])
    quadrics = None
    if placement == 'quadric':
        quadrics, _ = timed('quadrics', lambda: ops.mesh_cluster_quadrics(vertices, faces, clusters.vertex_cluster, nc, cell, origin))
    positions, out_colors, placed = timed('place', lambda: ops.mesh_cluster_place(
        clusters.cells, clusters.counts, clusters.position_sums, clusters.color_sums, quadrics, cell, origin, placement, rank_epsilon))
    max_move = timed('max_move', lambda: ops.mesh_cluster_max_move(vertices, clusters.vertex_cluster, positions))
    rewritten, keep, drops = timed('faces', lambda: ops.mesh_cluster_faces(faces, clusters.vertex_cluster))
    out_v, out_c, out_f, _ = timed('select', lambda: ops.mesh_select(positions, out_colors, rewritten, keep))
    census_out = timed('census_after', lambda: ops.mesh_edge_census(out_f, int(out_v.shape[0])))
    by_quadric = int(placed.sum().item()) if nc else 0
    report = {'cell': cell, 'placement': placement, 'origin': list(origin), 'rank_epsilon': rank_epsilon, 'clusters': nc,
              'vertices_in': nv, 'vertices_out': int(out_v.shape[0]), 'faces_in': nf, 'faces_out': int(out_f.shape[0]),
              'degenerate_faces': drops['degenerate_faces'], 'duplicate_faces': drops['duplicate_faces'],
              'nonfinite_faces': drops['nonfinite_faces'], 'placed_by_quadric': by_quadric,
              'fell_back': nc - by_quadric if placement == 'quadric' else 0, 'max_move': max_move,
              'max_move_bound': cell * math.sqrt(3.0), 'census_in': census_in, 'census_out': census_out, 'seconds': seconds}
    return out_v, out_c, out_f, report


def simplify(vertices, colors, faces, cell, placement=DEFAULT_PLACEMENT, origin=None, rank_epsilon=DEFAULT_RANK_EPSILON, device=None):
    """vertices (V,3) float32, colors (V,3) uint8 or None, faces (F,3) int32: host arrays -> (vertices, colors, faces, report), the
    simplified mesh as host arrays (colors None when none were given).  report: 'cell', 'placement', 'origin', 'rank_epsilon',
    'clusters', 'vertices_in' / 'vertices_out', 'faces_in' / 'faces_out', 'degenerate_faces', 'duplicate_faces', 'nonfinite_faces',
    'placed_by_quadric', 'fell_back', 'max_move' and 'max_move_bound' (cell * sqrt(3)), 'census_in' / 'census_out'
    (ops.mesh_edge_census), 'seconds' per stage."""
    check_options(cell, placement, origin, rank_epsilon)
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
        dc = None if colors is None else torch.from_numpy(colors).to(dev)
        upload = time.time() - t0
        out_v, out_c, out_f, report = simplify_device(dv, dc, df, cell, placement, origin, rank_epsilon)
        t0 = time.time()
        out = (out_v.cpu().numpy(), None if out_c is None else out_c.cpu().numpy(), out_f.cpu().numpy())
        report['seconds'].update(upload=upload, download=time.time() - t0)
    return out + (report,)


def _origin_arg(text):
    parts = text.split(',')
    try:
        values = tuple(float(p) for p in parts)
    except ValueError:
        raise argparse.ArgumentTypeError('expected x,y,z, got %r' % text)
    if len(values) != 3:
        raise argparse.ArgumentTypeError('expected x,y,z, got %r' % text)
    return values


def make_parser():
    parser = argparse.ArgumentParser(description='simplify a triangle mesh on the GPU: one vertex per occupied cell of a lattice, placed '
                                                 'by the cell\'s quadric (no edge collapse to a face count, no topology preservation)')
    parser.add_argument('--in', dest='input', required=True, help='the mesh: a PLY as mesh_fusion writes it (its colours are averaged) '
                                                                  'or a third-party triangle-mesh PLY')
    parser.add_argument('--out', required=True, help='the simplified mesh (a binary PLY)')
    parser.add_argument('--cell', type=float, required=True, metavar='C', help='the edge of a cell in the mesh\'s unit (no default: it '
                                                                               'depends on the scene)')
    parser.add_argument('--placement', default=DEFAULT_PLACEMENT, help='quadric (Lindstrom\'s placement: keeps edges and corners; the '
                                                                       'default, not a measured winner) or mean')
    parser.add_argument('--origin', type=_origin_arg, default=None, metavar='x,y,z', help='the corner of cell (0,0,0), written '
                        '--origin=x,y,z where a number is negative (default: the lower bound of the finite vertices)')
    parser.add_argument('--rank_epsilon', type=float, default=DEFAULT_RANK_EPSILON, metavar='E',
                        help='eigenvalues of a quadric at or below E times the largest are left out (default %g, Lindstrom\'s value: a '
                             'default, not a measurement)' % DEFAULT_RANK_EPSILON)
    parser.add_argument('--report', default=None, metavar='FILE.json', help='write what was merged and dropped here (default: print it)')
    parser.add_argument('--gpu_id', type=int, default=0)
    return parser


def cli(argv=None):
    parser = make_parser()
    args = parser.parse_args(argv)
    for name in ('cell', 'placement', 'rank_epsilon', 'origin'):
        try:
            check_options(**dict(dict(cell=1.0), **{name: getattr(args, name)}))
        except ValueError as e:
            parser.error('--%s' % e)
    if not os.path.isfile(args.input):
        parser.error('--in %s: no such file' % args.input)
    try:
        vertices, colors, faces = read_mesh(args.input)
    except ValueError as e:
        parser.error('--in: %s' % e)
    import torch
    torch.cuda.set_device(args.gpu_id)
    vertices, colors, faces, report = simplify(vertices, colors, faces, args.cell, args.placement, args.origin, args.rank_epsilon)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    ply.write_mesh(args.out, vertices, colors, faces)
    if args.report:
        write_json(args.report, report)
    else:
        print(json.dumps(report, indent=1, sort_keys=True))
    return report


if __name__ == '__main__':
    cli()
