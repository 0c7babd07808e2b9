"""The exact distance from every point of a cloud to a triangle mesh's surface on the MI355X -- what CloudCompare's cloud-to-mesh
distance and Tanks-and-Temples-style mesh scoring mean: DESIGN.md section 10.3f.

    python -m atvsnet_amd.atvsnet.mesh_distance --mesh M.ply --points P.ply --radius R [--out D.npy] [--closest C.ply]
           [--report R.json] [--max_refs N] [--gpu_id 0]

Per point the distance to the closest point of the closest triangle within R, found in double by the sequence include/atvsnet_hip.h
states and rounded once (ops.mesh_grid / ops.mesh_nearest, csrc/mesh_distance.hip); +inf in --out where no face is within R.  No
sample spacing enters.  --out: the distances (not squared) as a float32 .npy, one per point; --closest: the closest points of the
points that found a face, as a PLY cloud.  The report: `points`, `found`, `mean`, `median`, `max` of the found distances (None of
none), `faces`, `usable_faces`, `references`, `cell` (the grid's cell edge), `builds`, `radius`, `seconds`.

What this is not: a signed distance (no inside / outside), a mesh-to-mesh distance (the query side is points), a BVH (a uniform grid:
a mesh whose faces are far larger than R is searched through a coarser grid, by more faces per point).  There is no CPU fallback.
This module imports without a GPU; only `distance` needs one.
"""
from __future__ import print_function

import argparse
import json
import os
import time

import numpy as np

from ..tools import ply
from ..tools.common import write_json  # noqa: F401
from .clean_mesh import read_mesh

REPORT_KEYS = ('points', 'found', 'mean', 'median', 'max', 'faces', 'usable_faces', 'references', 'cell', 'builds', 'radius', 'seconds')


def check_options(radius, max_refs=None):
    """radius -> float: a positive finite number; max_refs None or an integer >= 0.  Anything else raises ValueError."""
    if isinstance(radius, (bool, str, bytes)) or not (float(radius) > 0.0 and np.isfinite(float(radius))):
        raise ValueError('radius must be a positive finite number, got %r' % (radius,))
    if max_refs is not None and (isinstance(max_refs, bool) or not isinstance(max_refs, int) or max_refs < 0):
        raise ValueError('max_refs must be an integer >= 0, got %r' % (max_refs,))
    return float(radius)


def distance(vertices, faces, points, radius, max_refs=None, closest=False, device=None):
    """Host arrays -> (d (m,) float32: the distances, +inf where no face is within `radius`; face (m,) int32, -1 there; closest (m,3)
    float32 or None, NaN there; report)."""
    radius = check_options(radius, max_refs)
    import torch
    from .. import ops
    v = np.ascontiguousarray(np.asarray(vertices, np.float32).reshape(-1, 3))
    f = np.ascontiguousarray(np.asarray(faces, np.int32).reshape(-1, 3))
    q = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    seconds = {}
    with torch.cuda.device(dev):
        t0 = time.time()
        dv, df, dq = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(q).to(dev)
        torch.cuda.synchronize()
        seconds['upload'] = time.time() - t0
        t0 = time.time()
        grid = ops.mesh_grid(dv, df, radius, max_refs)
        torch.cuda.synchronize()
        seconds['grid'] = time.time() - t0
        t0 = time.time()
        got = ops.mesh_nearest(grid, dq, closest=closest)
        torch.cuda.synchronize()
        seconds['search'] = time.time() - t0
        t0 = time.time()
        d2, face = got[0].cpu().numpy(), got[1].cpu().numpy()
        where = got[2].cpu().numpy() if closest else None
        seconds['download'] = time.time() - t0
    d = np.sqrt(d2.astype(np.float64))
    found = d[face >= 0]
    report = {'points': int(len(q)), 'found': int(len(found)), 'mean': float(found.mean()) if len(found) else None,
              'median': float(np.median(found)) if len(found) else None, 'max': float(found.max()) if len(found) else None,
              'faces': int(len(f)), 'usable_faces': grid.usable_faces, 'references': grid.refs, 'cell': grid.cell, 'builds': grid.rounds,
              'radius': grid.radius, 'seconds': seconds}
    return d.astype(np.float32), face, where, report


def make_parser():
    parser = argparse.ArgumentParser(description='the exact distance from every point of a cloud to a triangle mesh\'s surface, on the '
                                                 'GPU (unsigned; no samples, no spacing)')
    parser.add_argument('--mesh', required=True, help='the triangle mesh (PLY)')
    parser.add_argument('--points', required=True, help='the query points (PLY)')
    parser.add_argument('--radius', type=float, required=True, metavar='R', help='the search radius: a point further than R from '
                                                                                 'every face is not found')
    parser.add_argument('--out', default=None, metavar='D.npy', help='write the distances here (float32, +inf = not found)')
    parser.add_argument('--closest', default=None, metavar='C.ply', help='write the closest surface points of the found points here')
    parser.add_argument('--report', default=None, metavar='R.json', help='write the report here (default: print it)')
    parser.add_argument('--max_refs', type=int, default=None, metavar='N',
                        help='the grid\'s budget of face references (default: 32 per face, at least 2^20: a default, not a measurement); '
                             'cannot be seen in the result')
    parser.add_argument('--gpu_id', type=int, default=0)
    return parser


def cli(argv=None):
    parser = make_parser()
    args = parser.parse_args(argv)
    try:
        check_options(args.radius, args.max_refs)
    except ValueError as e:
        parser.error('--%s' % e)
    for name in ('mesh', 'points'):
        if not os.path.isfile(getattr(args, name)):
            parser.error('--%s %s: no such file' % (name, getattr(args, name)))
    try:
        vertices, _, faces = read_mesh(args.mesh)
    except ValueError as e:
        parser.error('--mesh: %s' % e)
    points = ply.read_ply_points(args.points)
    import torch
    torch.cuda.set_device(args.gpu_id)
    try:
        d, face, where, report = distance(vertices, faces, points, args.radius, args.max_refs, closest=args.closest is not None)
    except ValueError as e:
        parser.error(str(e))
    for path in (args.out, args.closest):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    if args.out:
        np.save(args.out, d)
    if args.closest:
        keep = where[face >= 0]
        ply.write_ply(args.closest, keep, np.full((len(keep), 3), 128, np.uint8), None)
    if args.report:
        write_json(args.report, report)
    else:
        print(json.dumps(report, indent=1, sort_keys=True))
    return report


if __name__ == '__main__':
    cli()
