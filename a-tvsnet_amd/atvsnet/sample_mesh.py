"""Sample a triangle mesh's surface uniformly by area on the MI355X, so that a mesh can be scored as the surface it describes and
not as its vertices: DESIGN.md section 10.3e.  Tanks and Temples, Open3D and ETH3D all score a mesh this way.

    python -m atvsnet_amd.atvsnet.sample_mesh --in mesh.ply --out samples.ply (--spacing S | --density D | --count N) [--seed K]
           [--normals] [--report samples.json] [--gpu_id 0]

Every face gets area * density samples, the fraction rounded stochastically by the face's own hashed number (ops.mesh_sample_counts:
marching tetrahedra emit many faces that deserve less than one sample, a plain floor would leave whole surfaces empty), and each
sample is a hashed point of its face with the vertices' colours mixed and, with --normals, the face's unit normal
(ops.mesh_sample_points).  `--spacing S` is the density 1 / S^2, `--count N` the density N / area (a first pass measures the area;
the result has about N samples, the report says how many).  Every number is a hash of (seed, face, sample within the face): the same
mesh, density and seed give the same file on every run.

`--spacing` has no default.  For scoring, a spacing of at most half the smallest tolerance is what the measurements of section 10.3e
support.  What this is not: blue-noise or Poisson-disk sampling (the samples are independent, so they clump as Open3D's
sample_points_uniformly do), exact point-to-triangle distances, texture lookups.  There is no CPU fallback.  This module imports
without a GPU; only `sample` and `sample_device` need one.
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

REPORT_KEYS = ('vertices', 'faces', 'area', 'density', 'spacing', 'seed', 'samples', 'expected_samples', 'skipped_index_faces',
               'skipped_nonfinite_faces', 'max_per_face', 'seconds')
GREY = 128                   # the colour of a sample of a mesh without colours


def _positive(value, name):
    if isinstance(value, (bool, str, bytes)):
        raise ValueError('%s must be a positive finite number, got %r' % (name, value))
    try:
        x = float(value)
    except (TypeError, ValueError):
        raise ValueError('%s must be a positive finite number, got %r' % (name, value))
    if not (x > 0.0 and math.isfinite(x)):
        raise ValueError('%s must be a positive finite number, got %r' % (name, value))
    return x


def check_options(spacing=None, density=None, count=None, seed=0):
    """-> (density float or None, count int or None, seed int): exactly one of spacing (density 1 / spacing^2), density and count
    (density count / area, known after a first pass) must be given; ValueError names a bad one."""
    given = [k for k, v in (('spacing', spacing), ('density', density), ('count', count)) if v is not None]
    if len(given) != 1:
        raise ValueError('exactly one of spacing, density and count must be given, got %s' % (', '.join(given) or 'none'))
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < (1 << 63):
        raise ValueError('seed must be an integer in 0..2^63-1, got %r' % (seed,))
    if spacing is not None:
        s = _positive(spacing, 'spacing')
        density = 1.0 / (s * s) if s * s > 0.0 else float('inf')
        if not (density > 0.0 and math.isfinite(density)):
            raise ValueError('spacing must be a positive finite number whose density 1 / spacing^2 is one too, got %r' % (spacing,))
    elif density is not None:
        density = _positive(density, 'density')
    else:
        if isinstance(count, bool) or not isinstance(count, (int, np.integer)) or int(count) < 1:
            raise ValueError('count must be a positive integer, got %r' % (count,))
        count = int(count)
    return density, count, int(seed)


def sample_device(vertices, colors, faces, spacing=None, density=None, count=None, seed=0, normals=False):
    """vertices (V,3) float32, colors (V,3) uint8 or None, faces (F,3) int32 on the current device -> (ops.MeshSamples, report)
    with the samples still on the device."""
    import torch
    from .. import ops
    density, count, seed = check_options(spacing, density, count, seed)
    dev = vertices.device
    seconds = {}

    def timed(name, fn):
        torch.cuda.synchronize(dev)
        t0 = time.time()
        out = fn()
        torch.cuda.synchronize(dev)
        seconds[name] = time.time() - t0
        return out

    if density is None:
        # the area does not depend on the density: any density that cannot reach the limit measures it
        _, areas, _ = timed('area', lambda: ops.mesh_sample_counts(vertices, faces, 1e-300, seed))
        area = float(areas.sum().item()) if int(faces.shape[0]) else 0.0
        if not area > 0.0:
            raise ValueError('count: the mesh has no area to spread %d samples over' % count)
        density = count / area
    samples, info = timed('sample', lambda: ops.mesh_sample(vertices, colors, faces, density, seed, normals))
    report = {'vertices': int(vertices.shape[0]), 'faces': int(faces.shape[0]), 'area': info['area'], 'density': density,
              'spacing': 1.0 / math.sqrt(density), 'seed': seed, 'samples': info['samples'], 'expected_samples': info['area'] * density,
              'skipped_index_faces': info['skipped_index_faces'], 'skipped_nonfinite_faces': info['skipped_nonfinite_faces'],
              'max_per_face': info['max_per_face'], 'seconds': seconds}
    return samples, report


def sample(vertices, colors, faces, spacing=None, density=None, count=None, seed=0, normals=False, device=None):
    """Host arrays -> (points (S,3) float32, colors (S,3) uint8 or None, normals (S,3) float32 or None, report).  report:
    'vertices', 'faces', 'area' (the float64 sum of the faces' areas), 'density', 'spacing' (1 / sqrt(density)), 'seed', 'samples',
    'expected_samples' (area * density), 'skipped_index_faces', 'skipped_nonfinite_faces', 'max_per_face', 'seconds' per stage."""
    check_options(spacing, density, count, seed)
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
        got, report = sample_device(dv, dc, df, spacing, density, count, seed, normals)
        t0 = time.time()
        out = (got.points.cpu().numpy(), None if got.colors is None else got.colors.cpu().numpy(),
               None if got.normals is None else got.normals.cpu().numpy())
        report['seconds'].update(upload=upload, download=time.time() - t0)
    return out + (report,)


def make_parser():
    parser = argparse.ArgumentParser(description='sample a triangle mesh\'s surface uniformly by area on the GPU (independent samples: '
                                                 'no blue noise, no texture lookups)')
    parser.add_argument('--in', dest='input', required=True, help='the mesh: a PLY as mesh_fusion writes it (its colours are mixed) '
                                                                  'or a third-party triangle-mesh PLY')
    parser.add_argument('--out', required=True, help='the samples (a binary PLY point cloud; grey where the mesh has no colours)')
    how = parser.add_mutually_exclusive_group(required=True)
    how.add_argument('--spacing', type=float, default=None, metavar='S', help='one sample per S x S of surface in the mesh\'s unit (no '
                                                                               'default; for scoring at most half the smallest tolerance)')
    how.add_argument('--density', type=float, default=None, metavar='D', help='samples per unit area')
    how.add_argument('--count', type=int, default=None, metavar='N', help='about N samples: the density N / area')
    parser.add_argument('--seed', type=int, default=0, metavar='K', help='0..2^63-1 (default 0); the same seed gives the same samples')
    parser.add_argument('--normals', action='store_true', help='write each sample\'s face normal')
    parser.add_argument('--report', default=None, metavar='FILE.json', help='write the counts here (default: print them)')
    parser.add_argument('--gpu_id', type=int, default=0)
    return parser


def cli(argv=None):
    parser = make_parser()
    args = parser.parse_args(argv)
    try:
        check_options(args.spacing, args.density, args.count, args.seed)
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
    try:
        points, out_colors, normals, report = sample(vertices, colors, faces, args.spacing, args.density, args.count, args.seed, args.normals)
    except ValueError as e:
        parser.error(str(e))
    if out_colors is None:
        out_colors = np.full((len(points), 3), GREY, np.uint8)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    ply.write_ply(args.out, points, out_colors, normals)
    if args.report:
        write_json(args.report, report)
    else:
        print(json.dumps(report, indent=1, sort_keys=True))
    return report


if __name__ == '__main__':
    cli()
