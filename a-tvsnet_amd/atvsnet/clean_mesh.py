"""Clean a triangle mesh on the MI355X: find its connected components and remove the ones that are too small (DESIGN.md section
10.3a).  The mesh's counterpart of clean_cloud: depth noise that survives the probability filter in two views meshes into small
shells floating off the surface, and a score or a rendering should not see them.

    python -m atvsnet_amd.atvsnet.clean_mesh --in mesh.ply --out clean.ply [--min_faces N] [--min_ratio R] [--keep_largest K]
           [--report clean.json] [--gpu_id 0]

Two vertices are connected when one face names both (ops.mesh_components).  A component is kept when ALL the criteria given hold:

    min_faces N       it has at least N faces
    min_ratio R       it has at least R times the faces of the largest component, compared exactly: R is read as the rational it
                      is written as (the string '0.1' is 1/10, a float is the binary fraction it holds) and count * den >=
                      num * largest is decided in integers
    keep_largest K    it is among the K components with the most faces, ties going to the lower id (the component whose
                      smallest vertex index is lower)

No criterion has a default: which fragments are noise depends on the scene and the voxel, and nothing here was measured.  The
faces that stay keep their order, the vertices they name keep theirs, the faces are renumbered (ops.mesh_select); the edge census
(ops.mesh_edge_census) is taken before and after.  Everything between the upload and the download stays on the device; the
criteria are decided on the host from the per-component counts, one number per component.  There is no CPU fallback.  What this is
not: components by shared edge rather than shared vertex, criteria by area, hole filling, normals (simplification is atvsnet/simplify_mesh.py).  This module
imports without a GPU; only `clean` and `clean_device` need one.
"""
from __future__ import print_function

import argparse
import json
import os
import time
from fractions import Fraction

import numpy as np

from ..tools import ply
from ..tools.common import write_json  # noqa: F401

REPORT_LARGEST = 16               # the report lists the sizes of this many largest components


def check_criteria(min_faces=None, min_ratio=None, keep_largest=None):
    """-> (min_faces int or None, min_ratio Fraction or None, keep_largest int or None); ValueError names a bad one, or that none
    is given."""
    if min_faces is None and min_ratio is None and keep_largest is None:
        raise ValueError('clean: at least one of min_faces, min_ratio, keep_largest is needed')
    if min_faces is not None:
        if isinstance(min_faces, bool) or int(min_faces) != min_faces or int(min_faces) < 1:
            raise ValueError('min_faces must be a positive integer, got %r' % (min_faces,))
        min_faces = int(min_faces)
    if min_ratio is not None:
        try:
            ratio = Fraction(min_ratio)
        except (TypeError, ValueError, OverflowError):
            raise ValueError('min_ratio must be a number in 0..1, got %r' % (min_ratio,))
        if not 0 <= ratio <= 1:
            raise ValueError('min_ratio must be a number in 0..1, got %r' % (min_ratio,))
        min_ratio = ratio
    if keep_largest is not None:
        if isinstance(keep_largest, bool) or int(keep_largest) != keep_largest or int(keep_largest) < 1:
            raise ValueError('keep_largest must be a positive integer, got %r' % (keep_largest,))
        keep_largest = int(keep_largest)
    return min_faces, min_ratio, keep_largest


def keep_components(face_count, min_faces=None, min_ratio=None, keep_largest=None):
    """face_count (C,) integers, the faces of components 0..C-1 -> (C,) bool: the components that meet every criterion given."""
    min_faces, min_ratio, keep_largest = check_criteria(min_faces, min_ratio, keep_largest)
    counts = [int(n) for n in np.asarray(face_count).reshape(-1)]
    keep = np.ones(len(counts), bool)
    if not counts:
        return keep
    if min_faces is not None:
        keep &= np.array([n >= min_faces for n in counts])
    if min_ratio is not None:
        largest = max(counts)
        keep &= np.array([n * min_ratio.denominator >= min_ratio.numerator * largest for n in counts])      # Python integers: exact
    if keep_largest is not None:
        ranked = sorted(range(len(counts)), key=lambda k: (-counts[k], k))
        among = np.zeros(len(counts), bool)
        among[ranked[:keep_largest]] = True
        keep &= among
    return keep


def _criteria_report(min_faces, min_ratio, keep_largest):
    return {'min_faces': min_faces, 'min_ratio': None if min_ratio is None else str(min_ratio), 'keep_largest': keep_largest}


def clean_device(vertices, colors, faces, min_faces=None, min_ratio=None, keep_largest=None):
    """vertices (V,3) float32, colors (V,3) uint8 or None, faces (F,3) int32 on the current device -> (vertices, colors, faces,
    report) with the kept mesh still on the device.  The per-component face counts (C numbers) cross to the host, where the
    criteria are decided; the flags go back."""
    import torch
    from .. import ops
    criteria = check_criteria(min_faces, min_ratio, keep_largest)
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
    _, face_component, face_count, _ = timed('components', lambda: ops.mesh_components(faces, nv))

    def choose():
        keep = keep_components(face_count.cpu().numpy(), *criteria)
        flags = torch.from_numpy(keep.astype(np.uint8)).to(dev)
        return keep, (flags[face_component.long()].contiguous() if nf else torch.zeros(0, dtype=torch.uint8, device=dev))

    keep, keep_faces = timed('criteria', choose)
    out_v, out_c, out_f, _ = timed('select', lambda: ops.mesh_select(vertices, colors, faces, keep_faces))
    census_out = timed('census_after', lambda: ops.mesh_edge_census(out_f, int(out_v.shape[0])))
    sizes = sorted((int(n) for n in face_count.cpu().tolist()), reverse=True)
    report = {'criteria': _criteria_report(*criteria), 'components': len(sizes), 'largest_components': sizes[:REPORT_LARGEST],
              'components_removed': int((~keep).sum()), 'faces_in': nf, 'vertices_in': nv, 'faces_out': int(out_f.shape[0]),
              'vertices_out': int(out_v.shape[0]), 'census_in': census_in, 'census_out': census_out, 'seconds': seconds}
    return out_v, out_c, out_f, report


def clean(vertices, colors, faces, min_faces=None, min_ratio=None, keep_largest=None, device=None):
    """vertices (V,3) float32, colors (V,3) uint8 or None, faces (F,3) int32: host arrays -> (vertices, colors, faces, report), the
    mesh without the components that miss a criterion, as host arrays (colors None when none were given).  report: 'components',
    'largest_components' (the sizes of the 16 largest, descending), 'faces_in' / 'vertices_in' / 'faces_out' / 'vertices_out',
    'components_removed', 'census_in' / 'census_out' (ops.mesh_edge_census), 'criteria', 'seconds' per stage."""
    check_criteria(min_faces, min_ratio, keep_largest)
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
        out_v, out_c, out_f, report = clean_device(dv, dc, df, min_faces, min_ratio, keep_largest)
        t0 = time.time()
        out = (out_v.cpu().numpy(), None if out_c is None else out_c.cpu().numpy(), out_f.cpu().numpy())
        report['seconds'].update(upload=upload, download=time.time() - t0)
    return out + (report,)


def add_options(parser, prefix=''):
    """The three criteria's options, named --<prefix>min_faces, --<prefix>min_ratio, --<prefix>keep_largest.  None has a default."""
    parser.add_argument('--%smin_faces' % prefix, type=int, default=None, metavar='N',
                        help='remove a connected component of the mesh with fewer than N faces (no default)')
    parser.add_argument('--%smin_ratio' % prefix, default=None, metavar='R',
                        help='remove a component with fewer than R times the faces of the largest one; R in 0..1, read as the '
                             'decimal or fraction it is written as and compared exactly (no default)')
    parser.add_argument('--%skeep_largest' % prefix, type=int, default=None, metavar='K',
                        help='keep only the K components with the most faces, ties going to the lower vertex index (no default)')


def options(parser, args, prefix=''):
    """The parsed options of add_options as clean's keyword arguments ({} when none is given); a bad one is an argument error.
    parser None: nothing is checked, and an option `args` lacks is not given."""
    out = {}
    for name in ('min_faces', 'min_ratio', 'keep_largest'):
        if getattr(args, prefix + name, None) is not None:
            out[name] = getattr(args, prefix + name)
    if out and parser is not None:
        try:
            check_criteria(**out)
        except ValueError as e:
            parser.error('--%s%s' % (prefix, e))
    return out


def make_parser():
    parser = argparse.ArgumentParser(description='clean a triangle mesh on the GPU: remove the connected components that are too '
                                                 'small (no hole filling; simplification is atvsnet/simplify_mesh.py)')
    parser.add_argument('--in', dest='input', required=True, help='the mesh: a PLY as mesh_fusion writes it (its colours are kept) '
                                                                  'or a third-party triangle-mesh PLY')
    parser.add_argument('--out', required=True, help='the cleaned mesh (a binary PLY)')
    add_options(parser)
    parser.add_argument('--report', default=None, metavar='FILE.json', help='write what was found and removed here (default: print it)')
    parser.add_argument('--gpu_id', type=int, default=0)
    return parser


def read_mesh(path):
    """-> (vertices, colors or None, faces): ply.read_mesh where the file has write_mesh's layout (its colours are kept), else
    ply.read_mesh_any."""
    try:
        return ply.read_mesh(path)
    except (ValueError, UnicodeDecodeError):
        vertices, faces = ply.read_mesh_any(path)
        return vertices, None, faces


def cli(argv=None):
    parser = make_parser()
    args = parser.parse_args(argv)
    criteria = options(parser, args)
    if not criteria:
        parser.error('nothing to do: give at least one of --min_faces, --min_ratio, --keep_largest')
    if not os.path.isfile(args.input):
        parser.error('--in %s: no such file' % args.input)
    try:
        vertices, colors, faces = read_mesh(args.input)
    except ValueError as e:
        parser.error('--in: %s' % e)
    import torch
    torch.cuda.set_device(args.gpu_id)
    vertices, colors, faces, report = clean(vertices, colors, faces, **criteria)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    ply.write_mesh(args.out, vertices, colors, faces)
    if args.report:
        write_json(args.report, report)
    else:
        print(json.dumps(report, indent=1, sort_keys=True))
    return report


if __name__ == '__main__':
    cli()
