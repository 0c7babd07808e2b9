"""Score the depth maps of a scene against a scan rendered into their cameras.

A user with an ETH3D or COLMAP scene has laser scans, not ground-truth depth maps.  Here the scan is splatted into every camera of
the scene on the device (ops.scan_render, csrc/scan_render.hip: the nearest depth per pixel, with a splat-and-tolerance test
against points seen through the holes of a nearer surface), and every predicted map is scored against its rendered map with the
reference's own metrics (eval_errors.calc_error, on the host: a map is a few 10^4 pixels).

    camera_rows          the driver's (2,4,4) cameras -> the 16 doubles per camera the kernel reads
    inverse_similarity   the inverse of a recon -> scan matrix (eval_cloud --register / --save_transform)
    render_scan          the scan, moved into the reconstruction's frame, rendered into the cameras; with occlusion meshes, the
                         pixels whose scan depth lies behind a mesh are taken out
    render_mesh          a triangle mesh rendered into the cameras (ops.mesh_render): an occluder, or the ground truth itself
    score_maps           calc_error per map, valid-pixel counts, coverage, the mean over the scored maps

This is NOT ETH3D's renderer: the scan's own visibility (which scanner position saw which point) and ETH3D's splat-file occluders
are not used; a point splat with a depth test stands in for the former.  Occlusion meshes (--occlusion_mesh) are rasterised exactly
(csrc/mesh_render.hip), and a mesh can be the ground truth itself (--gt_mesh).  `splat`, `occlusion_tol`
and `occlusion_mesh_tol` have defaults, not measurements.  This module imports without a GPU; only the renderers need one.

    python -m atvsnet_amd.atvsnet.eval_depth --scene <data_root>/eth3d/<scene> --maps <out>/<scene> --gt scan.ply[,...]
        [--transform T.txt] [--splat S --occlusion_tol E --pixel_centre C] --out depth_eval.json [--save_gt DIR]
        [--occlusion_mesh mesh.ply[,...] [--occlusion_mesh_tol E]]
    python -m atvsnet_amd.atvsnet.eval_depth --scene ... --maps ... --gt_mesh surface.ply[,...] [--occlusion_mesh ...] --out ...
"""
import argparse
import json
import os

import numpy as np

from ..tools.common import write_json  # noqa: F401
from . import eval_errors

DEFAULT_SPLAT = 2                  # a default, not a measurement: a 5 x 5 window closes the gaps of a scan about as dense as the map
DEFAULT_OCCLUSION_TOL = 0.05       # a default, not a measurement: 5 % of the depth
DEFAULT_OCCLUDER_TOL = 0.01        # a default, not a measurement: an occluder modelled ON the scan lies within 1 % of the scan's own depth
DEFAULT_PIXEL_CENTRE = 0.0         # fusion_pixel.h back-projects integer pixel coordinates: the convention that places the cloud
DEFAULT_MIN_VALID = 100            # as many jointly valid pixels as calc_error has depth bins
SIMILARITY_TOLERANCE = 1e-9

METRICS = eval_errors.err_metrics_namelist + eval_errors.acc_metrics_namelist


def camera_rows(cams):
    """cams (n,2,4,4) (or one (2,4,4)): [0] = extrinsic (world to camera), [1][:3,:3] = K, as eval_pointcloud writes them with
    write_cam for the 1/4-scale maps -> (n,16) float64 rows R (row-major), t, fx, fy, cx, cy.  A non-zero skew K[0,1] raises: the
    renderer's projection has none."""
    c = np.asarray(cams, np.float64)
    if c.ndim == 3:
        c = c[None]
    if c.ndim != 4 or c.shape[1:] != (2, 4, 4):
        raise ValueError('cams: expected (n,2,4,4) cameras, got shape %s' % (np.shape(cams),))
    if not np.isfinite(c[:, 0, :3, :4]).all() or not np.isfinite(c[:, 1, :3, :3]).all():
        raise ValueError('cams: a camera has a non-finite entry')
    K = c[:, 1, :3, :3]
    skew = np.nonzero(K[:, 0, 1] != 0.0)[0]
    if skew.size:
        raise ValueError('camera %d has skew K[0,1] = %r: scan_render projects with fx, fy, cx, cy only' % (skew[0], K[skew[0], 0, 1]))
    if (K[:, 1, 0] != 0.0).any() or (K[:, 2, :2] != 0.0).any() or (K[:, 2, 2] != 1.0).any():
        raise ValueError('cams: K must be [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]')
    rows = np.empty((len(c), 16), np.float64)
    rows[:, :9] = c[:, 0, :3, :3].reshape(len(c), 9)
    rows[:, 9:12] = c[:, 0, :3, 3]
    rows[:, 12], rows[:, 13], rows[:, 14], rows[:, 15] = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
    return rows


def inverse_similarity(T):
    """The inverse of a 4x4 similarity x -> s R x + t, in float64: [R^T / s | -R^T t / s].  Raises unless the last row is
    (0, 0, 0, 1) and the upper 3x3 is a scaled rotation within 1e-9 (A A^T = s^2 I, det > 0): the closed form is the inverse of
    nothing else."""
    T = np.asarray(T, np.float64)
    if T.size != 16 or not np.isfinite(T).all():
        raise ValueError('transform: expected the 16 finite numbers of a 4x4 matrix')
    T = T.reshape(4, 4)
    if not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError('transform: the last row must be 0 0 0 1, got %s' % T[3].tolist())
    A, t = T[:3, :3], T[:3, 3]
    G = A @ A.T
    s2 = float(np.trace(G)) / 3.0
    if not s2 > 0.0 or np.abs(G / s2 - np.eye(3)).max() > SIMILARITY_TOLERANCE or not np.linalg.det(A) > 0.0:
        raise ValueError('transform: the upper 3x3 is not a scaled rotation within %g (shear, unequal scales or a reflection)'
                         % SIMILARITY_TOLERANCE)
    inv = np.eye(4)
    inv[:3, :3] = A.T / s2
    inv[:3, 3] = -(A.T @ t) / s2
    return inv


def _camera_rows16(cams):
    c = np.asarray(cams, np.float64)
    return c if c.ndim == 2 and c.shape[1] == 16 else camera_rows(c)


def _points_on(points, dev, inv):
    """points (host array or tensor) -> (n,3) float32 on `dev`, moved by the 4x4 `inv` (ops.cloud_transform) unless it is None."""
    import torch
    from .. import ops
    if isinstance(points, torch.Tensor):
        p = points.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
    else:
        p = torch.from_numpy(np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))).to(dev)
    return p if inv is None else ops.cloud_transform(p, inv)


def concat_meshes(meshes):
    """[(vertices (V,3), faces (F,3)), ...] host arrays -> one (vertices float32, faces int32), face indices offset."""
    vs, fs, base = [], [], 0
    for v, f in meshes:
        v = np.asarray(v, np.float32).reshape(-1, 3)
        vs.append(v)
        fs.append(np.asarray(f, np.int64).reshape(-1, 3) + base)
        base += len(v)
    if not vs:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    return np.concatenate(vs, 0), np.concatenate(fs, 0).astype(np.int32)


def load_meshes(paths):
    """PLY triangle meshes (tools/ply.read_mesh where the file is this project's, ply.read_mesh_any otherwise) -> concat_meshes of
    them."""
    from ..tools import ply
    meshes = []
    for p in paths:
        try:
            v, _, f = ply.read_mesh(p)
        except (ValueError, IndexError):
            v, f = ply.read_mesh_any(p)
        meshes.append((v, f))
    return concat_meshes(meshes)


def render_mesh(vertices, faces, cams, rows, cols, transform=None, pixel_centre=DEFAULT_PIXEL_CENTRE, device=None):
    """vertices (V,3) float32 and faces (F,3) int32 (host arrays or device tensors); cams: (n_cams,2,4,4) driver cameras or
    (n_cams,16) rows.  transform: None, or the 4x4 recon -> scan matrix: the vertices are moved by its inverse exactly as render_scan
    moves the scan.  -> (depth (n_cams, rows, cols) float32, face (n_cams, rows, cols) int32) on the device (ops.mesh_render): the
    nearest depth of the mesh at every pixel centre and the face that gives it, (0, -1) where there is none."""
    import torch
    from .. import ops
    c = _camera_rows16(cams)
    inv = None if transform is None else inverse_similarity(transform)
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        v = _points_on(vertices, dev, inv)
        if isinstance(faces, torch.Tensor):
            f = faces.to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous()
        else:
            f = torch.from_numpy(np.ascontiguousarray(np.asarray(faces, np.int32).reshape(-1, 3))).to(dev)
        rows_d = torch.from_numpy(np.ascontiguousarray(c)).to(dev)
        return ops.mesh_render(v, f, rows_d, int(rows), int(cols), pixel_centre=pixel_centre)


def render_scan(points, cams, rows, cols, transform=None, pixel_centre=DEFAULT_PIXEL_CENTRE, splat=DEFAULT_SPLAT,
                occlusion_tol=DEFAULT_OCCLUSION_TOL, device=None, occluders=None, occluder_tol=DEFAULT_OCCLUDER_TOL):
    """points (n,3) float32 (host array or device tensor): the scan; cams: (n_cams,2,4,4) driver cameras or (n_cams,16) rows.
    transform: None, or the 4x4 recon -> scan matrix that eval_cloud --register found (--save_transform): the scan is moved by its
    inverse (ops.cloud_transform: float64, rounded once to float32) into the reconstruction's frame before it is rendered, so the
    depths come out in the reconstruction's units.  -> (n_cams, rows, cols) float32 on the device (ops.scan_render).

    occluders: None, or a list of (vertices, faces) occlusion meshes in the scan's frame.  They are concatenated, rendered by
    render_mesh under the same transform, and a pixel of the resolved scan map whose depth is further than the mesh's times
    (1 + occluder_tol) becomes 0 (ops.depth_occlude).  Applied after the scan is resolved, this is the test of every scan point
    against the occluder at its pixel: where the nearest point of a pixel is occluded, every farther one is too."""
    import torch
    from .. import ops
    c = _camera_rows16(cams)
    inv = None if transform is None else inverse_similarity(transform)
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        p = _points_on(points, dev, inv)
        rows_d = torch.from_numpy(np.ascontiguousarray(c)).to(dev)
        depth = ops.scan_render(p, rows_d, int(rows), int(cols), pixel_centre=pixel_centre, splat=splat, occlusion_tol=occlusion_tol)
        if occluders:
            v, f = concat_meshes(occluders)
            wall, _ = render_mesh(v, f, c, rows, cols, transform=transform, pixel_centre=pixel_centre, device=dev)
            ops.depth_occlude(depth, wall, tol=occluder_tol, out=depth)
        return depth


def _valid(a):
    with np.errstate(invalid='ignore'):
        return (a > 0.0) & (a < 1e10)          # calc_error's validity; NaN fails both


def score_maps(pred, gt, min_valid=DEFAULT_MIN_VALID, indices=None):
    """pred, gt (n,rows,cols) float32 host arrays -> a dict of plain Python values (JSON as it stands):
    maps: one entry per map: index (indices[k], default k), valid (pixels valid in both maps, calc_error's rule: finite, > 0,
    < 1e10), gt_valid, coverage (valid / pixels), skipped; a scored map also carries calc_error's metrics by name (the host
    eval_errors.calc_error, unchanged).  A map with fewer than min_valid jointly valid pixels is skipped, not scored.
    skipped: their indices.  n_scored, mean: the unweighted mean of every metric over the scored maps (None when there is none)."""
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    if pred.ndim != 3 or pred.shape != gt.shape:
        raise ValueError('pred %s and gt %s: expected two (n,rows,cols) stacks of one shape' % (pred.shape, gt.shape))
    if isinstance(min_valid, bool) or int(min_valid) != min_valid or int(min_valid) < 1:
        raise ValueError('min_valid: expected an integer >= 1, got %r' % (min_valid,))
    idx = list(range(len(pred))) if indices is None else [int(i) for i in indices]
    if len(idx) != len(pred):
        raise ValueError('%d indices for %d maps' % (len(idx), len(pred)))
    pixels = int(pred.shape[1] * pred.shape[2])
    maps, skipped, scored = [], [], []
    for k in range(len(pred)):
        gv = _valid(gt[k])
        n = int((gv & _valid(pred[k])).sum())
        entry = {'index': idx[k], 'valid': n, 'gt_valid': int(gv.sum()), 'coverage': n / float(pixels) if pixels else 0.0,
                 'skipped': n < int(min_valid)}
        if entry['skipped']:
            skipped.append(idx[k])
        else:
            with np.errstate(divide='ignore', invalid='ignore'):
                e, _ = eval_errors.calc_error(pred[k], gt[k])
            entry.update((name, float(v)) for name, v in zip(METRICS, e))
            scored.append(e.astype(np.float64))
        maps.append(entry)
    mean = None
    if scored:
        mean = dict((name, float(v)) for name, v in zip(METRICS, np.mean(np.stack(scored), axis=0)))
    return {'maps': maps, 'skipped': skipped, 'n_scored': len(scored), 'min_valid': int(min_valid), 'mean': mean}


def report(pred, gt, indices=None, min_valid=DEFAULT_MIN_VALID, transform=None, pixel_centre=DEFAULT_PIXEL_CENTRE,
           splat=DEFAULT_SPLAT, occlusion_tol=DEFAULT_OCCLUSION_TOL, occlusion_mesh_tol=None, occlusion_faces=None, gt_mesh=None):
    """score_maps plus the rendering's parameters: what depth_eval.json holds.  occlusion_mesh_tol and occlusion_faces (the
    occluders' tolerance and face count) and gt_mesh (the face count of a mesh that WAS the ground truth) appear only when given."""
    out = score_maps(pred, gt, min_valid=min_valid, indices=indices)
    out.update(rows=int(np.shape(pred)[1]), cols=int(np.shape(pred)[2]), pixel_centre=float(pixel_centre), splat=int(splat),
               occlusion_tol=float(occlusion_tol), transform=None if transform is None else np.asarray(transform, np.float64).reshape(4, 4).tolist())
    if occlusion_faces is not None or occlusion_mesh_tol is not None:
        out.update(occlusion_mesh_tol=float(DEFAULT_OCCLUDER_TOL if occlusion_mesh_tol is None else occlusion_mesh_tol),
                   occlusion_faces=int(occlusion_faces or 0))
    if gt_mesh is not None:
        out.update(gt_mesh=int(gt_mesh))
    return out


def scene_indices(scene_folder):
    """The reference image indices of <scene_folder>/pair.txt, in its order."""
    with open(os.path.join(scene_folder, 'pair.txt')) as f:
        tok = iter(f.read().split())
    out = []
    for _ in range(int(next(tok))):
        out.append(int(next(tok)))
        for _ in range(2 * int(next(tok))):
            next(tok)
    return out


def load_maps(maps_folder, indices=None):
    """The driver's output of one scene: <maps_folder>[/depths_atvsnet]/%08d.pfm (depth) and %08d.txt (the 1/4-scale camera) ->
    (indices, depth (n,rows,cols) float32, cams (n,2,4,4) float64), ascending by index.  indices: the maps to load (a missing one
    raises); None: every %08d.pfm that has its camera."""
    from .preprocess import load_cam, load_pfm
    folder = os.path.join(maps_folder, 'depths_atvsnet')
    if not os.path.isdir(folder):
        folder = maps_folder
    if indices is None:
        indices = [int(name[:8]) for name in os.listdir(folder)
                   if len(name) == 12 and name.endswith('.pfm') and name[:8].isdigit() and os.path.exists(os.path.join(folder, name[:8] + '.txt'))]
    indices = sorted(set(int(i) for i in indices))
    if not indices:
        raise ValueError('%s: no depth maps (%%08d.pfm with %%08d.txt)' % folder)
    depth, cams = [], []
    for i in indices:
        stem = os.path.join(folder, '%08d' % i)
        for ext in ('.pfm', '.txt'):
            if not os.path.exists(stem + ext):
                raise ValueError('%s%s is missing' % (stem, ext))
        with open(stem + '.pfm', 'rb') as f:
            depth.append(np.asarray(load_pfm(f), np.float32))
        with open(stem + '.txt') as f:
            cams.append(load_cam(f, 1.0))
        if depth[-1].ndim != 2 or depth[-1].shape != depth[0].shape:
            raise ValueError('%s.pfm: shape %s, the first map has %s: one scene holds maps of one size' % (stem, depth[-1].shape, depth[0].shape))
    return indices, np.stack(depth), np.stack(cams)


def add_options(parser, prefix=''):
    """The rendering options --<prefix>splat, occlusion_tol, pixel_centre, occlusion_mesh, occlusion_mesh_tol ('map_': the ETH3D driver's)."""
    parser.add_argument('--%ssplat' % prefix, type=int, default=DEFAULT_SPLAT, help='half-width of the occlusion window in pixels, 0..4')
    parser.add_argument('--%socclusion_tol' % prefix, type=float, default=DEFAULT_OCCLUSION_TOL,
                        help='a pixel is kept when its depth is within (1 + this) of the nearest depth in its window')
    parser.add_argument('--%spixel_centre' % prefix, type=float, default=DEFAULT_PIXEL_CENTRE,
                        help='image coordinate of the centre of pixel (0,0): 0 (the fusion\'s convention) or 0.5 (the plane sweep\'s)')
    parser.add_argument('--%socclusion_mesh' % prefix, default=None, metavar='FILE[,FILE...]',
                        help='triangle-mesh PLY file(s) in the ground truth\'s frame: a rendered ground-truth pixel that lies behind '
                             'them is taken out')
    parser.add_argument('--%socclusion_mesh_tol' % prefix, type=float, default=None, metavar='E' if prefix else None,      # as each tool had it
                        help='a pixel is kept when its depth is within (1 + this) of the occlusion mesh\'s (default %g)' % DEFAULT_OCCLUDER_TOL)


def options(parser, args, prefix=''):
    """The options of add_options as render_scan's splat, occlusion_tol and pixel_centre, with occlusion_mesh (the list of files) and
    occlusion_mesh_tol when given; a bad splat or occlusion mesh option is an argument error.  parser None: nothing is checked, and
    an option `args` lacks has its default.  This is the ETH3D driver's score_maps (with gt_ply only): after the scene's fusion the
    ground truth is rendered into the scene's cameras (in SceneFusion.order()) and the staged, probability-filtered depth planes --
    what enters the cloud -- are scored against it (score_maps) into <savepath>/<scene>/depth_eval.json.  With register the ground
    truth is moved by the inverse of the matrix already found (no second fit).  A rendered pixel that lies behind the meshes of
    occlusion_mesh= (in the ground truth's frame), within occlusion_mesh_tol=, is taken out first (render_scan's occluders)."""
    get = lambda name, default=None: getattr(args, prefix + name, default)          # noqa: E731
    out = dict(splat=get('splat', DEFAULT_SPLAT), occlusion_tol=get('occlusion_tol', DEFAULT_OCCLUSION_TOL),
               pixel_centre=get('pixel_centre', DEFAULT_PIXEL_CENTRE))
    files, tol = get('occlusion_mesh'), get('occlusion_mesh_tol')
    if parser is not None:
        if not 0 <= out['splat'] <= 4:
            parser.error('--%ssplat must be in 0..4' % prefix)
        if tol is not None and files is None:
            parser.error('--%socclusion_mesh_tol needs --%socclusion_mesh' % (prefix, prefix))
        if tol is not None and not (tol >= 0.0 and np.isfinite(tol)):
            parser.error('--%socclusion_mesh_tol must be >= 0 and finite' % prefix)
    if files:
        files = [p for p in files.split(',') if p] if isinstance(files, str) else list(files)
    if parser is not None and files is not None and not files:
        parser.error('--%socclusion_mesh names no file' % prefix)
    if files:
        out.update({'occlusion_mesh': files}, **({} if tol is None else {'occlusion_mesh_tol': tol}))
    return out


def make_parser():
    parser = argparse.ArgumentParser(description='score the depth maps of a scene against a scan rendered into their cameras '
                                                 '(a point splat with a depth test; not ETH3D\'s renderer)')
    parser.add_argument('--scene', default=None, help='<data_root>/eth3d/<scene>: its pair.txt names the maps to score '
                                                      '(default: every map found under --maps)')
    parser.add_argument('--maps', required=True, help='<savepath>/<scene> of eval_pointcloud: depths_atvsnet/%%08d.pfm and %%08d.txt')
    parser.add_argument('--gt', default=None, metavar='FILE[,FILE...]', help='the scan: PLY file(s), concatenated')
    parser.add_argument('--gt_mesh', default=None, metavar='FILE[,FILE...]',
                        help='instead of --gt: triangle-mesh PLY file(s); the ground-truth maps are the rendered mesh itself '
                             '(--splat and --occlusion_tol do not apply)')
    parser.add_argument('--transform', default=None, metavar='FILE',
                        help='text file with the 4x4 recon -> scan matrix (eval_cloud --save_transform); the scan is moved by its inverse')
    add_options(parser)
    parser.add_argument('--min_valid', type=int, default=DEFAULT_MIN_VALID, help='maps with fewer jointly valid pixels are skipped')
    parser.add_argument('--out', default=None, help='write the result as JSON here (default: print it)')
    parser.add_argument('--save_gt', default=None, metavar='DIR', help='write the rendered maps as DIR/%%08d_gt.npy')
    parser.add_argument('--gpu_id', type=int, default=0)
    return parser


def cli(argv=None):
    parser = make_parser()
    args = parser.parse_args(argv)
    render = options(parser, args)
    occ_paths, occ_tol = render.pop('occlusion_mesh', []), render.pop('occlusion_mesh_tol', DEFAULT_OCCLUDER_TOL)
    if not (args.occlusion_tol >= 0.0 and np.isfinite(args.occlusion_tol)):
        parser.error('--occlusion_tol must be >= 0 and finite')
    if not np.isfinite(args.pixel_centre):
        parser.error('--pixel_centre must be finite')
    if args.min_valid < 1:
        parser.error('--min_valid must be at least 1')
    if (args.gt is None) == (args.gt_mesh is None):
        parser.error('exactly one of --gt and --gt_mesh is required')
    gt_paths = [p for p in (args.gt if args.gt is not None else args.gt_mesh).split(',') if p]
    if not gt_paths:
        parser.error('%s names no file' % ('--gt' if args.gt is not None else '--gt_mesh'))
    for p in gt_paths + occ_paths + ([args.transform] if args.transform else []):
        if not os.path.isfile(p):
            parser.error('%s: no such file' % p)
    if not os.path.isdir(args.maps):
        parser.error('--maps %s: no such folder' % args.maps)
    if args.scene is not None and not os.path.isfile(os.path.join(args.scene, 'pair.txt')):
        parser.error('--scene %s: no pair.txt' % args.scene)
    from ..tools import ply
    from .eval_cloud import load_matrix
    transform = None
    if args.transform:
        try:
            transform = load_matrix(args.transform)
            inverse_similarity(transform)
        except ValueError as e:
            parser.error('--transform %s: %s' % (args.transform, e))
    indices, pred, cams = load_maps(args.maps, scene_indices(args.scene) if args.scene is not None else None)
    extra = {}
    try:
        occluder = load_meshes(occ_paths) if occ_paths else None
        surface = load_meshes(gt_paths) if args.gt_mesh is not None else None
    except ValueError as e:
        parser.error(str(e))
    if occluder is not None:
        extra.update(occlusion_mesh_tol=occ_tol, occlusion_faces=len(occluder[1]))
    import torch
    torch.cuda.set_device(args.gpu_id)
    if surface is None:
        scan = np.concatenate([ply.read_ply_points(p) for p in gt_paths], 0)
        gt = render_scan(scan, cams, pred.shape[1], pred.shape[2], transform=transform, occluders=occluder and [occluder],
                         occluder_tol=occ_tol, **render).cpu().numpy()
    else:
        from .. import ops
        extra.update(gt_mesh=len(surface[1]))
        gt, _ = render_mesh(surface[0], surface[1], cams, pred.shape[1], pred.shape[2], transform=transform, pixel_centre=args.pixel_centre)
        if occluder is not None:
            wall, _ = render_mesh(occluder[0], occluder[1], cams, pred.shape[1], pred.shape[2], transform=transform,
                                  pixel_centre=args.pixel_centre)
            ops.depth_occlude(gt, wall, tol=occ_tol, out=gt)
        gt = gt.cpu().numpy()
    if args.save_gt:
        os.makedirs(args.save_gt, exist_ok=True)
        for i, g in zip(indices, gt):
            np.save(os.path.join(args.save_gt, '%08d_gt.npy' % i), g)
    result = report(pred, gt, indices=indices, min_valid=args.min_valid, transform=transform, **dict(render, **extra))
    if args.out:
        write_json(args.out, result)
    else:
        print(json.dumps(result, indent=1, sort_keys=True))
    return result


if __name__ == '__main__':
    cli()
