"""A triangle mesh of a scene from its depth maps, on the device: the probability-filtered depth maps and
the images a scene's fusion holds are integrated into a block-sparse TSDF volume (ops.tsdf_integrate) and the volume is meshed by
marching tetrahedra (ops.tsdf_mesh), both csrc/tsdf.hip.

    mesh_maps      depth maps, cameras, images and a box -> the volume, the mesh, seconds per stage
    SceneMesh      the mesh of a depth_fusion.SceneFusion: its staged planes in fusion order, the box of its fused points
    mesh_report    blocks, valid voxels, vertices, faces, zero-area faces, boundary edges (ops.mesh_edge_census for a mesh on a GPU)
    render_views   the mesh rendered into cameras (ops.mesh_render), one %08d_mesh.pfm per map
    clean=         SceneMesh and the tool also give the mesh without its small connected components (clean_mesh, section 10.3a)
    simplify=      SceneMesh also gives the mesh -- the cleaned one with clean= -- simplified by vertex clustering on a lattice of
                   cell_voxels voxels (simplify_mesh, section 10.3d); off unless asked
    smooth=        SceneMesh also gives the mesh -- the cleaned one with clean= -- smoothed by Taubin's filter, with vertex normals when
                   asked (smooth_mesh, section 10.3g); simplify= then takes the smoothed mesh; off unless asked
    score=         SceneMesh.score samples each of these meshes' surfaces on the device (sample_mesh, section 10.3e) and scores the
                   samples against a ground truth (eval_cloud.evaluate); the ETH3D driver writes mesh_eval*.json; off unless asked

    carve_weight=  free-space carving (section 10.3b): a view that sees past a voxel pulls its value outside, so a shell that two views
                   agree on and the others look through is not meshed; off (None) unless asked

    consistent=    the fusion's geometric test per pixel (section 10.3c): only the depths that num_consistent other views agree on are
                   integrated -- the samples the point cloud is made of (ops.fusion_support); off unless asked
    weights=       per-pixel view weights (section 10.3c): 'agree', (1 + agreeing views) / (1 + num_consistent) from the same launch,
                   or on written maps 'prob', the probability map's value; a view then counts w where it counted 1; off unless asked
                   (SceneMesh's arguments; on written maps the command atvsnet/mesh_consistent.py, this tool with four more options)

What this is not: there are no weights from the viewing angle, the ETH3D driver has no probability weights (its staged slab does not
keep the probabilities; mesh_consistent reads them from the files) and no command-line option for consistent=, weights= and
simplify=, smooth= and score= (they are run_eval_pc's mesh arguments; a written mesh is simplified by the command
atvsnet/simplify_mesh.py and smoothed by atvsnet/smooth_mesh.py), no hole filling, and only the smoothed mesh's PLY carries normals
(smooth=dict(..., normals=True)).
Without carve_weight a view adds to a voxel only inside the narrow band around its depth.  Fragments are removed only when asked
(the clean_ options have no defaults).  `trunc_voxels` and `min_weight` have defaults, not measurements.  This module imports
without a GPU.

    python -m atvsnet_amd.atvsnet.mesh_fusion --scene <data_root>/eth3d/<scene> --maps <out>/<scene> --voxel V
        [--trunc_voxels 4 --min_weight 2 --prob_threshold 0.8 --pixel_centre 0 --max_blocks N --report mesh.json] --out mesh.ply
        [--carve [CW]] [--render DIR] [--clean_min_faces N --clean_min_ratio R --clean_keep_largest K --clean_out clean.ply]
"""
import argparse
import json
import os
import time

import numpy as np

from ..tools.common import write_json  # noqa: F401
from . import clean_mesh, eval_depth, sample_mesh, simplify_mesh, smooth_mesh

DEFAULT_TRUNC_VOXELS = 4.0         # a default, not a measurement: the band reaches four voxels either side of a depth
DEFAULT_MIN_WEIGHT = 2.0           # a default, not a measurement: the fusion's num_consistent
DEFAULT_MAX_BLOCKS = 131072        # 64 Mi voxels: 1.3 GB of tsdf, weight and colour while the volume is built
DEFAULT_PIXEL_CENTRE = 0.0         # fusion_pixel.h back-projects integer pixel coordinates: the convention that places the cloud
DEFAULT_CARVE_WEIGHT = 1.0         # a default, not a measurement: what a bare --carve gives a free vote, one in-band view's worth
WEIGHT_MODES = ('agree',)          # SceneMesh's and the ETH3D driver's: (1 + count) / (1 + num_consistent) of ops.fusion_support
TOOL_WEIGHT_MODES = ('agree', 'prob')      # the tool also reads the probability maps that stand beside the depth maps


def check_options(voxel, trunc_voxels=DEFAULT_TRUNC_VOXELS, min_weight=DEFAULT_MIN_WEIGHT, max_blocks=DEFAULT_MAX_BLOCKS,
                  pixel_centre=DEFAULT_PIXEL_CENTRE, render=False, clean=None, carve_weight=None, consistent=False, weights=None,
                  simplify=None, score=None, smooth=None):
    """-> the options as (voxel, trunc_voxels, min_weight, max_blocks, pixel_centre); a bad one raises ValueError.  render (whether
    the driver also renders the mesh) has nothing to check; clean (None, or a dict of clean_mesh.clean's criteria) is checked there,
    carve_weight by check_carve_weight, consistent and weights by check_support, simplify by check_simplify, score by check_score,
    smooth by check_smooth (they are not part of the tuple)."""
    if clean is not None:
        clean_mesh.check_criteria(**clean)
    check_simplify(simplify)
    check_smooth(smooth)
    check_score(score)
    check_carve_weight(carve_weight)
    check_support(consistent, weights)
    voxel, trunc_voxels, min_weight, pixel_centre = float(voxel), float(trunc_voxels), float(min_weight), float(pixel_centre)
    if not (voxel > 0.0 and np.isfinite(voxel)):
        raise ValueError('mesh voxel must be positive and finite, got %r' % (voxel,))
    if not (trunc_voxels >= 1.0 and np.isfinite(trunc_voxels)):
        raise ValueError('mesh trunc_voxels must be at least 1 and finite, got %r' % (trunc_voxels,))
    if not (min_weight >= 1.0 and np.isfinite(min_weight)):
        raise ValueError('mesh min_weight must be at least 1 and finite, got %r' % (min_weight,))
    if int(max_blocks) != max_blocks or int(max_blocks) < 1:
        raise ValueError('mesh max_blocks must be a positive integer, got %r' % (max_blocks,))
    if not np.isfinite(pixel_centre):
        raise ValueError('mesh pixel_centre must be finite, got %r' % (pixel_centre,))
    return voxel, trunc_voxels, min_weight, int(max_blocks), pixel_centre


def check_carve_weight(carve_weight):
    """-> None (no carving) or the weight of a free vote as a float; anything but None or a finite number > 0 raises ValueError."""
    if carve_weight is None:
        return None
    if isinstance(carve_weight, (bool, str, bytes)):
        raise ValueError('mesh carve_weight must be a finite number > 0, got %r' % (carve_weight,))
    try:
        cw = float(carve_weight)
    except (TypeError, ValueError):
        raise ValueError('mesh carve_weight must be a finite number > 0, got %r' % (carve_weight,))
    if not (cw > 0.0 and np.isfinite(cw)):
        raise ValueError('mesh carve_weight must be a finite number > 0, got %r' % (carve_weight,))
    return cw


def check_simplify(simplify):
    """-> None (no simplification) or (cell_voxels float, placement, rank_epsilon): simplify is a dict(cell_voxels=R[, placement=,
    rank_epsilon=]); the cell is R voxels and its origin the volume's, so the cells sit on the voxel lattice.  Anything else raises
    ValueError."""
    if simplify is None:
        return None
    if not isinstance(simplify, dict) or 'cell_voxels' not in simplify or set(simplify) - {'cell_voxels', 'placement', 'rank_epsilon'}:
        raise ValueError('mesh simplify must be a dict(cell_voxels=R[, placement=, rank_epsilon=]), got %r' % (simplify,))
    try:
        cell, placement, _, rank_epsilon = simplify_mesh.check_options(
            simplify['cell_voxels'], simplify.get('placement', simplify_mesh.DEFAULT_PLACEMENT), None,
            simplify.get('rank_epsilon', simplify_mesh.DEFAULT_RANK_EPSILON))
    except ValueError as e:
        raise ValueError('mesh simplify: %s' % str(e).replace('cell must', 'cell_voxels must'))
    return cell, placement, rank_epsilon


def check_smooth(smooth):
    """-> None (no smoothing) or dict(iterations=, lam=, mu=, pin_boundary=, normals=) with smooth_mesh's defaults filled in: smooth
    is a dict(iterations=N[, lam=, mu=, pin_boundary=, normals=]); mu=None is Laplacian smoothing.  Anything else raises
    ValueError."""
    if smooth is None:
        return None
    if not isinstance(smooth, dict) or 'iterations' not in smooth or set(smooth) - {'iterations', 'lam', 'mu', 'pin_boundary', 'normals'}:
        raise ValueError('mesh smooth must be a dict(iterations=N[, lam=, mu=, pin_boundary=, normals=]), got %r' % (smooth,))
    try:
        iterations, lam, mu, pin_boundary, normals, _ = smooth_mesh.check_options(
            smooth['iterations'], smooth.get('lam', smooth_mesh.DEFAULT_LAMBDA), smooth.get('mu', smooth_mesh.DEFAULT_MU),
            smooth.get('pin_boundary', False), smooth.get('normals', False))
    except ValueError as e:
        raise ValueError('mesh smooth: %s' % e)
    return dict(iterations=iterations, lam=lam, mu=mu, pin_boundary=pin_boundary, normals=normals)


def check_score(score):
    """-> None (the meshes are not scored) or (spacing float, seed int): score is a dict(spacing=S[, seed=K]), the spacing of the
    surface samples in the scene's unit (no default: at most half the smallest tolerance, section 10.3e) and their seed (default 0).
    Anything else raises ValueError."""
    if score is None:
        return None
    if not isinstance(score, dict) or 'spacing' not in score or set(score) - {'spacing', 'seed', 'exact'}:
        raise ValueError('mesh score must be a dict(spacing=S[, seed=K]) with at most exact=True beside them, got %r' % (score,))
    if not isinstance(score.get('exact', False), bool):
        raise ValueError('mesh score: exact must be True or False, got %r' % (score['exact'],))
    try:
        density, _, seed = sample_mesh.check_options(spacing=score['spacing'], seed=score.get('seed', 0))
    except ValueError as e:
        raise ValueError('mesh score: %s' % e)
    return float(score['spacing']), seed


def check_score_exact(score):
    """Whether a score dict that check_score accepts asks for exact completeness (exact=True): the distance of every ground-truth
    point to the mesh itself (section 10.3f) instead of to its samples.  False for None."""
    check_score(score)
    return bool(score is not None and score.get('exact', False))


def check_support(consistent=False, weights=None, modes=WEIGHT_MODES):
    """-> (consistent as a bool, weights as None or one of `modes`); anything else raises ValueError."""
    if not isinstance(consistent, (bool, np.bool_)):
        raise ValueError('mesh consistent must be True or False, got %r' % (consistent,))
    if weights is not None and (not isinstance(weights, str) or weights not in modes):
        raise ValueError('mesh weights must be None or one of %s, got %r' % (', '.join(modes), weights))
    return bool(consistent), weights


def box_of(lo, hi, voxel, trunc):
    """The volume's box around the points' bounds lo, hi (3 numbers each), padded by trunc plus one block -> (origin (3,) float64,
    dims (bx, by, bz))."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all()) or (hi < lo).any():
        raise ValueError('box_of: bad bounds %r, %r' % (lo, hi))
    pad = float(trunc) + 8.0 * float(voxel)
    origin = lo - pad
    dims = tuple(int(d) for d in np.maximum(np.ceil(((hi + pad) - origin) / (8.0 * float(voxel))), 1.0))
    return origin, dims


def depth_bounds(depths, cams16, pixel_centre=DEFAULT_PIXEL_CENTRE):
    """The bounds of the maps' own back-projected samples, on the host -> (lo, hi) float64 (3,), or (None, None) without a sample.
    depths (n,rows,cols), cams16 (n,16) as eval_depth.camera_rows gives them."""
    depths = np.asarray(depths, np.float32)
    lo, hi = None, None
    v, u = np.meshgrid(np.arange(depths.shape[1], dtype=np.float64), np.arange(depths.shape[2], dtype=np.float64), indexing='ij')
    for d, c in zip(depths, np.asarray(cams16, np.float64)):
        ok = np.isfinite(d) & (d > 0)
        if not ok.any():
            continue
        z = d[ok].astype(np.float64)
        cam = np.stack([(u[ok] + pixel_centre - c[14]) / c[12] * z, (v[ok] + pixel_centre - c[15]) / c[13] * z, z], axis=1) - c[9:12]
        world = cam @ c[:9].reshape(3, 3)                # R^T (c - t), per row
        world = world[np.isfinite(world).all(axis=1)]
        if len(world):
            lo = world.min(axis=0) if lo is None else np.minimum(lo, world.min(axis=0))
            hi = world.max(axis=0) if hi is None else np.maximum(hi, world.max(axis=0))
    return lo, hi


def mesh_maps(depths, cams16, images, lo, hi, voxel, trunc_voxels=DEFAULT_TRUNC_VOXELS, min_weight=DEFAULT_MIN_WEIGHT,
              max_blocks=DEFAULT_MAX_BLOCKS, pixel_centre=DEFAULT_PIXEL_CENTRE, carve_weight=None, weights=None):
    """depths (n,rows,cols) float32 and images (n,rows,cols,C>=3) float32 (b, g, r first) or None on the device, cams16 (n,16)
    float64 host rows (eval_depth.camera_rows), lo / hi the bounds of what is to be meshed -> (volume, (vertices, colors, faces)
    device tensors, {'integrate': s, 'extract': s}, each ended by a device synchronisation).  carve_weight: None, or the weight of
    a free vote (ops.tsdf_integrate's carve_weight); the volume then carries `free`.  weights: None, or (n,rows,cols) float32 on
    the depths' device, the weight of every pixel (ops.tsdf_integrate's weights); it is passed through."""
    import torch
    from .. import ops
    voxel, trunc_voxels, min_weight, max_blocks, pixel_centre = check_options(voxel, trunc_voxels, min_weight, max_blocks, pixel_centre)
    carve = {} if check_carve_weight(carve_weight) is None else {'carve_weight': check_carve_weight(carve_weight)}
    if weights is not None:
        carve['weights'] = weights
    trunc = trunc_voxels * voxel
    origin, dims = box_of(lo, hi, voxel, trunc)
    if dims[0] * dims[1] * dims[2] > ops.TSDF_MAX_DIRECTORY:
        raise ValueError('mesh voxel %r gives a box of %s blocks, more than 2^26: the scene spans %s' % (voxel, dims, (np.asarray(hi) - lo).tolist()))
    cams = torch.from_numpy(np.ascontiguousarray(cams16, np.float64)).to(depths.device)
    torch.cuda.synchronize(depths.device)
    t0 = time.time()
    volume = ops.tsdf_integrate(depths, cams, voxel, trunc, origin, dims, images=images, pixel_centre=pixel_centre, max_blocks=max_blocks,
                                **carve)
    torch.cuda.synchronize(depths.device)
    t1 = time.time()
    mesh = ops.tsdf_mesh(volume, min_weight)
    torch.cuda.synchronize(depths.device)
    return volume, mesh, {'integrate': t1 - t0, 'extract': time.time() - t1}


def support_of_maps(depths, cams, disp_threshold=0.01, num_consistent=2, consistent=True, weights=False):
    """The tool's consistency mask and agreement weights of written maps: depths (n,rows,cols) float32 on the device (probability
    filtered), cams (n,2,4,4) as eval_depth.load_maps gives them, packed with depth_fusion.projection_matrix / pack_cameras; the
    slab carries the fake normal, under which the normal test rejects nothing (depth_fusion.NORMAL_THRESHOLD).  One launch
    (ops.fusion_support) -> (the depths to integrate: masked when `consistent`, else as given; the weight plane or None; the
    report's `consistent` entry as a dict, {} without `consistent`)."""
    import torch
    from .. import ops
    from . import depth_fusion
    packed = torch.from_numpy(depth_fusion.pack_cameras([depth_fusion.projection_matrix(c) for c in np.asarray(cams, np.float64)])).to(depths.device)
    fake = torch.where(depths > 0, torch.full_like(depths, float(np.float32(1.0) / np.float32(1.732050808))), torch.zeros_like(depths))
    nd = torch.stack([fake, fake, fake, depths], dim=-1).contiguous()
    got = ops.fusion_support(packed, nd, float(disp_threshold), depth_fusion.NORMAL_THRESHOLD, int(num_consistent),
                             want=(('depth',) if consistent else ()) + (('weight',) if weights else ()))
    report = {}
    if consistent:
        report['consistent'] = {'disp_threshold': float(disp_threshold), 'num_consistent': int(num_consistent),
                                'samples': int((depths > 0).sum().item()), 'samples_kept': int((got['depth'] > 0).sum().item())}
    return (got['depth'] if consistent else depths), got.get('weight'), report


def host_boundary_edges(f, num_vertices):
    """The edges that lie in exactly one face, on the host: numpy.unique over all 3F sorted pairs.  f (F,3) int64."""
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, counts = np.unique(e[:, 0] * (int(num_vertices) + 1) + e[:, 1], return_counts=True)
    return int((counts == 1).sum())


def mesh_report(volume, mesh, min_weight, seconds=None, carve_weight=None):
    """-> a dict: the box, blocks, valid voxels, vertices, faces, zero-area faces, boundary edges (edges of one face), seconds.
    The boundary edges of a mesh on a GPU are counted there (ops.mesh_edge_census); host tensors are counted by numpy.unique.
    With carve_weight (the volume was integrated with it) also carve_weight, free_voxels (valid voxels with free > 0) and max_free."""
    vertices, _, faces = mesh
    v = vertices.cpu().numpy().astype(np.float64)
    f = faces.cpu().numpy().astype(np.int64)
    zero = boundary = 0
    if len(f):
        normal = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        zero = int((np.abs(normal).max(axis=1) == 0.0).sum())
        if faces.device.type == 'cuda':
            from .. import ops
            boundary = ops.mesh_edge_census(faces.contiguous(), len(v))['boundary']
        else:
            boundary = host_boundary_edges(f, len(v))
    report = {'origin': [float(o) for o in volume.origin], 'voxel': volume.voxel, 'trunc': volume.trunc, 'dims': list(volume.dims),
              'min_weight': float(min_weight), 'blocks': volume.num_blocks,
              'valid_voxels': int((volume.weight >= float(min_weight)).sum().item()) if volume.num_blocks else 0,
              'vertices': int(len(v)), 'faces': int(len(f)), 'zero_area_faces': zero, 'boundary_edges': boundary,
              'seconds': dict(seconds or {})}
    if carve_weight is not None:
        if volume.free is None:
            raise ValueError('mesh_report: carve_weight is given and the volume carries no free counts')
        some = volume.num_blocks > 0
        report.update(carve_weight=float(carve_weight),
                      free_voxels=int(((volume.weight >= float(min_weight)) & (volume.free > 0)).sum().item()) if some else 0,
                      max_free=float(volume.free.max().item()) if some else 0.0)
    return report


def render_views(vertices, faces, cams16, rows, cols, folder, indices, pixel_centre=DEFAULT_PIXEL_CENTRE):
    """The mesh (device tensors, as ops.tsdf_mesh returns them) rendered into the cameras cams16 (n,16) by ops.mesh_render and
    written as folder/%08d_mesh.pfm, one per index -> {'maps': n, 'covered_fraction': share of pixels that see the mesh,
    'seconds': render and download, ended by a device synchronisation}."""
    import torch
    from .preprocess import write_pfm
    torch.cuda.synchronize(vertices.device)
    t0 = time.time()
    depth, _ = eval_depth.render_mesh(vertices, faces, np.asarray(cams16, np.float64).reshape(-1, 16), rows, cols,
                                      pixel_centre=pixel_centre, device=vertices.device)
    depth = depth.cpu().numpy()
    seconds = time.time() - t0
    os.makedirs(folder, exist_ok=True)
    for i, d in zip(indices, depth):
        write_pfm(os.path.join(folder, '%08d_mesh.pfm' % int(i)), np.ascontiguousarray(d, np.float32))
    return {'maps': int(len(depth)), 'covered_fraction': float((depth > 0).mean()) if depth.size else 0.0, 'seconds': seconds}


class SceneMesh(object):
    """The mesh of a scene whose maps a depth_fusion.SceneFusion holds.

        mesh = SceneMesh(scene_fusion, cams, voxel)     # cams: {out_index: (2,4,4) camera}, or (n,2,4,4) in the order of add()
        mesh.write_ply(path)                            # = run() + tools/ply.write_mesh
        mesh.report()

    The box is the ops.cloud_bounds of the fused points of scene_fusion.run(), padded by trunc = trunc_voxels * voxel plus one
    block: the consistent points bound the volume, so a stray depth cannot inflate it.  The staged, probability-filtered depth
    planes (nd[..., 3]) and images (img) are integrated in scene_fusion.order().  run() -> (vertices (V,3) float32, colors (V,3)
    uint8 r, g, b, faces (F,3) int32) as numpy arrays.

    clean: None, or a dict of clean_mesh.clean's criteria (min_faces=, min_ratio=, keep_largest=).  With it run() also removes the
    mesh's small connected components on the device, before anything is downloaded (clean_mesh.clean_device); run()'s result and
    report() stay those of the whole mesh, and write_clean_ply(path), clean_result(), clean_report() and render(folder, clean=True)
    give the cleaned one.

    simplify: None, or dict(cell_voxels=R[, placement='quadric' | 'mean', rank_epsilon=1e-3]).  With it run() also simplifies the
    mesh -- the cleaned one when clean= is given -- on the device by vertex clustering (simplify_mesh.simplify_device) with cells of
    R voxels whose origin is the volume's, so they sit on the voxel lattice; run()'s result, report() and the cleaned mesh stay as
    they are, and simplify_result(), simplify_report() and write_simple_ply(path) give the simplified one (section 10.3d).

    smooth: None, or dict(iterations=N[, lam=0.5, mu=-0.53, pin_boundary=False, normals=False]).  With it run() also smooths the mesh
    -- the cleaned one when clean= is given -- on the device by Taubin's filter (smooth_mesh.smooth_device); colours and faces stay;
    with normals=True the smoothed mesh gets vertex normals whose area unit is voxel^2 (every face larger than a voxel's votes 1, the
    slivers of marching tetrahedra in proportion).  run()'s result, report() and the cleaned mesh stay as they are; smooth_result(),
    smooth_report() and write_smooth_ply(path) give the smoothed one (section 10.3g).  With simplify= also given, the simplification
    takes the smoothed mesh and its report's source is 'smooth'.

    carve_weight: None, or the weight of a free vote: the staged planes are integrated with free-space carving (section 10.3b) and
    report() gains carve_weight, free_voxels and max_free.

    consistent=True: scene_fusion.support()'s `depth` -- the staged depth where the fusion's num_consistent other views agree on it,
    0 elsewhere -- is integrated in place of the staged depth planes, so the mesh rests on the samples the cloud is made of;
    report() gains `consistent` (disp_threshold, num_consistent, samples, samples_kept).  weights='agree': support()'s `weight`,
    (1 + agreeing views) / (1 + num_consistent), is each pixel's view weight (ops.tsdf_integrate's weights); report() gains
    `weights`.  Both come from one launch; the thresholds are the scene_fusion's own (section 10.3c).

    score: None, or dict(spacing=S[, seed=K][, exact=True]).  run() does nothing with it; score(gt_points) samples the surface of the mesh, of the
    cleaned and of the simplified one where they exist, on the device at that spacing and scores each against the ground truth
    (section 10.3e)."""

    def __init__(self, scene_fusion, cams, voxel, trunc_voxels=DEFAULT_TRUNC_VOXELS, min_weight=DEFAULT_MIN_WEIGHT,
                 max_blocks=DEFAULT_MAX_BLOCKS, pixel_centre=DEFAULT_PIXEL_CENTRE, render=False, clean=None, carve_weight=None,
                 consistent=False, weights=None, simplify=None, score=None, smooth=None):
        self.options = check_options(voxel, trunc_voxels, min_weight, max_blocks, pixel_centre, clean=clean)
        self.simplify = check_simplify(simplify)
        self.smooth = check_smooth(smooth)
        self._device_smooth = self._smooth_result = self._smooth_report = None
        self.score_options = check_score(score)
        self.score_exact = check_score_exact(score)
        self._device_simple = self._simple_result = self._simple_report = None
        self.carve_weight = check_carve_weight(carve_weight)
        self.consistent, self.weights = check_support(consistent, weights)
        self.clean = None if clean is None else dict(clean)
        self._device_clean = self._clean_result = self._clean_report = None
        self.fusion = scene_fusion
        k = len(scene_fusion.index)
        if isinstance(cams, dict):
            missing = [i for i in scene_fusion.index if i not in cams]
            if missing:
                raise ValueError('SceneMesh: no camera for map %d' % missing[0])
            cams = [cams[i] for i in scene_fusion.index]
        self.cams16 = eval_depth.camera_rows(np.asarray(cams, np.float64))
        if len(self.cams16) != k:
            raise ValueError('SceneMesh: %d cameras for %d staged maps' % (len(self.cams16), k))
        self.volume = self.result = self._report = self._device_mesh = None

    def run(self):
        import torch
        from .. import ops
        if self.result is None:
            voxel, trunc_voxels, min_weight, max_blocks, pixel_centre = self.options
            fusion = self.fusion
            t0 = time.time()
            points, _ = fusion.run()                      # orders this stream after every staging
            dev = fusion.device
            lo, hi = ops.cloud_bounds(torch.from_numpy(np.ascontiguousarray(points, np.float32)).to(dev)) if len(points) else (None, None)
            seconds = {'bounds': time.time() - t0}
            if lo is None:
                raise RuntimeError('SceneMesh: the fusion has no finite point: there is nothing to bound the volume with')
            order = fusion.order()
            k = len(order)
            idx = torch.from_numpy(order).to(dev)
            depths = fusion.nd[:k, :, :, 3].index_select(0, idx).contiguous()
            images = fusion.img[:k] if np.array_equal(order, np.arange(k)) else fusion.img[:k].index_select(0, idx)
            weights, support = None, {}
            if self.consistent or self.weights is not None:
                t0 = time.time()
                got = fusion.support(want=(('depth',) if self.consistent else ()) + (('weight',) if self.weights is not None else ()))
                if self.consistent:
                    support['consistent'] = {'disp_threshold': fusion.disp_threshold, 'num_consistent': fusion.num_consistent,
                                             'samples': int((depths > 0).sum().item()), 'samples_kept': int((got['depth'] > 0).sum().item())}
                    depths = got['depth']
                if self.weights is not None:
                    support['weights'] = self.weights
                    weights = got['weight']
                torch.cuda.synchronize(dev)
                seconds['support'] = time.time() - t0
            self.volume, mesh, stage = mesh_maps(depths, self.cams16[order], images, lo, hi, voxel, trunc_voxels, min_weight, max_blocks,
                                                 pixel_centre, self.carve_weight, weights)
            seconds.update(stage)
            if self.clean is not None:
                vertices, colors, faces, self._clean_report = clean_mesh.clean_device(*mesh, **self.clean)
                self._device_clean = (vertices, colors, faces)
            source, source_name = (mesh, 'mesh') if self.clean is None else (self._device_clean, 'clean')
            if self.smooth is not None:
                vertices, colors, faces, normals, self._smooth_report = smooth_mesh.smooth_device(
                    *source, area_unit=voxel * voxel if self.smooth['normals'] else None, **self.smooth)
                self._smooth_report.update(source=source_name)
                self._device_smooth = (vertices, colors, faces, normals)
                source, source_name = (vertices, colors, faces), 'smooth'
            if self.simplify is not None:
                cell_voxels, placement, rank_epsilon = self.simplify
                vertices, colors, faces, self._simple_report = simplify_mesh.simplify_device(
                    *source, cell=cell_voxels * voxel, placement=placement, origin=self.volume.origin, rank_epsilon=rank_epsilon)
                self._simple_report.update(cell_voxels=cell_voxels, source=source_name)
                self._device_simple = (vertices, colors, faces)
            t0 = time.time()
            self.result = tuple(None if t is None else t.cpu().numpy() for t in mesh)
            self._device_mesh = mesh
            seconds['download'] = time.time() - t0
            t0 = time.time()
            self._report = dict(mesh_report(self.volume, mesh, min_weight, seconds, self.carve_weight), **support)
            seconds['report'] = self._report['seconds']['report'] = time.time() - t0          # zero-area faces on the host, the edge census on the device
        return self.result

    def report(self):
        self.run()
        return self._report

    def _cleaned(self):
        self.run()
        if self._device_clean is None:
            raise RuntimeError('SceneMesh: no clean= criteria were given: there is no cleaned mesh')
        return self._device_clean

    def clean_result(self):
        """run() -> the cleaned mesh (vertices, colors, faces) as numpy arrays."""
        device = self._cleaned()
        if self._clean_result is None:
            self._clean_result = tuple(None if t is None else t.cpu().numpy() for t in device)
        return self._clean_result

    def clean_report(self):
        """run() -> clean_mesh.clean_device's report: components, what was removed, the edge census before and after."""
        self._cleaned()
        return self._clean_report

    def write_clean_ply(self, path):
        """The cleaned mesh into a binary PLY at `path` -> the number of faces."""
        from ..tools import ply
        vertices, colors, faces = self.clean_result()
        ply.write_mesh(path, vertices, colors, faces)
        return len(faces)

    def _simplified(self):
        self.run()
        if self._device_simple is None:
            raise RuntimeError('SceneMesh: no simplify= was given: there is no simplified mesh')
        return self._device_simple

    def simplify_result(self):
        """run() -> the simplified mesh (vertices, colors, faces) as numpy arrays."""
        device = self._simplified()
        if self._simple_result is None:
            self._simple_result = tuple(None if t is None else t.cpu().numpy() for t in device)
        return self._simple_result

    def simplify_report(self):
        """run() -> simplify_mesh.simplify_device's report, with cell_voxels and the source ('mesh', 'clean' or 'smooth')."""
        self._simplified()
        return self._simple_report

    def write_simple_ply(self, path):
        """The simplified mesh into a binary PLY at `path` -> the number of faces."""
        from ..tools import ply
        vertices, colors, faces = self.simplify_result()
        ply.write_mesh(path, vertices, colors, faces)
        return len(faces)

    def _smoothed(self):
        self.run()
        if self._device_smooth is None:
            raise RuntimeError('SceneMesh: no smooth= was given: there is no smoothed mesh')
        return self._device_smooth

    def smooth_result(self):
        """run() -> the smoothed mesh (vertices, colors, faces, normals or None) as numpy arrays."""
        device = self._smoothed()
        if self._smooth_result is None:
            self._smooth_result = tuple(None if t is None else t.cpu().numpy() for t in device)
        return self._smooth_result

    def smooth_report(self):
        """run() -> smooth_mesh.smooth_device's report, with the source ('mesh' or 'clean')."""
        self._smoothed()
        return self._smooth_report

    def write_smooth_ply(self, path):
        """The smoothed mesh into a binary PLY at `path`, with its normals where smooth= asked for them -> the number of faces."""
        from ..tools import ply
        vertices, colors, faces, normals = self.smooth_result()
        ply.write_mesh(path, vertices, colors, faces, normals)
        return len(faces)

    def score(self, gt_points, transform=None):
        """run() -> {'mesh': result[, 'clean': result][, 'smooth': result][, 'simple': result]}: each mesh this object holds on the device sampled at
        score=dict(spacing=, seed=) (sample_mesh.sample_device: the tensors stay where they are) and the samples scored against
        gt_points by eval_cloud.evaluate at its default tolerances; transform: a 4x4 matrix applied to the samples first (the matrix
        a registration found for the scene's cloud: the meshes are not registered again).  A result carries `recon_mesh`, the
        sampling's report without `seconds`.  With score=dict(..., exact=True) completeness comes from the exact distance of every
        ground-truth point to the mesh on the device (evaluate's recon_surface, moved by the same matrix), accuracy from the samples
        as before, and a result carries `exact`."""
        from . import eval_cloud
        self.run()
        if self.score_options is None:
            raise RuntimeError('SceneMesh: no score= was given: there is no spacing to sample the meshes at')
        spacing, seed = self.score_options
        moved = {} if transform is None else {'init_transform': transform}
        out = {}
        for key, mesh in (('mesh', self._device_mesh), ('clean', self._device_clean), ('smooth', self._device_smooth),
                          ('simple', self._device_simple)):
            if mesh is None:
                continue
            vertices, _, faces = mesh[:3]
            samples, report = sample_mesh.sample_device(vertices.contiguous(), None, faces.contiguous(), spacing=spacing, seed=seed)
            surface = {'recon_surface': (vertices.contiguous(), faces.contiguous())} if self.score_exact else {}
            out[key] = eval_cloud.evaluate(samples.points, gt_points, device=vertices.device, **dict(moved, **surface))
            out[key]['recon_mesh'] = {k: report[k] for k in sample_mesh.REPORT_KEYS if k != 'seconds'}
        return out

    def render(self, folder, clean=False):
        """run(), then the mesh -- still on the device -- rendered into the scene's map cameras as folder/%08d_mesh.pfm
        (render_views); report() gains `render`.  clean=True: the cleaned mesh, and clean_report() gains `render`."""
        self.run()
        fusion = self.fusion
        order = fusion.order()
        vertices, _, faces = self._cleaned() if clean else self._device_mesh
        report = self._clean_report if clean else self._report
        report['render'] = render_views(vertices.contiguous(), faces.contiguous(), self.cams16[order], fusion.rows, fusion.cols,
                                        folder, [fusion.index[k] for k in order], self.options[4])
        return report['render']

    def write_ply(self, path):
        """run() into a binary PLY at `path` (tools/ply.write_mesh) -> the number of faces."""
        from ..tools import ply
        vertices, colors, faces = self.run()
        ply.write_mesh(path, vertices, colors, faces)
        return len(faces)


def add_options(parser, prefix='', tool=True):
    """The meshing options --<prefix>voxel, trunc_voxels, min_weight, max_blocks, carve and clean_mesh's criteria as --<prefix>clean_*.
    tool: this command line's form, where --voxel is required and trunc_voxels, min_weight, max_blocks default to DEFAULT_*; False:
    the ETH3D driver's (prefix 'mesh_'), where each defaults to None -- only what is given is passed on -- and shows a metavar.
    --render is not here: it is a directory in the tool and a flag in the driver."""
    def add(name, type, default, metavar, help):
        parser.add_argument('--%s%s' % (prefix, name), type=type, required=tool and default is None, default=default if tool else None,
                            metavar=None if tool else metavar, help=help)

    add('voxel', float, None, 'V', 'the voxel\'s edge in the scene\'s unit (the ETH3D driver, with --fuse: also mesh each scene -- TSDF '
                                   'fusion of the staged maps, marching tetrahedra -- into <savepath>/<scene>/final3d_mesh.ply and mesh.json)')
    add('trunc_voxels', float, DEFAULT_TRUNC_VOXELS, 'T', 'the band either side of a depth, in voxels (default %g: a default, not a '
                                                          'measurement)' % DEFAULT_TRUNC_VOXELS)
    add('min_weight', float, DEFAULT_MIN_WEIGHT, 'W', 'views a voxel needs to be meshed (default %g, the fusion\'s num_consistent)'
                                                      % DEFAULT_MIN_WEIGHT)
    add('max_blocks', int, DEFAULT_MAX_BLOCKS, 'N', 'blocks of 8^3 voxels the maps may mark (default %d)' % DEFAULT_MAX_BLOCKS)
    parser.add_argument('--%scarve' % prefix, type=float, nargs='?', default=None, const=DEFAULT_CARVE_WEIGHT, metavar='CW',
                        help='free-space carving: a view that sees past a voxel votes it outside with this weight (given bare: %g, a '
                             'default, not a measurement); the report gains carve_weight, free_voxels, max_free' % DEFAULT_CARVE_WEIGHT)
    clean_mesh.add_options(parser, prefix + 'clean_')


def add_support_options(parser):
    """The options of the consistency mask and the view weights (section 10.3c): --consistent, --disp_threshold, --num_consistent,
    --weights.  They are not among add_options': this tool's and the ETH3D driver's command lines keep the options they had, and
    atvsnet/mesh_consistent.py is the command that adds these to this tool's (cli reads them where the parser has them)."""
    parser.add_argument('--consistent', action='store_true',
                        help='integrate only the depths that --num_consistent other views agree on (the fusion\'s geometric test per '
                             'pixel, ops.fusion_support): the samples the point cloud is made of; the report gains `consistent`')
    parser.add_argument('--disp_threshold', type=float, default=None, help='--consistent / --weights agree: depth_fusion --disp_threshold (default 0.01)')
    parser.add_argument('--num_consistent', type=int, default=None, help='--consistent / --weights agree: depth_fusion --num_consistent (default 2)')
    parser.add_argument('--weights', choices=TOOL_WEIGHT_MODES, default=None,
                        help='per-pixel view weights: agree = (1 + agreeing views) / (1 + num_consistent), a default, not a measurement; '
                             'prob = the probability map\'s value; the report gains `weights`')


def options(parser, args, prefix=''):
    """The options of add_options that were given, as SceneMesh's keyword arguments voxel=, trunc_voxels=, min_weight=, max_blocks=,
    carve_weight= and clean= (clean_mesh's criteria; a bad one is an argument error) -- {} when none was.  parser None: nothing is
    checked, and an option `args` lacks is not given.  This is the ETH3D driver's mesh (with fuse only; it adds render=True for its
    --mesh_render): after the scene's fusion the staged depth planes and images are integrated into a TSDF volume bounded by the
    fused cloud and meshed by marching tetrahedra into <savepath>/<scene>/final3d_mesh.ply, with the report in mesh.json; clean=
    also writes final3d_mesh_clean.ply and mesh_clean.json, the mesh without the connected components that miss a criterion;
    render=True also renders the mesh into the scene's map cameras as <savepath>/<scene>/depths_mesh/%08d_mesh.pfm."""
    names = dict(voxel='voxel', trunc_voxels='trunc_voxels', min_weight='min_weight', max_blocks='max_blocks', carve='carve_weight')
    out = {key: getattr(args, prefix + name) for name, key in names.items() if getattr(args, prefix + name, None) is not None}
    clean = clean_mesh.options(parser, args, prefix + 'clean_')
    return dict(out, clean=clean) if clean else out


def rules(mesh, fuse, gt_ply=None):
    """The ETH3D driver's rules for its mesh, as (broken, message) rows: none without mesh; the rows of carve_weight, consistent,
    weights, clean, simplify, smooth and score only when they are given (consistent, weights, simplify, smooth and score reach the
    driver through run_eval_pc's mesh dict alone: its command line has no option for them).  score's rows stand behind the others."""
    if mesh is None:
        return []
    rows = [(fuse is None, '--mesh_voxel, --mesh_trunc_voxels, --mesh_min_weight and --mesh_max_blocks need --fuse (mesh needs fuse): the '
                           'mesh is integrated from the maps the fusion stages and bounded by its cloud'),
            (mesh.get('voxel') is None, '--mesh_trunc_voxels, --mesh_min_weight and --mesh_max_blocks need --mesh_voxel (mesh needs voxel=)')]
    if mesh.get('carve_weight') is not None:
        rows.insert(1, (mesh.get('voxel') is None, '--mesh_carve needs --mesh_voxel (mesh carve_weight= needs voxel=): there is no '
                                                   'volume to carve'))
    if mesh.get('weights') is not None:
        rows.insert(1, (mesh.get('voxel') is None, 'mesh weights= needs voxel=: there is no volume whose views could be weighted'))
    if mesh.get('consistent'):
        rows.insert(1, (mesh.get('voxel') is None, 'mesh consistent= needs voxel=: there is no volume to integrate the consistent '
                                                   'depths into'))
    if mesh.get('clean') is not None:                 # in front of the row above: its message names what was given
        rows.insert(1, (mesh.get('voxel') is None, '--mesh_clean_min_faces, --mesh_clean_min_ratio and --mesh_clean_keep_largest need '
                                                   '--mesh_voxel (mesh clean= needs voxel=): there is no mesh to clean'))
    if mesh.get('simplify') is not None:
        rows.insert(1, (mesh.get('voxel') is None, 'mesh simplify= needs voxel=: there is no mesh to simplify, and its cells are '
                                                   'counted in voxels'))
    if mesh.get('smooth') is not None:
        rows.insert(1, (mesh.get('voxel') is None, 'mesh smooth= needs voxel=: there is no mesh to smooth, and its normals\' area unit '
                                                   'is a voxel\'s'))
    if mesh.get('score') is not None:
        rows += [(mesh.get('voxel') is None, 'mesh score= needs voxel=: there is no mesh to score'),
                 (not gt_ply, 'mesh score= needs gt_ply: there is no ground truth to score the mesh\'s samples against')]
    return rows


def make_parser():
    parser = argparse.ArgumentParser(description='mesh the written depth maps of a scene: TSDF fusion and marching tetrahedra on the GPU '
                                                 '(free-space carving with --carve; simplification is atvsnet/simplify_mesh.py; no hole filling)')
    parser.add_argument('--scene', default=None, help='<data_root>/eth3d/<scene>: its pair.txt names the maps (default: every map under --maps)')
    parser.add_argument('--maps', required=True, help='<savepath>/<scene> of eval_pointcloud: depths_atvsnet/%%08d.pfm, _prob.pfm, .jpg, .txt')
    add_options(parser)
    parser.add_argument('--prob_threshold', type=float, default=0.8, help='a depth whose probability is below this is no sample (depth_fusion --prob_threshold)')
    parser.add_argument('--pixel_centre', type=float, default=DEFAULT_PIXEL_CENTRE, help='image coordinate of the centre of pixel (0,0): 0 (the fusion\'s) or 0.5')
    parser.add_argument('--bounds', default=None, metavar='PLY', help='bound the volume by this cloud (the scene\'s final3d_model.ply) instead of '
                                                                      'by the maps\' own back-projected depths')
    parser.add_argument('--report', default=None, metavar='FILE', help='write the report as JSON here')
    parser.add_argument('--render', default=None, metavar='DIR', help='render the mesh into the maps\' cameras (ops.mesh_render) as '
                                                                      'DIR/%%08d_mesh.pfm; the report gains `render`')
    parser.add_argument('--out', required=True, help='the mesh, a binary PLY')
    parser.add_argument('--clean_out', default=None, metavar='PLY', help='with a --clean_ criterion: the mesh without the connected '
                                                                         'components that miss it (clean_mesh); the report gains `clean`')
    parser.add_argument('--gpu_id', type=int, default=0)
    return parser


def _load_side_maps(maps_folder, indices, shape):
    """The probability maps and images that stand beside the depth maps: (prob (n,rows,cols) or None, bgr (n,rows,cols,3) or None)."""
    from .preprocess import load_pfm
    folder = os.path.join(maps_folder, 'depths_atvsnet')
    if not os.path.isdir(folder):
        folder = maps_folder
    probs, images = [], []
    for i in indices:
        stem = os.path.join(folder, '%08d' % i)
        if probs is not None and os.path.exists(stem + '_prob.pfm'):
            with open(stem + '_prob.pfm', 'rb') as f:
                probs.append(np.asarray(load_pfm(f), np.float32))
        else:
            probs = None
        if images is not None and os.path.exists(stem + '.jpg'):
            from PIL import Image
            images.append(np.asarray(Image.open(stem + '.jpg').convert('RGB'))[:, :, ::-1].astype(np.float32))
            if images[-1].shape[:2] != shape:
                images = None
        else:
            images = None
    return (None if probs is None else np.stack(probs)), (None if images is None else np.stack(images))


def cli(argv=None, parser=None):
    """parser: None (make_parser()), or a parser that also has add_support_options' options (atvsnet/mesh_consistent.py); without
    them the mask and the weights are off."""
    parser = make_parser() if parser is None else parser
    args = parser.parse_args(argv)
    for name, off in (('consistent', False), ('weights', None), ('disp_threshold', None), ('num_consistent', None)):
        if not hasattr(args, name):
            setattr(args, name, off)
    try:
        check_options(args.voxel, args.trunc_voxels, args.min_weight, args.max_blocks, args.pixel_centre, carve_weight=args.carve)
        check_support(args.consistent, args.weights, TOOL_WEIGHT_MODES)
    except ValueError as e:
        parser.error(str(e))
    agree = args.consistent or args.weights == 'agree'
    if not agree and (args.disp_threshold is not None or args.num_consistent is not None):
        parser.error('--disp_threshold and --num_consistent need --consistent or --weights agree')
    args.disp_threshold = 0.01 if args.disp_threshold is None else args.disp_threshold
    args.num_consistent = 2 if args.num_consistent is None else args.num_consistent
    if not (args.disp_threshold > 0.0 and np.isfinite(args.disp_threshold)) or args.num_consistent < 0:
        parser.error('--disp_threshold must be positive and finite, --num_consistent >= 0')
    if not os.path.isdir(args.maps):
        parser.error('--maps %s: no such folder' % args.maps)
    if args.scene is not None and not os.path.isfile(os.path.join(args.scene, 'pair.txt')):
        parser.error('--scene %s: no pair.txt' % args.scene)
    if args.bounds is not None and not os.path.isfile(args.bounds):
        parser.error('--bounds %s: no such file' % args.bounds)
    criteria = clean_mesh.options(parser, args, 'clean_')
    if bool(criteria) != (args.clean_out is not None):
        parser.error('--clean_out needs one of --clean_min_faces, --clean_min_ratio, --clean_keep_largest, and they need --clean_out')
    from ..tools import ply
    indices, depths, cams = eval_depth.load_maps(args.maps, eval_depth.scene_indices(args.scene) if args.scene is not None else None)
    probs, images = _load_side_maps(args.maps, indices, depths.shape[1:])
    if args.weights == 'prob' and probs is None:
        parser.error('--weights prob needs the probability maps (%%08d_prob.pfm) beside the depth maps under %s' % args.maps)
    depths = depths.copy()
    if probs is not None:
        depths[probs < args.prob_threshold] = 0          # depth_fusion.probability_filter
    cams16 = eval_depth.camera_rows(cams)
    if args.bounds is not None:
        points = ply.read_ply_points(args.bounds)
        points = points[np.isfinite(points).all(axis=1)]
        lo, hi = (points.min(axis=0), points.max(axis=0)) if len(points) else (None, None)
    else:
        lo, hi = depth_bounds(depths, cams16, args.pixel_centre)
    if lo is None:
        parser.error('there is no depth sample (or no point in --bounds) to bound the volume with')
    import torch
    torch.cuda.set_device(args.gpu_id)
    dev = torch.device('cuda', args.gpu_id)
    depths_d, weights_d, support = torch.from_numpy(depths).to(dev), None, {}
    if agree:
        depths_d, weights_d, support = support_of_maps(depths_d, cams, args.disp_threshold, args.num_consistent, args.consistent,
                                                       args.weights == 'agree')
    if args.weights == 'prob':
        weights_d = torch.from_numpy(np.ascontiguousarray(probs, np.float32)).to(dev)
    if args.weights is not None:
        support['weights'] = args.weights
    volume, mesh, seconds = mesh_maps(depths_d, cams16, None if images is None else torch.from_numpy(images).to(dev),
                                      lo, hi, args.voxel, args.trunc_voxels, args.min_weight, args.max_blocks, args.pixel_centre, args.carve,
                                      weights_d)
    vertices, colors, faces = (None if t is None else t.cpu().numpy() for t in mesh)
    ply.write_mesh(args.out, vertices, colors, faces)
    result = dict(mesh_report(volume, mesh, args.min_weight, seconds, args.carve), maps=[int(i) for i in indices], colored=images is not None,
                  probability_filtered=probs is not None, **support)
    if args.render:
        result['render'] = render_views(mesh[0], mesh[2], cams16, depths.shape[1], depths.shape[2], args.render, indices, args.pixel_centre)
    if criteria:
        clean_v, clean_c, clean_f, result['clean'] = clean_mesh.clean_device(*mesh, **criteria)
        ply.write_mesh(args.clean_out, clean_v.cpu().numpy(), None if clean_c is None else clean_c.cpu().numpy(), clean_f.cpu().numpy())
    if args.report:
        write_json(args.report, result)
    print(json.dumps({k: result[k] for k in ('blocks', 'valid_voxels', 'vertices', 'faces', 'zero_area_faces', 'boundary_edges')}))
    return result


if __name__ == '__main__':
    cli()
