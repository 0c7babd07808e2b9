"""ETH3D batch driver: depth + probability maps for every reference image of a set of scenes.

Mirror of /root/reference/atvsnet/eval_pointcloud.py (gen_data_list :60-94, load_data :97-203, run_eval_pc
:206-397, main :400-424): the same on-disk inputs (<scene>/pair.txt, images/%08d.jpg, cams/%08d_cam.txt) and
outputs (<savepath>/<scene>/depths_atvsnet/%08d.pfm, %08d_prob.pfm, %08d.jpg, %08d.txt, %08d.png,
zz_runtime.txt).  The session.run sequence of the reference (base per source, AAM1, refinement per source,
AAM2 with probability maps) is pipeline.infer_multiview(out_prob_map=True), replayed from one HIP graph per
input shape.  Not available here and therefore not done: the optional ground-truth depth range from
depths/*.exr (:170-192, needs an EXR reader).

One owner per job: eth3d_inputs reads a pair.txt entry, eth3d_maps runs the map loop, this module keeps what follows a scene's last
map, the option rules and the command line.  Each optional group -- fuse_normals, register, score_maps, clean, mesh -- is declared,
collected and ruled by the module that owns the feature (its add_options / options pair and its rules); they are only joined here.
"""
from __future__ import print_function

import argparse
import collections
import os
import time

import numpy as np
import torch

from ..flags import FLAGS
from ..tools.common import Notify
from . import clean_cloud, depth_fusion, eval_cloud, eval_depth, example, mesh_fusion
from .eth3d_inputs import (_ground_truth_depth_range, _inverse_depth_range, _sweep_cams, _view_cams, _view_paths,  # noqa: F401
                           gen_data_list, load_cams, load_data)
from .eth3d_maps import TIMES, _Decoder, _PipelineSource, _Pipelines, _run_scene, _SceneSource, _write_map, _Writer  # noqa: F401

ETH3D_LOW_RES_TEST = ['lakeside', 'sand_box', 'storage_room', 'storage_room_2', 'tunnel']

# what _end_scene's steps read: run_eval_pc's options, checked and loaded once
_SceneOptions = collections.namedtuple('_SceneOptions', 'device gt_points register_args init_cameras score_maps clean clean_keep_normals mesh')


def _write_cloud(scene_fusion, folder):
    """final3d_model.ply -> its point count.  After every map's result: the slots are idle; the fusion runs on this thread's
    (ordinary) stream."""
    t0 = time.time()
    n_points = scene_fusion.write_ply(os.path.join(folder, 'final3d_model.ply'))
    TIMES['fuse'] = time.time() - t0
    return n_points


def _source_planes(register_args):
    """Whether the registration runs over the fused cloud's own normals (point-to-plane, not over the ground truth's)."""
    return register_args.get('register_icp') == 'plane' and register_args.get('register_normals') != 'target'


def _score_cloud(points, folder, opts, normals=None):
    """cloud_eval.json -> the score.  normals: the fused points' own, for a point-to-plane registration."""
    t0 = time.time()
    plane = {'recon_normals': normals} if _source_planes(opts.register_args) else {}
    score = eval_cloud.evaluate(points, opts.gt_points, device=opts.device, **dict(opts.register_args, **plane))
    if opts.init_cameras is not None:
        score['init_cameras'] = opts.init_cameras
    eval_cloud.write_json(os.path.join(folder, 'cloud_eval.json'), score)
    TIMES['cloud_eval'] = time.time() - t0
    return score


def _score_maps(scene_fusion, map_cams, score, folder, opts):
    """depth_eval.json.  run() has ordered this stream after every staging; nd[..., 3] is the depth plane the fusion read."""
    t0 = time.time()
    device = opts.device
    order = scene_fusion.order()
    indices = [scene_fusion.index[k] for k in order]
    moved = score['registration']['matrix'] if 'registration' in score else None
    score_maps = dict(opts.score_maps)
    files, tol = score_maps.pop('occlusion_mesh', None), score_maps.pop('occlusion_mesh_tol', None)
    occlude, extra = {}, {}
    if files:                                                            # the occluded maps, and what occluded them in the report
        occluder = eval_depth.load_meshes(files)
        tol = eval_depth.DEFAULT_OCCLUDER_TOL if tol is None else tol
        occlude = dict(occluders=[occluder], occluder_tol=tol)
        extra = dict(occlusion_mesh_tol=tol, occlusion_faces=len(occluder[1]))
    gt_maps = eval_depth.render_scan(opts.gt_points, np.stack([map_cams[i] for i in indices]), scene_fusion.rows, scene_fusion.cols,
                                     transform=moved, device=device, **dict(score_maps, **occlude))
    pred = scene_fusion.nd[:len(indices), :, :, 3][torch.from_numpy(order).to(device)]
    eval_depth.write_json(os.path.join(folder, 'depth_eval.json'),
                          eval_depth.report(pred.cpu().numpy(), gt_maps.cpu().numpy(), indices=indices, transform=moved,
                                            **dict(score_maps, **extra)))
    TIMES['depth_eval'] = time.time() - t0


def _clean_cloud(points, colors, score, folder, opts, normals=None):
    """final3d_model_clean.ply and cloud_clean.json, with a score cloud_eval_clean.json -> the cleaned point count.  normals: the
    fused points' own; those of the rows that stay are written into the cleaned PLY."""
    from ..tools.ply import write_ply
    t0 = time.time()
    clean_normals = None
    if normals is None:
        clean_points, clean_colors, clean_report = clean_cloud.clean(points, colors, device=opts.device, **opts.clean)
    else:
        clean_points, clean_colors, clean_normals, clean_report = clean_cloud.clean(points, colors, device=opts.device, normals=normals, **opts.clean)
    write_ply(os.path.join(folder, 'final3d_model_clean.ply'), clean_points, clean_colors, clean_normals)
    clean_cloud.write_json(os.path.join(folder, 'cloud_clean.json'), clean_report)
    TIMES['cloud_clean'] = time.time() - t0
    if score is not None:
        # the same transform: the matrix found for the whole cloud (it includes the initial one), not a second fit
        moved = {}
        if 'registration' in score:
            moved['init_transform'] = score['registration']['matrix']
        elif 'init_transform' in score:
            moved['init_transform'] = score['init_transform']
        clean_score = eval_cloud.evaluate(clean_points, opts.gt_points, device=opts.device, **moved)
        eval_cloud.write_json(os.path.join(folder, 'cloud_eval_clean.json'), clean_score)
    return len(clean_points)


def _write_mesh(scene_fusion, map_cams, folder, mesh):
    """final3d_mesh.ply and mesh.json -> (the face count, the SceneMesh).  After the cloud: the fusion's result bounds the volume.
    With clean= in `mesh` also final3d_mesh_clean.ply and mesh_clean.json, the mesh without its small components (SceneMesh's
    clean=); with simplify= also final3d_mesh_simple.ply and mesh_simple.json, the mesh (the cleaned one with clean=) after vertex
    clustering; with smooth= also final3d_mesh_smooth.ply (with normals when smooth= asks for them) and mesh_smooth.json, the mesh
    (the cleaned one with clean=) after Taubin's filter, which simplify= then takes.  score= writes nothing here: _score_mesh does,
    once the cloud's score is known."""
    t0 = time.time()
    scene_mesh = mesh_fusion.SceneMesh(scene_fusion, map_cams, **mesh)
    n_faces = scene_mesh.write_ply(os.path.join(folder, 'final3d_mesh.ply'))
    if mesh.get('render'):
        scene_mesh.render(os.path.join(folder, 'depths_mesh'))
    mesh_fusion.write_json(os.path.join(folder, 'mesh.json'), scene_mesh.report())
    if mesh.get('clean'):
        scene_mesh.write_clean_ply(os.path.join(folder, 'final3d_mesh_clean.ply'))
        mesh_fusion.write_json(os.path.join(folder, 'mesh_clean.json'), scene_mesh.clean_report())
    if mesh.get('smooth'):
        scene_mesh.write_smooth_ply(os.path.join(folder, 'final3d_mesh_smooth.ply'))
        mesh_fusion.write_json(os.path.join(folder, 'mesh_smooth.json'), scene_mesh.smooth_report())
    if mesh.get('simplify'):
        scene_mesh.write_simple_ply(os.path.join(folder, 'final3d_mesh_simple.ply'))
        mesh_fusion.write_json(os.path.join(folder, 'mesh_simple.json'), scene_mesh.simplify_report())
    TIMES['mesh'] = time.time() - t0
    return n_faces, scene_mesh


def _score_mesh(scene_mesh, score, folder, opts):
    """mesh_eval.json, with clean= also mesh_eval_clean.json, with smooth= also mesh_eval_smooth.json, with simplify= also
    mesh_eval_simple.json: each mesh's surface sampled
    on the device (mesh score=dict(spacing=, seed=)) and scored against the ground truth, moved by the matrix found for the cloud
    (as _clean_cloud moves the cleaned cloud), not registered again."""
    t0 = time.time()
    moved = None
    if score is not None and 'registration' in score:
        moved = score['registration']['matrix']
    elif score is not None and 'init_transform' in score:
        moved = score['init_transform']
    names = {'mesh': 'mesh_eval.json', 'clean': 'mesh_eval_clean.json', 'smooth': 'mesh_eval_smooth.json', 'simple': 'mesh_eval_simple.json'}
    for key, result in scene_mesh.score(opts.gt_points, moved).items():
        eval_cloud.write_json(os.path.join(folder, names[key]), result)
    TIMES['mesh_eval'] = time.time() - t0


def _end_scene(name, scene_fusion, map_cams, folder, opts):
    """A fused scene's files, each group by its own step: the PLY, the mesh, the cloud's score, the maps' score, the cleaned cloud,
    the meshes' scores.
    opts: the _SceneOptions of the run."""
    n_points = _write_cloud(scene_fusion, folder)
    scene_mesh = None
    if opts.mesh is not None:
        n_faces, scene_mesh = _write_mesh(scene_fusion, map_cams, folder, opts.mesh)
        print(Notify.INFO, '%s: %d mesh faces' % (name, n_faces), Notify.ENDC)
    points, colors, score, normals = None, None, None, None
    if opts.gt_points is not None or opts.clean:
        points, colors = scene_fusion.run()
        points = points.copy()
        points[~np.isfinite(points).all(axis=1)] = 0.0          # as tools/ply.write_ply stores them
        if _source_planes(opts.register_args) or opts.clean_keep_normals:
            normals = scene_fusion.normals().copy()
            normals[~np.isfinite(normals).all(axis=1)] = 0.0     # likewise
    if opts.gt_points is not None:
        score = _score_cloud(points, folder, opts, normals)
    if opts.score_maps is not None:
        _score_maps(scene_fusion, map_cams, score, folder, opts)
    if opts.clean:
        n_clean = _clean_cloud(points, colors, score, folder, opts, normals if opts.clean_keep_normals else None)
        print(Notify.INFO, '%s: %d points after cleaning' % (name, n_clean), Notify.ENDC)
    if scene_mesh is not None and opts.mesh.get('score') is not None:
        _score_mesh(scene_mesh, score, folder, opts)
    print(Notify.INFO, '%s: %d fused points' % (name, n_points), Notify.ENDC)


def _option_rules(use_graph=True, scene_cache=False, write_thread=True, fuse=None, map_files=True, gt_ply=None, register=None,
                  clean=None, score_maps=None, fuse_normals=None, clean_keep_normals=False, mesh=None):
    """What each of run_eval_pc's options needs -> every rule as (broken by these values, message): the six rows of the options
    this module owns, with each group's own rows around them in a fixed order -- fuse_normals' in front; register's (target
    normals, point-to-plane, global), clean_keep_normals' and mesh's at the end.  A group's rows are listed only for a caller that
    gives the group: without it there is nothing they could refuse."""
    fused_normals = (fuse_normals or {}).get('normals') == 'depth'
    return depth_fusion.normal_rules(fuse_normals, fuse) + [
        (scene_cache and not use_graph, '--scene_cache replays captured graphs: it cannot be combined with --eager (use_graph=False)'),
        (not map_files and fuse is None, '--no_map_files needs --fuse (map_files=False needs fuse): the run would write nothing'),
        (bool(gt_ply) and fuse is None, '--gt_ply needs --fuse (gt_ply needs fuse): there is no point cloud to score'),
        (register is not None and not gt_ply, '--register needs --gt_ply (register needs gt_ply): there is nothing to align to'),
        (bool(clean) and fuse is None, '--clean_voxel, --clean_sor and --clean_radius_filter need --fuse (clean needs fuse): there is no '
                                       'point cloud to clean'),
        (score_maps is not None and not gt_ply, '--score_maps needs --gt_ply (score_maps needs gt_ply): there is no scan to render')
    ] + (eval_cloud.register_rules(register, fused_normals) + clean_cloud.keep_normals_rules(clean, clean_keep_normals, fused_normals)
         + mesh_fusion.rules(mesh, fuse, gt_ply))


def _check_options(**options):
    """Raises ValueError with the message of the first of _option_rules that `options` break, else with the first bad value of
    mesh or fuse_normals (their owners' checks)."""
    for broken, message in _option_rules(**options):
        if broken:
            raise ValueError(message)
    if options.get('mesh') is not None:
        mesh_fusion.check_options(**options['mesh'])
    if options.get('fuse_normals') is not None:
        depth_fusion.check_normal_options(**options['fuse_normals'])


def run_eval_pc(savepath, image_infos, use_graph=True, scene_cache=False, write_thread=True, fuse=None, map_files=True,
                gt_ply=None, register=None, clean=None, score_maps=None, fuse_normals=None, clean_keep_normals=False, mesh=None):
    """(reference :206-397) image_infos: [[[dense_path, image_folder, scene_name], format], ...]
    scene_cache: every image prepared and run through the towers once per scene (atvsnet/scene.py), the files written by one
    background thread (write_thread=False: in this thread, same bytes).
    fuse: None, or dict(prob_threshold=, disp_threshold=, num_consistent=): every map is also staged on the device as it is
    finished (depth_fusion.SceneFusion) and each scene ends with <savepath>/<scene>/final3d_model.ply, the point cloud
    depth_fusion.main makes from the written files.  map_files=False (with fuse only): no per-map files.
    gt_ply (with fuse only): ground-truth PLY paths; each scene's fused points, as the PLY stores them, are scored against them
    (eval_cloud.evaluate, default tolerances) into <savepath>/<scene>/cloud_eval.json -- what eval_cloud's CLI gives on that PLY.
    The optional groups, each None or a dict its owner describes; every other output is what it is without the group:
    fuse_normals (with fuse only): SceneFusion's normal options -- depth_fusion.options.
    register (with gt_ply only): the cloud is aligned to the ground truth before it is scored -- eval_cloud.register_arguments.
    score_maps (with gt_ply only): the depth maps that entered the cloud against the rendered scan -- eval_depth.options.
    clean (with fuse only): clean_cloud.clean's steps dict(voxel=, sor=(k, ratio, radius), radius_filter=(radius, min_neighbours)) into
    final3d_model_clean.ply and cloud_clean.json; with gt_ply the cleaned cloud is scored too, into cloud_eval_clean.json (moved by the
    matrix found for the uncleaned cloud, not registered again); clean_keep_normals (with clean and fuse_normals normals='depth'
    only): the cleaned PLY carries the normals of the rows that stay -- clean_cloud.options.
    mesh (with fuse only): mesh_fusion.SceneMesh's arguments, with render=True also depths_mesh/ -- mesh_fusion.options; its
    simplify=dict(cell_voxels=R) (no command-line option) also writes final3d_mesh_simple.ply and mesh_simple.json; its
    smooth=dict(iterations=N[, lam=, mu=, pin_boundary=, normals=]) (no command-line option) also writes final3d_mesh_smooth.ply and
    mesh_smooth.json, and the simplification then takes the smoothed mesh; its
    score=dict(spacing=S[, seed=K][, exact=True]) (with gt_ply only, no command-line option) samples each written mesh's surface on
    the device and scores it into mesh_eval.json, mesh_eval_clean.json, mesh_eval_smooth.json and mesh_eval_simple.json (moved by the cloud's matrix with
    register); with exact=True completeness comes from the exact distance of every ground-truth point to the mesh itself
    (ops.mesh_nearest) and the files carry `exact`."""
    assert FLAGS.view_num > 2, 'the ETH3D driver runs the multi-view (AANet) pipeline'
    _check_options(use_graph=use_graph, scene_cache=scene_cache, fuse=fuse, map_files=map_files, gt_ply=gt_ply, register=register,
                   clean=clean, score_maps=score_maps, fuse_normals=fuse_normals, clean_keep_normals=clean_keep_normals, mesh=mesh)
    if fuse_normals is not None:
        fuse = dict(fuse, **fuse_normals)
    gt_points, register_args, init_cameras = None, {}, None
    if gt_ply:
        from ..tools.ply import read_ply_points
        gt_points = np.concatenate([read_ply_points(p) for p in gt_ply], 0)
    if register is not None:
        register_args = eval_cloud.register_arguments(global_=register.get('global'), **register)
        if register.get('init_cameras'):
            from . import register_cloud
            init, matched, rms = register_cloud.init_from_cameras(*register['init_cameras'])
            register_args['init_transform'] = init
            init_cameras = {'recon_sparse': str(register['init_cameras'][0]), 'gt_sparse': str(register['init_cameras'][1]),
                            'matched_images': matched, 'rms': rms}
    example._load_weights()
    torch.cuda.set_device(FLAGS.gpu_id)          # every kernel launches on the current device's stream
    device = torch.device('cuda:%d' % FLAGS.gpu_id)
    opts = _SceneOptions(device, gt_points, register_args, init_cameras, score_maps, clean, clean_keep_normals, mesh)
    source = _SceneSource(device) if scene_cache else _PipelineSource(device, use_graph)
    try:
        for image_info, _fmt in image_infos:
            mvs_list = gen_data_list(image_info[0])
            savepath_current = os.path.join(savepath, image_info[2])
            writer = _Writer(scene_cache and write_thread, timed=scene_cache)
            try:
                scene_fusion, map_cams, scene_runtime = _run_scene(source, mvs_list, savepath_current, writer, map_files, fuse,
                                                                   score_maps is not None or mesh is not None, device)
            finally:
                writer.close()
            if scene_fusion is not None:
                _end_scene(image_info[2], scene_fusion, map_cams, savepath_current, opts)
            print(Notify.INFO, '%s: %d depth maps, %.2f s' % (image_info[2], len(mvs_list), scene_runtime), Notify.ENDC)
    finally:
        source.close()


def _normal_options(flags):
    """run_eval_pc's fuse_normals from cli's --fuse_normal* options: those that were given, None when none was."""
    return depth_fusion.options(None, flags, 'fuse_') or None


def _target_options(flags):
    """The entries of run_eval_pc's register dict from cli's --register_normal* options: those that were given."""
    names = dict(register_normals='normal_side', register_normal_k='normal_k', register_normal_radius='normal_radius')
    given = {key: getattr(flags, option) for option, key in names.items() if getattr(flags, option, None) is not None}
    if given.get('normal_side') == 'source':
        del given['normal_side']                                    # the default: nothing new is passed on
    return given


def _global_options(flags):
    """The entry `global` of run_eval_pc's register dict: absent without --register_global, else eval_cloud.global_options'."""
    given = eval_cloud.global_options(flags)
    return {} if given is None else {'global': given}


def _run_options(flags, parser=None):
    """run_eval_pc's keyword arguments from a namespace of cli's options (FLAGS, cli's parsed arguments): one it lacks is off.
    Each group's value comes from its owner's options(); with `parser` what an owner refuses is an argument error."""
    opt = lambda name, default=None: getattr(flags, name, default)          # noqa: E731
    mesh = dict(mesh_fusion.options(parser, flags, 'mesh_'), **({'render': True} if opt('mesh_render') else {}))
    return dict(
        {'mesh': mesh} if mesh else {},
        use_graph=not opt('eager'), scene_cache=opt('scene_cache', False), write_thread=not opt('sync_write'),
        fuse=dict(prob_threshold=flags.prob_threshold, disp_threshold=flags.disp_threshold, num_consistent=flags.num_consistent)
        if opt('fuse') else None,
        fuse_normals=_normal_options(flags),
        map_files=not opt('no_map_files'), gt_ply=opt('gt_ply') or None, clean=opt('clean') or None,
        register=dict(dict(icp='plane') if opt('register_icp') == 'plane' else {}, with_scale=opt('with_scale', False),
                      init_cameras=opt('init_cameras') or None, **dict(_target_options(flags), **_global_options(flags)))
        if opt('register') else None,
        clean_keep_normals=bool(opt('clean_keep_normals')),
        score_maps=eval_depth.options(parser, flags, 'map_') if opt('score_maps') else None)


def main(scene_list=None, base_path='eth3d/', options=None):
    """(reference :400-424)  options: run_eval_pc's keyword arguments (default: _run_options(FLAGS))."""
    scene_list = ETH3D_LOW_RES_TEST if scene_list is None else scene_list
    os.makedirs(FLAGS.savepath, exist_ok=True)
    FLAGS.max_h = int(FLAGS.max_h / 32) * 32
    FLAGS.max_w = int(FLAGS.max_w / 32) * 32
    image_infos = []
    for scene in scene_list:
        folder = os.path.join(FLAGS.data_root, base_path + scene)
        image_infos.append([[folder, os.path.join(folder, 'images'), scene], 'preprocessed'])
    run_eval_pc(FLAGS.savepath, image_infos, **(_run_options(FLAGS) if options is None else options))


def make_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--data_root', type=str, default=FLAGS.data_root)
    parser.add_argument('--savepath', type=str, default=FLAGS.savepath)
    parser.add_argument('--pretrained_model_ckpt_path', type=str, default=FLAGS.pretrained_model_ckpt_path)
    parser.add_argument('--view_num', type=int, default=8)
    parser.add_argument('--max_d', type=int, default=128)
    parser.add_argument('--max_w', type=int, default=FLAGS.max_w)
    parser.add_argument('--max_h', type=int, default=FLAGS.max_h)
    parser.add_argument('--gpu_id', type=int, default=FLAGS.gpu_id)
    parser.add_argument('--scenes', type=str, default=None, help='comma-separated scene folders under data_root/eth3d/')
    parser.add_argument('--synthetic_weights', action='store_true')
    parser.add_argument('--write_upsampled', action='store_true')
    parser.add_argument('--eager', action='store_true')
    parser.add_argument('--maps_in_flight', choices=('serial', 'cu_split'), default='serial',
                        help='serial: one depth map on the GPU at a time (default); cu_split: the two queued depth maps run concurrently, '
                             'each on its own half of every XCD (example.cu_split_streams: no SIMD shared between them; same bits, '
                             'more depth maps per second, twice the latency of one)')
    parser.add_argument('--scene_cache', action='store_true',
                        help='prepare each image on the GPU and run the 2-D towers on it once per scene; maps are assembled from '
                             'the cached features (atvsnet/scene.py); files are written by a background thread')
    parser.add_argument('--sync_write', action='store_true', help='--scene_cache: write the files in the driver thread')
    parser.add_argument('--fuse', action='store_true',
                        help='stage every depth map on the GPU as it is finished and end each scene with <savepath>/<scene>/'
                             'final3d_model.ply, the point cloud depth_fusion makes from the written files (depth_fusion.SceneFusion)')
    parser.add_argument('--prob_threshold', type=float, default=0.8, help='--fuse: depth_fusion --prob_threshold')
    parser.add_argument('--disp_threshold', type=float, default=0.01, help='--fuse: depth_fusion --disp_threshold')
    parser.add_argument('--num_consistent', type=float, default=2, help='--fuse: depth_fusion --num_consistent')
    parser.add_argument('--no_map_files', action='store_true',
                        help='--fuse: do not write the per-map files of depths_atvsnet/ (zz_runtime.txt is still written)')
    depth_fusion.add_options(parser, 'fuse_', defaults=False)                  # --fuse: depth_fusion's --normals ...
    parser.add_argument('--gt_ply', type=str, default=None, metavar='FILE[,FILE...]',
                        help='--fuse: score each scene\'s fused cloud against these ground-truth PLY file(s) (eval_cloud: accuracy, '
                             'completeness, F-score; not the official ETH3D evaluator) into <savepath>/<scene>/cloud_eval.json')
    eval_cloud.add_register_arguments(parser)                                  # --gt_ply: eval_cloud's --register ...
    parser.add_argument('--score_maps', action='store_true',
                        help='--gt_ply: render the ground truth into the scene\'s cameras and score the depth maps that entered the '
                             'cloud against it (eval_depth: mae, rmse, ..., inlier ratios per map; a point splat, not ETH3D\'s '
                             'renderer) into <savepath>/<scene>/depth_eval.json; with --register the matrix found is used')
    eval_depth.add_options(parser, 'map_')                                     # --score_maps: eval_depth's --splat ...
    clean_cloud.add_options(parser, 'clean_')                                  # --fuse: clean_cloud's --voxel ...
    mesh_fusion.add_options(parser, 'mesh_', tool=False)                       # --fuse: mesh_fusion's --voxel ...
    parser.add_argument('--mesh_render', action='store_true',
                        help='--mesh_voxel: render the mesh into the scene\'s map cameras (ops.mesh_render) as '
                             '<savepath>/<scene>/depths_mesh/%%08d_mesh.pfm; mesh.json gains `render`')
    return parser


def cli(argv=None):
    parser = make_parser()
    args = parser.parse_args(argv)
    # what only the command line can break; the rest is the owners' options() and _check_options
    if (args.with_scale or args.init_cameras) and not args.register:
        parser.error('--with_scale and --init_cameras need --register')
    if args.register_icp is not None and not args.register:
        parser.error('--register_icp needs --register')
    if (args.register_normals, args.register_normal_k, args.register_normal_radius) != (None, None, None) and not args.register:
        parser.error('--register_normals, --register_normal_k and --register_normal_radius need --register')
    eval_cloud.check_register_values(parser, args)
    if any(v is not None and not (v > 0.0 and np.isfinite(v)) for v in (args.global_voxel, args.global_tau)):
        parser.error('--global_voxel and --global_tau must be positive and finite')
    if not args.score_maps and (args.map_splat != eval_depth.DEFAULT_SPLAT or args.map_occlusion_tol != eval_depth.DEFAULT_OCCLUSION_TOL
                                or args.map_pixel_centre != eval_depth.DEFAULT_PIXEL_CENTRE):
        parser.error('--map_splat, --map_occlusion_tol and --map_pixel_centre need --score_maps')
    if not args.score_maps and (args.map_occlusion_mesh is not None or args.map_occlusion_mesh_tol is not None):
        parser.error('--map_occlusion_mesh and --map_occlusion_mesh_tol need --score_maps')
    args.gt_ply = [p for p in args.gt_ply.split(',') if p] if args.gt_ply else None
    args.clean = clean_cloud.options(parser, args, 'clean_') or None
    options = _run_options(args, parser)                    # each group's value, once
    for given, names in ((args.mesh_render, '--mesh_render needs'), (args.mesh_carve is not None, '--mesh_carve needs'),
                         (options.get('mesh', {}).get('clean'), '--mesh_clean_min_faces, --mesh_clean_min_ratio and --mesh_clean_keep_largest need')):
        if given and args.mesh_voxel is None:
            parser.error(names + ' --mesh_voxel')
    if not (args.map_occlusion_tol >= 0.0 and np.isfinite(args.map_occlusion_tol)) or not np.isfinite(args.map_pixel_centre):
        parser.error('--map_occlusion_tol must be >= 0 and finite, --map_pixel_centre finite')
    try:
        _check_options(**options)
    except ValueError as e:
        parser.error(str(e))
    scenes = args.scenes.split(',') if args.scenes else None
    _Pipelines.CO_RESIDENT = 'cu_split' if args.maps_in_flight == 'cu_split' else False
    for k, v in vars(args).items():
        if k not in ('scenes', 'maps_in_flight'):
            setattr(FLAGS, k, v)
    print('Evaluate A-TVSNet pointcloud with %d views' % (FLAGS.view_num))
    main(scenes, options=options)


if __name__ == '__main__':
    cli()
