"""The mesh simplification through its drivers: SceneMesh(simplify=) against the restatement applied to the mesh (to the cleaned
mesh with clean=), run_eval_pc's mesh dict beside an unchanged run, and simplify_mesh's command line on a written PLY."""
import json
import os
import sys

import numpy as np
import pytest

import atvsnet_amd  # noqa: F401
from atvsnet_amd import FLAGS, ops
from atvsnet_amd.atvsnet import depth_fusion as DF, eval_pointcloud as E, mesh_fusion, simplify_mesh
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_simplify_restated as S  # noqa: E402
import mesh_topology_restated as T  # noqa: E402
from fusion_scene import make_scene  # noqa: E402
from test_gpu_depth_normals import _write_scene_dir  # noqa: E402
from test_gpu_mesh_driver import _cameras  # noqa: E402

pytestmark = pytest.mark.gpu

VOXEL, TRUNC_VOXELS, MIN_WEIGHT, CELL_VOXELS = 0.1, 4.0, 1.0, 3
LOW_MARGIN = 1e-6


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_mesh(got, want):
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert got[2].dtype == np.int32 and got[0].dtype == np.float32


def _is_the_restatement(got, report, source, cell, origin, placement='quadric'):
    """A simplified mesh and its report against the restatement applied to `source` = (vertices, colors, faces): counts, faces and
    colours exactly; the positions bit for bit with the mean, and with the quadric to the solve's allowance plus a float32 spacing
    on the clusters that sit on no decision (at most 1 % may)."""
    want = S.simplify(source[0], source[1], source[2], cell, origin, placement)
    for key, n in want['counts'].items():
        if key not in ('placed_by_quadric', 'fell_back'):
            assert report[key] == n, key
    assert np.array_equal(got[2], want['out'][2]) and got[2].dtype == np.int32 and np.array_equal(got[1], want['out'][1])
    assert report['census_out'] == T.edge_census(want['out'][2], len(want['out'][0]))
    assert report['census_in'] == T.edge_census(source[2], len(source[0]))
    assert 0.0 < report['max_move'] <= report['max_move_bound'] == cell * np.sqrt(3.0)
    if placement == 'mean':
        assert np.array_equal(_bits(got[0]), _bits(want['out'][0]))
        return want
    margin = want['place']['margin']
    unsure = int((margin < LOW_MARGIN).sum())
    assert unsure <= 0.01 * len(margin) and abs(report['placed_by_quadric'] - want['counts']['placed_by_quadric']) <= unsure
    rows = margin[want['cluster_map'] >= 0] >= LOW_MARGIN
    w = want['out'][0][rows]
    err = np.abs(got[0][rows].astype(np.float64) - w.astype(np.float64))
    allowance = cell * ops.MESH_SIMPLIFY_SOLVE_UNITS * 2.0 ** -53 / 1e-3
    print('simplified %d -> %d faces, %d clusters, %d placed by their quadric; largest position error %.3g'
          % (report['faces_in'], report['faces_out'], report['clusters'], report['placed_by_quadric'], err.max(initial=0.0)))
    assert (err <= allowance + np.spacing(np.abs(w)).astype(np.float64)).all()
    return want


def test_scene_mesh_simplifies_on_the_device_what_the_restatement_simplifies(cuda, tmp_path):
    Ps, depths, _, images = make_scene()[:4]
    n, rows, cols = depths.shape
    depths = depths.copy()
    for view, (r, c) in ((0, (8, 10)), (1, (20, 24))):                 # fragments off the surface, as in test_gpu_mesh_clean_driver.py
        depths[view, r:r + 5, c:c + 5] -= 1.0
    cams = _cameras(Ps, rows, cols)
    fusion = DF.SceneFusion(n, rows, cols, cuda, prob_threshold=0.5, disp_threshold=0.01, num_consistent=2, inverse_depth=False)
    for k in range(n):
        fusion.add(k * 10, np.ascontiguousarray(depths[k]), np.ones((rows, cols), np.float32), images[k], cams[k])
    cam_of = {k * 10: cams[k] for k in range(n)}
    plain = mesh_fusion.SceneMesh(fusion, cam_of, VOXEL, TRUNC_VOXELS, MIN_WEIGHT)
    whole = plain.run()
    with pytest.raises(RuntimeError, match='no simplify= was given'):
        plain.simplify_report()
    for placement in ('quadric', 'mean'):
        scene_mesh = mesh_fusion.SceneMesh(fusion, cam_of, VOXEL, TRUNC_VOXELS, MIN_WEIGHT, simplify=dict(cell_voxels=CELL_VOXELS, placement=placement))
        _same_mesh(scene_mesh.run(), whole)                              # run() stays the whole mesh
        assert scene_mesh.report() == dict(plain.report(), seconds=scene_mesh.report()['seconds'])
        assert set(scene_mesh.report()['seconds']) == {'bounds', 'integrate', 'extract', 'download', 'report'}
        report = scene_mesh.simplify_report()
        assert report['source'] == 'mesh' and report['cell_voxels'] == CELL_VOXELS and report['cell'] == CELL_VOXELS * VOXEL
        assert report['origin'] == [float(o) for o in scene_mesh.volume.origin] and report['placement'] == placement
        want = _is_the_restatement(scene_mesh.simplify_result(), report, whole, CELL_VOXELS * VOXEL, report['origin'], placement)
        assert 0 < report['faces_out'] < report['faces_in'] // 4 and report['degenerate_faces'] > 0
    path = str(tmp_path / 'simple.ply')
    assert scene_mesh.write_simple_ply(path) == len(want['out'][2])
    _same_mesh(ply.read_mesh(path), scene_mesh.simplify_result())
    # with clean= it is the cleaned mesh that is simplified
    both = mesh_fusion.SceneMesh(fusion, cam_of, VOXEL, TRUNC_VOXELS, MIN_WEIGHT, clean=dict(keep_largest=1), simplify=dict(cell_voxels=CELL_VOXELS))
    _same_mesh(both.run(), whole)
    cleaned = both.clean_result()
    assert len(cleaned[2]) < len(whole[2]) and both.simplify_report()['source'] == 'clean'
    _is_the_restatement(both.simplify_result(), both.simplify_report(), cleaned, CELL_VOXELS * VOXEL, both.simplify_report()['origin'])
    assert both.simplify_report()['faces_in'] == len(cleaned[2])


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


def _drive(argv, simplify):
    """eval_pointcloud.cli's own steps with simplify= added to the mesh dict: the command line has no option for it."""
    parser = E.make_parser()
    args = parser.parse_args(argv)
    args.gt_ply = args.clean = None
    options = E._run_options(args, parser)
    options['mesh'] = dict(options['mesh'], simplify=simplify)
    E._check_options(**options)
    for k, v in vars(args).items():
        if k not in ('scenes', 'maps_in_flight'):
            setattr(FLAGS, k, v)
    E.main(args.scenes.split(','), options=options)


def test_driver_writes_the_simplified_mesh_beside_an_unchanged_run(cuda, tmp_path, weights, capsys):
    root = str(tmp_path)
    _write_scene_dir(root)
    base = ['--data_root', root, '--view_num', '3', '--max_d', '16', '--max_w', '160', '--max_h', '128', '--synthetic_weights',
            '--scenes', 'toy', '--fuse', '--no_map_files', '--prob_threshold', '0.5', '--disp_threshold', '0.5', '--num_consistent', '1',
            '--mesh_voxel', '0.05', '--mesh_min_weight', '1']
    meshed, simple = os.path.join(root, 'out_mesh'), os.path.join(root, 'out_simple')
    try:
        FLAGS.reset()
        E.cli(base + ['--savepath', meshed])
        FLAGS.reset()
        _drive(base + ['--savepath', simple], dict(cell_voxels=CELL_VOXELS))
    finally:
        FLAGS.reset()
        E._Pipelines.CO_RESIDENT = False
    before = ['depths_atvsnet', 'final3d_mesh.ply', 'final3d_model.ply', 'mesh.json', 'zz_runtime.txt']
    assert sorted(os.listdir(os.path.join(meshed, 'toy'))) == before                 # the listing is as it was without the argument
    assert sorted(os.listdir(os.path.join(simple, 'toy'))) == sorted(before + ['final3d_mesh_simple.ply', 'mesh_simple.json'])
    for name in ('final3d_mesh.ply', 'final3d_model.ply'):
        assert _read(os.path.join(meshed, 'toy', name)) == _read(os.path.join(simple, 'toy', name))
    reports = []                                                        # mesh.json carries wall-clock seconds: every other byte is the same
    for folder in (meshed, simple):
        with open(os.path.join(folder, 'toy', 'mesh.json')) as f:
            reports.append(json.load(f))
        assert set(reports[-1]['seconds']) == {'bounds', 'integrate', 'extract', 'download', 'report'}
        reports[-1]['seconds'] = None
    assert json.dumps(reports[0], sort_keys=True) == json.dumps(reports[1], sort_keys=True)
    whole = ply.read_mesh(os.path.join(simple, 'toy', 'final3d_mesh.ply'))
    written = ply.read_mesh(os.path.join(simple, 'toy', 'final3d_mesh_simple.ply'))
    with open(os.path.join(simple, 'toy', 'mesh_simple.json')) as f:
        report = json.load(f)
    print({k: v for k, v in report.items() if k != 'seconds'})
    assert report['cell'] == CELL_VOXELS * 0.05 and report['origin'] == reports[1]['origin'] and report['source'] == 'mesh'
    _is_the_restatement(written, report, whole, report['cell'], report['origin'])
    # the tool on the written mesh gives the same mesh
    capsys.readouterr()
    out, out_report = str(tmp_path / 'tool' / 'simple.ply'), str(tmp_path / 'tool' / 'simple.json')
    result = simplify_mesh.cli(['--in', os.path.join(simple, 'toy', 'final3d_mesh.ply'), '--out', out, '--cell', repr(report['cell']),
                                '--origin=' + ','.join(repr(o) for o in report['origin']), '--report', out_report])
    assert _read(out) == _read(os.path.join(simple, 'toy', 'final3d_mesh_simple.ply'))
    with open(out_report) as f:
        assert json.load(f) == json.loads(json.dumps(result))
    same = lambda r: {k: v for k, v in r.items() if k not in ('seconds', 'cell_voxels', 'source')}      # noqa: E731
    assert same(result) == same(report)
