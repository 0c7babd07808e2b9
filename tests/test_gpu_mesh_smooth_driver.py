"""The mesh smoothing through its drivers, on the scene of tests/test_gpu_mesh_simplify_driver.py: SceneMesh(smooth=) against the
restatement applied to the mesh (to the cleaned mesh with clean=), the simplification that then takes the smoothed mesh,
run_eval_pc's mesh=dict(voxel=, smooth=) beside a run without the key, and smooth_mesh's command line on the written PLY."""
import json
import os
import sys

import numpy as np
import pytest

import atvsnet_amd  # noqa: F401
from atvsnet_amd import FLAGS
from atvsnet_amd.atvsnet import depth_fusion as DF, eval_pointcloud as E, mesh_fusion, smooth_mesh
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_smooth_restated as R  # noqa: E402
from fusion_scene import make_scene  # noqa: E402
from test_gpu_depth_normals import _write_scene_dir  # noqa: E402
from test_gpu_mesh_driver import _cameras  # noqa: E402
from test_gpu_mesh_simplify_driver import CELL_VOXELS, MIN_WEIGHT, TRUNC_VOXELS, VOXEL, _bits, _read, _same_mesh  # noqa: E402
from test_gpu_mesh_sample_driver import _drive  # noqa: E402

pytestmark = pytest.mark.gpu

SMOOTH = dict(iterations=3, normals=True)


def _is_the_restatement(got, report, source, voxel, **options):
    """A smoothed mesh (vertices, colors, faces, normals) and its report against the restatement applied to `source`."""
    want, info = R.smooth(source[0], source[2], options.get('iterations', 3), options.get('lam', 0.5), options.get('mu', -0.53),
                          options.get('pin_boundary', False))
    assert info['clamped'] == 0
    assert np.array_equal(_bits(got[0]), _bits(want)) and np.array_equal(got[1], source[1]) and np.array_equal(got[2], source[2])
    assert got[2].dtype == np.int32 and got[0].dtype == np.float32
    for key in R.ADJACENCY_INFO + ('step', 'origin', 'nonfinite_vertices'):
        assert report[key] == info[key], key
    assert set(report) == set(smooth_mesh.REPORT_KEYS) | {'source'}
    assert report['vertices'] == len(source[0]) and report['faces'] == len(source[2]) and 0 < report['moved'] <= len(source[0])
    assert report['max_move'] > 0.0 and report['area_unit'] == (voxel * voxel if options.get('normals') else None)
    if options.get('normals'):
        sums, incidences = R.vertex_normal_sums(want, source[2], voxel * voxel)
        n = R.normals_from_sums(sums)
        # the device's sums may differ from the restatement's by a unit per incidence and axis (tests/test_gpu_mesh_smooth.py): a
        # sum N of length L then turns by at most 2 sqrt(3) incidences / L, and each float32 rounding adds 2^-24; a vertex of
        # slivers alone, whose sum is 0 here, is left out
        L = np.linalg.norm(sums.astype(np.float64), axis=1)
        rows = L > 0.0
        assert got[3].dtype == np.float32 and got[3].shape == want.shape and not got[3][incidences == 0].any()
        err = np.abs(got[3][rows].astype(np.float64) - n[rows].astype(np.float64)).max(1)
        print('%d vertices: the normals differ from the restatement\'s by at most %.3g' % (len(n), err.max(initial=0.0)))
        assert (err <= 2.0 * np.sqrt(3.0) * incidences[rows] / L[rows] + 2.0 ** -23).all()
    else:
        assert got[3] is None
    return want


def test_scene_mesh_smooths_on_the_device_what_the_restatement_smooths(cuda, tmp_path):
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
    with pytest.raises(RuntimeError, match='no smooth= was given'):
        plain.smooth_report()
    scene_mesh = mesh_fusion.SceneMesh(fusion, cam_of, VOXEL, TRUNC_VOXELS, MIN_WEIGHT, smooth=SMOOTH)
    _same_mesh(scene_mesh.run(), whole)                                  # run() stays the whole mesh
    assert scene_mesh.report() == dict(plain.report(), seconds=scene_mesh.report()['seconds'])
    assert set(scene_mesh.report()['seconds']) == {'bounds', 'integrate', 'extract', 'download', 'report'}
    report = scene_mesh.smooth_report()
    assert report['source'] == 'mesh' and report['iterations'] == 3 and (report['lam'], report['mu']) == (0.5, -0.53)
    _is_the_restatement(scene_mesh.smooth_result(), report, whole, VOXEL, **SMOOTH)
    path = str(tmp_path / 'smooth.ply')
    assert scene_mesh.write_smooth_ply(path) == len(whole[2])
    written = ply.read_mesh_normals(path)
    _same_mesh(written[:3], scene_mesh.smooth_result()[:3])
    assert np.array_equal(_bits(written[3]), _bits(scene_mesh.smooth_result()[3]))
    with pytest.raises(RuntimeError, match='no simplify= was given'):
        scene_mesh.simplify_report()
    # with clean= it is the cleaned mesh that is smoothed; with simplify= the simplification takes the smoothed mesh
    options = dict(iterations=2, pin_boundary=True)
    both = mesh_fusion.SceneMesh(fusion, cam_of, VOXEL, TRUNC_VOXELS, MIN_WEIGHT, clean=dict(keep_largest=1), smooth=options,
                                 simplify=dict(cell_voxels=CELL_VOXELS, placement='mean'))
    _same_mesh(both.run(), whole)
    cleaned = both.clean_result()
    assert len(cleaned[2]) < len(whole[2]) and both.smooth_report()['source'] == 'clean' and both.smooth_report()['pinned'] > 0
    smoothed = _is_the_restatement(both.smooth_result(), both.smooth_report(), cleaned, VOXEL, **options)
    assert both.simplify_report()['source'] == 'smooth' and both.simplify_report()['faces_in'] == len(cleaned[2])
    import mesh_simplify_restated as S
    want = S.simplify(smoothed, cleaned[1], cleaned[2], CELL_VOXELS * VOXEL, both.simplify_report()['origin'], 'mean')
    _same_mesh(both.simplify_result(), want['out'])
    unsmoothed = mesh_fusion.SceneMesh(fusion, cam_of, VOXEL, TRUNC_VOXELS, MIN_WEIGHT, clean=dict(keep_largest=1),
                                       simplify=dict(cell_voxels=CELL_VOXELS, placement='mean'))
    assert unsmoothed.simplify_report()['source'] == 'clean'
    _same_mesh(unsmoothed.simplify_result(), S.simplify(cleaned[0], cleaned[1], cleaned[2], CELL_VOXELS * VOXEL,
                                                        unsmoothed.simplify_report()['origin'], 'mean')['out'])


def _json(path):
    with open(path) as f:
        return json.load(f)


def test_driver_writes_the_smoothed_mesh_beside_an_unchanged_run(cuda, tmp_path, weights, capsys):
    root = str(tmp_path)
    _write_scene_dir(root)
    base = ['--data_root', root, '--view_num', '3', '--max_d', '16', '--max_w', '160', '--max_h', '128', '--synthetic_weights',
            '--scenes', 'toy', '--fuse', '--no_map_files', '--prob_threshold', '0.5', '--disp_threshold', '0.5', '--num_consistent', '1',
            '--mesh_voxel', '0.05', '--mesh_min_weight', '1']
    without, given = os.path.join(root, 'out_without'), os.path.join(root, 'out_smooth')
    simplify = dict(cell_voxels=CELL_VOXELS)
    try:
        FLAGS.reset()
        _drive(base + ['--savepath', without], simplify=simplify)
        FLAGS.reset()
        _drive(base + ['--savepath', given], simplify=simplify, smooth=SMOOTH)
    finally:
        FLAGS.reset()
        E._Pipelines.CO_RESIDENT = False
    before = ['depths_atvsnet', 'final3d_mesh.ply', 'final3d_mesh_simple.ply', 'final3d_model.ply', 'mesh.json', 'mesh_simple.json', 'zz_runtime.txt']
    assert sorted(os.listdir(os.path.join(without, 'toy'))) == before              # the listing is as it was without the key
    assert sorted(os.listdir(os.path.join(given, 'toy'))) == sorted(before + ['final3d_mesh_smooth.ply', 'mesh_smooth.json'])
    for name in ('final3d_mesh.ply', 'final3d_model.ply'):
        assert _read(os.path.join(without, 'toy', name)) == _read(os.path.join(given, 'toy', name)), name
    a, b = _json(os.path.join(without, 'toy', 'mesh.json')), _json(os.path.join(given, 'toy', 'mesh.json'))
    assert set(a['seconds']) == set(b['seconds']) == {'bounds', 'integrate', 'extract', 'download', 'report'}
    a['seconds'] = b['seconds'] = None                                 # wall-clock seconds: every other byte is the same
    assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)
    # without the key the simplification takes the mesh, as before; with it, the smoothed mesh
    assert _json(os.path.join(without, 'toy', 'mesh_simple.json'))['source'] == 'mesh'
    assert _json(os.path.join(given, 'toy', 'mesh_simple.json'))['source'] == 'smooth'
    whole = ply.read_mesh(os.path.join(given, 'toy', 'final3d_mesh.ply'))
    written = ply.read_mesh_normals(os.path.join(given, 'toy', 'final3d_mesh_smooth.ply'))
    report = _json(os.path.join(given, 'toy', 'mesh_smooth.json'))
    print({k: v for k, v in report.items() if k != 'seconds'})
    assert report['source'] == 'mesh' and report['area_unit'] == 0.05 * 0.05
    _is_the_restatement(written, report, whole, 0.05, **SMOOTH)
    import mesh_simplify_restated as S
    for folder, source in ((without, whole), (given, written)):          # each simplified mesh is the restatement's of its source
        simple, simple_report = ply.read_mesh(os.path.join(folder, 'toy', 'final3d_mesh_simple.ply')), _json(os.path.join(folder, 'toy', 'mesh_simple.json'))
        want = S.simplify(source[0], source[1], source[2], simple_report['cell'], simple_report['origin'], 'quadric')['out']
        assert np.array_equal(simple[2], want[2]) and np.array_equal(simple[1], want[1])
    # the tool on the written mesh gives the same mesh
    capsys.readouterr()
    out, out_report = str(tmp_path / 'tool' / 'smooth.ply'), str(tmp_path / 'tool' / 'smooth.json')
    result = smooth_mesh.cli(['--in', os.path.join(given, 'toy', 'final3d_mesh.ply'), '--out', out, '--iterations', '3', '--normals',
                              '--normal_area_unit', repr(0.05 * 0.05), '--report', out_report])
    assert _read(out) == _read(os.path.join(given, 'toy', 'final3d_mesh_smooth.ply'))
    assert _json(out_report) == json.loads(json.dumps(result))
    same = lambda r: {k: v for k, v in r.items() if k not in ('seconds', 'source')}      # noqa: E731
    assert same(result) == same(report)
    # --iterations 0 --normals only adds normals
    smooth_mesh.cli(['--in', os.path.join(given, 'toy', 'final3d_mesh.ply'), '--out', out, '--iterations', '0', '--normals', '--report', out_report])
    only = ply.read_mesh_normals(out)
    _same_mesh(only[:3], whole)
    assert only[3] is not None and _json(out_report)['moved'] == 0
