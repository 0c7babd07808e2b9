"""The mesh cleaning through its drivers: SceneMesh(clean=) against the restatement applied to the uncleaned mesh, eval_pointcloud's
--mesh_clean_ options beside an unchanged run, and clean_mesh's command line on a written PLY."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
from atvsnet_amd import FLAGS
from atvsnet_amd.atvsnet import clean_mesh, depth_fusion as DF, eval_pointcloud as E, mesh_fusion
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_topology_restated as T  # noqa: E402
from fusion_scene import make_scene  # noqa: E402
from test_gpu_depth_normals import _write_scene_dir  # noqa: E402
from test_gpu_mesh_driver import _cameras  # noqa: E402

pytestmark = pytest.mark.gpu

VOXEL, TRUNC_VOXELS, MIN_WEIGHT = 0.1, 4.0, 1.0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_mesh(got, want):
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert got[2].dtype == np.int32 and got[0].dtype == np.float32


def test_scene_mesh_cleans_on_the_device_what_the_restatement_cleans(cuda, tmp_path):
    Ps, depths, _, images = make_scene()[:4]
    n, rows, cols = depths.shape
    depths = depths.copy()
    # depth blobs one unit in front of the plane in two views: beyond the band of 0.4 either side of the surface, inside the box's
    # pad of 1.2.  No other view agrees, so the cloud does not hold them; with min_weight 1 the mesh does, as fragments
    for view, (r, c) in ((0, (8, 10)), (0, (30, 44)), (1, (20, 24)), (1, (36, 8))):
        depths[view, r:r + 5, c:c + 5] -= 1.0
    cams = _cameras(Ps, rows, cols)
    fusion = DF.SceneFusion(n, rows, cols, cuda, prob_threshold=0.5, disp_threshold=0.01, num_consistent=2, inverse_depth=False)
    for k in range(n):
        fusion.add(k * 10, np.ascontiguousarray(depths[k]), np.ones((rows, cols), np.float32), images[k], cams[k])
    cam_of = {k * 10: cams[k] for k in range(n)}
    plain = mesh_fusion.SceneMesh(fusion, cam_of, VOXEL, TRUNC_VOXELS, MIN_WEIGHT)
    whole = plain.run()
    with pytest.raises(RuntimeError, match='no clean= criteria'):
        plain.clean_report()
    _, face_component, face_count, _ = T.components(whole[2], len(whole[0]))
    print('components', sorted(face_count.tolist()))
    assert len(face_count) >= 3 and sorted(face_count.tolist())[-2] * 4 < face_count.max()          # fragments exist, one giant
    for criteria in (dict(keep_largest=1), dict(min_ratio='1/10', min_faces=2), dict(keep_largest=2)):
        scene_mesh = mesh_fusion.SceneMesh(fusion, cam_of, VOXEL, TRUNC_VOXELS, MIN_WEIGHT, clean=criteria)
        _same_mesh(scene_mesh.run(), whole)                              # run() stays the whole mesh
        keep = clean_mesh.keep_components(face_count, **criteria)
        want = T.clean(whole[0], whole[1], whole[2], keep)
        _same_mesh(scene_mesh.clean_result(), want)
        report = scene_mesh.clean_report()
        assert report['components'] == len(face_count) and report['components_removed'] == int((~keep).sum()) >= 1
        assert report['largest_components'] == sorted(face_count.tolist(), reverse=True)[:16]
        assert (report['faces_in'], report['vertices_in']) == (len(whole[2]), len(whole[0]))
        assert (report['faces_out'], report['vertices_out']) == (len(want[2]), len(want[0]))
        assert report['census_in'] == T.edge_census(whole[2], len(whole[0])) and report['census_out'] == T.edge_census(want[2], len(want[0]))
        assert scene_mesh.report() == dict(plain.report(), seconds=scene_mesh.report()['seconds'])
        assert set(scene_mesh.report()['seconds']) == {'bounds', 'integrate', 'extract', 'download', 'report'}
    path = str(tmp_path / 'clean.ply')
    assert scene_mesh.write_clean_ply(path) == len(want[2])
    _same_mesh(ply.read_mesh(path), want)
    seen = scene_mesh.render(str(tmp_path / 'clean_maps'), clean=True)
    everything = scene_mesh.render(str(tmp_path / 'maps'))
    assert seen['maps'] == everything['maps'] == n and 0 < seen['covered_fraction'] <= everything['covered_fraction']
    assert scene_mesh.clean_report()['render'] == seen and scene_mesh.report()['render'] == everything
    assert sorted(os.listdir(str(tmp_path / 'clean_maps'))) == ['%08d_mesh.pfm' % (k * 10) for k in range(n)]


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


def test_driver_writes_the_cleaned_mesh_beside_an_unchanged_run(cuda, tmp_path, weights, capsys):
    root = str(tmp_path)
    _write_scene_dir(root)
    base = ['--data_root', root, '--view_num', '3', '--max_d', '16', '--max_w', '160', '--max_h', '128', '--synthetic_weights',
            '--scenes', 'toy', '--fuse', '--no_map_files', '--prob_threshold', '0.5', '--disp_threshold', '0.5', '--num_consistent', '1',
            '--mesh_voxel', '0.05', '--mesh_min_weight', '1']
    meshed, cleaned = os.path.join(root, 'out_mesh'), os.path.join(root, 'out_clean')
    try:
        FLAGS.reset()
        E.cli(base + ['--savepath', meshed])
        FLAGS.reset()
        E.cli(base + ['--savepath', cleaned, '--mesh_clean_keep_largest', '1'])
    finally:
        FLAGS.reset()
        E._Pipelines.CO_RESIDENT = False
    before = ['depths_atvsnet', 'final3d_mesh.ply', 'final3d_model.ply', 'mesh.json', 'zz_runtime.txt']
    assert sorted(os.listdir(os.path.join(meshed, 'toy'))) == before                 # the listing is as it was without the options
    assert sorted(os.listdir(os.path.join(cleaned, 'toy'))) == sorted(before + ['final3d_mesh_clean.ply', 'mesh_clean.json'])
    for name in ('final3d_mesh.ply', 'final3d_model.ply'):
        assert _read(os.path.join(meshed, 'toy', name)) == _read(os.path.join(cleaned, 'toy', name))
    # mesh.json carries wall-clock seconds, which no two runs share: every other byte is the same
    reports = []
    for folder in (meshed, cleaned):
        with open(os.path.join(folder, 'toy', 'mesh.json')) as f:
            reports.append(json.load(f))
        assert set(reports[-1]['seconds']) == {'bounds', 'integrate', 'extract', 'download', 'report'}
        reports[-1]['seconds'] = None
    assert json.dumps(reports[0], sort_keys=True) == json.dumps(reports[1], sort_keys=True)
    whole = ply.read_mesh(os.path.join(cleaned, 'toy', 'final3d_mesh.ply'))
    _, _, face_count, _ = T.components(whole[2], len(whole[0]))
    want = T.clean(whole[0], whole[1], whole[2], clean_mesh.keep_components(face_count, keep_largest=1))
    _same_mesh(ply.read_mesh(os.path.join(cleaned, 'toy', 'final3d_mesh_clean.ply')), want)
    with open(os.path.join(cleaned, 'toy', 'mesh_clean.json')) as f:
        report = json.load(f)
    print({k: v for k, v in report.items() if k != 'seconds'})
    assert report['components'] == len(face_count) and report['faces_out'] == len(want[2]) == int(face_count.max())
    assert report['criteria'] == {'min_faces': None, 'min_ratio': None, 'keep_largest': 1}
    assert report['census_out'] == T.edge_census(want[2], len(want[0]))
    # the tool on the written mesh gives the same file
    capsys.readouterr()
    out, out_report = str(tmp_path / 'tool' / 'clean.ply'), str(tmp_path / 'tool' / 'clean.json')
    result = clean_mesh.cli(['--in', os.path.join(cleaned, 'toy', 'final3d_mesh.ply'), '--out', out, '--keep_largest', '1', '--report', out_report])
    assert _read(out) == _read(os.path.join(cleaned, 'toy', 'final3d_mesh_clean.ply'))
    with open(out_report) as f:
        assert json.load(f) == json.loads(json.dumps(result))
    assert {k: v for k, v in result.items() if k != 'seconds'} == {k: v for k, v in report.items() if k != 'seconds'}
    # a cleaned mesh is a fixed point; a third-party layout (no colours) goes through read_mesh_any
    again = clean_mesh.clean(*ply.read_mesh(out), min_faces=1)
    _same_mesh(again[:3], want)
    assert again[3]['components_removed'] == 0 and again[3]['components'] == 1


def test_the_meshing_tool_also_writes_the_cleaned_mesh(cuda, tmp_path):
    """mesh_fusion's command line with --clean_keep_largest and --clean_out on written maps with a depth blob in one of them."""
    from atvsnet_amd.atvsnet.preprocess import write_cam, write_pfm
    Ps, depths, _, _ = make_scene()[:4]
    n, rows, cols = depths.shape
    depths = depths.copy()
    depths[0, 8:13, 10:15] -= 1.0
    depths[2, 30:35, 40:45] -= 1.0
    cams = _cameras(Ps, rows, cols)
    folder = tmp_path / 'toy' / 'depths_atvsnet'
    folder.mkdir(parents=True)
    for k in range(n):
        write_pfm(str(folder / ('%08d.pfm' % k)), depths[k])
        write_cam(str(folder / ('%08d.txt' % k)), cams[k])
    out, clean_out, report_path = (str(tmp_path / name) for name in ('mesh.ply', 'clean.ply', 'mesh.json'))
    result = mesh_fusion.cli(['--maps', str(tmp_path / 'toy'), '--voxel', str(VOXEL), '--min_weight', '1', '--out', out,
                              '--clean_keep_largest', '1', '--clean_out', clean_out, '--report', report_path])
    whole = ply.read_mesh(out)
    _, _, face_count, _ = T.components(whole[2], len(whole[0]))
    print('components', sorted(face_count.tolist()))
    assert len(face_count) >= 2
    want = T.clean(whole[0], whole[1], whole[2], clean_mesh.keep_components(face_count, keep_largest=1))
    _same_mesh(ply.read_mesh(clean_out), want)
    assert result['clean']['components'] == len(face_count) and result['clean']['faces_out'] == int(face_count.max()) == len(want[2])
    assert result['faces'] == len(whole[2]) and result['boundary_edges'] == T.edge_census(whole[2], len(whole[0]))['boundary']
    with open(report_path) as f:
        assert json.load(f) == json.loads(json.dumps(result))
