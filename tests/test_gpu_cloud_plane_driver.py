"""-m gpu: eval_pointcloud --fuse --fuse_normals depth --register --register_icp plane --clean_keep_normals on the toy scene of
tests/test_gpu_depth_normals.py: the normals SceneFusion returns reach the registration and the cleaned PLY."""
import json
import os
import sys

import numpy as np
import pytest

import atvsnet_amd  # noqa: F401
from atvsnet_amd import FLAGS
from atvsnet_amd.atvsnet import eval_pointcloud as E
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_knn_restated as KR  # noqa: E402
from test_gpu_depth_normals import _write_scene_dir  # noqa: E402

pytestmark = pytest.mark.gpu


def test_driver_registers_by_planes_and_keeps_the_normals_through_cleaning(cuda, tmp_path, weights):
    """Two runs of the same scene.  The first writes final3d_model.ply with normals.  The second takes that file as its ground truth
    and registers its own (identical) cloud to it by point-to-plane ICP: every residual is exactly 0, so every increment is the
    identity and every point has a partner at distance 0; and it cleans with --clean_keep_normals: the cleaned PLY carries
    normals[rows] of the restated clean.  Every other file of the second run is what the first wrote."""
    root = str(tmp_path)
    _write_scene_dir(root)
    base = ['--data_root', root, '--view_num', '3', '--max_d', '16', '--max_w', '160', '--max_h', '128', '--synthetic_weights',
            '--scenes', 'toy', '--fuse', '--no_map_files', '--prob_threshold', '0.5', '--disp_threshold', '0.5', '--num_consistent', '1',
            '--fuse_normals', 'depth', '--fuse_normal_threshold', '80', '--fuse_normal_step', '2', '--fuse_normal_depth_gate', '0.5']
    first, second = os.path.join(root, 'out_first'), os.path.join(root, 'out_second')
    fused = os.path.join(first, 'toy', 'final3d_model.ply')
    try:
        FLAGS.reset()
        E.cli(base + ['--savepath', first])
        FLAGS.reset()
        E.cli(base + ['--savepath', second, '--gt_ply', fused, '--register', '--register_icp', 'plane', '--clean_voxel', '0.05',
                      '--clean_keep_normals'])
    finally:
        FLAGS.reset()
        E._Pipelines.CO_RESIDENT = False
    with open(fused, 'rb') as f, open(os.path.join(second, 'toy', 'final3d_model.ply'), 'rb') as g:
        assert f.read() == g.read()
    pts, cols, nrm = ply.read_ply_normals(fused)
    assert nrm is not None and len(pts) > 100
    with open(os.path.join(second, 'toy', 'cloud_eval.json')) as f:
        score = json.load(f)
    reg = score['registration']
    print('%d points; registration %s' % (len(pts), reg['stages']))
    assert reg['icp'] == 'plane' and all('plane_rmse' in s and s['iterations'] == 1 and s['converged'] for s in reg['stages'])
    assert np.array_equal(np.array(reg['matrix']), np.eye(4)) and all(s['plane_rmse'] == 0.0 for s in reg['stages'])
    assert all(t['accuracy'] == 1.0 and t['completeness'] == 1.0 for t in score['tolerances'])
    want_p, want_c, rows = KR.clean(pts, cols, voxel=0.05)
    got_p, got_c, got_n = ply.read_ply_normals(os.path.join(second, 'toy', 'final3d_model_clean.ply'))
    assert 0 < len(rows) < len(pts) and got_p.tobytes() == want_p.tobytes() and np.array_equal(got_c, want_c)
    assert got_n is not None and got_n.tobytes() == nrm[rows].tobytes()
