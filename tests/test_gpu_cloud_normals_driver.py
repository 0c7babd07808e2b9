"""-m gpu: eval_pointcloud --fuse --register --register_icp plane --register_normals target WITHOUT --fuse_normals depth on the toy
scene of tests/test_gpu_depth_normals.py, and the cloud_normals tool on the cloud it fused."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
from atvsnet_amd import FLAGS, ops
from atvsnet_amd.atvsnet import cloud_normals as CN, eval_pointcloud as E
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_depth_normals import _write_scene_dir  # noqa: E402

pytestmark = pytest.mark.gpu


def test_driver_registers_over_the_ground_truths_planes_without_fused_normals(cuda, tmp_path, weights, capsys):
    """Two runs of the same scene, neither with --fuse_normals depth.  The first writes final3d_model.ply, a cloud without normals.
    The second takes that file as its ground truth and registers its own (identical) cloud to it over the ground truth's planes,
    whose normals it estimates: source and target are the same float32 positions, so every residual is exactly 0 and the matrix
    is the identity exactly, one iteration per stage (as tests/test_gpu_cloud_plane_driver.py pins for the source side).  Without the new option the command is refused as it
    was, with the new way out named.  Then the tool: cloud_normals --in / --out writes what ops.cloud_normals returns."""
    root = str(tmp_path)
    _write_scene_dir(root)
    base = ['--data_root', root, '--view_num', '3', '--max_d', '16', '--max_w', '160', '--max_h', '128', '--synthetic_weights',
            '--scenes', 'toy', '--fuse', '--no_map_files', '--prob_threshold', '0.5', '--disp_threshold', '0.5', '--num_consistent', '1']
    first, second = os.path.join(root, 'out_first'), os.path.join(root, 'out_second')
    fused = os.path.join(first, 'toy', 'final3d_model.ply')
    plane = ['--savepath', second, '--gt_ply', fused, '--register', '--register_icp', 'plane']
    try:
        FLAGS.reset()
        with pytest.raises(SystemExit) as refused:
            E.cli(base + plane)
        message = ' '.join(capsys.readouterr().err.split())
        assert refused.value.code == 2 and '--register_icp plane needs --fuse_normals depth' in message
        assert 'runs over the fused cloud\'s own normals' in message and 'or give --register_normals target' in message
        assert not os.path.exists(second)
        FLAGS.reset()
        E.cli(base + ['--savepath', first])
        FLAGS.reset()
        E.cli(base + plane + ['--register_normals', 'target'])
    finally:
        FLAGS.reset()
        E._Pipelines.CO_RESIDENT = False
    with open(fused, 'rb') as f, open(os.path.join(second, 'toy', 'final3d_model.ply'), 'rb') as g:
        assert f.read() == g.read()
    assert not ply.has_normals(fused)
    pts, cols = ply.read_ply(fused)
    with open(os.path.join(second, 'toy', 'cloud_eval.json')) as f:
        score = json.load(f)
    reg = score['registration']
    print('%d points; registration %s' % (len(pts), {k: v for k, v in reg.items() if k != 'init'}))
    assert reg['icp'] == 'plane' and reg['normal_side'] == 'target' and reg['normal_k'] == 16 and reg['normal_radius'] == 4.0 * reg['voxel']
    assert 0 < reg['n_gt_normals'] <= reg['n_gt'] and len(pts) > 100
    # q = T src is not rounded to float32 and T starts as the identity: every residual is exactly 0, every increment the identity
    assert all(s['converged'] and s['iterations'] == 1 and s['plane_rmse'] == 0.0 and s['rmse'] == 0.0 for s in reg['stages'])
    assert np.array_equal(np.array(reg['matrix']), np.eye(4))
    assert all(t['accuracy'] == 1.0 and t['completeness'] == 1.0 for t in score['tolerances'])
    # the tool, on the same cloud
    out, report = str(tmp_path / 'with_normals.ply'), str(tmp_path / 'variation.json')
    rep = CN.cli(['--in', fused, '--out', out, '--k', '8', '--radius', '0.3', '--viewpoint', '0,0,0', '--variation_json', report])
    got_p, got_c, got_n = ply.read_ply_normals(out)
    dev = torch.from_numpy(pts).to(cuda)
    idx = ops.cloud_knn(ops.cloud_grid(dev, 0.3), dev, 8, exclude_same_index=True)[1]
    want = ops.cloud_normals(dev, dev, idx, self_counts=True, viewpoints=[(0.0, 0.0, 0.0)]).cpu().numpy()
    assert got_p.tobytes() == pts.tobytes() and np.array_equal(got_c, cols) and got_n.tobytes() == want.tobytes()
    with open(report) as f:
        assert json.load(f) == json.loads(json.dumps(rep))
    nonzero = want.any(axis=1)
    assert rep['n_points'] == len(pts) and rep['n_zero_normals'] == int((~nonzero).sum()) < 0.5 * len(pts)
    assert (np.einsum('ij,ij->i', want[nonzero].astype(np.float64), -pts[nonzero].astype(np.float64)) >= -1e-5).all()  # towards the origin
