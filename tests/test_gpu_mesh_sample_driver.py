"""The surface sampling through the ETH3D driver: run_eval_pc's mesh=dict(voxel=, simplify=, score=dict(spacing=)) with gt_ply
writes mesh_eval.json and mesh_eval_simple.json beside a run that is otherwise unchanged, and SceneMesh.score gives what
eval_cloud.evaluate gives on the samples of the meshes it holds."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
from atvsnet_amd import FLAGS
from atvsnet_amd.atvsnet import eval_cloud, eval_pointcloud as E, sample_mesh
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_sample_restated as R  # noqa: E402
from test_gpu_depth_normals import _write_scene_dir  # noqa: E402

pytestmark = pytest.mark.gpu

CELL_VOXELS, VOXEL, SPACING = 3, 0.05, 0.02
GAP_BOUND = 0.02                          # the simplified mesh's completeness at the largest tolerance against the unsimplified one's


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


def _json(path):
    with open(path) as f:
        return json.load(f)


def _drive(argv, gt_ply=None, **mesh):
    """eval_pointcloud.cli's own steps with entries added to the mesh dict: the command line has no option for them."""
    parser = E.make_parser()
    args = parser.parse_args(argv)
    args.gt_ply = args.clean = None
    options = E._run_options(args, parser)
    options['mesh'] = dict(options['mesh'], **mesh)
    options['gt_ply'] = gt_ply
    E._check_options(**options)
    for k, v in vars(args).items():
        if k not in ('scenes', 'maps_in_flight'):
            setattr(FLAGS, k, v)
    E.main(args.scenes.split(','), options=options)


def test_driver_scores_each_mesh_by_its_surface_beside_an_unchanged_run(cuda, tmp_path, weights):
    root = str(tmp_path)
    _write_scene_dir(root)
    base = ['--data_root', root, '--view_num', '3', '--max_d', '16', '--max_w', '160', '--max_h', '128', '--synthetic_weights',
            '--scenes', 'toy', '--fuse', '--no_map_files', '--prob_threshold', '0.5', '--disp_threshold', '0.5', '--num_consistent', '1',
            '--mesh_voxel', repr(VOXEL), '--mesh_min_weight', '1']
    first, plain, scored = (os.path.join(root, name) for name in ('out_first', 'out_plain', 'out_scored'))
    simplify = dict(cell_voxels=CELL_VOXELS)
    try:
        FLAGS.reset()
        _drive(base + ['--savepath', first], simplify=simplify)           # its cloud is the ground truth of the two runs compared
        gt = os.path.join(first, 'toy', 'final3d_model.ply')
        FLAGS.reset()
        _drive(base + ['--savepath', plain], [gt], simplify=simplify)
        FLAGS.reset()
        _drive(base + ['--savepath', scored], [gt], simplify=simplify, score=dict(spacing=SPACING))
    finally:
        FLAGS.reset()
        E._Pipelines.CO_RESIDENT = False
    before = ['cloud_eval.json', 'depths_atvsnet', 'final3d_mesh.ply', 'final3d_mesh_simple.ply', 'final3d_model.ply', 'mesh.json',
              'mesh_simple.json', 'zz_runtime.txt']
    assert sorted(os.listdir(os.path.join(plain, 'toy'))) == before                  # the listing is as it was without score=
    assert sorted(os.listdir(os.path.join(scored, 'toy'))) == sorted(before + ['mesh_eval.json', 'mesh_eval_simple.json'])
    for name in ('final3d_mesh.ply', 'final3d_mesh_simple.ply', 'final3d_model.ply', 'cloud_eval.json'):
        assert _read(os.path.join(plain, 'toy', name)) == _read(os.path.join(scored, 'toy', name)), name
    for name in ('mesh.json', 'mesh_simple.json'):                     # they carry wall-clock seconds: every other byte is the same
        a, b = _json(os.path.join(plain, 'toy', name)), _json(os.path.join(scored, 'toy', name))
        assert set(a['seconds']) == set(b['seconds'])
        a['seconds'] = b['seconds'] = None
        assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True), name
    whole, simple = _json(os.path.join(scored, 'toy', 'mesh_eval.json')), _json(os.path.join(scored, 'toy', 'mesh_eval_simple.json'))
    gt_points = ply.read_ply_points(gt)
    torch.cuda.set_device(cuda)
    for result, name in ((whole, 'final3d_mesh.ply'), (simple, 'final3d_mesh_simple.ply')):
        report = result['recon_mesh']
        v, c, f = ply.read_mesh(os.path.join(scored, 'toy', name))
        assert set(report) == set(sample_mesh.REPORT_KEYS) - {'seconds'} and report['faces'] == len(f) and report['seed'] == 0
        assert result['n_recon'] == report['samples'] > 0 and result['n_gt'] == len(gt_points) and abs(report['spacing'] - SPACING) < 1e-15
        want = R.sample(v, None, f, 1.0 / (SPACING * SPACING), 0)
        unsure = int((want['counts']['margin'] < R.SURE).sum())
        assert unsure <= 0.01 * len(f) and abs(report['samples'] - want['counts']['info']['samples']) <= unsure
        if not unsure:                                                 # the file's score: the samples of the written mesh
            again = eval_cloud.evaluate(want['samples']['points'], gt_points)
            assert {k: v for k, v in result.items() if k != 'recon_mesh'} == json.loads(json.dumps(again))
    top = max(t['tolerance'] for t in whole['tolerances'])
    at = lambda r: [t for t in r['tolerances'] if t['tolerance'] == top][0]['completeness']      # noqa: E731
    print('completeness at %g: %.4f by %d samples of the mesh, %.4f by %d samples of the simplified mesh (gap %.4f); by their vertices '
          'the simplified mesh has %d' % (top, at(whole), whole['n_recon'], at(simple), simple['n_recon'], abs(at(whole) - at(simple)),
                                          simple['recon_mesh']['vertices']))
    assert abs(at(whole) - at(simple)) <= GAP_BOUND
    assert simple['recon_mesh']['vertices'] < whole['recon_mesh']['vertices'] // 4
