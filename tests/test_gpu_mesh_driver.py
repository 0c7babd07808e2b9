"""-m gpu: mesh_fusion.SceneMesh on the toy scene of tests/fusion_scene.py against tests/tsdf_restated.py, and
eval_pointcloud --fuse --mesh_voxel on the toy scene of tests/test_gpu_depth_normals.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
from atvsnet_amd import FLAGS, ops
from atvsnet_amd.atvsnet import depth_fusion as DF, eval_depth, eval_pointcloud as E, mesh_fusion
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_restated as R  # noqa: E402
from fusion_scene import make_scene  # noqa: E402
from test_gpu_depth_normals import _write_scene_dir  # noqa: E402

pytestmark = pytest.mark.gpu

VOXEL, TRUNC_VOXELS, MIN_WEIGHT = 0.1, 4.0, 2.0


def _cameras(Ps, rows, cols):
    """make_scene's projection matrices K [R | t] as the (2,4,4) cameras the driver writes."""
    K = np.array([[60.0, 0, cols / 2.0], [0, 60.0, rows / 2.0], [0, 0, 1]])
    cams = np.zeros((len(Ps), 2, 4, 4))
    for k, P in enumerate(Ps):
        cams[k, 0] = np.eye(4)
        cams[k, 0, :3, :] = np.linalg.inv(K) @ P
        cams[k, 1, :3, :3] = K
        cams[k, 1, 3] = (2.0, 0.05, 16, 2.8)
    return cams


def test_scene_mesh_is_the_restatement_on_the_staged_planes(cuda, tmp_path):
    Ps, depths, _, images = make_scene()[:4]
    n, rows, cols = depths.shape
    depths = depths.copy()
    depths[1, 10:20, 30:40] = 0                          # a hole in one view: weights differ across the surface
    cams = _cameras(Ps, rows, cols)
    fusion = DF.SceneFusion(n, rows, cols, cuda, prob_threshold=0.5, disp_threshold=0.01, num_consistent=2, inverse_depth=False)
    out_index = [30, 10, 20, 0]                          # fusion order differs from the order of add()
    for k in range(n):
        fusion.add(out_index[k], np.ascontiguousarray(depths[k]), np.ones((rows, cols), np.float32), images[k], cams[k])
    scene_mesh = mesh_fusion.SceneMesh(fusion, {out_index[k]: cams[k] for k in range(n)}, VOXEL, TRUNC_VOXELS, MIN_WEIGHT)
    got = scene_mesh.run()
    # the restatement, from what the fusion holds
    points, _ = fusion.run()
    finite = points[np.isfinite(points).all(axis=1)]
    lo, hi = finite.min(axis=0).astype(np.float64), finite.max(axis=0).astype(np.float64)
    origin, dims = mesh_fusion.box_of(lo, hi, VOXEL, TRUNC_VOXELS * VOXEL)
    assert (origin + 8 * VOXEL + TRUNC_VOXELS * VOXEL <= lo + 1e-9).all() and (origin + np.array(dims) * 8 * VOXEL >= hi + TRUNC_VOXELS * VOXEL).all()
    order = fusion.order()
    assert order.tolist() == [3, 1, 2, 0]
    nd, img = fusion.nd.cpu().numpy()[order], fusion.img.cpu().numpy()[order]
    assert np.array_equal(nd[..., 3], depths[order])
    want_volume = R.integrate(nd[..., 3], eval_depth.camera_rows(cams[order]), VOXEL, TRUNC_VOXELS * VOXEL, origin, dims, img)
    volume = scene_mesh.volume
    assert volume.dims == dims and np.array_equal(volume.origin, origin)
    assert np.array_equal(volume.blocks.cpu().numpy(), want_volume['blocks']) and len(want_volume['blocks']) > 4
    f, w, c = volume.to_dense()
    assert np.array_equal(f.view(np.uint32), want_volume['tsdf'].view(np.uint32)) and np.array_equal(w, want_volume['weight'])
    assert np.array_equal(c.view(np.uint32), want_volume['color'].view(np.uint32)) and w.max() == n
    want = R.mesh(want_volume['tsdf'], want_volume['weight'], want_volume['color'], origin, VOXEL, MIN_WEIGHT)
    assert len(want[2]) > 1000
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    # the surface is the plane n . X + d0 = 0 of the scene.  A view's sdf is linear across the plane but for the depth being that of
    # the nearest pixel, off by at most half the step between neighbouring pixels (0.0192 / 2 + 0.0054 / 2 = 0.0123); a mean of such
    # fields, interpolated linearly, crosses zero within that of the plane: one full step, 0.02, is the cap
    normal, d0 = make_scene()[4:]
    assert np.abs(got[0].astype(np.float64) @ normal + d0).max() < 0.02
    # the report and the file
    report = scene_mesh.report()
    _, undirected = R.edge_stats(got[2])
    assert report['vertices'] == len(got[0]) and report['faces'] == len(got[2]) and report['blocks'] == len(want_volume['blocks'])
    assert report['valid_voxels'] == int((want_volume['weight'] >= MIN_WEIGHT).sum())
    assert report['boundary_edges'] == sum(1 for k in undirected.values() if k == 1) > 0 and max(undirected.values()) == 2
    assert set(report['seconds']) == {'bounds', 'integrate', 'extract', 'download', 'report'}
    path = str(tmp_path / 'mesh.ply')
    assert scene_mesh.write_ply(path) == len(got[2])
    back = ply.read_mesh(path)
    assert all(np.array_equal(a, b) for a, b in zip(back, got))


def test_driver_writes_the_mesh_and_leaves_the_cloud_as_it_was(cuda, tmp_path, weights):
    root = str(tmp_path)
    _write_scene_dir(root)
    base = ['--data_root', root, '--view_num', '3', '--max_d', '16', '--max_w', '160', '--max_h', '128', '--synthetic_weights',
            '--scenes', 'toy', '--fuse', '--no_map_files', '--prob_threshold', '0.5', '--disp_threshold', '0.5', '--num_consistent', '1']
    plain, meshed = os.path.join(root, 'out_plain'), os.path.join(root, 'out_mesh')
    try:
        FLAGS.reset()
        E.cli(base + ['--savepath', plain])
        FLAGS.reset()
        E.cli(base + ['--savepath', meshed, '--mesh_voxel', '0.05', '--mesh_min_weight', '1'])
    finally:
        FLAGS.reset()
        E._Pipelines.CO_RESIDENT = False
    assert sorted(os.listdir(os.path.join(plain, 'toy'))) == ['depths_atvsnet', 'final3d_model.ply', 'zz_runtime.txt']
    assert sorted(os.listdir(os.path.join(meshed, 'toy'))) == ['depths_atvsnet', 'final3d_mesh.ply', 'final3d_model.ply', 'mesh.json',
                                                               'zz_runtime.txt']
    with open(os.path.join(plain, 'toy', 'final3d_model.ply'), 'rb') as f, open(os.path.join(meshed, 'toy', 'final3d_model.ply'), 'rb') as g:
        assert f.read() == g.read()
    vertices, colors, faces = ply.read_mesh(os.path.join(meshed, 'toy', 'final3d_mesh.ply'))
    with open(os.path.join(meshed, 'toy', 'mesh.json')) as f:
        report = json.load(f)
    print({k: v for k, v in report.items() if k != 'seconds'})
    assert report['vertices'] == len(vertices) > 0 and report['faces'] == len(faces) > 0 and report['blocks'] > 0
    assert report['voxel'] == 0.05 and report['trunc'] == 0.05 * 4 and report['min_weight'] == 1.0
    assert sorted(set(faces.reshape(-1).tolist())) == list(range(len(vertices)))
    _, undirected = R.edge_stats(faces)
    assert max(undirected.values()) <= 2
    # inside the volume's box, which the fused cloud bounds
    cloud = ply.read_ply_points(os.path.join(meshed, 'toy', 'final3d_model.ply'))
    pad = report['trunc'] + 8 * report['voxel']
    assert (vertices >= cloud.min(axis=0) - pad).all() and (vertices <= cloud.max(axis=0) + pad + 8 * report['voxel']).all()
    assert np.array_equal(ply.read_ply_points(os.path.join(meshed, 'toy', 'final3d_mesh.ply')), vertices)


def test_the_tool_meshes_written_maps(cuda, tmp_path):
    """mesh_fusion's command line on the files a driver run leaves -- %08d.pfm, _prob.pfm, .jpg, .txt -- against ops.tsdf_integrate and
    ops.tsdf_mesh on what those files hold: the probability filter, the box from the maps' own depths, the mesh file, the report."""
    from PIL import Image
    from atvsnet_amd.atvsnet.preprocess import write_cam, write_pfm
    Ps, depths, _, images = make_scene()[:4]
    n, rows, cols = depths.shape
    cams = _cameras(Ps, rows, cols)
    folder = tmp_path / 'toy' / 'depths_atvsnet'
    folder.mkdir(parents=True)
    prob = np.ones((n, rows, cols), np.float32)
    prob[2, :, :20] = 0.3                                # filtered at the default threshold of 0.8
    for k in range(n):
        stem = str(folder / ('%08d' % (k * 10)))
        write_pfm(stem + '.pfm', depths[k])
        write_pfm(stem + '_prob.pfm', prob[k])
        write_cam(stem + '.txt', cams[k])
        Image.fromarray(np.ascontiguousarray(images[k][:, :, ::-1])).save(stem + '.jpg')
    out, report_path = str(tmp_path / 'mesh.ply'), str(tmp_path / 'mesh.json')
    result = mesh_fusion.cli(['--maps', str(tmp_path / 'toy'), '--voxel', str(VOXEL), '--min_weight', '2', '--out', out, '--report', report_path])
    # the same, by hand
    indices, loaded, loaded_cams = eval_depth.load_maps(str(tmp_path / 'toy'))
    assert indices == [0, 10, 20, 30] and np.array_equal(loaded, depths)
    filtered = loaded.copy()
    filtered[prob < 0.8] = 0
    assert (filtered[2, :, :20] == 0).all() and (filtered[2, :, 20:] > 0).all()
    bgr = np.stack([np.asarray(Image.open(str(folder / ('%08d.jpg' % i))).convert('RGB'))[:, :, ::-1].astype(np.float32) for i in indices])
    cams16 = eval_depth.camera_rows(loaded_cams)
    lo, hi = mesh_fusion.depth_bounds(filtered, cams16)
    origin, dims = mesh_fusion.box_of(lo, hi, VOXEL, 4 * VOXEL)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in (filtered, cams16, bgr)]
    volume = ops.tsdf_integrate(dev[0], dev[1], VOXEL, 4 * VOXEL, origin, dims, images=dev[2])
    want = [t.cpu().numpy() for t in ops.tsdf_mesh(volume, 2.0)]
    got = ply.read_mesh(out)
    assert len(want[2]) > 1000 and all(np.array_equal(a, b) for a, b in zip(got, want))
    with open(report_path) as f:
        assert json.load(f) == json.loads(json.dumps(result))
    assert result['faces'] == len(want[2]) and result['blocks'] == volume.num_blocks and result['maps'] == indices
    assert result['colored'] and result['probability_filtered'] and result['dims'] == list(dims)
    # bounded by a cloud instead: the mesh's own vertices stand in for one
    bounded = mesh_fusion.cli(['--maps', str(tmp_path / 'toy'), '--voxel', str(VOXEL), '--bounds', out, '--out', str(tmp_path / 'again.ply')])
    o, d = mesh_fusion.box_of(got[0].min(axis=0), got[0].max(axis=0), VOXEL, 4 * VOXEL)
    assert bounded['origin'] == o.tolist() != result['origin'] and bounded['dims'] == list(d) and bounded['faces'] > 1000
