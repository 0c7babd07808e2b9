"""-m gpu: mesh_fusion.mesh_maps and mesh_fusion.SceneMesh with carve_weight on the floater scene of tests/tsdf_carve_restated.py:
the report's new keys, the floater gone; without the option the report's keys and the mesh's bits are what they were."""
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
from atvsnet_amd import ops
from atvsnet_amd.atvsnet import depth_fusion as DF, eval_depth, mesh_fusion

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_carve_restated as CR  # noqa: E402
import tsdf_restated as R  # noqa: E402

pytestmark = pytest.mark.gpu

TODAY = {'origin', 'voxel', 'trunc', 'dims', 'min_weight', 'blocks', 'valid_voxels', 'vertices', 'faces', 'zero_area_faces',
         'boundary_edges', 'seconds'}
CARVE = {'carve_weight', 'free_voxels', 'max_free'}
MIN_WEIGHT = 2.0


def _radii(vertices):
    v = vertices.cpu().numpy() if isinstance(vertices, torch.Tensor) else vertices
    return np.linalg.norm(v.astype(np.float64), axis=1)


def _bounds(scene):
    return mesh_fusion.depth_bounds(scene.depths, scene.cams)


def test_mesh_maps_carves_the_floater_and_reports_it(cuda):
    scene = CR.floater()
    d, im = torch.from_numpy(scene.depths).to(cuda), torch.from_numpy(scene.images).to(cuda)
    lo, hi = _bounds(scene)
    plain_volume, plain, _ = mesh_fusion.mesh_maps(d, scene.cams, im, lo, hi, CR.VOXEL, min_weight=MIN_WEIGHT)
    volume, mesh, seconds = mesh_fusion.mesh_maps(d, scene.cams, im, lo, hi, CR.VOXEL, min_weight=MIN_WEIGHT, carve_weight=1.0)
    assert plain_volume.free is None and volume.free is not None and set(seconds) == {'integrate', 'extract'}
    assert _radii(plain[0]).max() > 1.1 and _radii(mesh[0]).max() <= 1.0
    # the dense restatement on the driver's own box
    want = CR.integrate(scene.depths, scene.cams, CR.VOXEL, volume.trunc, volume.origin, volume.dims, scene.images)
    assert np.array_equal(volume.blocks.cpu().numpy(), want['blocks'])
    f, w, _ = volume.to_dense()
    assert np.array_equal(f.view(np.uint32), want['tsdf'].view(np.uint32)) and np.array_equal(w, want['weight'])
    report = mesh_fusion.mesh_report(volume, mesh, MIN_WEIGHT, seconds, 1.0)
    assert set(report) == TODAY | CARVE
    assert report['carve_weight'] == 1.0 and report['max_free'] == float(want['free'].max()) >= 2
    assert report['free_voxels'] == int(((want['weight'] >= MIN_WEIGHT) & (want['free'] > 0)).sum()) > 0
    # without the option: today's keys, today's bits
    assert set(mesh_fusion.mesh_report(plain_volume, plain, MIN_WEIGHT, seconds)) == TODAY
    today = ops.tsdf_integrate(d, torch.from_numpy(scene.cams).to(cuda), CR.VOXEL, plain_volume.trunc, plain_volume.origin, plain_volume.dims,
                               images=im)
    for a, b in zip(plain, ops.tsdf_mesh(today, MIN_WEIGHT)):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    with pytest.raises(ValueError, match='carve_weight'):
        mesh_fusion.mesh_maps(d, scene.cams, im, lo, hi, CR.VOXEL, carve_weight=0.0)
    with pytest.raises(ValueError, match='no free counts'):
        mesh_fusion.mesh_report(plain_volume, plain, MIN_WEIGHT, seconds, 1.0)


def _cam44(cams16):
    cam44 = np.zeros((len(cams16), 2, 4, 4))
    for k, c in enumerate(cams16):
        cam44[k, 0] = np.eye(4)
        cam44[k, 0, :3, :3], cam44[k, 0, :3, 3] = c[:9].reshape(3, 3), c[9:12]
        cam44[k, 1, :3, :3] = [[c[12], 0, c[14]], [0, c[13], c[15]], [0, 0, 1]]
        cam44[k, 1, 3] = (1.0, 0.02, 128, 3.6)
    return cam44


def test_scene_mesh_carves_the_floater_and_is_as_it_was_without(cuda):
    scene = CR.floater()
    n, rows, cols = scene.depths.shape
    cams = _cam44(scene.cams)
    assert np.array_equal(eval_depth.camera_rows(cams), scene.cams)
    fusion = DF.SceneFusion(n, rows, cols, cuda, prob_threshold=0.5, disp_threshold=0.25, num_consistent=2, inverse_depth=False)
    for k in range(n):
        fusion.add(k, np.ascontiguousarray(scene.depths[k]), np.ones((rows, cols), np.float32),
                   np.clip(scene.images[k], 0, 255).astype(np.uint8), cams[k])
    plain = mesh_fusion.SceneMesh(fusion, cams, CR.VOXEL, min_weight=MIN_WEIGHT)
    carved = mesh_fusion.SceneMesh(fusion, cams, CR.VOXEL, min_weight=MIN_WEIGHT, carve_weight=0.5)
    pv, pc, pf = plain.run()
    cv, cc, cf = carved.run()
    assert _radii(pv).max() > 1.1 and _radii(cv).max() <= 1.0 and len(cf) < len(pf)
    assert set(plain.report()) == TODAY and set(carved.report()) == TODAY | CARVE
    report = carved.report()
    assert report['carve_weight'] == 0.5 and report['free_voxels'] > 0 and report['max_free'] >= 2
    assert report['blocks'] == plain.report()['blocks'] and report['valid_voxels'] == plain.report()['valid_voxels']
    assert plain.volume.free is None and torch.equal(plain.volume.weight, carved.volume.weight)
    # without carving: the bits of ops.tsdf_integrate and ops.tsdf_mesh on what the fusion holds
    order = fusion.order()
    idx = torch.from_numpy(order).to(cuda)
    today = ops.tsdf_integrate(fusion.nd[:n, :, :, 3].index_select(0, idx).contiguous(), torch.from_numpy(scene.cams[order]).to(cuda),
                               CR.VOXEL, plain.volume.trunc, plain.volume.origin, plain.volume.dims,
                               images=fusion.img[:n].index_select(0, idx).contiguous())
    tv, tc, tf = (t.cpu().numpy() for t in ops.tsdf_mesh(today, MIN_WEIGHT))
    assert np.array_equal(pv.view(np.uint32), tv.view(np.uint32)) and np.array_equal(pc, tc) and np.array_equal(pf, tf)
    # and the carved volume is the restatement's on the same planes
    nd, img = fusion.nd.cpu().numpy()[order], fusion.img.cpu().numpy()[order]
    want = CR.integrate(nd[..., 3], scene.cams[order], CR.VOXEL, carved.volume.trunc, carved.volume.origin, carved.volume.dims, img,
                        carve_weight=0.5)
    f, w, _ = carved.volume.to_dense()
    assert np.array_equal(f.view(np.uint32), want['tsdf'].view(np.uint32)) and np.array_equal(w, want['weight'])
    assert report['max_free'] == float(want['free'].max())
    assert R.edge_stats(cf)[1] and sorted(set(cf.reshape(-1).tolist())) == list(range(len(cv)))
