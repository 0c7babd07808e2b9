"""-m gpu: the mesh renderer in the tools -- eval_depth --occlusion_mesh / --gt_mesh, eval_pointcloud --score_maps
--map_occlusion_mesh and --mesh_voxel --mesh_render -- on the toy scene of tests/fusion_scene.py (5 images, maps of 48 x 64: a
tilted plane at depth ~ 5), against tests/scan_render_restated.py and tests/mesh_render_restated.py."""
import functools
import json
import os
import sys

import numpy as np
import pytest

import atvsnet_amd                                   # noqa: F401
from atvsnet_amd.atvsnet import eval_depth, mesh_fusion
from atvsnet_amd.atvsnet import eval_pointcloud as E
from atvsnet_amd.atvsnet import preprocess as P
from atvsnet_amd.flags import FLAGS
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fusion_scene  # noqa: E402
import mesh_render_restated as MR  # noqa: E402
import scan_render_restated as SR  # noqa: E402

pytestmark = pytest.mark.gpu

N_IMAGES, ROWS, COLS = 5, 48, 64
TOL = eval_depth.DEFAULT_OCCLUDER_TOL


@functools.lru_cache(maxsize=None)
def _scene():
    """-> (map cameras (n,2,4,4), exact depth maps, images, the scan: the plane's points as every view's depth map sees them)."""
    Ps, depths, _, images, _, _ = fusion_scene.make_scene(N_IMAGES, ROWS, COLS)
    K = np.array([[60.0, 0, COLS / 2.0], [0, 60.0, ROWS / 2.0], [0, 0, 1]])
    ys, xs = np.meshgrid(np.arange(ROWS, dtype=np.float64), np.arange(COLS, dtype=np.float64), indexing='ij')
    rays = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K).T
    cams, scan = np.zeros((N_IMAGES, 2, 4, 4)), []
    for v in range(N_IMAGES):
        Rt = np.linalg.inv(K) @ Ps[v]
        cams[v, 0] = np.eye(4)
        cams[v, 0, :3, :4] = Rt
        cams[v, 1, :3, :3] = K
        cams[v, 1, 3] = (4.0, 0.125, 16, 0.0)                        # the plane lies at depth ~ 5
        cam_pts = rays * depths[v].astype(np.float64)[..., None]
        scan.append((cam_pts.reshape(-1, 3) - Rt[:, 3]) @ Rt[:, :3])      # R^T (x - t)
    return cams, depths, images, np.concatenate(scan, 0).astype(np.float32)


def _write_scene_dir(root):
    """The scene as an ETH3D-style folder: images and cameras at four times the maps' size, a ring pair.txt, two sources each."""
    from PIL import Image
    cams, _, images, _ = _scene()
    scene = os.path.join(root, 'eth3d', 'toy')
    os.makedirs(os.path.join(scene, 'images'))
    os.makedirs(os.path.join(scene, 'cams'))
    for v in range(N_IMAGES):
        cam = cams[v].copy()
        cam[1, :2, :3] *= 4
        P.write_cam(os.path.join(scene, 'cams', '%08d_cam.txt' % v), cam)
        big = np.repeat(np.repeat(images[v], 4, axis=0), 4, axis=1)
        Image.fromarray(np.ascontiguousarray(big[:, :, ::-1])).save(os.path.join(scene, 'images', '%08d.jpg' % v), quality=95)
    with open(os.path.join(scene, 'pair.txt'), 'w') as f:
        f.write('%d\n' % N_IMAGES)
        for v in range(N_IMAGES):
            f.write('%d\n2 %d 1.0 %d 1.0\n' % (v, (v + 1) % N_IMAGES, (v + 2) % N_IMAGES))
    return scene


def _write_maps_dir(root):
    """The exact depth maps as a driver run would leave them: depths_atvsnet/%08d.pfm and %08d.txt."""
    cams, depths, _, _ = _scene()
    folder = os.path.join(root, 'maps', 'depths_atvsnet')
    os.makedirs(folder)
    for v in range(N_IMAGES):
        P.write_pfm(os.path.join(folder, '%08d.pfm' % v), depths[v])
        P.write_cam(os.path.join(folder, '%08d.txt' % v), cams[v])
    return os.path.dirname(folder)


@functools.lru_cache(maxsize=None)
def _quad(offset, half=False, pad=1.0):
    """A quad (two triangles) parallel to the scene's plane, `offset` along its normal towards the cameras (negative: behind it),
    over the whole scan padded by `pad`, or over the half of it with the larger first in-plane coordinate."""
    _, _, _, _, n, d0 = fusion_scene.make_scene(N_IMAGES, ROWS, COLS)
    scan = _scene()[3].astype(np.float64)
    e1 = np.cross(n, [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(n, e1)
    a, b = scan @ e1, scan @ e2
    a0 = 0.5 * (a.min() + a.max()) if half else a.min() - pad
    corners = [(a0, b.min() - pad), (a.max() + pad, b.min() - pad), (a.max() + pad, b.max() + pad), (a0, b.max() + pad)]
    v = np.array([x * e1 + y * e2 + (offset - d0) * n for x, y in corners])          # n . X + d0 = offset
    return v.astype(np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32)


@functools.lru_cache(maxsize=None)
def _restated(offset, tol=TOL, splat=eval_depth.DEFAULT_SPLAT, occlusion_tol=eval_depth.DEFAULT_OCCLUSION_TOL):
    """-> (the scan's maps, those maps occluded by the half wall at `offset`): scan render, mesh render, the occlude rule."""
    cams, _, _, scan = _scene()
    rows16 = eval_depth.camera_rows(cams)
    plain = SR.scan_render(scan, rows16, ROWS, COLS, 0.0, splat, occlusion_tol)
    wall, _ = MR.mesh_render(*_quad(offset, half=True), rows16, ROWS, COLS, 0.0)
    return plain, MR.depth_occlude(plain, wall, tol)


def _saved(folder):
    return np.stack([np.load(os.path.join(folder, '%08d_gt.npy' % v)) for v in range(N_IMAGES)])


def test_eval_depth_occlusion_mesh_zeroes_what_the_restatement_zeroes(cuda, tmp_path):
    root = str(tmp_path)
    maps = _write_maps_dir(root)
    scan_ply, wall_ply, back_ply = (os.path.join(root, n) for n in ('scan.ply', 'wall.ply', 'back.ply'))
    scan = _scene()[3]
    ply.write_ply(scan_ply, scan, np.zeros((len(scan), 3), np.uint8))
    ply.write_mesh(wall_ply, _quad(1.5, half=True)[0], None, _quad(1.5, half=True)[1])
    ply.write_mesh(back_ply, _quad(-1.5, half=True)[0], None, _quad(-1.5, half=True)[1])
    plain, occluded = _restated(1.5)
    gone = (plain > 0) & (occluded == 0)
    share = gone.reshape(N_IMAGES, -1).sum(1) / (plain > 0).reshape(N_IMAGES, -1).sum(1)
    assert ((share > 0.1) & (share < 0.9)).any(), share                 # the wall hides part of the scan, by the restatement alone
    base = ['--maps', maps, '--gt', scan_ply]
    without = eval_depth.cli(base + ['--out', os.path.join(root, 'a.json'), '--save_gt', os.path.join(root, 'gt_a')])
    assert np.array_equal(_saved(os.path.join(root, 'gt_a')), plain)    # byte-identical to the maps without the option
    assert not {'occlusion_mesh_tol', 'occlusion_faces', 'gt_mesh'} & set(without)
    with_wall = eval_depth.cli(base + ['--occlusion_mesh', wall_ply, '--out', os.path.join(root, 'b.json'),
                                       '--save_gt', os.path.join(root, 'gt_b')])
    got = _saved(os.path.join(root, 'gt_b'))
    assert np.array_equal(got, occluded) and np.array_equal((got == 0) & (plain > 0), gone)
    assert with_wall['occlusion_mesh_tol'] == TOL and with_wall['occlusion_faces'] == 2
    assert [m['gt_valid'] for m in with_wall['maps']] == [int((o > 0).sum()) for o in occluded]
    with open(os.path.join(root, 'b.json')) as f:
        assert json.load(f) == json.loads(json.dumps(with_wall))
    # a wall behind the plane changes nothing; both walls together hide what the front one hides
    behind = eval_depth.cli(base + ['--occlusion_mesh', back_ply, '--occlusion_mesh_tol', '0.02', '--save_gt', os.path.join(root, 'gt_c')])
    assert np.array_equal(_saved(os.path.join(root, 'gt_c')), plain) and behind['occlusion_mesh_tol'] == 0.02
    assert np.array_equal(_restated(-1.5, 0.02)[1], plain)
    both = eval_depth.cli(base + ['--occlusion_mesh', back_ply + ',' + wall_ply, '--save_gt', os.path.join(root, 'gt_d')])
    assert np.array_equal(_saved(os.path.join(root, 'gt_d')), occluded) and both['occlusion_faces'] == 4


def test_eval_depth_gt_mesh_scores_the_exact_maps(cuda, tmp_path, capsys):
    root = str(tmp_path)
    maps = _write_maps_dir(root)
    plane_ply, wall_ply = os.path.join(root, 'plane.ply'), os.path.join(root, 'wall.ply')
    ply.write_mesh(plane_ply, _quad(0.0)[0], None, _quad(0.0)[1])
    ply.write_mesh(wall_ply, _quad(1.5, half=True)[0], None, _quad(1.5, half=True)[1])
    result = eval_depth.cli(['--maps', maps, '--gt_mesh', plane_ply, '--save_gt', os.path.join(root, 'gt')])
    cams, depths, _, _ = _scene()
    want, _ = MR.mesh_render(*_quad(0.0), eval_depth.camera_rows(cams), ROWS, COLS, 0.0)
    assert np.array_equal(_saved(os.path.join(root, 'gt')), want) and (want > 0).all()
    assert result['gt_mesh'] == 2 and result['n_scored'] == N_IMAGES and 'occlusion_faces' not in result
    # the maps are the float32 roundings of the plane's depths and so is the rendering, of a plane whose corners were rounded to
    # float32 (coordinates below 8: within 2^-22 each): the spacing of float32 between 4 and 8, 2^-21, bounds the mean
    assert depths.max() < 8.0 and np.abs(_quad(0.0)[0]).max() < 8.0
    assert result['mean']['mae'] < 2.0 ** -21, result['mean']
    occluded = eval_depth.cli(['--maps', maps, '--gt_mesh', plane_ply, '--occlusion_mesh', wall_ply, '--save_gt', os.path.join(root, 'gt2')])
    wall, _ = MR.mesh_render(*_quad(1.5, half=True), eval_depth.camera_rows(cams), ROWS, COLS, 0.0)
    assert np.array_equal(_saved(os.path.join(root, 'gt2')), MR.depth_occlude(want, wall, TOL)) and occluded['occlusion_faces'] == 2
    capsys.readouterr()
    for argv, text in ((['--maps', maps, '--gt', plane_ply, '--gt_mesh', plane_ply], 'exactly one of --gt and --gt_mesh'),
                       (['--maps', maps], 'exactly one of --gt and --gt_mesh')):
        with pytest.raises(SystemExit) as e:
            eval_depth.cli(argv)
        assert e.value.code == 2 and text in ' '.join(capsys.readouterr().err.split())


@pytest.fixture(scope='module')
def driver_runs(cuda, tmp_path_factory, weights):
    """Two runs of the driver on the toy scene: scored and meshed; the same with an occlusion mesh and the mesh rendered."""
    root = str(tmp_path_factory.mktemp('mesh_render_driver'))
    _write_scene_dir(root)
    scan = _scene()[3]
    gt_ply, wall_ply = os.path.join(root, 'scan.ply'), os.path.join(root, 'wall.ply')
    ply.write_ply(gt_ply, scan, np.zeros((len(scan), 3), np.uint8))
    ply.write_mesh(wall_ply, _quad(1.5, half=True)[0], None, _quad(1.5, half=True)[1])
    base = ['--data_root', root, '--view_num', '3', '--max_d', '16', '--max_w', '160', '--max_h', '128', '--synthetic_weights',
            '--scenes', 'toy', '--scene_cache', '--fuse', '--prob_threshold', '0.1', '--disp_threshold', '0.5', '--num_consistent', '1',
            '--gt_ply', gt_ply, '--score_maps', '--map_splat', '1', '--map_occlusion_tol', '0.1', '--mesh_voxel', '0.05',
            '--mesh_min_weight', '1']
    out = {}
    try:
        for name, extra in (('plain', []), ('new', ['--map_occlusion_mesh', wall_ply, '--map_occlusion_mesh_tol', '0.02', '--mesh_render'])):
            FLAGS.reset()
            out[name] = os.path.join(root, 'out_' + name, 'toy')
            E.cli(base + ['--savepath', os.path.dirname(out[name])] + extra)
    finally:
        FLAGS.reset()
        E._Pipelines.CO_RESIDENT = False
    return out, gt_ply, wall_ply


def test_driver_scores_against_the_occluded_maps_and_leaves_the_rest(cuda, driver_runs):
    out, gt_ply, wall_ply = driver_runs
    for name in ('final3d_model.ply', 'cloud_eval.json', 'final3d_mesh.ply'):
        with open(os.path.join(out['plain'], name), 'rb') as f, open(os.path.join(out['new'], name), 'rb') as g:
            assert f.read() == g.read(), name
    with open(os.path.join(out['new'], 'depth_eval.json')) as f:
        got = json.load(f)
    with open(os.path.join(out['plain'], 'depth_eval.json')) as f:
        plain = json.load(f)
    assert 'occlusion_faces' not in plain and got['occlusion_faces'] == 2 and got['occlusion_mesh_tol'] == 0.02
    indices, depth, cams = eval_depth.load_maps(out['new'])
    assert indices == list(range(N_IMAGES))
    pred = depth.copy()
    for k, i in enumerate(indices):
        with open(os.path.join(out['new'], 'depths_atvsnet', '%08d_prob.pfm' % i), 'rb') as f:
            pred[k][P.load_pfm(f) < np.float32(0.1)] = 0
    occluder = eval_depth.load_meshes([wall_ply])
    gt = eval_depth.render_scan(ply.read_ply_points(gt_ply), cams, pred.shape[1], pred.shape[2], pixel_centre=0.0, splat=1,
                                occlusion_tol=0.1, device=cuda, occluders=[occluder], occluder_tol=0.02).cpu().numpy()
    want = eval_depth.report(pred, gt, indices=indices, pixel_centre=0.0, splat=1, occlusion_tol=0.1, occlusion_mesh_tol=0.02,
                             occlusion_faces=2)
    assert json.loads(json.dumps(want)) == got
    rows16 = eval_depth.camera_rows(cams)
    scan_maps = SR.scan_render(ply.read_ply_points(gt_ply), rows16, pred.shape[1], pred.shape[2], 0.0, 1, 0.1)
    wall, _ = MR.mesh_render(*occluder, rows16, pred.shape[1], pred.shape[2], 0.0)
    assert np.array_equal(gt, MR.depth_occlude(scan_maps, wall, 0.02))
    assert sum(m['gt_valid'] for m in got['maps']) < 0.9 * sum(m['gt_valid'] for m in plain['maps'])


def test_driver_renders_the_mesh_it_wrote(cuda, driver_runs):
    out, _, _ = driver_runs
    assert not os.path.exists(os.path.join(out['plain'], 'depths_mesh'))
    with open(os.path.join(out['plain'], 'mesh.json')) as f:
        assert 'render' not in json.load(f)
    with open(os.path.join(out['new'], 'mesh.json')) as f:
        report = json.load(f)
    assert sorted(os.listdir(os.path.join(out['new'], 'depths_mesh'))) == ['%08d_mesh.pfm' % i for i in range(N_IMAGES)]
    vertices, _, faces = ply.read_mesh(os.path.join(out['new'], 'final3d_mesh.ply'))
    indices, depth, cams = eval_depth.load_maps(out['new'])              # the driver's maps: a quarter of its 160 x 128 images
    want, _ = eval_depth.render_mesh(vertices, faces, cams, depth.shape[1], depth.shape[2], pixel_centre=mesh_fusion.DEFAULT_PIXEL_CENTRE, device=cuda)
    want = want.cpu().numpy()
    for k, i in enumerate(indices):
        with open(os.path.join(out['new'], 'depths_mesh', '%08d_mesh.pfm' % i), 'rb') as f:
            assert np.array_equal(P.load_pfm(f), want[k]), i
    assert report['render']['maps'] == N_IMAGES and report['render']['covered_fraction'] == float((want > 0).mean()) > 0.2
    assert report['render']['seconds'] > 0
