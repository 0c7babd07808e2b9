"""-m gpu: a scan rendered into cameras (csrc/scan_render.hip, ops.scan_render, atvsnet/eval_depth.py, eval_pointcloud
--score_maps).

Every comparison of depth maps with the restatement (tests/scan_render_restated.py) is exact: np.array_equal."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd                                   # noqa: F401
from atvsnet_amd import ops
from atvsnet_amd.atvsnet import eval_depth
from atvsnet_amd.atvsnet import eval_pointcloud as E
from atvsnet_amd.atvsnet import preprocess as P
from atvsnet_amd.flags import FLAGS
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_register_restated as RR  # noqa: E402
import fusion_scene  # noqa: E402
import scan_render_restated as SR  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS, COLS = 37, 53                                  # odd, no multiple of anything
TILE = 256                                           # points per workgroup (csrc/scan_render.hip kThreads)


def _gpu(dev, pts, cams, rows, cols, centre=0.0, splat=0, tol=0.0):
    p = torch.from_numpy(np.array(pts, np.float32).reshape(-1, 3)).to(dev)              # a copy: the shared inputs are read-only
    c = torch.from_numpy(np.array(cams, np.float64).reshape(-1, 16)).to(dev)
    out = ops.scan_render(p, c, rows, cols, pixel_centre=centre, splat=splat, occlusion_tol=tol)
    assert out.dtype == torch.float32 and tuple(out.shape) == (len(c), rows, cols) and out.device == p.device
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _random_cloud():
    """200 000 points in a box around 9 cameras on a ring (one camera group of 8 and a remainder of 1): points in front of,
    behind and beside every camera, some very close to one."""
    rng = np.random.default_rng(11)
    cams = SR.ring_cameras(9, ROWS, COLS, radius=3.0)
    pts = rng.uniform(-4.0, 4.0, (200000, 3)).astype(np.float32)
    pts.setflags(write=False)
    cams.setflags(write=False)
    return pts, cams


@functools.lru_cache(maxsize=None)
def _random_want(n_cams, centre, splat, tol):
    pts, cams = _random_cloud()
    want = SR.scan_render(pts, cams[:n_cams], ROWS, COLS, centre, splat, tol)
    want.setflags(write=False)
    return want


@pytest.mark.parametrize('centre', [0.0, 0.5])
@pytest.mark.parametrize('splat,tol', [(0, 0.0), (1, 0.05), (4, 0.05)])
def test_random_cloud_is_the_restatement(cuda, splat, tol, centre):
    pts, cams = _random_cloud()
    want = _random_want(9, centre, splat, tol)
    got = _gpu(cuda, pts, cams, ROWS, COLS, centre, splat, tol)
    assert np.array_equal(got, want)
    covered = (want > 0).mean(axis=(1, 2))
    if splat == 0:
        assert (covered > 0.9).all()                             # every camera sees the cloud all over its image
    else:                                                        # a volume, not a surface: the occlusion test removes much, not all
        assert (covered > 0).all() and (covered < (_random_want(9, centre, 0, 0.0) > 0).mean(axis=(1, 2))).all()
    again = _gpu(cuda, pts, cams, ROWS, COLS, centre, splat, tol)
    assert np.array_equal(again, got)                            # the same bits on every run


@pytest.mark.parametrize('splat,tol', [(0, 0.0), (2, 0.05)])
def test_one_camera_and_few_points(cuda, splat, tol):
    pts, cams = _random_cloud()
    assert np.array_equal(_gpu(cuda, pts, cams[4:5], ROWS, COLS, 0.0, splat, tol), SR.scan_render(pts, cams[4:5], ROWS, COLS, 0.0, splat, tol))
    # a point every camera sees, first: n = 1 renders it
    few = np.concatenate([np.array([[0.05, -0.02, 0.01]], np.float32), pts[:TILE]], 0)
    for n_cams in (1, 9):
        for n in (0, 1, TILE + 1):
            got = _gpu(cuda, few[:n], cams[:n_cams], ROWS, COLS, 0.0, splat, tol)
            assert np.array_equal(got, SR.scan_render(few[:n], cams[:n_cams], ROWS, COLS, 0.0, splat, tol)), (n_cams, n)
            if n == 0:
                assert not got.any()
            else:
                assert ((got > 0).reshape(n_cams, -1).sum(axis=1) >= 1).all()


IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 4, 4, 0, 0], np.float64)        # fx = fy = 4, cx = cy = 0


def _at(xs, ys, z=2.0, fx=4.0):
    """A point that the IDENTITY camera projects to exactly (xs, ys) at pixel_centre 0 (all values exact in float32)."""
    return [(xs - 0.5) * z / fx, (ys - 0.5) * z / fx, z]


@pytest.mark.parametrize('splat', [0, 2])
def test_borders(cuda, splat):
    rows, cols = 5, 7
    inf, nan = np.inf, np.nan
    pts = np.array([_at(0.0, 0.0), _at(float(cols), 1.5), _at(1.5, float(rows)),             # exactly 0: in; exactly cols / rows: out
                    _at(-float(splat), 2.5, 3.0), _at(2.5, -float(splat), 3.0),              # exactly -splat: in the window
                    _at(-float(splat) - 0.5, 3.5), _at(cols + splat - 0.5, 3.5, 2.5),        # just outside / inside the window
                    _at(cols + float(splat), 4.5, 2.5),
                    [0.5, 0.5, 0.0], [0.5, 0.5, -0.0], [0.5, 0.5, -2.0],                     # c_2 = 0 and < 0
                    [nan, 0.5, 2.0], [0.5, nan, 2.0], [0.5, 0.5, nan], [inf, 0.5, 2.0], [-inf, 0.5, 2.0], [0.5, inf, 2.0],
                    [0.5, 0.5, inf], [0.5, 0.5, -inf], [inf, inf, inf],
                    [1e30, 0.5, 2.0], [0.5, -1e30, 2.0], [3e38, 3e38, 1e-30], [-3e38, 1.0, 1e-38],   # 1e30 pixels away and more
                    [0.5, 0.5, 1e-45], [0.5, 0.5, 3e38],                                     # the smallest and a huge float32 depth
                    _at(3.5, 2.5, 6.0)], np.float32)
    cams = np.stack([IDENTITY, IDENTITY])
    cams[1, 11] = 1e39                                           # camera 1: every c_2 beyond float32 -> nothing takes part
    want = SR.scan_render(pts, cams, rows, cols, 0.0, splat, 0.05)
    got = _gpu(cuda, pts, cams, rows, cols, 0.0, splat, 0.05)
    assert np.array_equal(got, want)
    assert not got[1].any()
    assert got[0, 0, 0] == 2.0 and got[0, 2, 3] == 6.0
    assert got[0, 1, cols - 1] == 0.0 and got[0, rows - 1, 1] == 0.0
    if splat == 0:
        assert got[0, 2, 0] == 3.0 and got[0, 0, 2] == 3.0           # xs = -0 = 0: inside
        assert got[0, 3, cols - 1] == 2.5                            # xs = cols - 0.5
    else:
        assert got[0, 2, 0] == 0.0 and got[0, 3, cols - 1] == 0.0    # those landed outside the image: the front plane only


def test_one_pixel_takes_the_nearest_of_many(cuda):
    # 5 000 points on the optical axis of a camera whose principal point lies inside pixel (10, 6): ever nearer, ever farther, ties
    cam = IDENTITY.copy()
    cam[14], cam[15] = 10.25, 6.25
    rng = np.random.default_rng(5)
    z = np.concatenate([np.linspace(9.0, 2.0, 2000), np.linspace(2.0, 9.0, 2000), np.full(500, 2.0), rng.uniform(2.0, 9.0, 500)])
    z = z.astype(np.float32)
    pts = np.stack([np.zeros_like(z), np.zeros_like(z), z], 1)
    for splat, tol in ((0, 0.0), (3, 0.0)):
        got = _gpu(cuda, pts, cam[None], 13, 17, 0.0, splat, tol)
        want = np.zeros((1, 13, 17), np.float32)
        want[0, 6, 10] = z.min()
        assert z.min() == np.float32(2.0) and np.array_equal(got, want)
        assert np.array_equal(got, SR.scan_render(pts, cam[None], 13, 17, 0.0, splat, tol))
    # nearer by one ulp wins
    pts[1234, 2] = np.nextafter(np.float32(2.0), np.float32(0))
    assert _gpu(cuda, pts, cam[None], 13, 17)[0, 6, 10] == pts[1234, 2]


# identity rotation, t = (0.5, -0.25, 0.5), fx = fy = 32, cx = 16, cy = 12: every number below is exact in float32 and float64
LATTICE_CAM = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5, -0.25, 0.5, 32, 32, 16, 12], np.float64)


def _lattice(depth, k_x, k_y):
    """World points at camera depth `depth` whose image coordinates are x = k / 2 + 0.25 for k in k_x (y: k_y): two per pixel and
    axis, a quarter of a pixel from every pixel border.  c_0 = (x - 16) depth / 32 is a small multiple of 2^-9: exact, so
    (c_0 / depth) * 32 + 16 is x to within an ulp and floor(x + 0.5) is the pixel it was built for."""
    x = np.asarray(list(k_x), np.float64) / 2 + 0.25
    y = np.asarray(list(k_y), np.float64) / 2 + 0.25
    X = (x - 16.0) * depth / 32.0 - 0.5
    Y = (y - 12.0) * depth / 32.0 + 0.25
    gx, gy = np.meshgrid(X, Y)
    pts = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, depth - 0.5)], 1)
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)
    return pts.astype(np.float32)


def test_known_answer_fronto_parallel_lattice(cuda):
    rows, cols = 24, 32
    # x from 5.25 to 30.25 -> xs = x + 0.5 in [5.75, 30.75] -> u = 5..30; y from 3.25 to 17.75 -> v = 3..18
    pts = _lattice(2.5, range(10, 61), range(6, 36))
    want = np.zeros((rows, cols), np.float32)
    want[3:19, 5:31] = np.float32(2.5)
    for splat, tol in ((0, 0.0), (1, 0.0), (4, 0.0)):               # one depth: the occlusion test removes nothing
        assert np.array_equal(_gpu(cuda, pts, LATTICE_CAM[None], rows, cols, 0.0, splat, tol)[0], want), splat
    # one point at x = 5.75, y = 3.75: pixel (6, 4) where integer coordinates are pixel centres, (5, 3) where they are corners
    one = _lattice(2.5, [11], [7])
    assert np.argwhere(_gpu(cuda, one, LATTICE_CAM[None], rows, cols, 0.0)[0]).tolist() == [[4, 6]]
    assert np.argwhere(_gpu(cuda, one, LATTICE_CAM[None], rows, cols, 0.5)[0]).tolist() == [[3, 5]]


def test_occlusion(cuda):
    rows, cols = 24, 32
    back = _lattice(4.0, range(0, 64), range(0, 48))                # dense: two points per pixel and axis, the whole image
    # sparse: one point every third pixel (k = 2 u: x = u + 0.25, inside pixel u), u = 7, 10, .., 22 and v = 5, 8, .., 17
    us, vs = list(range(7, 23, 3)), list(range(5, 18, 3))
    fore = _lattice(2.0, [2 * u for u in us], [2 * v for v in vs])
    pts = np.concatenate([back, fore], 0)
    fg = np.zeros((rows, cols), bool)
    fg[np.ix_(vs, us)] = True
    foot = np.zeros((rows, cols), bool)                             # the foreground's footprint at splat 2
    foot[vs[0] - 2:vs[-1] + 3, us[0] - 2:us[-1] + 3] = True
    # z / zf is 1 or 2 everywhere: nowhere near 1 + tol
    through = SR.scan_render(pts, LATTICE_CAM[None], rows, cols, 0.0, 0, 0.0)[0]
    closed = SR.scan_render(pts, LATTICE_CAM[None], rows, cols, 0.0, 2, 0.05)[0]
    assert (through[fg] == 2.0).all() and (through[~fg] == 4.0).all()              # the background shows through the gaps
    assert (closed[fg] == 2.0).all() and (closed[foot & ~fg] == 0.0).all() and (closed[~foot] == 4.0).all()
    assert np.array_equal(_gpu(cuda, pts, LATTICE_CAM[None], rows, cols, 0.0, 0, 0.0)[0], through)
    assert np.array_equal(_gpu(cuda, pts, LATTICE_CAM[None], rows, cols, 0.0, 2, 0.05)[0], closed)


def _driver_cameras(rows16, depth_range=(1.0, 0.1, 16, 0.0)):
    cams = np.zeros((len(rows16), 2, 4, 4))
    cams[:, 0] = np.eye(4)
    cams[:, 0, :3, :3] = rows16[:, :9].reshape(-1, 3, 3)
    cams[:, 0, :3, 3] = rows16[:, 9:12]
    cams[:, 1, 0, 0], cams[:, 1, 1, 1], cams[:, 1, 0, 2], cams[:, 1, 1, 2] = rows16[:, 12], rows16[:, 13], rows16[:, 14], rows16[:, 15]
    cams[:, 1, 2, 2] = 1.0
    cams[:, 1, 3] = depth_range
    return cams


def test_transform_moves_the_scan_by_the_inverse(cuda):
    rng = np.random.default_rng(2)
    rows16 = SR.ring_cameras(3, ROWS, COLS, radius=3.0)
    cams = _driver_cameras(rows16)
    assert np.array_equal(eval_depth.camera_rows(cams), rows16)
    recon = rng.uniform(-1.0, 1.0, (20000, 3)).astype(np.float32)
    a = np.deg2rad(30.0)
    T = np.eye(4)
    T[:3, :3] = 2.5 * np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    T[:3, 3] = (4.0, -7.0, 1.5)
    scan = RR.transform(recon, T)                                    # the scan's frame: recon -> scan is T
    back = RR.transform(scan, eval_depth.inverse_similarity(T))      # ops.cloud_transform's stated rounding
    assert np.abs(back - recon).max() < 1e-5 and not np.array_equal(back, recon)
    got = eval_depth.render_scan(scan, cams, ROWS, COLS, transform=T, pixel_centre=0.0, splat=1, occlusion_tol=0.05, device=cuda)
    assert np.array_equal(got.cpu().numpy(), SR.scan_render(back, rows16, ROWS, COLS, 0.0, 1, 0.05))
    same = eval_depth.render_scan(torch.from_numpy(back).to(cuda), rows16, ROWS, COLS, pixel_centre=0.0, splat=1, occlusion_tol=0.05)
    assert torch.equal(same, got)
    # the defaults are eval_depth's, and rendering in the scan's frame without the matrix sees something else
    assert np.array_equal(eval_depth.render_scan(back, cams, ROWS, COLS, device=cuda).cpu().numpy(),
                          SR.scan_render(back, rows16, ROWS, COLS, eval_depth.DEFAULT_PIXEL_CENTRE, eval_depth.DEFAULT_SPLAT,
                                         eval_depth.DEFAULT_OCCLUSION_TOL))
    assert not np.array_equal(eval_depth.render_scan(scan, cams, ROWS, COLS, splat=1, device=cuda).cpu().numpy(), got.cpu().numpy())


def test_ops_scan_render_checks_the_cameras(cuda):
    p = torch.zeros(5, 3, device=cuda)
    c = torch.zeros(2, 16, dtype=torch.float64, device=cuda)
    with pytest.raises(TypeError, match='cams'):
        ops.scan_render(p, c.float(), 4, 4)
    with pytest.raises(ValueError, match='cams'):
        ops.scan_render(p, torch.zeros(2, 18, dtype=torch.float64, device=cuda), 4, 4)
    with pytest.raises(ValueError, match='cameras'):
        ops.scan_render(p, c[:0], 4, 4)
    with pytest.raises(RuntimeError, match='cams'):
        ops.scan_render(p, c.cpu(), 4, 4)
    with pytest.raises(ValueError, match='2\\^31'):
        ops.scan_render(p, c, 1 << 15, 1 << 15)
    assert not ops.scan_render(p, c, 4, 4).any()                     # c_2 = 0 everywhere: all-zero maps


# ------------------------------------------------------------------------------------------------------------------- driver

_N_IMAGES, _ROWS, _COLS = 5, 48, 64


def _write_scene_dir(root):
    """tests/fusion_scene.py's tilted plane as an ETH3D-style scene (images and cameras at four times the maps' size, ring
    pair.txt with two sources each) -> (scene folder, the scan: the plane's points as every view's exact depth map sees them)."""
    from PIL import Image
    Ps, depths, _, images, _, _ = fusion_scene.make_scene(_N_IMAGES, _ROWS, _COLS)
    scene = os.path.join(root, 'eth3d', 'toy')
    os.makedirs(os.path.join(scene, 'images'))
    os.makedirs(os.path.join(scene, 'cams'))
    K = np.array([[60.0, 0, _COLS / 2.0], [0, 60.0, _ROWS / 2.0], [0, 0, 1]])
    ys, xs = np.meshgrid(np.arange(_ROWS, dtype=np.float64), np.arange(_COLS, dtype=np.float64), indexing='ij')
    rays = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K).T
    scan = []
    for v in range(_N_IMAGES):
        Rt = np.linalg.inv(K) @ Ps[v]
        cam = np.zeros((2, 4, 4))
        cam[0] = np.eye(4)
        cam[0, :3, :4] = Rt
        cam[1, :3, :3] = K
        cam[1, :2, :3] *= 4
        cam[1, 3] = (4.0, 0.125, 16, 0.0)                            # the plane lies at depth ~ 5
        P.write_cam(os.path.join(scene, 'cams', '%08d_cam.txt' % v), cam)
        big = np.repeat(np.repeat(images[v], 4, axis=0), 4, axis=1)
        Image.fromarray(np.ascontiguousarray(big[:, :, ::-1])).save(os.path.join(scene, 'images', '%08d.jpg' % v), quality=95)
        cam_pts = rays * depths[v].astype(np.float64)[..., None]
        scan.append((cam_pts.reshape(-1, 3) - Rt[:, 3]) @ Rt[:, :3])          # R^T (x - t)
    with open(os.path.join(scene, 'pair.txt'), 'w') as f:
        f.write('%d\n' % _N_IMAGES)
        for v in range(_N_IMAGES):
            f.write('%d\n2 %d 1.0 %d 1.0\n' % (v, (v + 1) % _N_IMAGES, (v + 2) % _N_IMAGES))
    return scene, np.concatenate(scan, 0).astype(np.float32)


def test_driver_scores_the_maps_that_entered_the_cloud(cuda, tmp_path, weights):
    root = str(tmp_path)
    _, scan = _write_scene_dir(root)
    gt_ply = os.path.join(root, 'scan.ply')
    ply.write_ply(gt_ply, scan, np.zeros((len(scan), 3), np.uint8))
    base = ['--data_root', root, '--view_num', '3', '--max_d', '16', '--max_w', '160', '--max_h', '128', '--synthetic_weights',
            '--scenes', 'toy', '--scene_cache', '--fuse', '--prob_threshold', '0.1', '--disp_threshold', '0.5', '--num_consistent', '1',
            '--gt_ply', gt_ply]
    out = {}
    try:
        for name, extra in (('plain', []), ('scored', ['--score_maps', '--map_splat', '1', '--map_occlusion_tol', '0.1'])):
            FLAGS.reset()
            out[name] = os.path.join(root, 'out_' + name, 'toy')
            E.cli(base + ['--savepath', os.path.dirname(out[name])] + extra)
    finally:
        FLAGS.reset()
        E._Pipelines.CO_RESIDENT = False
    assert not os.path.exists(os.path.join(out['plain'], 'depth_eval.json'))
    for name in ('final3d_model.ply', 'cloud_eval.json'):
        with open(os.path.join(out['plain'], name), 'rb') as f, open(os.path.join(out['scored'], name), 'rb') as g:
            assert f.read() == g.read(), name
    with open(os.path.join(out['scored'], 'depth_eval.json')) as f:
        got = json.load(f)
    # the same arrays: the written maps through the probability filter (what SceneFusion stages), the written cameras
    indices, depth, cams = eval_depth.load_maps(out['scored'])
    assert indices == list(range(_N_IMAGES))
    pred = depth.copy()
    for k, i in enumerate(indices):
        with open(os.path.join(out['scored'], 'depths_atvsnet', '%08d_prob.pfm' % i), 'rb') as f:
            pred[k][P.load_pfm(f) < np.float32(0.1)] = 0
    gt = eval_depth.render_scan(ply.read_ply_points(gt_ply), cams, pred.shape[1], pred.shape[2], pixel_centre=0.0, splat=1,
                                occlusion_tol=0.1, device=cuda).cpu().numpy()
    want = eval_depth.report(pred, gt, indices=indices, pixel_centre=0.0, splat=1, occlusion_tol=0.1)
    assert json.loads(json.dumps(want)) == got
    assert [m['index'] for m in got['maps']] == indices and got['transform'] is None
    assert got['n_scored'] + len(got['skipped']) == _N_IMAGES
    # the scan is the scene's surface seen from these very cameras: it covers the maps
    assert min(m['gt_valid'] for m in got['maps']) > 0.9 * pred.shape[1] * pred.shape[2]
    assert np.array_equal(gt, SR.scan_render(ply.read_ply_points(gt_ply), eval_depth.camera_rows(cams), pred.shape[1], pred.shape[2],
                                             0.0, 1, 0.1))
