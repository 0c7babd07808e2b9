"""CPU: the host side of the scan renderer -- the restatement (tests/scan_render_restated.py) against a literal loop, eval_depth's
camera rows, similarity inverse and map scores, the argument checks of ops.scan_render (no CPU fallback), the command lines'
refusals, the library's new entry points."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd                                   # noqa: F401
from atvsnet_amd import _lib, ops
from atvsnet_amd.atvsnet import eval_depth, eval_errors, eval_pointcloud

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_render_restated as SR  # noqa: E402


def _tiny(seed=0):
    rng = np.random.default_rng(seed)
    rows, cols = 7, 9
    cams = SR.ring_cameras(3, rows, cols, radius=3.0)
    pts = rng.uniform(-1.2, 1.2, (400, 3)).astype(np.float32)
    pts[3] = np.nan
    pts[4, 1] = np.inf
    pts[5] = pts[6]                                             # a tie
    pts[7] = (cams[0, :9].reshape(3, 3).T @ -cams[0, 9:12]).astype(np.float32)          # (about) a camera centre: c_2 ~ 0
    pts[8:12] *= 1e30                                           # far outside every image, and beyond float32 depths squared
    return pts, cams, rows, cols


@pytest.mark.parametrize('splat,tol,centre', [(0, 0.0, 0.0), (1, 0.0, 0.5), (2, 0.05, 0.0), (4, 0.3, 0.5)])
def test_restatement_against_the_literal_loop(splat, tol, centre):
    pts, cams, rows, cols = _tiny()
    got = SR.scan_render(pts, cams, rows, cols, centre, splat, tol)
    want = SR.scan_render_loop(pts, cams, rows, cols, centre, splat, tol)
    assert got.dtype == np.float32 and got.shape == (3, rows, cols)
    assert np.array_equal(got, want)
    assert (SR.scan_render(pts, cams, rows, cols, centre, 0, 0.0) > 0).sum() > 40 and (got > 0).sum() >= 10       # not an empty case
    if splat == 0:                                               # every near pixel survives
        near = np.stack([SR.planes(pts, c, rows, cols, centre, 0)[0] for c in cams])
        assert np.array_equal(got > 0, near != SR.EMPTY)
    else:
        assert (got > 0).sum() <= (SR.scan_render(pts, cams, rows, cols, centre, 0, 0.0) > 0).sum()


def test_restatement_borders_and_occlusion_by_hand():
    # identity camera, fx = fy = 4, cx = cy = 0: a point (X, Y, 2) lands at xs = 2 X + 0.5
    cam = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 4, 4, 0, 0], np.float64)
    # xs = 0 (inside), 4 = cols (outside), -0.5 (outside); then pixel (1, 1) three times at depths 2, 4, 4 (xs = 1.5, 1.0, 1.5);
    # then the same ray behind the camera and on its plane
    pts = np.array([[-0.25, 0, 2], [1.75, 0, 2], [-0.5, 0, 2], [0.5, 0.5, 2], [0.5, 0.5, 4], [1.0, 0.5, 4], [0.5, 0.5, -2],
                    [0.5, 0.5, 0]], np.float32)
    d = SR.scan_render(pts, cam[None], 3, 4, 0.0, 0, 0.0)[0]
    want = np.zeros((3, 4), np.float32)
    want[0, 0], want[1, 1] = 2, 2
    assert np.array_equal(d, want)
    # the far point alone in pixel (2, 1), next to the near one: kept without a window, dropped with one
    pts2 = np.array([[0.5, 0.5, 2], [2.0, 1.0, 4]], np.float32)  # xs = 1.5 / 2.5, ys = 1.5 / 1.5
    assert np.array_equal(SR.scan_render(pts2, cam[None], 3, 4, 0.0, 0, 0.0)[0][1], np.array([0, 2, 4, 0], np.float32))
    assert np.array_equal(SR.scan_render(pts2, cam[None], 3, 4, 0.0, 1, 0.5)[0][1], np.array([0, 2, 0, 0], np.float32))
    assert np.array_equal(SR.scan_render(pts2, cam[None], 3, 4, 0.0, 1, 1.0)[0][1], np.array([0, 2, 4, 0], np.float32))


def _driver_cams(n=3):
    cams = np.zeros((n, 2, 4, 4))
    for k in range(n):
        a = 0.2 * k
        cams[k, 0] = np.eye(4)
        cams[k, 0, :3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        cams[k, 0, :3, 3] = (0.1 * k, -0.2, 0.3)
        cams[k, 1, :3, :3] = [[50.0 + k, 0, 31.5], [0, 51.0, 23.25], [0, 0, 1]]
        cams[k, 1, 3] = (0.5, 0.01, 128, 3.0)
    return cams


def test_camera_rows():
    cams = _driver_cams()
    rows = eval_depth.camera_rows(cams)
    assert rows.shape == (3, 16) and rows.dtype == np.float64
    for k in range(3):
        assert np.array_equal(rows[k, :9].reshape(3, 3), cams[k, 0, :3, :3]) and np.array_equal(rows[k, 9:12], cams[k, 0, :3, 3])
        assert rows[k, 12:].tolist() == [50.0 + k, 51.0, 31.5, 23.25]
    assert np.array_equal(eval_depth.camera_rows(cams[1]), rows[1:2])
    assert np.array_equal(eval_depth.camera_rows(cams.astype(np.float32)), eval_depth.camera_rows(cams.astype(np.float32).astype(np.float64)))
    bad = cams.copy()
    bad[2, 1, 0, 1] = 1e-3
    with pytest.raises(ValueError, match='camera 2 has skew'):
        eval_depth.camera_rows(bad)
    with pytest.raises(ValueError, match='expected'):
        eval_depth.camera_rows(np.zeros((3, 4, 4)))
    bad = cams.copy()
    bad[0, 0, 1, 3] = np.nan
    with pytest.raises(ValueError, match='non-finite'):
        eval_depth.camera_rows(bad)


def _similarity(deg=30.0, scale=2.5, t=(0.3, -1.1, 4.0)):
    a = np.deg2rad(deg)
    axis = np.array([0.3, -0.5, 0.8])
    axis /= np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = scale * R, t
    return T


def test_inverse_similarity_round_trip_and_refusals():
    T = _similarity()
    inv = eval_depth.inverse_similarity(T)
    assert inv.dtype == np.float64
    assert np.abs(inv @ T - np.eye(4)).max() < 1e-14 and np.abs(T @ inv - np.eye(4)).max() < 1e-14
    assert np.abs(eval_depth.inverse_similarity(inv) - T).max() < 1e-14
    assert np.array_equal(eval_depth.inverse_similarity(np.eye(4).tolist()), np.eye(4))
    shear = T.copy()
    shear[0, 1] += 1e-6
    with pytest.raises(ValueError, match='scaled rotation'):
        eval_depth.inverse_similarity(shear)
    squash = T.copy()
    squash[:3, 0] *= 1.0 + 1e-7
    with pytest.raises(ValueError, match='scaled rotation'):
        eval_depth.inverse_similarity(squash)
    mirror = T.copy()
    mirror[:3, 0] *= -1
    with pytest.raises(ValueError, match='scaled rotation'):
        eval_depth.inverse_similarity(mirror)
    row = T.copy()
    row[3, 0] = 1e-3
    with pytest.raises(ValueError, match='last row'):
        eval_depth.inverse_similarity(row)
    with pytest.raises(ValueError, match='16 finite'):
        eval_depth.inverse_similarity(np.eye(3))


def test_score_maps_skips_and_means():
    rng = np.random.default_rng(3)
    gt = rng.uniform(1.0, 3.0, (4, 12, 16)).astype(np.float32)
    pred = (gt * rng.uniform(0.95, 1.05, gt.shape)).astype(np.float32)
    gt[0, :6] = 0.0                                              # half the map without ground truth
    pred[0, 6:, :4] = np.nan
    gt[1] = 0.0                                                  # nothing: skipped
    gt[1, 0, :5] = 2.0
    pred[3, 0, 0] = 1e12                                         # calc_error's upper bound
    out = eval_depth.score_maps(pred, gt, min_valid=10, indices=[7, 3, 11, 12])
    assert [m['index'] for m in out['maps']] == [7, 3, 11, 12]
    assert [m['valid'] for m in out['maps']] == [6 * 12, 5, 12 * 16, 12 * 16 - 1]
    assert [m['gt_valid'] for m in out['maps']] == [6 * 16, 5, 12 * 16, 12 * 16]
    assert out['maps'][0]['coverage'] == 72 / 192.0
    assert [m['skipped'] for m in out['maps']] == [False, True, False, False]
    assert out['skipped'] == [3] and out['n_scored'] == 3 and out['min_valid'] == 10
    assert 'mae' not in out['maps'][1]
    names = eval_errors.err_metrics_namelist + eval_errors.acc_metrics_namelist
    per_map = []
    for k in (0, 2, 3):
        e, _ = eval_errors.calc_error(pred[k], gt[k])
        assert [out['maps'][k][n] for n in names] == [float(v) for v in e]
        per_map.append(e.astype(np.float64))
    assert [out['mean'][n] for n in names] == np.mean(np.stack(per_map), axis=0).tolist()
    none = eval_depth.score_maps(pred[1:2], gt[1:2], min_valid=10)
    assert none['mean'] is None and none['skipped'] == [0] and none['n_scored'] == 0
    with pytest.raises(ValueError, match='min_valid'):
        eval_depth.score_maps(pred, gt, min_valid=0)
    with pytest.raises(ValueError, match='one shape'):
        eval_depth.score_maps(pred, gt[:, :5])
    rep = eval_depth.report(pred, gt, min_valid=10, transform=np.eye(4), splat=1, occlusion_tol=0.1, pixel_centre=0.5)
    assert (rep['rows'], rep['cols'], rep['splat'], rep['occlusion_tol'], rep['pixel_centre']) == (12, 16, 1, 0.1, 0.5)
    assert rep['transform'] == np.eye(4).tolist()


def test_ops_scan_render_refuses_bad_arguments_no_fallback():
    P, C = torch.zeros(5, 3), torch.zeros(2, 16, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.scan_render(P, C, 4, 4)
    for kw, text in ((dict(splat=5), 'splat'), (dict(splat=-1), 'splat'), (dict(splat=1.5), 'splat'),
                     (dict(occlusion_tol=-0.1), 'occlusion_tol'), (dict(occlusion_tol=float('inf')), 'occlusion_tol'),
                     (dict(occlusion_tol=float('nan')), 'occlusion_tol'), (dict(pixel_centre=float('nan')), 'pixel_centre')):
        with pytest.raises(ValueError, match=text):
            ops.scan_render(P, C, 4, 4, **kw)
    with pytest.raises(ValueError, match='rows'):
        ops.scan_render(P, C, 0, 4)
    with pytest.raises(TypeError, match='points'):
        ops.scan_render(P.double(), C, 4, 4)
    with pytest.raises(ValueError, match='points'):
        ops.scan_render(torch.zeros(5, 4), C, 4, 4)
    assert ops.SCAN_RENDER_MAX_SPLAT == 4 and ops.SCAN_RENDER_MAX_CAMS == 65535
    assert (ops.CLOUD_MAX_TOLERANCES, ops.CLOUD_MAX_K, ops.CLOUD_SCAN_MAX_WINDOW, ops.CLOUD_MAX_POINTS) == (16, 32, 2, 1 << 30)


def test_library_exports_the_renderer_and_checks_arguments_on_the_host():
    names = _lib.declared_symbols()
    L = _lib.lib()
    for n in ('atvs_scan_render_scratch_size', 'atvs_scan_render'):
        assert n in names and hasattr(L, n), n
    assert _lib.header_abi_version() >= 51 and L.atvs_abi_version() == _lib.header_abi_version()
    assert 'scan_render' not in _lib.OWNS_ITS_SIMD
    flags = _lib.flags_for(os.path.join(_lib.CSRC, 'scan_render.hip'))
    assert '-ffp-contract=off' in flags and '-fno-slp-vectorize' in flags
    nbytes = ctypes.c_long(0)
    assert L.atvs_scan_render_scratch_size(50, 120, 228, ctypes.byref(nbytes)) == 0 and nbytes.value == 2 * 4 * 50 * 120 * 228
    assert L.atvs_scan_render_scratch_size(65535, 181, 181, ctypes.byref(nbytes)) == 0           # 2 146 992 135 < 2^31
    assert L.atvs_scan_render_scratch_size(32768, 256, 256, ctypes.byref(nbytes)) == -2          # = 2^31
    assert L.atvs_scan_render_scratch_size(65536, 1, 1, ctypes.byref(nbytes)) == -2
    assert L.atvs_scan_render_scratch_size(0, 4, 4, ctypes.byref(nbytes)) == -2
    assert L.atvs_scan_render_scratch_size(1, 4, 4, None) == -1
    fake, lng, dbl = ctypes.c_void_p(256), ctypes.c_long, ctypes.c_double       # never dereferenced: refused before a launch
    call = lambda n=10, cams=2, rows=4, cols=4, centre=0.0, splat=0, tol=0.0, sb=1 << 20, pts=fake: L.atvs_scan_render(  # noqa: E731
        pts, lng(n), fake, cams, rows, cols, dbl(centre), splat, dbl(tol), fake, lng(sb), fake, None)
    for kw in (dict(splat=-1), dict(splat=5), dict(tol=-1e-9), dict(tol=float('inf')), dict(tol=float('nan')),
               dict(centre=float('nan'))):
        assert call(**kw) == -3, kw
    for kw in (dict(sb=2 * 4 * 2 * 16 - 1), dict(cams=65536, rows=1, cols=1), dict(cams=32768, rows=256, cols=256, sb=1 << 40),
               dict(n=-1), dict(n=(1 << 30) + 1), dict(cams=0), dict(rows=0)):
        assert call(**kw) == -2, kw
    assert call(pts=None) == -1
    assert L.atvs_scan_render(fake, lng(1), None, 2, 4, 4, dbl(0), 0, dbl(0), fake, lng(1 << 20), fake, None) == -1


def test_command_lines_refuse(capsys, tmp_path):
    def refused(cli, argv, text):
        with pytest.raises(SystemExit) as e:
            cli(argv)
        assert e.value.code == 2 and text in ' '.join(capsys.readouterr().err.split())

    refused(eval_pointcloud.cli, ['--fuse', '--score_maps'], '--score_maps needs --gt_ply')
    refused(eval_pointcloud.cli, ['--score_maps', '--gt_ply', 'a.ply'], '--gt_ply needs --fuse')
    refused(eval_pointcloud.cli, ['--fuse', '--gt_ply', 'a.ply', '--map_splat', '1'], 'need --score_maps')
    refused(eval_pointcloud.cli, ['--fuse', '--gt_ply', 'a.ply', '--score_maps', '--map_splat', '5'], '--map_splat must be in 0..4')
    refused(eval_pointcloud.cli, ['--fuse', '--gt_ply', 'a.ply', '--score_maps', '--map_occlusion_tol', '-1'], '--map_occlusion_tol')
    with pytest.raises(ValueError, match='needs gt_ply'):
        eval_pointcloud.run_eval_pc('out', [], fuse=dict(), score_maps=dict())

    maps, scan = tmp_path / 'maps', tmp_path / 'scan.ply'
    maps.mkdir()
    scan.write_bytes(b'')
    io = ['--maps', str(maps), '--gt', str(scan)]
    refused(eval_depth.cli, ['--gt', str(scan)], '--maps')
    refused(eval_depth.cli, ['--maps', str(maps)], '--gt')
    refused(eval_depth.cli, io + ['--splat', '5'], '--splat must be in 0..4')
    refused(eval_depth.cli, io + ['--occlusion_tol', '-0.5'], '--occlusion_tol must be >= 0')
    refused(eval_depth.cli, io + ['--min_valid', '0'], '--min_valid')
    refused(eval_depth.cli, ['--maps', str(maps), '--gt', str(tmp_path / 'none.ply')], 'no such file')
    refused(eval_depth.cli, ['--maps', str(tmp_path / 'none'), '--gt', str(scan)], 'no such folder')
    refused(eval_depth.cli, io + ['--scene', str(tmp_path)], 'no pair.txt')
    sheared = tmp_path / 'T.txt'
    T = _similarity()
    T[0, 1] += 1e-3
    np.savetxt(str(sheared), T, fmt='%.17g')
    refused(eval_depth.cli, io + ['--transform', str(sheared)], 'scaled rotation')
    assert 'not ETH3D' in ' '.join(eval_depth.make_parser().format_help().split())


def test_load_maps_and_scene_indices(tmp_path):
    from atvsnet_amd.atvsnet import preprocess as P
    folder = tmp_path / 'out' / 'depths_atvsnet'
    folder.mkdir(parents=True)
    cams = _driver_cams(3)
    rng = np.random.default_rng(0)
    depth = rng.uniform(1, 2, (3, 6, 8)).astype(np.float32)
    for k, i in enumerate((12, 3, 7)):
        P.write_pfm(str(folder / ('%08d.pfm' % i)), depth[k])
        P.write_pfm(str(folder / ('%08d_prob.pfm' % i)), depth[k])
        P.write_cam(str(folder / ('%08d.txt' % i)), cams[k])
    idx, d, c = eval_depth.load_maps(str(tmp_path / 'out'))
    assert idx == [3, 7, 12] and np.array_equal(d, depth[[1, 2, 0]]) and np.array_equal(c, cams[[1, 2, 0]])
    idx, d, c = eval_depth.load_maps(str(folder), [12, 3])
    assert idx == [3, 12] and np.array_equal(d, depth[[1, 0]])
    with pytest.raises(ValueError, match='missing'):
        eval_depth.load_maps(str(folder), [3, 4])
    (tmp_path / 'pair.txt').write_text('3\n12\n2 3 0.5 7 0.25\n3\n1 12 1.0\n7\n0\n')
    assert eval_depth.scene_indices(str(tmp_path)) == [12, 3, 7]
