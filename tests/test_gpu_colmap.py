"""-m gpu: COLMAP import (csrc/colmap.hip, atvsnet/colmap.py, atvsnet/colmap_scene.py).

Depth ranges bit for bit against a vectorised numpy restatement of estimate_max_disparities (colmap_helpers.py:317-331) and, on
small models with exact arithmetic, against its literal loops; co-visibility against Python set intersections (:333-347); a
COLMAP dense folder of a rendered plane imported and run through eval_pointcloud --scene_cache --fuse, against the same scene
written by hand from the test's own restatements."""
import ctypes
import os
import shutil

import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
from atvsnet_amd import FLAGS, _lib, ops
from atvsnet_amd.atvsnet import colmap_scene
from atvsnet_amd.atvsnet import eval_pointcloud as E
from atvsnet_amd.atvsnet import preprocess as P

from colmap_model import neighbours_restated, quat_rotation, ranges_numpy, rotation_quat, write_text

pytestmark = pytest.mark.gpu


def _rows(R, t, intr, size):
    return np.ascontiguousarray(np.concatenate([R.reshape(-1, 9), t, intr, size.astype(np.float64)], 1))


def _gpu_ranges(cuda, xyz, R, t, intr, size, p):
    n, lo, hi = ops.colmap_depth_range(torch.from_numpy(np.ascontiguousarray(xyz)).to(cuda),
                                       torch.from_numpy(_rows(R, t, intr, size)).to(cuda), p)
    return n.cpu(), lo.cpu(), hi.cpu()


def _assert_ranges(cuda, xyz, R, t, intr, size, p=0.99):
    n, lo, hi = _gpu_ranges(cuda, xyz, R, t, intr, size, p)
    wn, wlo, whi = ranges_numpy(xyz, R, t, intr, size, p)
    assert torch.equal(n, torch.from_numpy(wn))
    assert torch.equal(lo, torch.from_numpy(wlo)) and torch.equal(hi, torch.from_numpy(whi))
    return wn


def _random_model(rng, n_images, n_points):
    q = rng.normal(size=(n_images, 4)) * np.array([4.0, 0.3, 0.3, 0.3])
    R = quat_rotation(q)
    C_ = rng.uniform(-1, 1, (n_images, 3)) * np.array([2.0, 1.0, 0.5])
    t = -np.einsum('kij,kj->ki', R, C_)
    size = np.stack([rng.integers(64, 2000, n_images), rng.integers(48, 1500, n_images)], 1)
    f = rng.uniform(0.6, 1.4, n_images) * size[:, 0]
    intr = np.stack([f, f * rng.uniform(0.98, 1.02, n_images), size[:, 0] * rng.uniform(0.4, 0.6, n_images),
                     size[:, 1] * rng.uniform(0.4, 0.6, n_images)], 1)
    xyz = rng.normal(size=(n_points, 3)) * np.array([3.0, 2.0, 2.0]) + np.array([0.0, 0.0, 6.0])
    return xyz, R, t, intr, size


@pytest.mark.parametrize('n_images,n_points,p', [(1, 1000, 0.99), (7, 4097, 0.99), (37, 50000, 0.9), (300, 20000, 0.99),
                                                 (16, 1000000, 0.99), (5, 3000, 0.5)])
def test_depth_range_is_the_numpy_restatement(cuda, n_images, n_points, p):
    rng = np.random.default_rng(n_images * 1000 + n_points)
    wn = _assert_ranges(cuda, *_random_model(rng, n_images, n_points), p=p)
    assert (wn > 0).any() and (wn < n_points).any()


def test_depth_range_borders_signs_and_ties(cuda):
    """Image 0 (and its copy 3): x = 0 and y = 0 exactly (in view), x = width and y = height exactly (not), z = 0, z < 0, -0.0,
    NaN, 5000 equal disparities among a few others; image 1: one point in view; image 2: none."""
    W, H, f, cx, cy = 64, 32, 16.0, 32.0, 16.0
    R = np.stack([np.eye(3)] * 4)
    t = np.zeros((4, 3))
    t[1] = (0.0, 0.0, -100.0)                  # only points with z > 100 are in front of image 1
    t[2] = (0.0, 0.0, -1e6)                    # nothing in front of image 2
    intr = np.array([[f, f, cx, cy]] * 4)
    size = np.array([[W, H]] * 4)
    pts = [(-2.0, 0.0, 1.0), (0.0, -1.0, 1.0),                       # x = 0, y = 0: in
           (2.0, 0.0, 1.0), (0.0, 1.0, 1.0),                         # x = width, y = height: out
           (2.0 - 2.0 ** -40, 1.0 - 2.0 ** -40, 1.0),               # just inside both
           (0.0, 0.0, 0.0), (1.0, 1.0, 0.0), (0.0, 0.0, -0.0), (0.5, 0.5, -1.0), (np.nan, 0.0, 1.0),
           (0.0, 0.0, 101.0)]                                       # the single point of image 1
    rng = np.random.default_rng(1)
    ties = np.concatenate([rng.uniform(-0.5, 0.5, (5000, 2)) * 4.0, np.full((5000, 1), 4.0)], 1)
    xyz = np.concatenate([np.array(pts), ties, rng.uniform(-1, 1, (40, 3)) + np.array([0, 0, 3.0])])
    wn = _assert_ranges(cuda, xyz, R, t, intr, size)
    assert wn[1] == 1 and wn[2] == 0 and wn[0] > 5000
    n, lo, hi = _gpu_ranges(cuda, xyz, R, t, intr, size, 0.99)
    assert lo[1] == hi[1] == 1.0 / 1.0 and lo[2] == hi[2] == 0.0
    assert hi[0] == 0.25 and lo[0] == 0.25                           # the tie at z = 4 holds both ranks
    n5, _, _ = _gpu_ranges(cuda, xyz[:5], R[:1], t[:1], intr[:1], size[:1], 0.99)
    assert int(n5[0]) == 3                                           # x = 0 / y = 0 in; width / height out; just inside in


def _literal_estimate(xyz, R, t, intr, size, percentile=0.99):
    """estimate_max_disparities (colmap_helpers.py:317-331) as written: 4x4 extrinsic, extrinsic.dot, np.sort, its indices."""
    out = []
    for k in range(len(R)):
        extrinsic = np.eye(4)
        extrinsic[:3, :3], extrinsic[:3, 3] = R[k], t[k]
        disparity_list = []
        for X in xyz:
            coord = extrinsic.dot(np.array([X[0], X[1], X[2], 1.0]))
            new_x = (coord[0] / coord[2] * intr[k, 0] + intr[k, 2])
            new_y = (coord[1] / coord[2] * intr[k, 1] + intr[k, 3])
            new_d = 1.0 / coord[2]
            if new_x >= 0.0 and new_x < size[k, 0] and new_y >= 0.0 and new_y < size[k, 1] and new_d > 0.0:
                disparity_list.append(new_d)
        disparity_list = np.sort(np.array(disparity_list))
        n = disparity_list.shape[0]
        out.append((n, disparity_list[int(n * (1.0 - percentile))], disparity_list[int(n * percentile)]))
    return out


def test_depth_range_is_the_literal_reference_on_exact_models(cuda):
    """Dyadic rotations (signed permutations), translations and points: every product and sum is exact, so the 4x4 dot's own
    summation order cannot differ; only the divisions round, identically."""
    rng = np.random.default_rng(7)
    n_img, n_pts = 6, 700
    R = np.stack([np.eye(3)[rng.permutation(3)] * rng.choice([-1.0, 1.0], 3)[:, None] for _ in range(n_img)])
    R[:, 2] = np.abs(R[:, 2])                                          # keep some points in front
    t = rng.integers(-64, 64, (n_img, 3)) / 64.0
    t[:, 2] += 8.0
    intr = np.array([[64.0, 64.0, 48.0, 32.0]] * n_img)
    size = np.array([[96, 64]] * n_img)
    xyz = rng.integers(-256, 256, (n_pts, 3)) / 64.0
    want = _literal_estimate(xyz, R, t, intr, size)
    n, lo, hi = _gpu_ranges(cuda, xyz, R, t, intr, size, 0.99)
    assert all(w[0] > 0 for w in want)
    assert [int(v) for v in n] == [w[0] for w in want]
    assert lo.numpy().tobytes() == np.array([w[1] for w in want]).tobytes()
    assert hi.numpy().tobytes() == np.array([w[2] for w in want]).tobytes()


def _covis_sets(sets, n_images):
    return np.array([[0 if i == j else len(sets[i] & sets[j]) for j in range(n_images)] for i in range(n_images)], np.int32)


def _csr(sets, n_points):
    """per-image point sets -> (offsets, observers) int32 of the distinct observing images per point, ascending."""
    obs = [[] for _ in range(n_points)]
    for i, s in enumerate(sets):
        for p in s:
            obs[p].append(i)
    off = np.zeros(n_points + 1, np.int32)
    off[1:] = np.cumsum([len(o) for o in obs])
    return off, np.array(sum(obs, []), np.int32)


def _gpu_covis(cuda, off, observers, n_images):
    return ops.colmap_covisibility(torch.from_numpy(off).to(cuda), torch.from_numpy(observers).to(cuda), n_images).cpu().numpy()


def test_covisibility_is_set_intersection(cuda):
    rng = np.random.default_rng(3)
    n_images, n_points = 41, 900
    sets = [set(rng.choice(n_points, size=rng.integers(0, 150), replace=False).tolist()) for _ in range(n_images)]
    sets[5] = set()                                                    # an image with no observations
    off, obs = _csr(sets, n_points)
    lengths = np.diff(off)
    assert (lengths == 1).any() and (lengths == 0).any()               # tracks of length 1 (and unobserved points)
    assert _gpu_covis(cuda, off, obs, n_images).tobytes() == _covis_sets(sets, n_images).tobytes()


def test_covisibility_long_track(cuda):
    """One track of 2000 observers spread over the lanes, plus short tracks."""
    rng = np.random.default_rng(5)
    n_images = 2001
    sets = [set() for _ in range(n_images)]
    for i in range(2000):
        sets[i].add(0)
    for p in range(1, 300):
        for i in rng.choice(n_images, size=rng.integers(1, 6), replace=False).tolist():
            sets[i].add(p)
    off, obs = _csr(sets, 300)
    assert off[1] - off[0] == 2000
    got = _gpu_covis(cuda, off, obs, n_images)
    assert got.tobytes() == _covis_sets(sets, n_images).tobytes()


def test_covisibility_refuses_more_than_16384_images(cuda):
    dummy = torch.zeros(4, dtype=torch.int32, device=cuda)
    rc = _lib.lib().atvs_colmap_covisibility(ctypes.c_void_p(dummy.data_ptr()), ctypes.c_void_p(dummy.data_ptr()), 1, 2, 16385,
                                              ctypes.c_void_p(dummy.data_ptr()), ctypes.c_void_p(0))
    assert rc == -2
    with pytest.raises(ValueError, match='16384'):
        ops.colmap_covisibility(dummy[:2], dummy[:2], 16385)


# ------------------------------------------------------------------------------------------------------------------ end to end

_N_CAMS, _H, _W = 9, 140, 200
_K = (180.0, 180.0, 100.0, 70.0)


def _rig():
    Rs, ts = [], []
    for i in range(_N_CAMS):
        a, b = np.deg2rad(2.5 * (i - 4)), np.deg2rad(1.0 * (i % 3 - 1))
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        R = Rx @ Ry
        C_ = np.array([0.25 * (i - 4), 0.03 * (i % 3), 0.0])
        Rs.append(R)
        ts.append(-R @ C_)
    return np.stack(Rs), np.stack(ts)


def _render(R, t):
    """The textured plane n.X + d0 = 0 (tests/fusion_scene.py's construction) seen through K, [R | t] -> BGR uint8."""
    fx, fy, cx, cy = _K
    nrm = np.array([0.1, -0.05, -1.0])
    nrm /= np.linalg.norm(nrm)
    C_ = -R.T @ t
    ys, xs = np.meshgrid(np.arange(_H, dtype=np.float64), np.arange(_W, dtype=np.float64), indexing='ij')
    rays = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(xs)], -1) @ R
    s = -(nrm @ C_ + 5.0) / (rays @ nrm)
    X = C_ + s[..., None] * rays
    img = 127.0 + 100.0 * np.stack([np.sin(X[..., 0] * 9.0), np.cos(X[..., 1] * 11.0), np.sin(5.0 * (X[..., 0] + X[..., 1]))], -1)
    return np.clip(img, 0, 255).astype(np.uint8)


def _write_dense(root, Rs, ts):
    from PIL import Image
    rng = np.random.default_rng(11)
    nrm = np.array([0.1, -0.05, -1.0])
    nrm /= np.linalg.norm(nrm)
    xy = rng.uniform([-4.0, -2.5], [4.0, 2.5], (2500, 2))
    z = -(5.0 + nrm[0] * xy[:, 0] + nrm[1] * xy[:, 1]) / nrm[2]          # on the plane
    xyz = np.concatenate([xy, z[:, None]], 1)
    os.makedirs(os.path.join(root, 'images'))
    qs = [rotation_quat(R) for R in Rs]
    images, tracks, sets = [], [[] for _ in range(len(xyz))], []
    ids = [10 + 3 * i for i in range(_N_CAMS)][::-1]                       # IMAGE_IDs not in camera order
    for i in range(_N_CAMS):
        name = 'frame_%02d.jpg' % i
        Image.fromarray(_render(Rs[i], ts[i])[:, :, ::-1]).save(os.path.join(root, 'images', name), quality=95)
        c = xyz @ Rs[i].T + ts[i]
        u, v = c[:, 0] / c[:, 2] * _K[0] + _K[2], c[:, 1] / c[:, 2] * _K[1] + _K[3]
        vis = np.flatnonzero((c[:, 2] > 0) & (u >= 0) & (u < _W) & (v >= 0) & (v < _H))
        obs = [(float(u[p]), float(v[p]), int(p) + 1) for p in vis] + [(1.0, 1.0, -1)]
        sets.append(set(int(p) + 1 for p in vis))
        for k, p in enumerate(vis):
            tracks[p].append((ids[i], k))
        images.append((ids[i], tuple(qs[i]), tuple(ts[i]), 1, name, obs))
    points = [(p + 1, tuple(xyz[p]), tracks[p]) for p in range(len(xyz))]
    write_text(os.path.join(root, 'sparse'), [(1, 'PINHOLE', _W, _H, _K)], images, points)
    return ids, qs, xyz, sets


def _files(d):
    return {f: open(os.path.join(d, f), 'rb').read() for f in sorted(os.listdir(d)) if f.endswith('.pfm')}


def test_import_then_fuse_is_the_hand_written_scene(cuda, tmp_path, weights):
    root = str(tmp_path)
    Rs, ts = _rig()
    dense = os.path.join(root, 'dense')
    ids, qs, xyz, obs_sets = _write_dense(dense, Rs, ts)
    imported = os.path.join(root, 'data', 'eth3d', 'imported')
    max_d, num, p, stretch = 16, 4, 0.99, 1.33333
    colmap_scene.main(['--dense_folder', dense, '--out', imported, '--max_d', str(max_d), '--num_neighbors', str(num)])
    # the same scene by hand: scene index = rank of the IMAGE_ID
    order = np.argsort(ids, kind='stable')                               # scene index k -> camera order[k]
    hand = os.path.join(root, 'data', 'eth3d', 'hand')
    os.makedirs(os.path.join(hand, 'cams'))
    os.makedirs(os.path.join(hand, 'images'))
    R_q = quat_rotation(np.stack([qs[i] for i in order]))
    t_k = np.stack([ts[i] for i in order])
    intr = np.array([_K] * _N_CAMS)
    size = np.array([[_W, _H]] * _N_CAMS)
    n, lo, hi = ranges_numpy(xyz, R_q, t_k, intr, size, p)
    assert (n > 0).all()
    for k, i in enumerate(order):
        cam = np.zeros((2, 4, 4))
        cam[0, :3, :3], cam[0, :3, 3], cam[0, 3, 3] = R_q[k], t_k[k], 1.0
        cam[1, 0, 0], cam[1, 1, 1], cam[1, 0, 2], cam[1, 1, 2], cam[1, 2, 2] = _K[0], _K[1], _K[2], _K[3], 1.0
        depth_min, depth_max = 1.0 / float(hi[k] * stretch), 1.0 / float(lo[k] / stretch)   # preprocess_colmap.py:204-214
        cam[1, 3] = (depth_min, (depth_max - depth_min) / float(max_d - 1), max_d, depth_max)
        P.write_cam(os.path.join(hand, 'cams', '%08d_cam.txt' % k), cam)
        shutil.copyfile(os.path.join(dense, 'images', 'frame_%02d.jpg' % i), os.path.join(hand, 'images', '%08d.jpg' % k))
    with open(os.path.join(hand, 'pair.txt'), 'w') as f:
        f.write(neighbours_restated([obs_sets[i] for i in order], [True] * _N_CAMS, num))
    for k in range(_N_CAMS):
        a, b = ('%08d_cam.txt' % k, '%08d_cam.txt' % k)
        assert open(os.path.join(imported, 'cams', a)).read() == open(os.path.join(hand, 'cams', b)).read()
        with open(os.path.join(imported, 'cams', a)) as f:
            cam = P.load_cam(f)
        i = order[k]
        assert np.abs(cam[0, :3, :3] - Rs[i]).max() <= 1e-12 and np.abs(cam[0, :3, 3] - ts[i]).max() <= 1e-12
    assert open(os.path.join(imported, 'pair.txt')).read() == open(os.path.join(hand, 'pair.txt')).read()
    assert open(os.path.join(imported, 'images', '00000000.jpg'), 'rb').read() == \
        open(os.path.join(dense, 'images', 'frame_%02d.jpg' % order[0]), 'rb').read()
    # both scenes through the driver, scene mode with in-run fusion
    out = {}
    try:
        for name in ('imported', 'hand'):
            FLAGS.reset()
            out[name] = os.path.join(root, 'out', name)
            E.cli(['--data_root', os.path.join(root, 'data'), '--view_num', '3', '--max_d', str(max_d), '--max_w', '160', '--max_h',
                   '128', '--synthetic_weights', '--scenes', name, '--savepath', os.path.join(root, 'out'), '--scene_cache', '--fuse',
                   '--prob_threshold', '0.5', '--disp_threshold', '0.5', '--num_consistent', '1'])
    finally:
        FLAGS.reset()
    maps = {k: _files(os.path.join(v, 'depths_atvsnet')) for k, v in out.items()}
    assert len(maps['hand']) == 2 * _N_CAMS and maps['imported'] == maps['hand']
    ply = {k: open(os.path.join(v, 'final3d_model.ply'), 'rb').read() for k, v in out.items()}
    assert len(ply['hand']) > 300 and ply['imported'] == ply['hand']
