"""-m gpu: point-cloud scoring (csrc/cloud.hip, ops/cloud.py, atvsnet/eval_cloud.py, eval_pointcloud --gt_ply).

Every comparison with the brute-force restatement (tests/cloud_restated.py) is exact: np.array_equal on d2 AND idx."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd                                   # noqa: F401
from atvsnet_amd import ops, synthetic
from atvsnet_amd.atvsnet import eval_cloud
from atvsnet_amd.atvsnet import eval_pointcloud as E
from atvsnet_amd.atvsnet import preprocess as P
from atvsnet_amd.flags import FLAGS
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_restated as CR  # noqa: E402

pytestmark = pytest.mark.gpu


def _gpu(dev, Q, Pts, R, grid=None):
    """-> (d2, idx) numpy of the kernels, and the grid"""
    g = grid if grid is not None else ops.cloud_grid(torch.from_numpy(np.ascontiguousarray(Pts, np.float32)).to(dev), R)
    d2, idx = ops.cloud_nearest(g, torch.from_numpy(np.ascontiguousarray(Q, np.float32)).to(dev))
    return d2.cpu().numpy(), idx.cpu().numpy(), g


def _same(dev, Q, Pts, R):
    want_d2, want_idx = CR.nearest(Q, Pts, R)
    d2, idx, g = _gpu(dev, Q, Pts, R)
    assert d2.dtype == np.float32 and idx.dtype == np.int32
    assert np.array_equal(d2, want_d2) and np.array_equal(idx, want_idx)
    return want_d2, want_idx, g


def test_random_cloud_equals_the_restatement(cuda):
    rng = np.random.default_rng(5)
    Pts = rng.uniform(0, 4, (20000, 3)).astype(np.float32)
    Q = (Pts + rng.normal(0, 0.03, Pts.shape)).astype(np.float32)
    Q[:2000] += 3.0
    want_d2, _, _ = _same(cuda, Q, Pts, 0.05)
    found = np.isfinite(want_d2).mean()
    print('found share %.3f' % found)
    assert 0.2 <= found <= 0.9                          # neither branch is vacuous


def test_ties_take_the_lowest_index(cuda):
    a = np.arange(16, dtype=np.float32)
    lattice = np.stack(np.meshgrid(a, a, a, indexing='ij'), -1).reshape(-1, 3)
    Pts = np.concatenate([lattice, lattice], 0)                        # every point again at a higher index
    Q = np.concatenate([lattice, lattice[:2000] + np.float32(0.5)], 0)   # lattice points and cell centres (8 equidistant corners)
    want_d2, want_idx, _ = _same(cuda, Q, Pts, 1.0)
    assert np.array_equal(want_idx[:len(lattice)], np.arange(len(lattice))) and (want_d2[len(lattice):] == 0.75).all()
    assert (want_idx < len(lattice)).all()


@pytest.mark.parametrize('shift', [(0.0, 0.0, 0.0), (1000.0, -1000.0, 3.0)])
def test_trap_pairs(cuda, shift):
    """A neighbour two cells away under a cell edge of exactly R (tests/test_cloud_host.py::test_restatement_of_the_trap_pair): the
    pair at reference x = 0.5, whose float32 d2 is exactly R * R, and the pair at 0.5 + 2^-20; alone and among other points."""
    s = np.array(shift, np.float32)
    qx = np.float32(0.25 - 2.0 ** -26)
    for px in (0.5, 0.5 + 2.0 ** -20):
        Q = np.array([[qx, 0, 0]], np.float32) + s
        Pts = np.array([[px, 0, 0]], np.float32) + s
        want_d2, _, _ = _same(cuda, Q, Pts, 0.25)
        if shift == (0.0, 0.0, 0.0):
            assert np.isfinite(want_d2[0]) == (px == 0.5)
        # with an origin at 0 and more cells around: the box starts at (0, 0, 0) + shift
        more = np.array([[0, 0, 0], [2, 2, 2], [px, 0, 0], [0.75 + 2.0 ** -20, 0, 0]], np.float32) + s
        _same(cuda, np.array([[qx, 0, 0], [0.25, 0, 0], [1.25, 2, 2]], np.float32) + s, more, 0.25)
        # ... and both directions
        _same(cuda, more, np.array([[qx, 0, 0], [0.25, 0, 0]], np.float32) + s, 0.25)


def test_radius_at_below_and_above_an_exact_distance(cuda):
    """3-4-5 triangles: d2 = 25 exactly for the first three queries; the fourth's float32 d2 is the next float32 above 25."""
    Pts = np.array([[0, 0, 0], [40, 40, 40]], np.float32)
    Q = np.array([[3, 4, 0], [0, 3, 4], [43, 40, 44], [3, 4, 0.001]], np.float32)
    five = np.float32(5)
    for R, idx in ((five, [0, 0, 1, -1]), (np.nextafter(five, np.float32(0)), [-1, -1, -1, -1]),
                   (np.nextafter(five, np.float32(9)), [0, 0, 1, 0])):
        want_d2, want_idx, _ = _same(cuda, Q, Pts, R)
        assert want_idx.tolist() == idx and (want_d2[:3] == 25.0).all() == (idx[0] == 0)


def test_non_finite_empty_and_degenerate_clouds(cuda):
    rng = np.random.default_rng(11)
    Pts = rng.uniform(-1, 1, (3000, 3)).astype(np.float32)
    Q = rng.uniform(-1.2, 1.2, (2500, 3)).astype(np.float32)
    Pts[::7, 0], Pts[3::11, 1], Pts[5::13, 2] = np.nan, np.inf, -np.inf
    Q[::9, 2], Q[4::10, 0], Q[1::17, 1] = np.nan, -np.inf, np.inf
    want_d2, want_idx, g = _same(cuda, Q, Pts, 0.1)
    assert np.isfinite(want_d2).any() and np.isinf(want_d2[::9]).all()
    # two calls on one grid: bitwise equal
    a = _gpu(cuda, Q, Pts, 0.1, grid=g)
    b = _gpu(cuda, Q, Pts, 0.1, grid=g)
    assert a[0].tobytes() == b[0].tobytes() == want_d2.tobytes() and np.array_equal(a[1], b[1])
    empty = np.zeros((0, 3), np.float32)
    _same(cuda, Q, empty, 0.1)                                        # n = 0: nothing found
    d2, idx, _ = _gpu(cuda, empty, Pts, 0.1)                          # m = 0
    assert d2.shape == (0,) and idx.shape == (0,)
    _same(cuda, Q, np.full((5, 3), np.nan, np.float32), 0.1)          # no finite reference point
    _same(cuda, np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 0.56], [9, 9, 9]], np.float32), np.array([[0.5, 0.5, 0.5]], np.float32), 0.1)   # n = 1
    same = np.tile(np.array([[1.5, -2.5, 3.25]], np.float32), (500, 1))                # one cell, every point identical
    want_d2, want_idx, _ = _same(cuda, np.array([[1.5, -2.5, 3.25], [1.5, -2.5, 3.3], [1.5, -2.5, 4.0]], np.float32), same, 0.1)
    assert want_idx[0] == 0 and want_idx[1] == 0 and want_idx[2] == -1
    plane = rng.uniform(0, 2, (4000, 3)).astype(np.float32)
    plane[:, 1] = 0.75                                                                 # zero extent on one axis
    qp = plane[:1500] + rng.normal(0, 0.02, (1500, 3)).astype(np.float32)
    want_d2, _, _ = _same(cuda, qp, plane, 0.05)
    assert 0.05 < np.isfinite(want_d2).mean() < 1.0


def test_sparse_cloud_beyond_the_cell_cap(cuda):
    """Two clusters 10^4 apart with R = 10^-3: 10^21 cells of edge R; the grid takes a coarser cell, the output does not change, and
    the grid stays within the documented O(n + cells) bytes (cells <= max(4096, 8 n))."""
    rng = np.random.default_rng(3)
    n = 6000
    Pts = (rng.uniform(0, 0.02, (n, 3)) + np.where(np.arange(n)[:, None] % 2, 1e4, 0.0)).astype(np.float32)
    Q = Pts[rng.permutation(n)[:3000]] + rng.normal(0, 5e-4, (3000, 3)).astype(np.float32)
    want_d2, _, g = _same(cuda, Q.astype(np.float32), Pts, 1e-3)
    assert 0.05 < np.isfinite(want_d2).mean() < 1.0
    assert g.nbytes <= n * 20 + 4 * (max(4096, 8 * n) + 2) + 4096


def test_permuting_the_reference_cloud(cuda):
    rng = np.random.default_rng(8)
    a = np.arange(10, dtype=np.float32) * np.float32(0.25)
    lattice = np.stack(np.meshgrid(a, a, a, indexing='ij'), -1).reshape(-1, 3)
    away = np.array([5, 0, 0], np.float32)              # the random part beside the lattice, so that it breaks none of its ties
    Pts = np.concatenate([lattice, rng.uniform(0, 2.25, (3000, 3)).astype(np.float32) + away], 0)
    Q = np.concatenate([lattice + np.float32(0.125), rng.uniform(0, 2.25, (2000, 3)).astype(np.float32) + away], 0)
    R = 0.25
    want_d2, want_idx, uniq = CR.nearest(Q, Pts, R, unique=True)
    assert uniq.sum() > 500 and (np.isfinite(want_d2) & ~uniq).sum() > 500
    perm = rng.permutation(len(Pts))
    d2a, idxa, _ = _gpu(cuda, Q, Pts, R)
    d2b, idxb, _ = _gpu(cuda, Q, Pts[perm], R)
    assert np.array_equal(d2a, want_d2) and np.array_equal(idxa, want_idx)
    assert d2a.tobytes() == d2b.tobytes()
    back = np.where(idxb >= 0, perm[np.maximum(idxb, 0)], -1)
    assert np.array_equal(back[uniq], idxa[uniq]) and np.array_equal(idxb < 0, idxa < 0)
    # under the permutation too the lowest index of the permuted cloud wins
    assert np.array_equal(idxb, CR.nearest(Q, Pts[perm], R)[1])


def test_counts(cuda):
    rng = np.random.default_rng(2)
    Pts = rng.uniform(0, 2, (5000, 3)).astype(np.float32)
    Q = np.concatenate([Pts[:3000] + rng.normal(0, 0.03, (3000, 3)).astype(np.float32),
                        Pts[:1] + np.array([[0.0625, 0, 0]], np.float32), Pts[1:2] + np.array([[0, 0.125, 0]], np.float32)], 0)
    R = 0.125
    want_d2, _ = CR.nearest(Q, Pts, R)
    d2, idx = ops.cloud_nearest(ops.cloud_grid(torch.from_numpy(Pts).to(cuda), R), torch.from_numpy(Q).to(cuda))
    assert np.array_equal(d2.cpu().numpy(), want_d2)
    exact = float(np.sqrt(np.float64(want_d2[np.isfinite(want_d2)][7])))     # a tolerance whose square may equal a d2
    tol = [0.0, 0.01, 0.03, 0.0625, exact, 0.1, R]
    got = ops.cloud_counts(d2, tol, R)
    assert got.dtype == torch.int64 and got.cpu().tolist() == CR.counts(want_d2, tol)
    assert got.cpu().tolist() == [int((d2.double() <= t * t).sum()) for t in tol]
    assert got[-1].item() == int(np.isfinite(want_d2).sum()) and 0 < got[1].item() < got[3].item() < got[-1].item()
    # d2 = 0.0625^2 exactly for a query at an exactly representable offset, if no nearer point exists: counted at tau = 0.0625
    assert ops.cloud_counts(torch.tensor([0.0625 * 0.0625, 0.015625, np.inf], device=cuda), [0.0625, 0.125], R).cpu().tolist() == [1, 2]
    assert ops.cloud_counts(torch.zeros(0, device=cuda), [0.1], R).cpu().tolist() == [0]
    with pytest.raises(ValueError, match='tolerance'):
        ops.cloud_counts(d2, [0.2], R)


def test_large_surface(cuda):
    """2,000,000 reference x 1,000,000 query points on a noisy sphere."""
    Pts, Q = CR.surface(2000000, 1), CR.surface(1000000, 2, noise=0.006)          # a k-d tree finds 96.5 % of these within R
    R = 0.01
    dP = torch.from_numpy(Pts).to(cuda)
    g = ops.cloud_grid(dP, R)
    d2, idx = ops.cloud_nearest(g, torch.from_numpy(Q).to(cuda))
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    found = idx >= 0
    print('found share %.4f' % found.mean())
    assert 0.5 < found.mean() < 0.99 and np.isinf(d2[~found]).all() and (idx < len(Pts)).all()
    # (a) a random sample against the whole reference cloud by the restatement
    pick = np.random.default_rng(9).choice(len(Q), 4096, replace=False)
    want_d2, want_idx = CR.nearest(Q[pick], Pts, R)
    assert np.array_equal(d2[pick], want_d2) and np.array_equal(idx[pick], want_idx)
    # (b) every reported d2 is the float32 expression of the reported index
    assert np.array_equal(CR.d2_pairs(Q[found], Pts[idx[found]]), d2[found])
    assert (d2[found].astype(np.float64) <= float(np.float32(R)) ** 2).all()
    # (c) a float64 k-d tree over all queries
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return
    Rd = float(np.float32(R))
    dist, ti = cKDTree(Pts.astype(np.float64)).query(Q.astype(np.float64), distance_upper_bound=Rd, workers=16)
    tfound = np.isfinite(dist)
    # the float32 expression is within about 4 * 2^-24 = 2.4e-7 relative of the exact d2, half that on d: 1e-6 is far outside it
    band = np.abs(dist - Rd) <= 1e-6 * Rd
    assert band.mean() < 1e-3
    both = tfound & found
    assert (d2[both] <= CR.d2_pairs(Q[both], Pts[ti[both]])).all()          # the kernel's is the minimum over everything
    assert np.array_equal(found[~band], tfound[~band])


def _lattice(n, spacing):
    a = np.arange(n, dtype=np.float32) * np.float32(spacing)
    return np.stack(np.meshgrid(a, a, a, indexing='ij'), -1).reshape(-1, 3)


def test_evaluate_end_to_end_and_command_line(cuda, tmp_path):
    rng = np.random.default_rng(4)
    cloud = rng.uniform(0, 1, (5000, 3)).astype(np.float32)
    tol = [0.01, 0.02, 0.05]
    m = eval_cloud.evaluate(cloud, cloud, tol)
    assert all(t['accuracy'] == t['completeness'] == t['f1'] == 1.0 for t in m['tolerances'])
    assert m['mean_recon'] == m['mean_gt'] == m['median_recon'] == 0.0 and m['not_found_recon'] == m['not_found_gt'] == 0
    tau = 0.125                                         # exact in binary: the shift 1.5 tau and the lattice are exact too
    lat = _lattice(12, 5 * tau)
    shifted = lat + np.array([1.5 * tau, 0, 0], np.float32)
    m = eval_cloud.evaluate(lat, shifted, [tau, 2 * tau])
    assert [(t['accuracy'], t['completeness'], t['f1']) for t in m['tolerances']] == [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0)]
    assert m['mean_recon'] == 1.5 * tau and m['radius'] == 2 * tau
    # a transform that undoes the shift
    T = np.eye(4)
    T[0, 3] = -1.5 * tau
    m = eval_cloud.evaluate(lat, shifted, [tau], gt_transform=T)
    assert m['tolerances'][0]['f1'] == 1.0 and m['mean_gt'] == 0.0
    # the command line on files: two ground-truth files, a reconstruction with noise
    recon = (cloud[:3000] + rng.normal(0, 0.01, (3000, 3))).astype(np.float32)
    white = np.full((1, 3), 255, np.uint8)
    ply.write_ply(str(tmp_path / 'recon.ply'), recon, np.repeat(white, len(recon), 0))
    ply.write_ply(str(tmp_path / 'gt1.ply'), cloud[:2500], np.repeat(white, 2500, 0))
    ply.write_ply(str(tmp_path / 'gt2.ply'), cloud[2500:], np.repeat(white, 2500, 0))
    out = str(tmp_path / 'score' / 'cloud_eval.json')
    eval_cloud.cli(['--recon', str(tmp_path / 'recon.ply'), '--gt', str(tmp_path / 'gt1.ply'), str(tmp_path / 'gt2.ply'),
                    '--tolerances', '0.005,0.02,0.05', '--out', out, '--distances', str(tmp_path / 'dist')])
    want = eval_cloud.evaluate(recon, cloud, [0.005, 0.02, 0.05])
    with open(out) as f:
        got = json.load(f)
    assert got == json.loads(json.dumps(want))
    assert 0.0 < got['tolerances'][0]['accuracy'] < got['tolerances'][2]['accuracy'] <= 1.0
    want_d2, want_idx = CR.nearest(recon, cloud, want['radius'])
    assert np.array_equal(np.load(str(tmp_path / 'dist_d2_recon.npy')), want_d2)
    assert np.array_equal(np.load(str(tmp_path / 'dist_idx_recon.npy')), want_idx)
    assert np.load(str(tmp_path / 'dist_d2_gt.npy')).shape == (5000,)


_N_IMAGES, _H, _W = 5, 140, 200


def _write_scene_dir(root):
    """ETH3D-style scene: 5 synthetic images, ring pair.txt with two sources each."""
    from PIL import Image
    scene = os.path.join(root, 'eth3d', 'toy')
    os.makedirs(os.path.join(scene, 'images'))
    os.makedirs(os.path.join(scene, 'cams'))
    cams = synthetic.make_cams(_N_IMAGES, _H, _W, 16)
    for v in range(_N_IMAGES):
        img = np.clip(synthetic.make_images(1, _H, _W, seed=v)[0], 0, 255).astype(np.uint8)
        Image.fromarray(img[:, :, ::-1]).save(os.path.join(scene, 'images', '%08d.jpg' % v), quality=95)
        cam = cams[v].astype(np.float64).copy()
        cam[1, :2, :3] *= 4
        cam[1, 3] = (2.0, 0.05, 16, 0.0)
        P.write_cam(os.path.join(scene, 'cams', '%08d_cam.txt' % v), cam)
    with open(os.path.join(scene, 'pair.txt'), 'w') as f:
        f.write('%d\n' % _N_IMAGES)
        for v in range(_N_IMAGES):
            f.write('%d\n2 %d 1.0 %d 1.0\n' % (v, (v + 1) % _N_IMAGES, (v + 2) % _N_IMAGES))
    return scene


def test_driver_scores_the_fused_cloud(cuda, tmp_path, weights):
    root = str(tmp_path)
    _write_scene_dir(root)
    base = ['--data_root', root, '--view_num', '3', '--max_d', '16', '--max_w', '160', '--max_h', '128', '--synthetic_weights',
            '--scenes', 'toy', '--scene_cache', '--fuse', '--prob_threshold', '0.5', '--disp_threshold', '0.5', '--num_consistent', '1']
    out = {}
    try:
        for name in ('plain', 'scored'):
            FLAGS.reset()
            out[name] = os.path.join(root, 'out_' + name, 'toy')
            extra = []
            if name == 'scored':
                # ground truth: the plain run's own cloud, part of it moved, in two files
                pts, cols = ply.read_ply(os.path.join(out['plain'], 'final3d_model.ply'))
                assert len(pts) >= 100
                gt = pts.copy()
                gt[::3, 2] += np.float32(0.03)
                gt[1::3] += np.float32(50.0)
                half = len(gt) // 2
                ply.write_ply(os.path.join(root, 'gt_a.ply'), gt[:half], cols[:half])
                ply.write_ply(os.path.join(root, 'gt_b.ply'), gt[half:], cols[half:])
                extra = ['--gt_ply', os.path.join(root, 'gt_a.ply') + ',' + os.path.join(root, 'gt_b.ply')]
            E.cli(base + ['--savepath', os.path.dirname(out[name])] + extra)
    finally:
        FLAGS.reset()
        E._Pipelines.CO_RESIDENT = False
    assert not os.path.exists(os.path.join(out['plain'], 'cloud_eval.json'))
    with open(os.path.join(out['plain'], 'final3d_model.ply'), 'rb') as f, open(os.path.join(out['scored'], 'final3d_model.ply'), 'rb') as g:
        assert f.read() == g.read()
    with open(os.path.join(out['scored'], 'cloud_eval.json')) as f:
        got = json.load(f)
    after = str(tmp_path / 'after.json')
    eval_cloud.cli(['--recon', os.path.join(out['scored'], 'final3d_model.ply'), '--gt', os.path.join(root, 'gt_a.ply'),
                    os.path.join(root, 'gt_b.ply'), '--out', after])
    with open(after) as f:
        assert json.load(f) == got
    assert got['n_recon'] == got['n_gt'] >= 100 and got['not_found_gt'] > 0
    acc = [t['accuracy'] for t in got['tolerances']]
    assert 0.0 < acc[0] <= acc[2] <= acc[-1] <= 1.0
