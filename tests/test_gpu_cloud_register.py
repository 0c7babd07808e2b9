"""-m gpu: registration of a cloud to the ground truth (csrc/cloud_register.hip, ops/cloud.py, atvsnet/register_cloud.py,
eval_cloud --register / --init_cameras / --voxel).

cloud_transform and cloud_voxel_downsample are compared with the restatement (tests/cloud_register_restated.py) bit for bit;
cloud_pair_moments' count exactly and its 18 sums within the bound that the reduction's stated shape gives."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd                                   # noqa: F401
from atvsnet_amd import _lib, ops
from atvsnet_amd.atvsnet import eval_cloud, register_cloud as RC
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_register_restated as RR  # noqa: E402
import cloud_restated as CR  # noqa: E402
import colmap_model as CM  # noqa: E402

pytestmark = pytest.mark.gpu

SHIFT = (1000.0, -1000.0, 3.0)
STAGES = (0.2, 0.1, 0.05)


def _up(dev, a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def test_transform_equals_the_restatement_bit_for_bit(cuda):
    rng = np.random.default_rng(1)
    pts = (rng.normal(0, 30, (50001, 3))).astype(np.float32)
    M = RR.similarity(RR.rotation((1, -2, 0.5), 77.0), (3.5, -1e3, 0.001), 1.7)
    for T in (M, np.eye(4), np.diag([1e3, 1e3, 1e3, 1.0]), M[:3]):
        got = ops.cloud_transform(_up(cuda, pts), T).cpu().numpy()
        assert got.dtype == np.float32 and _bits(got) == _bits(RR.transform(pts, T))
    assert _bits(ops.cloud_transform(_up(cuda, pts), np.eye(4)).cpu().numpy()) == _bits(pts)
    # within one float32 ulp of the host form, whose BLAS order is not defined
    host = eval_cloud.transform_points(pts, M)
    got = ops.cloud_transform(_up(cuda, pts), M).cpu().numpy()
    assert (np.abs(got.astype(np.float64) - host.astype(np.float64)) <= np.spacing(np.abs(host))).all()
    # non-finite rows propagate as IEEE gives them
    bad = pts[:64].copy()
    bad[::5, 0], bad[1::7, 1], bad[2::9, 2] = np.nan, np.inf, -np.inf
    got, want = ops.cloud_transform(_up(cuda, bad), M).cpu().numpy(), RR.transform(bad, M)
    assert _bits(got) == _bits(want) and np.isnan(got).any() and np.isinf(got).any()
    # n = 0, and in place
    assert ops.cloud_transform(torch.zeros((0, 3), device=cuda), M).shape == (0, 3)
    d = _up(cuda, pts)
    assert ops.cloud_transform(d, M, out=d) is d and _bits(d.cpu().numpy()) == _bits(RR.transform(pts, M))


def _same_voxels(dev, pts, voxel, origin):
    want_p, want_f = RR.voxel_downsample(pts, voxel, origin)
    got_p, got_f = ops.cloud_voxel_downsample(_up(dev, pts), voxel, origin)
    got_p, got_f = got_p.cpu().numpy(), got_f.cpu().numpy()
    assert got_p.dtype == np.float32 and got_f.dtype == np.int32 and got_p.shape == want_p.shape
    assert np.array_equal(got_f, want_f) and _bits(got_p) == _bits(want_p)
    return want_p, want_f


def test_voxel_downsample_equals_the_restatement_bit_for_bit(cuda):
    rng = np.random.default_rng(2)
    pts = rng.uniform(0, 1, (30000, 3)).astype(np.float32)
    want_p, _ = _same_voxels(cuda, pts, 0.05, (0, 0, 0))
    assert 7000 < len(want_p) <= 8000                              # 20^3 voxels, nearly all occupied, several points each
    _same_voxels(cuda, pts, 0.013, (-0.5, -0.25, -1.0))
    # the default origin: the floor of the finite minimum
    got = ops.cloud_voxel_downsample(_up(cuda, pts + np.float32(7.3)), 0.05)
    want = RR.voxel_downsample(pts + np.float32(7.3), 0.05, (7, 7, 7))
    assert _bits(got[0].cpu().numpy()) == _bits(want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    # 10^4 points in one voxel
    one = (rng.uniform(0.5, 0.75, (10000, 3))).astype(np.float32)
    want_p, want_f = _same_voxels(cuda, one, 0.25, (0.5, 0.5, 0.5))
    assert len(want_p) == 1 and want_f[0] == 0
    # points exactly on voxel faces (multiples of the edge, which is a power of two)
    a = np.arange(9, dtype=np.float32) * np.float32(0.125)
    lattice = np.stack(np.meshgrid(a, a, a, indexing='ij'), -1).reshape(-1, 3)
    want_p, _ = _same_voxels(cuda, np.concatenate([lattice, lattice + np.float32(0.0625)]), 0.125, (0, 0, 0))
    assert len(want_p) == 9 ** 3
    # the shape far from the origin
    far = (RR.shape(20000, 3) + SHIFT).astype(np.float32)
    _same_voxels(cuda, far, 0.02, np.floor(far.min(axis=0)))
    # non-finite rows are dropped
    bad = pts[:5000].copy()
    bad[::7, 0], bad[3::11, 1], bad[5::13, 2] = np.nan, np.inf, -np.inf
    want_p, want_f = _same_voxels(cuda, bad, 0.1, (0, 0, 0))
    assert np.isfinite(want_p).all() and np.isfinite(bad[want_f]).all()
    got = ops.cloud_voxel_downsample(_up(cuda, np.full((6, 3), np.nan, np.float32)), 0.1)
    assert got[0].shape == (0, 3) and got[1].shape == (0,)
    # n = 0 and n = 1
    got = ops.cloud_voxel_downsample(torch.zeros((0, 3), device=cuda), 0.1)
    assert got[0].shape == (0, 3) and got[1].shape == (0,)
    _same_voxels(cuda, np.array([[0.3, 0.7, 0.2]], np.float32), 0.25, (0, 0, 0))
    # the scan runs over n + 1 counters: 2048 fill one tile of it, 2049 begin a second
    for n in (2047, 2048):
        _same_voxels(cuda, pts[:n], 0.05, (0, 0, 0))
    # a permutation of the input gives the same SET of points
    perm = rng.permutation(len(pts))
    a = ops.cloud_voxel_downsample(_up(cuda, pts), 0.05, (0, 0, 0))[0].cpu().numpy()
    b = ops.cloud_voxel_downsample(_up(cuda, pts[perm]), 0.05, (0, 0, 0))[0].cpu().numpy()
    assert _bits(a[np.lexsort(a.T)]) == _bits(b[np.lexsort(b.T)])


def test_voxel_downsample_refuses_a_cell_beyond_2_to_21(cuda):
    pts = np.array([[0.5, 0.5, 0.5], [3.0, 0.25, 0.75]], np.float32)
    with pytest.raises(ValueError, match=r'2\^21 voxels.*smallest voxel that fits') as e:
        ops.cloud_voxel_downsample(_up(cuda, pts), 1e-6, (0, 0, 0))
    fit = float(str(e.value).rsplit(' ', 1)[1])
    assert 3.0 / 2 ** 21 <= fit <= 3.0 / 2 ** 21 * 1.001
    got = ops.cloud_voxel_downsample(_up(cuda, pts), fit, (0, 0, 0))            # the voxel size it names does fit
    assert got[0].shape == (2, 3)
    with pytest.raises(ValueError, match='below the origin'):
        ops.cloud_voxel_downsample(_up(cuda, pts), 0.1, (1, 0, 0))
    # the C entry point: count -1, outputs untouched
    import ctypes
    d = _up(cuda, pts)
    out = torch.full((2, 3), -7.0, device=cuda)
    first = torch.full((2,), -7, dtype=torch.int32, device=cuda)
    count = torch.zeros(1, dtype=torch.int64, device=cuda)
    nbytes = ctypes.c_long(0)
    L = _lib.lib()
    assert L.atvs_cloud_voxel_downsample_scratch_size(ctypes.c_long(2), ctypes.byref(nbytes)) == 0
    scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=cuda)
    origin = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    rc = L.atvs_cloud_voxel_downsample(ctypes.c_void_p(d.data_ptr()), ctypes.c_long(2), ctypes.c_double(1e-6), origin,
                                       ctypes.c_void_p(scratch.data_ptr()), ctypes.c_long(nbytes.value), ctypes.c_void_p(out.data_ptr()),
                                       ctypes.c_void_p(count.data_ptr()), ctypes.c_void_p(first.data_ptr()),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0 and count.item() == -1 and (out == -7.0).all() and (first == -7).all()


def _moment_run():
    with open(_lib.HEADER) as f:
        return int(f.read().split('#define ATVS_CLOUD_MOMENT_RUN')[1].split()[0])


@pytest.mark.parametrize('m', [1, 255, 256, 257, 10 ** 6])
def test_pair_moments_within_the_bound_of_the_stated_reduction(cuda, m):
    """Each sum within (L + ceil(log2 m) + 2) * 2^-53 * sum |term| of math.fsum of the restated terms: L serial additions and then
    a tree, every addition rounding once (the header states L; the bound is derived from that shape, not tuned)."""
    L = _moment_run()
    assert L <= 64
    rng = np.random.default_rng(m)
    n = max(3, m // 2)
    shift = np.array(SHIFT)
    src = (rng.normal(0, 1, (m, 3)) + shift).astype(np.float32)
    dst = (rng.normal(0, 1, (n, 3)) + shift).astype(np.float32)
    idx = rng.integers(0, n, m).astype(np.int32)
    d2 = rng.uniform(0, 1, m).astype(np.float32)
    bound = (L + math.ceil(math.log2(m)) + 2) * 2.0 ** -53
    cases = [('all pairs', idx, np.inf, (0, 0, 0), (0, 0, 0)), ('pivots', idx, np.inf, shift + 0.25, shift - 0.5)]
    if m >= 255:
        gone = idx.copy()
        gone[rng.uniform(size=m) < 0.3] = -1
        cases += [('trim', idx, math.sqrt(0.5), shift, shift), ('idx -1', gone, np.inf, shift, shift), ('both', gone, 0.8, shift, shift)]
    for name, ix, trim, ps, pd in cases:
        count, sums, mags = RR.pair_moments(src, dst, ix, d2, trim, ps, pd)
        args = (_up(cuda, src), _up(cuda, dst), _up(cuda, ix, np.int32), _up(cuda, d2))
        got_count, got = ops.cloud_pair_moments(*args, trim=trim, pivot_src=ps, pivot_dst=pd)
        again = ops.cloud_pair_moments(*args, trim=trim, pivot_src=ps, pivot_dst=pd)
        assert got.dtype == np.float64 and got.shape == (18,)
        assert got_count == count == again[0] and _bits(got) == _bits(again[1])              # two runs: bitwise equal
        if name != 'all pairs' and name != 'pivots':
            assert 0.2 <= count / float(m) <= 0.8, name                                      # neither branch is vacuous
        excess = np.abs(got - sums) / np.maximum(bound * mags, 1e-300)
        print('m %d, %s: %d pairs, worst |error| / bound %.3f' % (m, name, count, excess.max()))
        assert (np.abs(got - sums) <= bound * mags).all(), name
    # nothing takes part; m = 0
    none = ops.cloud_pair_moments(_up(cuda, src), _up(cuda, dst), _up(cuda, np.full(m, -1), np.int32), _up(cuda, d2))
    assert none[0] == 0 and not none[1].any()
    z3, z1 = torch.zeros((0, 3), device=cuda), torch.zeros(0, device=cuda)
    none = ops.cloud_pair_moments(z3, _up(cuda, dst), z1.int(), z1)
    assert none[0] == 0 and not none[1].any()
    with pytest.raises(ValueError, match='one entry per row'):
        ops.cloud_pair_moments(_up(cuda, src), _up(cuda, dst), z1.int(), z1)


@pytest.mark.parametrize('shift', [(0.0, 0.0, 0.0), SHIFT])
@pytest.mark.parametrize('scale', [1.0, 1.03])
def test_register_recovers_the_moved_shape(cuda, shift, scale):
    """GPU against truth: every moved source coordinate within 2 ulp(float32) of the largest coordinate magnitude of its true
    partner (the bar of tests/test_cloud_register_host.py's restated ICP; there: why)."""
    gt, src, pick, M = RR.moved_pair(shift, scale)
    reg = RC.register(src, gt, with_scale=scale != 1.0, distances=STAGES, voxel=0, min_move=0, max_iterations=100)
    T = np.array(reg['matrix'])
    moved = ops.cloud_transform(_up(cuda, src), T).cpu().numpy()
    err = np.abs(moved.astype(np.float64) - gt[pick].astype(np.float64)).max()
    print('stages %s, max error %.3e, bar %.3e, |T - M| %.3e' % (reg['stages'], err, RR.ulp_bar(gt), np.abs(T - M).max()))
    assert all(s['pairs'] == len(src) and s['converged'] for s in reg['stages'])
    assert err <= RR.ulp_bar(gt)
    # half a float32 ulp of noise per coordinate (3e-5 at 1000) over an extent of ~1, before any averaging
    assert abs(reg['scale'] - scale) <= 1e-4 and (scale != 1.0 or abs(reg['scale'] - 1.0) <= 1e-12)


@pytest.mark.parametrize('with_scale', [False, True])
def test_register_equals_the_restated_icp_on_a_noisy_pair(cuda, with_scale):
    """Independent noisy samples of the shape (sigma = 0.003), 4000 ground-truth x 2000 source points: the device's matrix and the
    restated float64 ICP's agree to 1e-9 max-abs.  Search and down-sampling are exact on both sides and the moments differ by
    ~1e-16 relative, so the matrices differ by ~1e-15 per iteration; the only amplifier is a moved point whose float32 rounding
    flips (1 ulp ~ 1e-7 in one of ~1e4 coordinates: <= 1e-11 in a moment)."""
    gt = RR.shape(4000, 11, noise=0.003).astype(np.float32)
    M = RR.similarity(RR.rotation((1, 2, 3), 4.0), (0.06, -0.04, 0.05), 1.03 if with_scale else 1.0, gt.mean(axis=0).astype(np.float64))
    Mi = np.linalg.inv(M)
    src = (RR.shape(2000, 12, noise=0.003) @ Mi[:3, :3].T + Mi[:3, 3]).astype(np.float32)
    want, stages = RR.icp(src, gt, with_scale=with_scale, distances=STAGES, max_iterations=100, min_move=0.0)
    reg = RC.register(src, gt, with_scale=with_scale, distances=STAGES, voxel=0, min_move=0, max_iterations=100)
    got = np.array(reg['matrix'])
    diff = np.abs(got - want).max()
    print('GPU vs restated ICP: max |difference| %.3e; iterations %s vs %s; |T - M| %.3e' % (
        diff, [s['iterations'] for s in reg['stages']], [s[0] for s in stages], np.abs(got - M).max()))
    # it did register: far nearer to M than where it started (not exact: among noisy independent samples nearest-neighbour pairs
    # pull the scale below the true one)
    assert np.abs(got - M).max() < 0.25 * np.abs(np.eye(4) - M).max()
    assert diff <= 1e-9


def _camera_models(root, M, n=6):
    """Two COLMAP models of the same n cameras: centres C in the first, M C in the second (text and binary)."""
    rng = np.random.default_rng(5)
    sR = M[:3, :3]
    R0 = sR / np.cbrt(np.linalg.det(sR))
    cams = [(1, 'PINHOLE', 640, 480, (500.0, 500.0, 320.0, 240.0))]
    first, second = [], []
    for i in range(n):
        R = RR.rotation(rng.normal(size=3), rng.uniform(0, 180))
        C = rng.uniform(-1, 3, 3)
        first.append((i + 1, CM.rotation_quat(R), -R @ C, 1, 'img_%02d.jpg' % i, [(10.0, 20.0, 1)]))
        C2, R2 = sR @ C + M[:3, 3], R @ R0.T
        second.append((50 - i, CM.rotation_quat(R2), -R2 @ C2, 1, 'img_%02d.jpg' % i, [(10.0, 20.0, 1)]))
    a, b = os.path.join(root, 'recon_sparse'), os.path.join(root, 'gt_sparse')
    CM.write_text(a, cams, first, [(1, (0.0, 0.0, 5.0), [(1, 0)])])
    CM.write_binary(b, cams, second, [(1, (0.0, 0.0, 5.0), [(50, 0)])])
    return a, b


def _write(path, pts):
    ply.write_ply(path, pts, np.full((len(pts), 3), 255, np.uint8))


def _scores(result):
    return {k: result[k] for k in ('n_recon', 'n_gt', 'radius', 'tolerances', 'mean_recon', 'median_recon', 'mean_gt', 'median_gt',
                                   'not_found_recon', 'not_found_gt')}


def test_command_line_registers_saves_and_reloads(cuda, tmp_path):
    gt, src, pick, M = RR.moved_pair((0, 0, 0), 1.0)
    recon_ply, gt_ply = str(tmp_path / 'recon.ply'), str(tmp_path / 'gt.ply')
    _write(recon_ply, src)
    _write(gt_ply, gt)
    base = ['--recon', recon_ply, '--gt', gt_ply, '--tolerances', '0.01,0.02,0.05']
    # without the new options: the JSON of a result computed without the new keyword arguments, byte for byte
    plain = str(tmp_path / 'plain.json')
    before = eval_cloud.cli(base + ['--out', plain])
    want = str(tmp_path / 'want.json')
    eval_cloud.write_json(want, eval_cloud.evaluate(ply.read_ply_points(recon_ply), ply.read_ply_points(gt_ply), [0.01, 0.02, 0.05]))
    with open(plain, 'rb') as f, open(want, 'rb') as g:
        assert f.read() == g.read()
    assert 'registration' not in before and before['tolerances'][0]['f1'] < 0.1
    # registered
    out, saved = str(tmp_path / 'reg.json'), str(tmp_path / 'T.txt')
    after = eval_cloud.cli(base + ['--register', '--register_distances', '0.2,0.1,0.05', '--register_voxel', '0', '--save_transform', saved,
                                   '--out', out])
    print('after: %s' % after['tolerances'][0], after['registration']['stages'])
    assert all(t['accuracy'] == 1.0 for t in after['tolerances'])                # every source point is a ground-truth point
    with open(out) as f:
        assert json.load(f) == json.loads(json.dumps(after))
    T = eval_cloud.load_matrix(saved)
    assert np.array_equal(T, np.array(after['registration']['matrix'])) and np.abs(T - M).max() < 1e-3
    # the saved matrix through --init_transform, without --register: the same scores
    again = eval_cloud.cli(base + ['--init_transform', saved, '--out', str(tmp_path / 'again.json')])
    assert 'registration' not in again and _scores(again) == _scores(after)
    # the defaults (voxel down-sampling before the fit, stages from the tolerances, the default stopping rule) register too
    easy = eval_cloud.cli(base + ['--register', '--out', str(tmp_path / 'easy.json')])
    assert easy['registration']['voxel'] == 0.025 and easy['registration']['n_gt'] < len(gt)
    assert [s['distance'] for s in easy['registration']['stages']] == [0.2, 0.1, 0.05]
    assert easy['tolerances'][0]['accuracy'] > 0.99


def test_command_line_init_cameras_far_outside_the_basin(cuda, tmp_path):
    """The frames differ by 40 degrees and a scale of 2.5: ICP alone cannot; the camera centres of two COLMAP models can."""
    gt = RR.shape(40000, 7).astype(np.float32)
    M = RR.similarity(RR.rotation((0.3, -1, 2), 40.0), (5.0, -2.0, 1.0), 2.5)
    Mi = np.linalg.inv(M)
    pick = np.random.default_rng(8).permutation(len(gt))[:15000]
    src = (gt[pick].astype(np.float64) @ Mi[:3, :3].T + Mi[:3, 3]).astype(np.float32)
    a, b = _camera_models(str(tmp_path), M)
    recon_ply, gt_ply = str(tmp_path / 'recon.ply'), str(tmp_path / 'gt.ply')
    _write(recon_ply, src)
    _write(gt_ply, gt)
    base = ['--recon', recon_ply, '--gt', gt_ply, '--tolerances', '0.01,0.02,0.05']
    assert eval_cloud.cli(base + ['--out', str(tmp_path / 'plain.json')])['tolerances'][0]['f1'] < 0.1
    with pytest.raises(ValueError, match='too far off|collinear'):
        eval_cloud.cli(base + ['--register', '--with_scale', '--register_distances', '0.2,0.1,0.05', '--register_voxel', '0'])
    saved = str(tmp_path / 'T.txt')
    after = eval_cloud.cli(base + ['--register', '--with_scale', '--init_cameras', a, b, '--register_distances', '0.2,0.1,0.05',
                                   '--register_voxel', '0', '--save_transform', saved, '--out', str(tmp_path / 'reg.json')])
    print('after: %s' % after['tolerances'][0], after['registration']['stages'], after['init_cameras'])
    assert after['init_cameras']['matched_images'] == 6 and after['init_cameras']['rms'] < 1e-9
    assert all(t['accuracy'] == 1.0 for t in after['tolerances']) and abs(after['registration']['scale'] - 2.5) < 1e-4
    again = eval_cloud.cli(base + ['--init_transform', saved, '--out', str(tmp_path / 'again.json')])
    assert _scores(again) == _scores(after)


def test_voxel_scores_the_downsampled_clouds(cuda):
    gt = RR.shape(4000, 11, noise=0.003).astype(np.float32)
    recon = RR.shape(2000, 12, noise=0.003).astype(np.float32)
    tol, v = [0.005, 0.01, 0.02], 0.02
    m = eval_cloud.evaluate(recon, gt, tol, voxel=v)
    r_ds = RR.voxel_downsample(recon, v, np.floor(recon.min(axis=0)))[0]
    g_ds = RR.voxel_downsample(gt, v, np.floor(gt.min(axis=0)))[0]
    assert (m['voxel'], m['n_recon_full'], m['n_gt_full'], m['n_recon'], m['n_gt']) == (v, 2000, 4000, len(r_ds), len(g_ds))
    assert len(r_ds) < 2000 and len(g_ds) < 4000
    R = m['radius']
    assert [t['n_recon_within'] for t in m['tolerances']] == CR.counts(CR.nearest(r_ds, g_ds, R)[0], tol)
    assert [t['n_gt_within'] for t in m['tolerances']] == CR.counts(CR.nearest(g_ds, r_ds, R)[0], tol)
    full = eval_cloud.evaluate(recon, gt, tol)
    assert 'voxel' not in full and full['n_recon'] == 2000
