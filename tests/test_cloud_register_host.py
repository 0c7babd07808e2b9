"""CPU: the host side of the registration -- the closed-form fit from points and from moments, the camera initialisation, the
restated ICP on a shape without symmetry (tests/cloud_register_restated.py), the command lines' new options, and the library's
new entry points."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd                                   # noqa: F401
from atvsnet_amd import _lib, ops
from atvsnet_amd.atvsnet import eval_cloud, register_cloud as RC

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_register_restated as RR  # noqa: E402
import colmap_model as CM  # noqa: E402

SHIFT = (1000.0, -1000.0, 3.0)


def _known(scale):
    return RR.similarity(RR.rotation((1, 2, 3), 4.0), (0.06, -0.04, 0.05), scale, (0.9, 0.5, 0.2))


def test_similarity_from_points_recovers_known_transforms():
    """Exact float64 correspondences: the only error is the round-off of a 3x3 SVD and a few products, 1e-12 is far above it."""
    rng = np.random.default_rng(1)
    P = rng.uniform(-1, 1, (200, 3))
    for scale, with_scale in ((1.0, False), (1.0, True), (1.03, True), (2.5, True)):
        M = _known(scale)
        T = RC.similarity_from_points(P, RC.apply(M, P), with_scale)
        assert np.abs(T - M).max() <= 1e-12 and np.array_equal(T[3], [0, 0, 0, 1])
    big = RR.similarity(RR.rotation((-2, 1, 0.5), 140.0), (3.0, -7.0, 0.5), 1.0)
    assert np.abs(RC.similarity_from_points(P, RC.apply(big, P)) - big).max() <= 1e-12
    # a mirrored target: the best ROTATION, never a reflection
    T = RC.similarity_from_points(P, P * np.array([1.0, 1.0, -1.0]), True)
    assert np.linalg.det(T[:3, :3]) > 0
    # a planar cloud (rank 2) is determined
    flat = P.copy()
    flat[:, 2] = 0.0
    assert np.abs(RC.similarity_from_points(flat, RC.apply(big, flat)) - big).max() <= 1e-12
    with pytest.raises(ValueError, match='at least 3'):
        RC.similarity_from_points(P[:2], P[:2])
    line = np.outer(np.linspace(0, 1, 50), [1.0, 2.0, -0.5]) + [0.3, 0.1, 0.2]
    with pytest.raises(ValueError, match='collinear'):
        RC.similarity_from_points(line, RC.apply(big, line))
    with pytest.raises(ValueError, match='collinear'):
        RC.similarity_from_points(np.tile(P[:1], (10, 1)), np.tile(P[:1], (10, 1)))


@pytest.mark.parametrize('shift,pivots', [((0, 0, 0), 'zero'), ((0, 0, 0), 'off'), (SHIFT, 'near')])
@pytest.mark.parametrize('with_scale', [False, True])
def test_similarity_from_moments_equals_the_fit_from_points(shift, pivots, with_scale):
    """The restatement's exact sums (math.fsum) through similarity_from_moments against similarity_from_points on the same pairs,
    1e-12.  Zero pivots at the origin; pivots 0.3 away from the centroid; and the cloud at (1000, -1000, 3) with pivots near it --
    what pivots are for: with zero pivots THERE the sums of products are 1e6 and their own rounding (1e-16 relative) is 1e-10 of
    the cloud's extent, which no fit can undo."""
    rng = np.random.default_rng(3)
    src = (rng.uniform(0, 1, (500, 3)) + shift).astype(np.float32)
    dst = (RC.apply(_known(1.03 if with_scale else 1.0), src.astype(np.float64) - shift) + shift).astype(np.float32)
    idx = np.arange(500, dtype=np.int32)
    idx[::7] = -1
    d2 = np.zeros(500, np.float32)
    ps, pd = {'zero': (np.zeros(3), np.zeros(3)), 'off': (np.array([0.8, 0.2, 0.5]), np.array([0.3, 0.7, 0.6])),
              'near': (np.array(shift) + 0.4, np.array(shift) + 0.6)}[pivots]
    count, sums, _ = RR.pair_moments(src, dst, idx, d2, np.inf, ps, pd)
    keep = idx >= 0
    assert count == keep.sum()
    want = RC.similarity_from_points(src[keep].astype(np.float64), dst[keep].astype(np.float64), with_scale)
    got = RC.similarity_from_moments(count, sums, ps, pd, with_scale)
    print('max |difference| %.3e' % np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-12
    # ... and the independent restated fit
    assert np.abs(got - RR.fit(src[keep].astype(np.float64), dst[keep].astype(np.float64), with_scale)).max() <= 1e-12
    with pytest.raises(ValueError, match='at least 3'):
        RC.similarity_from_moments(2, sums, ps, pd, with_scale)


def _models(tmp_path, n=7):
    """Two COLMAP models of the same cameras: the second is the first through a known similarity, written in the other format,
    with other image ids and order, one image missing and one that the first does not have."""
    rng = np.random.default_rng(5)
    M = RR.similarity(RR.rotation((0.3, -1, 2), 40.0), (5.0, -2.0, 1.0), 2.5)
    sR = M[:3, :3]
    R0 = sR / np.cbrt(np.linalg.det(sR))
    cams = [(1, 'PINHOLE', 640, 480, (500.0, 500.0, 320.0, 240.0))]
    first, second = [], []
    for i in range(n):
        R = RR.rotation(rng.normal(size=3), rng.uniform(0, 180))
        C = rng.uniform(-2, 2, 3)
        name = 'img_%02d.jpg' % i
        first.append((i + 1, CM.rotation_quat(R), -R @ C, 1, name, [(10.0, 20.0, 1)]))
        C2, R2 = sR @ C + M[:3, 3], R @ R0.T
        second.append((100 - i, CM.rotation_quat(R2), -R2 @ C2, 1, name, [(10.0, 20.0, 1)]))
    del second[2]
    R = RR.rotation((1, 0, 0), 10.0)
    second.append((200, CM.rotation_quat(R), np.array([9.0, 9.0, 9.0]), 1, 'other.jpg', [(1.0, 2.0, 1)]))
    pts = [(1, (0.0, 0.0, 5.0), [(1, 0)])]
    a, b = str(tmp_path / 'recon_sparse'), str(tmp_path / 'gt_sparse')
    CM.write_text(a, cams, first, pts)
    CM.write_binary(b, cams, second, [(1, (0.0, 0.0, 5.0), [(200, 0)])])
    return a, b, M, first, cams, pts


def test_init_from_cameras(tmp_path):
    a, b, M, first, cams, pts = _models(tmp_path)
    T, matched, rms = RC.init_from_cameras(a, b)
    print('max |T - M| %.3e, rms %.3e' % (np.abs(T - M).max(), rms))
    assert matched == 6 and np.abs(T - M).max() <= 1e-9 and rms <= 1e-9
    # fewer than 3 common names
    few = str(tmp_path / 'few')
    CM.write_text(few, cams, first[:2] + [(50, first[3][1], first[3][2], 1, 'unknown.jpg', first[3][5])], pts)
    with pytest.raises(ValueError, match='2 image names in common'):
        RC.init_from_cameras(few, b)
    # collinear centres
    line = str(tmp_path / 'line')
    imgs = [(i + 1, (1.0, 0.0, 0.0, 0.0), (-float(i), 0.0, 0.0), 1, 'img_%02d.jpg' % i, [(1.0, 2.0, 1)]) for i in range(5)]
    CM.write_text(line, cams, imgs, pts)
    with pytest.raises(ValueError, match='do not determine'):
        RC.init_from_cameras(line, line)


@pytest.mark.parametrize('shift', [(0.0, 0.0, 0.0), SHIFT])
@pytest.mark.parametrize('scale', [1.0, 1.03])
def test_restated_icp_recovers_the_moved_shape(shift, scale):
    """The float64 ICP of the restatement, stages 0.2 / 0.1 / 0.05, stopped only by an exact fixed point: every moved source
    coordinate ends within 2 ulp(float32) of the largest coordinate magnitude of its true partner (half an ulp from rounding the
    source, half from rounding the result; the fit itself is ~1e-10)."""
    gt, src, pick, M = RR.moved_pair(shift, scale)
    assert np.abs(src - gt[pick]).max() > 0.05                     # the clouds do not start aligned
    T, stages = RR.icp(src, gt, with_scale=scale != 1.0, distances=(0.2, 0.1, 0.05), max_iterations=100, min_move=0.0)
    err = np.abs(RR.transform(src, T).astype(np.float64) - gt[pick].astype(np.float64)).max()
    print('stages (iterations, pairs) %s, max error %.3e, bar %.3e, |T - M| %.3e' % (stages, err, RR.ulp_bar(gt), np.abs(T - M).max()))
    assert all(p == len(src) for _, p in stages) and stages[0][0] < 100
    assert err <= RR.ulp_bar(gt)


def test_restated_kernels_by_hand():
    T = np.array([[2.0, 0, 0, 1], [0, 0, -1, 0], [0, 1, 0, 0.5], [0, 0, 0, 1]])
    got = RR.transform([[1, 2, 3], [np.inf, 0, 0]], T)
    assert np.array_equal(got[0], np.array([3, -3, 2.5], np.float32))
    assert got[1, 0] == np.inf and np.isnan(got[1, 1]) and np.isnan(got[1, 2])          # 0 * inf, as IEEE gives it
    # two points share voxel (0,0,0) of edge 0.5 at origin 1, one is alone, a NaN row is dropped; order: lowest index
    pts = np.array([[2.25, 1.0, 1.0], [1.125, 1.25, 1.0], [np.nan, 0, 0], [1.375, 1.25, 1.25]], np.float32)
    means, first = RR.voxel_downsample(pts, 0.5, (1, 1, 1))
    assert first.tolist() == [0, 1] and np.array_equal(means, np.array([[2.25, 1, 1], [1.25, 1.25, 1.125]], np.float32))
    with pytest.raises(ValueError):
        RR.voxel_downsample(pts, 0.5, (2, 1, 1))                   # a point below the origin
    count, sums, mags = RR.pair_moments([[1, 0, 0], [0, 2, 0], [5, 5, 5]], [[0, 0, 1], [0, 3, 0]], [1, 0, -1], [0.5, 0.25, np.inf])
    assert count == 2 and sums[:6].tolist() == [1, 2, 0, 0, 3, 1] and sums[15:].tolist() == [5.0, 10.0, 0.75]
    assert sums[6:15].reshape(3, 3).tolist() == [[0, 3, 0], [0, 0, 2], [0, 0, 0]]
    assert RR.pair_moments([[1, 0, 0], [0, 2, 0]], [[0, 0, 1], [0, 3, 0]], [1, 0], [0.5, 0.25], trim=0.5)[0] == 1


def test_eval_cloud_command_line_options(capsys):
    p = eval_cloud.make_parser()
    base = ['--recon', 'a.ply', '--gt', 'b.ply']
    assert eval_cloud.register_options(p, p.parse_args(base)) == {}
    o = eval_cloud.register_options(p, p.parse_args(base + ['--register', '--with_scale', '--register_distances', '0.4,0.2,0.1',
                                                           '--register_voxel', '0.05', '--init_transform', 'T.txt',
                                                           '--save_transform', 'out.txt', '--voxel', '0.02']))
    assert o == {'register': True, 'with_scale': True, 'register_distances': [0.4, 0.2, 0.1], 'register_voxel': 0.05,
                 'init_transform_path': 'T.txt', 'save_transform_path': 'out.txt', 'voxel': 0.02}
    o = eval_cloud.register_options(p, p.parse_args(base + ['--register', '--init_cameras', 'r/sparse', 'g/sparse']))
    assert o == {'register': True, 'with_scale': False, 'init_cameras': ('r/sparse', 'g/sparse')}
    for extra, message in ((['--with_scale'], '--with_scale needs --register'),
                           (['--register_distances', '1,2'], '--register_distances needs --register'),
                           (['--register', '--register_distances', '0.1,0.2'], 'decreasing'),
                           (['--register', '--init_cameras', 'a', 'b', '--init_transform', 'T.txt'], 'choose one'),
                           (['--save_transform', 'x.txt'], '--save_transform needs'),
                           (['--voxel', '0'], '--voxel must be positive')):
        with pytest.raises(SystemExit) as e:
            eval_cloud.cli(base + extra)                           # refused before any file or device is touched
        assert e.value.code == 2 and message in capsys.readouterr().err, extra
    from atvsnet_amd.atvsnet import eval_pointcloud
    for extra, message in ((['--fuse', '--scene_cache', '--register'], '--register needs --gt_ply'),
                           (['--fuse', '--scene_cache', '--gt_ply', 'g.ply', '--with_scale'], 'need --register')):
        with pytest.raises(SystemExit) as e:
            eval_pointcloud.cli(extra)
        assert e.value.code == 2 and message in capsys.readouterr().err


def test_metrics_without_the_new_options_is_unchanged():
    inf = np.float32(np.inf)
    m = eval_cloud.metrics(np.array([0.0, 0.25, 1.0, 4.0, inf], np.float32), np.array([0.25, 0.25, inf, 0.0], np.float32), [0.5, 2.0], 2.0)
    assert m == {'n_recon': 5, 'n_gt': 4, 'radius': 2.0, 'not_found_recon': 1, 'mean_recon': 1.1, 'median_recon': 1.0,
                 'not_found_gt': 1, 'mean_gt': 0.75, 'median_gt': 0.5,
                 'tolerances': [{'tolerance': 0.5, 'accuracy': 0.4, 'completeness': 0.75, 'f1': 2 * 0.4 * 0.75 / (0.4 + 0.75),
                                 'n_recon_within': 2, 'n_gt_within': 3},
                                {'tolerance': 2.0, 'accuracy': 0.8, 'completeness': 0.75, 'f1': 2 * 0.8 * 0.75 / (0.8 + 0.75),
                                 'n_recon_within': 4, 'n_gt_within': 3}]}
    import inspect
    sig = inspect.signature(eval_cloud.evaluate)
    assert [sig.parameters[k].default for k in ('register', 'with_scale', 'register_distances', 'register_voxel', 'init_transform',
                                                'voxel')] == [False, False, None, None, None, None]


def test_ops_refuse_bad_arguments_no_fallback():
    P = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.cloud_transform(P, np.eye(4))
    with pytest.raises(ValueError, match='4x4'):
        ops.cloud_transform(torch.empty(5, 3, device='meta'), np.eye(3))
    with pytest.raises(TypeError):
        ops.cloud_transform(torch.empty(5, 3, dtype=torch.float64, device='meta'), np.eye(4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.cloud_voxel_downsample(P, 0.1, (0, 0, 0))
    for v in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='voxel'):
            ops.cloud_voxel_downsample(torch.empty(5, 3, device='meta'), v, (0, 0, 0))
    with pytest.raises(ValueError, match='origin'):
        ops.cloud_voxel_downsample(torch.empty(5, 3, device='meta'), 0.1, (0, np.nan, 0))
    idx, d2 = torch.zeros(5, dtype=torch.int32), torch.zeros(5)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.cloud_pair_moments(P, P, idx, d2)
    with pytest.raises(TypeError):
        ops.cloud_pair_moments(P.double(), P, idx, d2)
    with pytest.raises(ValueError, match='trim'):
        ops.cloud_pair_moments(P, P, idx, d2, trim=-1.0)
    with pytest.raises(ValueError, match='pivot_src'):
        ops.cloud_pair_moments(P, P, idx, d2, pivot_src=(0, 0))
    with pytest.raises(ValueError, match='decreasing'):
        RC.register(np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), distances=(0.1, 0.2))


def test_library_exports_the_registration_entry_points_and_checks_arguments_on_the_host():
    names = _lib.declared_symbols()
    L = _lib.lib()
    for n in ('atvs_cloud_transform', 'atvs_cloud_pair_moments_scratch_size', 'atvs_cloud_pair_moments',
              'atvs_cloud_voxel_downsample_scratch_size', 'atvs_cloud_voxel_downsample'):
        assert n in names and hasattr(L, n), n
    assert _lib.header_abi_version() >= 49
    src = os.path.join(_lib.CSRC, 'cloud_register.hip')
    assert src in _lib.sources() and '-ffp-contract=off' in _lib.flags_for(src) and '-fno-slp-vectorize' in _lib.flags_for(src)
    with open(_lib.HEADER) as f:
        run = int(f.read().split('#define ATVS_CLOUD_MOMENT_RUN')[1].split()[0])
    assert 1 <= run <= 64                                           # L of the issue: the longest serial run of additions
    with open(src) as f:
        text = f.read()
    for word in ('atomicAdd(float', 'atomicAdd(double', 'unsafeAtomicAdd', 'atomic_fadd', 'atomicAdd_system'):
        assert word not in text, word                               # integer atomics only
    lng, dbl = ctypes.c_long, ctypes.c_double
    nbytes = ctypes.c_long(0)
    assert L.atvs_cloud_voxel_downsample_scratch_size(lng(1000), ctypes.byref(nbytes)) == 0
    assert 0 < nbytes.value <= 40 * 2048 + 8 * 1001 + 8 * 256       # 40 B per slot of 2 n rounded up to a power of two, 8 B per point
    assert L.atvs_cloud_voxel_downsample_scratch_size(lng((1 << 30) + 1), ctypes.byref(nbytes)) == -2
    assert L.atvs_cloud_pair_moments_scratch_size(lng(10 ** 6), ctypes.byref(nbytes)) == 0
    assert 0 < nbytes.value <= 152 * (10 ** 6 // (256 * run) + 3) + 256
    assert L.atvs_cloud_pair_moments_scratch_size(lng(-1), ctypes.byref(nbytes)) == -2
    fake = ctypes.c_void_p(256)                     # never dereferenced: every call below is refused before a launch
    three = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    bad3 = (ctypes.c_double * 3)(0.0, float('inf'), 0.0)
    m12 = (ctypes.c_double * 12)(*([0.0] * 12))
    assert L.atvs_cloud_transform(fake, lng(-1), m12, fake, None) == -2
    assert L.atvs_cloud_transform(fake, lng(5), None, fake, None) == -1
    assert L.atvs_cloud_transform(None, lng(0), m12, None, None) == 0                       # n = 0: nothing launched
    assert L.atvs_cloud_pair_moments(fake, fake, lng(5), fake, fake, lng(5), dbl(-1.0), three, three, fake, lng(1 << 20), fake, None) == -3
    assert L.atvs_cloud_pair_moments(fake, fake, lng(5), fake, fake, lng(5), dbl(float('nan')), three, three, fake, lng(1 << 20), fake, None) == -3
    assert L.atvs_cloud_pair_moments(fake, fake, lng(5), fake, fake, lng(5), dbl(1.0), bad3, three, fake, lng(1 << 20), fake, None) == -3
    assert L.atvs_cloud_pair_moments(fake, fake, lng(5), fake, fake, lng(5), dbl(1.0), three, three, fake, lng(8), fake, None) == -2
    assert L.atvs_cloud_pair_moments(fake, fake, lng(5), fake, fake, lng(5), dbl(1.0), three, three, fake, lng(1 << 20), None, None) == -1
    for v in (0.0, -1.0, float('nan'), float('inf')):
        assert L.atvs_cloud_voxel_downsample(fake, lng(5), dbl(v), three, fake, lng(1 << 30), fake, fake, fake, None) == -3, v
    assert L.atvs_cloud_voxel_downsample(fake, lng(5), dbl(0.1), bad3, fake, lng(1 << 30), fake, fake, fake, None) == -3
    assert L.atvs_cloud_voxel_downsample(fake, lng(5), dbl(0.1), three, fake, lng(64), fake, fake, fake, None) == -2
    assert L.atvs_cloud_voxel_downsample(fake, lng((1 << 30) + 1), dbl(0.1), three, fake, lng(1 << 30), fake, fake, fake, None) == -2
