"""CPU: the host side of the point-cloud neighbourhoods -- the restatement (tests/cloud_knn_restated.py) against a second
formulation, the argument checks of ops.cloud_knn* (no CPU fallback), the library's new entry points, the command lines' refusals."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd                                   # noqa: F401
from atvsnet_amd import _lib, ops
from atvsnet_amd.atvsnet import clean_cloud
from atvsnet_amd.atvsnet import eval_pointcloud

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_knn_restated as KR  # noqa: E402
import cloud_restated as CR  # noqa: E402


def _tiny():
    rng = np.random.default_rng(0)
    P = rng.uniform(0, 1, (60, 3)).astype(np.float32)
    P[5] = np.nan
    P[40, 2] = np.inf
    P[17] = P[3]                                      # a duplicate position at a higher index
    Q = rng.uniform(0, 1, (25, 3)).astype(np.float32)
    Q[2, 1] = np.inf
    return P, Q


def test_restatement_against_sorted_tuples():
    P, Q = _tiny()
    for exclude, queries in ((False, Q), (True, P)):
        for k in (1, 3, 7, 32):
            a, b = KR.knn(queries, P, 0.3, k, exclude), KR.knn_by_tuples(queries, P, 0.3, k, exclude)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        count = KR.radius_count(queries, P, 0.3, exclude)
        d2, idx = KR.knn(queries, P, 0.3, 32, exclude)
        assert count.max() < 32 and np.array_equal(count, (idx >= 0).sum(axis=1)) and np.array_equal(idx >= 0, np.isfinite(d2))
    # k = 1 is the nearest neighbour of cloud_restated
    a, b = KR.knn(Q, P, 0.3, 1), CR.nearest(Q, P, 0.3)
    assert np.array_equal(a[0][:, 0], b[0]) and np.array_equal(a[1][:, 0], b[1])
    # one index is excluded, not one position: row 3's first neighbour is its duplicate 17 at distance 0, and the other way round
    d2, idx = KR.knn(P, P, 0.3, 2, True)
    assert (idx[3, 0], d2[3, 0], idx[17, 0], d2[17, 0]) == (17, 0.0, 3, 0.0)
    assert (idx[5] == -1).all() and (idx[40] == -1).all() and not (idx == 5).any() and not (idx == 40).any()
    assert KR.knn(Q, np.zeros((0, 3), np.float32), 0.3, 3)[1].tolist() == [[-1] * 3] * len(Q)


def test_restated_mean_and_stats():
    rng = np.random.default_rng(1)
    d2 = rng.uniform(0, 1, (500, 5)).astype(np.float32)
    d2[::7, 4] = np.inf
    s = KR.knn_mean(d2)
    assert np.isinf(s[::7]).all() and np.isfinite(np.delete(s, np.arange(0, 500, 7))).all()
    j = 3
    want = 0.0
    for t in range(5):
        want += float(np.sqrt(np.float64(d2[j, t])))
    assert s[j] == want / 5.0
    c, mean, std, (mag, dev) = KR.sor_stats(s)
    f = s[np.isfinite(s)]
    assert c == len(f) == 500 - len(s[::7])
    assert abs(mean - f.mean()) <= 1e-14 * abs(mean) and abs(std - np.std(f, ddof=1)) <= 1e-13 * std
    assert mag == pytest.approx(np.abs(f).sum(), rel=1e-13) and dev == pytest.approx(((f - mean) ** 2).sum(), rel=1e-12)
    assert KR.sor_stats(np.array([np.inf, 2.5]))[:3] == (1, 2.5, 0.0) and KR.sor_stats(np.zeros(0))[:3] == (0, 0.0, 0.0)


def test_restated_clean_keeps_order_and_colours():
    rng = np.random.default_rng(2)
    pts = np.concatenate([rng.uniform(0, 1, (400, 2)), rng.normal(0, 0.002, (400, 1))], 1).astype(np.float32)
    pts[100] = (0.5, 0.5, 0.4)                                              # a floater
    cols = rng.integers(0, 256, (400, 3)).astype(np.uint8)
    p, c, rows = KR.clean(pts, cols, sor=(4, 2.0, 0.3))
    assert 100 not in rows and (np.diff(rows) > 0).all() and np.array_equal(p, pts[rows]) and np.array_equal(c, cols[rows])
    p, c, rows = KR.clean(pts, cols, radius_filter=(0.2, 3))
    assert 100 not in rows and len(rows) > 390
    p, c, rows = KR.clean(pts, cols, voxel=0.1)
    assert len(p) < 400 and np.array_equal(c, cols[rows]) and (np.diff(rows) > 0).all()


def test_ops_cloud_knn_refuse_bad_arguments_no_fallback():
    P = torch.zeros(5, 3)
    g = ops.CloudGrid(torch.empty(0, dtype=torch.uint8), 5, 1.0)
    meta = ops.CloudGrid(torch.empty(0, dtype=torch.uint8, device='meta'), 5, 1.0)
    with pytest.raises(TypeError, match='CloudGrid'):
        ops.cloud_knn(P, P, 3)
    with pytest.raises(TypeError, match='CloudGrid'):
        ops.cloud_radius_count(P, P)
    with pytest.raises(RuntimeError, match='queries.*no CPU fallback'):
        ops.cloud_knn(g, P, 3)
    with pytest.raises(RuntimeError, match='queries.*no CPU fallback'):
        ops.cloud_radius_count(g, P)
    for k in (0, 33, -1, 2.5, True, None):
        with pytest.raises(ValueError, match='k: expected an integer in 1..32'):
            ops.cloud_knn(g, P, k)
    with pytest.raises(TypeError, match='queries'):
        ops.cloud_knn(g, P.double(), 3)
    with pytest.raises(ValueError, match='queries.*shape'):
        ops.cloud_knn(g, torch.empty(5, 2, device='meta'), 3)
    with pytest.raises(ValueError, match='exclude_same_index.*4 queries, 5 reference'):
        ops.cloud_knn(meta, torch.empty(4, 3, device='meta'), 3, exclude_same_index=True)
    with pytest.raises(ValueError, match='exclude_same_index'):
        ops.cloud_radius_count(meta, torch.empty(6, 3, device='meta'), exclude_same_index=True)
    with pytest.raises(RuntimeError, match='d2.*no CPU fallback'):
        ops.cloud_knn_mean(torch.zeros(4, 3))
    with pytest.raises(ValueError, match='d2: expected shape'):
        ops.cloud_knn_mean(torch.empty(4, device='meta'))
    with pytest.raises(ValueError, match='d2: expected shape'):
        ops.cloud_knn_mean(torch.empty(4, 33, device='meta'))
    with pytest.raises(TypeError, match='d2'):
        ops.cloud_knn_mean(torch.empty(4, 3, dtype=torch.float64, device='meta'))
    with pytest.raises(RuntimeError, match='s: .*no CPU fallback'):
        ops.cloud_sor_stats(torch.zeros(4, dtype=torch.float64))
    with pytest.raises(TypeError, match='s: '):
        ops.cloud_sor_stats(torch.empty(4, device='meta'))
    with pytest.raises(RuntimeError, match='points.*no CPU fallback'):
        ops.cloud_bounds(P)


def test_library_exports_the_neighbourhood_entry_points_and_checks_arguments_on_the_host():
    names = _lib.declared_symbols()
    new = ['atvs_cloud_knn_scratch_size', 'atvs_cloud_knn', 'atvs_cloud_radius_count', 'atvs_cloud_knn_mean',
           'atvs_cloud_sor_stats_scratch_size', 'atvs_cloud_sor_stats', 'atvs_cloud_bounds']
    L = _lib.lib()
    for n in new:
        assert n in names and hasattr(L, n), n
    assert _lib.header_abi_version() >= 50 and ops.CLOUD_MAX_K == 32
    assert 'cloud_knn' not in _lib.OWNS_ITS_SIMD
    flags = _lib.flags_for(os.path.join(_lib.CSRC, 'cloud_knn.hip'))
    assert '-ffp-contract=off' in flags and '-fno-slp-vectorize' in flags
    nbytes, other = ctypes.c_long(0), ctypes.c_long(0)
    lng = ctypes.c_long
    assert L.atvs_cloud_knn_scratch_size(lng(1000), lng(700), ctypes.byref(nbytes)) == 0
    assert L.atvs_cloud_nearest_scratch_size(lng(1000), lng(700), ctypes.byref(other)) == 0 and nbytes.value == other.value > 0
    assert L.atvs_cloud_knn_scratch_size(lng(10), lng((1 << 30) + 1), ctypes.byref(nbytes)) == -2
    assert L.atvs_cloud_sor_stats_scratch_size(lng(10 ** 7), ctypes.byref(nbytes)) == 0 and 0 < nbytes.value < 1 << 20
    assert L.atvs_cloud_sor_stats_scratch_size(lng(-1), ctypes.byref(nbytes)) == -2
    fake = ctypes.c_void_p(256)                     # never dereferenced: every call below is refused before a launch
    big = lng(1 << 30)
    for k in (0, 33):
        assert L.atvs_cloud_knn(fake, big, lng(10), fake, lng(10), k, 0, fake, big, fake, fake, None) == -2
        assert L.atvs_cloud_knn_mean(fake, lng(10), k, fake, None) == -2
    assert L.atvs_cloud_knn(fake, big, lng(10), fake, lng(9), 4, 1, fake, big, fake, fake, None) == -2       # the flag with m != n
    assert L.atvs_cloud_knn(fake, lng(64), lng(10), fake, lng(10), 4, 0, fake, big, fake, fake, None) == -2   # short grid
    assert L.atvs_cloud_knn(fake, big, lng(10), fake, lng(10), 4, 0, fake, lng(64), fake, fake, None) == -2   # short scratch
    assert L.atvs_cloud_radius_count(fake, big, lng(10), fake, lng(9), 1, fake, big, fake, None) == -2
    assert L.atvs_cloud_radius_count(fake, big, lng(10), fake, lng(10), 0, fake, lng(64), fake, None) == -2
    assert L.atvs_cloud_sor_stats(fake, lng(10), fake, lng(8), fake, None) == -2
    assert L.atvs_cloud_bounds(fake, lng(-1), fake, None) == -2


def test_clean_refuses_bad_steps_before_touching_a_device():
    pts = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match='at least one'):
        clean_cloud.clean(pts)
    for bad in (dict(voxel=0.0), dict(voxel=float('nan')), dict(sor=(0, 2.0, 1.0)), dict(sor=(33, 2.0, 1.0)), dict(sor=(8, 2.0)),
                dict(sor=(8, float('inf'), 1.0)), dict(sor=(8, 2.0, 0.0)), dict(radius_filter=(0.0, 3)), dict(radius_filter=(1.0, -1)),
                dict(radius_filter=(1.0, 2.5))):
        with pytest.raises(ValueError, match=list(bad)[0]):
            clean_cloud.clean(pts, **bad)


def test_command_lines_refuse(capsys):
    def refused(cli, argv, text):
        with pytest.raises(SystemExit) as e:
            cli(argv)
        assert e.value.code == 2 and text in capsys.readouterr().err

    io = ['--in', 'a.ply', '--out', 'b.ply']
    refused(clean_cloud.cli, io, 'at least one of --voxel, --sor, --radius_filter')
    refused(clean_cloud.cli, io + ['--sor', '8,2.0'], '--sor needs a horizon')
    refused(clean_cloud.cli, io + ['--sor_radius', '0.1'], '--sor_radius needs --sor')
    refused(clean_cloud.cli, io + ['--sor', '8', '--sor_radius', '0.1'], 'expected K,RATIO')
    refused(clean_cloud.cli, io + ['--sor', '40,2', '--sor_radius', '0.1'], 'k must be an integer in 1..32')
    refused(clean_cloud.cli, io + ['--radius_filter', '0.1'], 'expected R,N')
    refused(clean_cloud.cli, io + ['--voxel', '-1'], '--voxel must be positive')
    refused(clean_cloud.cli, ['--out', 'b.ply', '--voxel', '1'], '--in')
    refused(eval_pointcloud.cli, ['--scene_cache', '--clean_voxel', '0.1'], 'need --fuse')
    refused(eval_pointcloud.cli, ['--scene_cache', '--clean_radius_filter', '0.1,3'], 'need --fuse')
    refused(eval_pointcloud.cli, ['--fuse', '--clean_sor', '8,2.0'], '--clean_sor needs a horizon')
    # the default horizon is 8 voxel edges, and says so
    parser = clean_cloud.make_parser()
    args = parser.parse_args(io + ['--voxel', '0.5', '--sor', '8,2.0'])
    assert clean_cloud.options(parser, args) == {'voxel': 0.5, 'sor': (8, 2.0, 4.0)}
    assert 'a default, not a measurement' in ' '.join(parser.format_help().split())
    with pytest.raises(ValueError, match='needs fuse'):
        eval_pointcloud.run_eval_pc('out', [], clean=dict(voxel=0.1))
