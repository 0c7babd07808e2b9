"""CPU: the host side of PCA normals and target-side point-to-plane registration -- the restatement
(tests/cloud_normals_restated.py) against plain loops, the step from the target-side 37 sums against a least-squares fit from
explicit rows, the comparison of the restated loops, the argument checks, the library's new entry points
and the command lines' refusals."""
import ctypes
import inspect
import math
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd                                   # noqa: F401
from atvsnet_amd import _lib, ops
from atvsnet_amd.atvsnet import cloud_normals as CN, eval_cloud, eval_pointcloud, register_cloud as RC
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_knn_restated as KR  # noqa: E402
import cloud_normals_restated as NR  # noqa: E402
import cloud_plane_restated as PR  # noqa: E402
import cloud_register_restated as RR  # noqa: E402


def test_restated_normals_against_a_plain_loop_and_by_hand():
    """Exact rational sums and an SVD instead of math.fsum and eigh: the same lines to 1e-9 on a noisy plane with padded rows, a
    non-finite point and an index past the end; the zero rows the same rows."""
    rng = np.random.default_rng(3)
    pts = np.concatenate([rng.uniform(0, 1, (300, 2)), rng.normal(0, 0.01, (300, 1))], 1).astype(np.float32) + np.float32([100, -50, 7])
    pts[17] = np.nan
    idx = KR.knn(pts, pts, 0.15, 8, exclude_same_index=True)[1]
    idx[5, 2:], idx[6, 1:], idx[7, 3] = -1, -1, 300                          # 2 samples (+ self = 3), 1 sample, past the end
    for self_counts in (False, True):
        got, var, lam, count = NR.normals(pts, pts, idx, self_counts)
        want = NR.normals_plain(pts, pts, idx, self_counts)
        zero = ~got.any(axis=1)
        assert np.array_equal(zero, ~want.any(axis=1)) and zero[17] and zero[6] and zero[7] and zero[5] == (not self_counts)
        assert (np.isnan(var) == zero).all() and (np.isnan(lam).all(axis=1) == zero).all()
        assert 250 < (~zero).sum() and np.abs(np.linalg.norm(got[~zero], axis=1) - 1.0).max() <= 1e-15
        assert NR.sin_angle(got[~zero], want[~zero]).max() <= 1e-9
        assert (np.einsum('ij,ij->i', got[~zero], want[~zero]) > 0).all()              # both canonical
        full = count == 8 + self_counts
        assert full.sum() > 250 and np.abs(got[full & ~zero, 2]).min() > 0.7             # the plane's normal is z
        assert (count[~zero] >= 3).all() and count.max() == 8 + self_counts
    # by hand: the four corners of a unit square in z = 2 around the query -> the normal is +z, variation 0
    sq = np.float32([[1, 1, 2], [-1, 1, 2], [-1, -1, 2], [1, -1, 2]])
    n, var, lam, count = NR.normals(sq, [[0, 0, 2]], [[0, 1, 2, 3]], True)
    assert n.tolist() == [[0, 0, 1]] and var[0] == 0.0 and lam[0].tolist() == [0, 4, 4] and count[0] == 5
    # the sign: towards a viewpoint below; canonical when the viewpoint lies in the plane, is out of range or absent
    for view, want in (((0, 0, -5), -1.0), ((0, 0, 9), 1.0), ((3, 3, 2), 1.0)):
        assert NR.normals(sq, [[0, 0, 2]], [[0, 1, 2, 3]], True, [view])[0][0, 2] == want
    assert NR.normals(sq, [[0, 0, 2]], [[0, 1, 2, 3]], True, [(0, 0, -5)], [-1])[0][0, 2] == 1.0
    assert NR.canonical([0.5, -0.5, 0.1]).tolist() == [0.5, -0.5, 0.1] and NR.canonical([-0.5, 0.5, 0.1]).tolist() == [0.5, -0.5, -0.1]
    # collinear and coincident integer samples: the zero normal
    line = np.float32([[k, 2 * k, -k] for k in range(6)])
    assert not NR.normals(line, line[:1], [[1, 2, 3, 4, 5]], True)[0].any()
    assert not NR.normals(np.ones((6, 3), np.float32), [[1, 1, 1]], [[1, 2, 3, 4, 5]], True)[0].any()


def _target_pairs(m, n, seed, shift=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    src = (rng.normal(0, 1, (m, 3)) + shift).astype(np.float32)
    dst = (rng.normal(0, 1, (n, 3)) + shift).astype(np.float32)
    nrm = rng.normal(0, 1, (n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    return src, dst, nrm, rng.integers(0, n, m).astype(np.int32), rng.uniform(0, 1, m).astype(np.float32)


def test_restated_target_moments_against_a_plain_loop_over_pairs():
    src, dst, nrm, idx, d2 = _target_pairs(300, 40, 1, (10.0, -20.0, 3.0))
    idx[::9], idx[5] = -1, 40
    d2[::7], d2[3] = 2.0, np.nan
    nrm[11], nrm[12, 1], nrm[13, 2] = 0.0, np.nan, np.inf
    T = RR.similarity(RR.rotation((1, -2, 0.5), 33.0), (0.3, -0.2, 0.1), 1.25, (10.0, -20.0, 3.0))
    p, trim = (10.25, -19.5, 3.125), 1.2
    sums, count = [[] for _ in range(37)], 0
    for i in range(300):
        j = int(idx[i])
        if j < 0 or j >= 40 or not float(d2[i]) <= trim * trim:
            continue
        n = [float(v) for v in nrm[j]]
        if not all(math.isfinite(v) for v in n) or not (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2] > 0.0:
            continue
        x, y, z = (float(v) for v in src[i])
        q = [(((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * z) + T[k, 3]) - p[k] for k in range(3)]
        g = [float(dst[j, k]) - p[k] for k in range(3)]
        r = ((q[0] - g[0]) * n[0] + (q[1] - g[1]) * n[1]) + (q[2] - g[2]) * n[2]
        J = [q[1] * n[2] - q[2] * n[1], q[2] * n[0] - q[0] * n[2], q[0] * n[1] - q[1] * n[0], n[0], n[1], n[2],
             (q[0] * n[0] + q[1] * n[1]) + q[2] * n[2]]
        terms = [J[a] * J[b] for a in range(7) for b in range(a, 7)] + [J[a] * r for a in range(7)] + [r * r, float(d2[i])]
        for k in range(37):
            sums[k].append(terms[k])
        count += 1
    got_count, got, mags = NR.plane_moments(src, T, dst, nrm, idx, d2, trim, p)
    assert got_count == count and 100 < count < 250 and {11, 12, 13} & set(idx.tolist())
    assert got.tolist() == [math.fsum(s) for s in sums] and mags.tolist() == [math.fsum(abs(v) for v in s) for s in sums]
    # flipping every normal changes no sum; by hand: q = (1, 2, 3), g = (1, 0, 0), n = (0, 0, 1) -> r = 3, J = [2, -1, 0, 0, 0, 1, 3]
    assert NR.plane_moments(src, T, dst, -nrm, idx, d2, trim, p)[1].tolist() == got.tolist()
    count, got, _ = NR.plane_moments([[1, 2, 3]], np.eye(4), [[1, 0, 0]], [[0, 0, 1]], [0], [0.5])
    A = np.zeros((7, 7))
    A[np.triu_indices(7)] = got[:28]
    assert count == 1 and np.array_equal(A, np.triu(np.outer([2, -1, 0, 0, 0, 1, 3], [2, -1, 0, 0, 0, 1, 3])))
    assert got[28:].tolist() == [6, -3, 0, 0, 0, 3, 9, 9, 0.5]


@pytest.mark.parametrize('shift', [(0.0, 0.0, 0.0), (1000.0, -1000.0, 3.0)])
@pytest.mark.parametrize('with_scale', [False, True])
def test_motion_from_target_plane_moments_equals_the_fit_from_rows(shift, with_scale):
    """tests/test_cloud_plane_host.py's check and bar (1e-11: condition ~1e2 after the extent scaling, squared by the normal
    equations, times 1e-16) for the target side: the restatement's exact sums through the product's unchanged host step against
    numpy.linalg.lstsq on the explicit rows [q x n, n, q . n] of the same pairs."""
    p, n = PR.shape_with_normals(600, 9)
    M = RR.similarity(RR.rotation((1, 2, 3), 2.0), (0.02, -0.01, 0.015), 1.01 if with_scale else 1.0, (1.0, 0.6, 0.4))
    src = (p + shift).astype(np.float32)
    dst, nrm = (RC.apply(M, p) + shift).astype(np.float32), (n @ M[:3, :3].T / np.cbrt(np.linalg.det(M[:3, :3]))).astype(np.float32)
    idx, d2 = np.arange(600, dtype=np.int32), np.zeros(600, np.float32)
    idx[::11] = -1
    T = RR.similarity(RR.rotation((0, 1, 0), 1.0), (0.01, 0.0, 0.0), 1.0, shift)
    pivot = np.array(shift) + (1.0, 0.6, 0.4)
    count, sums, _ = NR.plane_moments(src, T, dst, nrm, idx, d2, np.inf, pivot)
    _, _, _, r, J, _ = NR.plane_pairs(src, T, dst, nrm, idx, d2, np.inf, pivot)
    want = PR.motion_from_points(J, r, pivot, with_scale)
    got = RC.motion_from_plane_moments(count, sums, pivot, with_scale, extent=1.2)
    print('max |difference| %.3e' % np.abs(got - want).max())
    assert count == len(r) and np.abs(got - want).max() <= 1e-11
    assert np.abs(got - np.eye(4)).max() > 1e-3                                      # a real step, not the identity
    moved = RC.apply(got @ T, src.astype(np.float64))                                # one step from near the truth lands on it
    assert np.abs(((moved - dst.astype(np.float64)) * nrm.astype(np.float64))[idx >= 0].sum(axis=1)).max() < 2e-3


def test_target_plane_icp_needs_at_most_half_the_iterations_and_is_no_worse():
    """The comparison of DESIGN.md section 12.1a with the target's normals estimated by the restated PCA (k = 16, radius 0.2),
    restated loops only.  Measured: target-plane 5 + 1 + 1 iterations, corner error 3.74e-4; point-to-point 50 + 1 + 1, 2.35e-3
    (source-plane with analytic normals 5 + 1 + 1, 2.67e-4).  Every row of the 8000 has a full neighbourhood; the smallest relative
    eigen-gap (lambda_1 - lambda_0) / lambda_2 is 0.023."""
    _, src, _, M = PR.comparison_pair()
    nrm, _, lam, count, _ = NR.comparison_normals()
    (T_point, st_point), (T_plane, st_plane) = PR.comparison_point(), NR.comparison_plane_target()
    e_point, e_plane = PR.corner_error(T_point, M, src), PR.corner_error(T_plane, M, src)
    gap = ((lam[:, 1] - lam[:, 0]) / lam[:, 2]).min()
    print('point-to-point: stages %s, corner error %.3e; target-plane: stages %s, corner error %.3e; full rows %d, smallest gap %.3g' % (
        st_point, e_point, st_plane, e_plane, (count == NR.NORMAL_K + 1).sum(), gap))
    assert nrm.any(axis=1).all() and (count == NR.NORMAL_K + 1).all() and gap >= NR.GAP_FLOOR
    assert all(s[0] < 100 for s in st_point + st_plane)                              # both stopped by their rule
    assert 2 * sum(s[0] for s in st_plane) <= sum(s[0] for s in st_point)
    assert e_plane <= e_point


def test_ops_and_register_refuse_bad_arguments_no_fallback():
    P = torch.zeros(5, 3)
    idx, d2, knn = torch.zeros(5, dtype=torch.int32), torch.zeros(5), torch.zeros((5, 4), dtype=torch.int32)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.cloud_normals(P, P, knn)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.cloud_plane_moments_target(P, np.eye(4), P, P, idx, d2)
    with pytest.raises(TypeError, match='points'):
        ops.cloud_normals(P.double(), P, knn)
    for bad in (idx, torch.zeros((5, 33), dtype=torch.int32), torch.zeros((5, 0), dtype=torch.int32)):
        with pytest.raises(ValueError, match='idx: expected shape'):
            ops.cloud_normals(P, P, bad)
    with pytest.raises(TypeError, match='idx'):
        ops.cloud_normals(P, P, knn.numpy())
    with pytest.raises(TypeError, match='self_counts'):
        ops.cloud_normals(P, P, knn, self_counts=1)
    for bad in ((0, 0), np.zeros((2, 2)), (0, np.nan, 0), np.zeros((0, 3))):
        with pytest.raises(ValueError, match='viewpoints'):
            ops.cloud_normals(P, P, knn, viewpoints=bad)
    with pytest.raises(ValueError, match='view_of needs viewpoints'):
        ops.cloud_normals(P, P, knn, view_of=idx)
    with pytest.raises(TypeError, match='src'):
        ops.cloud_plane_moments_target(P.double(), np.eye(4), P, P, idx, d2)
    with pytest.raises(ValueError, match='trim'):
        ops.cloud_plane_moments_target(P, np.eye(4), P, P, idx, d2, trim=-1.0)
    with pytest.raises(ValueError, match='pivot'):
        ops.cloud_plane_moments_target(P, np.eye(4), P, P, idx, d2, pivot=(0, np.inf, 0))
    for bad in (np.eye(3), np.full((4, 4), np.nan)):
        with pytest.raises(ValueError, match='T: '):
            ops.cloud_plane_moments_target(P, bad, P, P, idx, d2)
    pts = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="normal_side must be 'source' or 'target'"):
        RC.register(pts, pts, icp='plane', normals=pts, normal_side='both')
    with pytest.raises(ValueError, match="normal_side='target' is used by icp='plane' only"):
        RC.register(pts, pts, normal_side='target')
    with pytest.raises(ValueError, match='normals= is not used'):
        RC.register(pts, pts, icp='plane', normal_side='target', normals=pts)
    with pytest.raises(ValueError, match="gt_normals are used by normal_side='target' only"):
        RC.register(pts, pts, icp='plane', normals=pts, gt_normals=pts)
    for k in (1, 33, 2.5, True):
        with pytest.raises(ValueError, match='normal_k'):
            RC.register(pts, pts, icp='plane', normal_side='target', normal_k=k)
    with pytest.raises(ValueError, match='normal_radius'):
        RC.register(pts, pts, icp='plane', normal_side='target', normal_radius=0.0)
    with pytest.raises(ValueError, match="icp='plane' needs the reconstruction's normals"):             # the source side is what it was
        RC.register(pts, pts, icp='plane')
    with pytest.raises(ValueError, match="needs register_icp='plane'"):
        eval_cloud.evaluate(pts, pts, register=True, register_normals='target')
    with pytest.raises(ValueError, match='recon_normals is not used'):
        eval_cloud.evaluate(pts, pts, register=True, register_icp='plane', register_normals='target', recon_normals=pts)
    with pytest.raises(ValueError, match="need register_normals='target'"):
        eval_cloud.evaluate(pts, pts, register=True, register_icp='plane', recon_normals=pts, register_normal_k=8)
    with pytest.raises(ValueError, match='go together'):
        eval_cloud.evaluate(pts, pts, register=True, register_icp='plane')
    with pytest.raises(ValueError, match='k: expected'):
        CN.estimate(pts, k=1, radius=1.0)
    with pytest.raises(ValueError, match='radius'):
        CN.estimate(pts, k=4)
    with pytest.raises(ValueError, match='viewpoint'):
        CN.estimate(pts, k=4, radius=1.0, viewpoint=(0, 0))
    sig = inspect.signature(RC.register).parameters
    assert sig['normal_side'].default == 'source' and sig['gt_normals'].default is None and sig['normal_k'].default == 16
    assert sig['normal_radius'].default is None and inspect.signature(eval_cloud.evaluate).parameters['register_normals'].default == 'source'


def test_library_exports_the_new_entry_points_and_checks_arguments_on_the_host():
    names = _lib.declared_symbols()
    L = _lib.lib()
    for n in ('atvs_cloud_normals', 'atvs_cloud_plane_moments_target_scratch_size', 'atvs_cloud_plane_moments_target'):
        assert n in names and hasattr(L, n), n
    assert _lib.header_abi_version() >= 56 and L.atvs_abi_version() == _lib.header_abi_version()
    lng, dbl, integer = ctypes.c_long, ctypes.c_double, ctypes.c_int
    a, b = ctypes.c_long(0), ctypes.c_long(0)
    for m in (0, 1, 4097, 1050000):
        assert L.atvs_cloud_plane_moments_target_scratch_size(lng(m), ctypes.byref(a)) == 0
        assert L.atvs_cloud_plane_moments_scratch_size(lng(m), ctypes.byref(b)) == 0 and a.value == b.value
    assert L.atvs_cloud_plane_moments_target_scratch_size(lng(-1), ctypes.byref(a)) == -2
    assert L.atvs_cloud_plane_moments_target_scratch_size(lng(5), None) == -1
    fake = ctypes.c_void_p(256)                     # never dereferenced: every call below is refused before a launch
    three = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    bad3 = (ctypes.c_double * 3)(0.0, float('inf'), 0.0)
    eye12 = (ctypes.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    nan12 = (ctypes.c_double * 12)(*([1.0] * 11 + [float('nan')]))

    def moments(m12=eye12, n=5, m=5, trim=1.0, pivot=three, scratch=fake, scratch_bytes=1 << 20, out=fake, normals=fake):
        return L.atvs_cloud_plane_moments_target(fake, m12, fake, normals, lng(n), fake, fake, lng(m), dbl(trim), pivot, scratch,
                                                 lng(scratch_bytes), out, None)
    assert moments(trim=-1.0) == -3 and moments(trim=float('nan')) == -3 and moments(pivot=bad3) == -3 and moments(m12=nan12) == -3
    assert moments(scratch_bytes=8) == -2 and moments(m=-1) == -2 and moments(n=(1 << 30) + 1) == -2
    assert moments(out=None) == -1 and moments(normals=None) == -1 and moments(pivot=None) == -1 and moments(m12=None) == -1

    def normals(points=fake, n=5, queries=fake, m=5, idx=fake, k=4, self_counts=0, views=None, n_views=0, view_of=None, out=fake):
        return L.atvs_cloud_normals(points, lng(n), queries, lng(m), idx, integer(k), integer(self_counts), views, integer(n_views),
                                    view_of, out, None, None)
    assert normals(k=0) == -2 and normals(k=33) == -2 and normals(m=-1) == -2 and normals(n=(1 << 30) + 1) == -2 and normals(n_views=-1) == -2
    assert normals(self_counts=2) == -3 and normals(n_views=1) == -3 and normals(views=fake) == -3 and normals(view_of=fake) == -3
    assert normals(queries=None) == -1 and normals(idx=None) == -1 and normals(out=None) == -1 and normals(points=None) == -1
    assert normals(m=0, queries=None, idx=None, out=None) == 0                                    # nothing to do, nothing read
    with open(os.path.join(_lib.CSRC, 'cloud_register.hip')) as f:
        text = f.read()
    assert text.count('moment_row<kPlaneSums>') == 2 and text.count('moment_fold<kPlaneSums>') == 2      # the shared tree, twice
    assert ops.cloud_normals.__doc__ and ops.cloud_plane_moments_target.__doc__


def _plys(tmp_path):
    pts = np.random.default_rng(0).uniform(0, 1, (50, 3)).astype(np.float32)
    cols = np.full((50, 3), 200, np.uint8)
    plain, with_n = str(tmp_path / 'plain.ply'), str(tmp_path / 'normals.ply')
    ply.write_ply(plain, pts, cols)
    ply.write_ply(with_n, pts, cols, np.tile(np.array([[0, 0, 1]], np.float32), (50, 1)))
    return plain, with_n


def test_command_lines_parse_and_refuse(capsys, tmp_path):
    plain, with_n = _plys(tmp_path)
    p = eval_cloud.make_parser()
    base = ['--recon', plain, '--gt', plain]
    o = eval_cloud.register_options(p, p.parse_args(base + ['--register', '--register_icp', 'plane', '--register_normals', 'target']))
    assert o == {'register': True, 'with_scale': False, 'register_icp': 'plane', 'register_normals': 'target'}       # no normals needed
    o = eval_cloud.register_options(p, p.parse_args(base + ['--register', '--register_icp', 'plane', '--register_normals', 'target',
                                                           '--register_normal_k', '8', '--register_normal_radius', '0.3']))
    assert o['register_normal_k'] == 8 and o['register_normal_radius'] == 0.3
    o = eval_cloud.register_options(p, p.parse_args(['--recon', with_n, '--gt', plain, '--register', '--register_icp', 'plane',
                                                     '--register_normals', 'source']))
    assert o == {'register': True, 'with_scale': False, 'register_icp': 'plane'}                 # source is the default: nothing new
    for argv, message in ((base + ['--register', '--register_normals', 'target'], '--register_normals target needs --register_icp plane'),
                          (base + ['--register', '--register_icp', 'point', '--register_normals', 'target'],
                           '--register_normals target needs --register_icp plane'),
                          (base + ['--register_normals', 'target'], '--register_normals needs --register'),
                          (base + ['--register', '--register_icp', 'plane', '--register_normal_k', '8'],
                           '--register_normal_k and --register_normal_radius need --register_normals target'),
                          (base + ['--register', '--register_icp', 'plane', '--register_normals', 'target', '--register_normal_k', '1'],
                           '--register_normal_k must be in 2..32'),
                          (base + ['--register', '--register_icp', 'plane', '--register_normals', 'target', '--register_normal_radius', '0'],
                           '--register_normal_radius must be positive'),
                          (base + ['--register', '--register_icp', 'plane', '--register_normals', 'both'], 'invalid choice'),
                          # the old refusal, with the new way out
                          (base + ['--register', '--register_icp', 'plane'], 'depth_fusion --normals depth'),
                          (base + ['--register', '--register_icp', 'plane'], '--register_normals target')):
        with pytest.raises(SystemExit) as e:
            eval_cloud.cli(argv)                                   # refused before a device is touched
        assert e.value.code == 2 and message in ' '.join(capsys.readouterr().err.split()), argv
    with pytest.raises(ValueError, match='--register_normals target'):
        eval_cloud.evaluate_files(plain, [plain], register=True, register_icp='plane')
    fused = ['--fuse', '--scene_cache', '--gt_ply', 'g.ply']
    for argv, message in ((fused + ['--register', '--register_icp', 'plane'], '--register_icp plane needs --fuse_normals depth'),
                          (fused + ['--register', '--register_icp', 'plane'], 'or give --register_normals target'),
                          (fused + ['--register', '--register_normals', 'target'], '--register_normals target needs --register_icp plane'),
                          (fused + ['--register_normals', 'target'], 'need --register'),
                          (fused + ['--register', '--register_icp', 'plane', '--register_normal_k', '8'], 'need --register_normals target'),
                          (fused + ['--register', '--register_icp', 'plane', '--register_normals', 'target', '--register_normal_k', '40'],
                           '--register_normal_k must be in 2..32')):
        with pytest.raises(SystemExit) as e:
            eval_pointcloud.cli(argv)
        assert e.value.code == 2 and message in ' '.join(capsys.readouterr().err.split()), argv
    ok = dict(fuse=dict(prob_threshold=0.8), gt_ply=['g.ply'])
    rules = eval_pointcloud._option_rules(register=dict(icp='plane', normal_side='target', normal_k=8), **ok)       # no fuse_normals
    assert not any(b for b, _ in rules) and len(rules) == len(eval_pointcloud._option_rules(**ok)) + 2
    with pytest.raises(ValueError, match='normal_side=target needs icp=plane'):
        eval_pointcloud.run_eval_pc('out', [], register=dict(normal_side='target'), **ok)
    # the cloud_normals tool
    q = CN.make_parser()
    assert CN.options(q, q.parse_args(['--in', plain, '--out', 'o.ply', '--radius', '0.5'])) == dict(k=16, radius=0.5, viewpoint=None)
    assert CN.options(q, q.parse_args(['--in', plain, '--out', 'o.ply', '--radius', '0.5', '--k', '8', '--viewpoint', '1,-2,3.5'])) == dict(
        k=8, radius=0.5, viewpoint=[1.0, -2.0, 3.5])
    out = str(tmp_path / 'o.ply')
    for argv, message in ((['--in', plain, '--out', out], '--radius'),
                          (['--in', plain, '--out', out, '--radius', '0'], '--radius must be positive'),
                          (['--in', plain, '--out', out, '--radius', '1', '--k', '1'], '--k must be in 2..32'),
                          (['--in', plain, '--out', out, '--radius', '1', '--viewpoint', '1,2'], '--viewpoint: expected x,y,z'),
                          (['--in', plain, '--out', out, '--radius', '1', '--viewpoint', 'a,b,c'], '--viewpoint: expected x,y,z'),
                          (['--in', str(tmp_path / 'none.ply'), '--out', out, '--radius', '1'], 'cannot read')):
        with pytest.raises(SystemExit) as e:
            CN.cli(argv)
        assert e.value.code == 2 and message in ' '.join(capsys.readouterr().err.split()), argv
    assert not os.path.exists(out)
    rep = CN.report(np.float32([[0, 0, 1], [0, 0, 0], [1, 0, 0]]), np.float32([0.25, np.nan, 0.75]), 8, 0.5, None)
    assert rep['n_zero_normals'] == 1 and rep['variation']['median'] == 0.5 and rep['n_points'] == 3
