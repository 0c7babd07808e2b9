"""CPU: the host side of point-to-plane registration -- the restated moments (tests/cloud_plane_restated.py) against a plain loop,
the step from 37 sums against a least-squares fit from explicit rows, the comparison of the two restated ICP loops (DESIGN.md
section 12.1a), the argument checks, the library's new entry points and the command lines' refusals."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd                                   # noqa: F401
from atvsnet_amd import _lib, ops
from atvsnet_amd.atvsnet import clean_cloud, eval_cloud, eval_pointcloud, register_cloud as RC
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_knn_restated as KR  # noqa: E402
import cloud_plane_restated as PR  # noqa: E402
import cloud_register_restated as RR  # noqa: E402


def _random_pairs(m, n, seed, shift=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    src = (rng.normal(0, 1, (m, 3)) + shift).astype(np.float32)
    dst = (rng.normal(0, 1, (n, 3)) + shift).astype(np.float32)
    nrm = rng.normal(0, 1, (m, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    idx = rng.integers(0, n, m).astype(np.int32)
    d2 = rng.uniform(0, 1, m).astype(np.float32)
    return src, nrm, dst, idx, d2


def test_shape_with_normals_is_the_shape_and_its_normals_are_the_surfaces():
    for noise in (0.0, 0.003):
        p, n = PR.shape_with_normals(3000, 5, noise)
        assert np.array_equal(p, RR.shape(3000, 5, noise))
    p, n = PR.shape_with_normals(3000, 5)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 1e-15
    for axis in range(3):                                  # floor and walls: the coordinate along the normal is 0
        on = n[:, axis] == 1.0
        assert on.sum() > 300 and not p[on, axis].any()
    ball = ~(n == 1.0).any(axis=1)
    assert ball.sum() > 100 and np.abs((p[ball] - [1.3, 0.4, 0.0]) - 0.25 * n[ball]).max() <= 1e-15
    _, noisy = PR.shape_with_normals(3000, 5, normal_noise=0.06)
    angle = np.degrees(np.arccos(np.clip((noisy * n).sum(axis=1), -1, 1)))
    assert np.abs(np.linalg.norm(noisy, axis=1) - 1.0).max() <= 1e-15 and 3.0 < angle.mean() < 6.0


def test_restated_moments_against_a_plain_loop_over_pairs():
    """Python floats, one pair at a time, the operations in the order the header states them; some pairs excluded by every rule."""
    src, nrm, dst, idx, d2 = _random_pairs(300, 40, 1, (10.0, -20.0, 3.0))
    idx[::9], idx[5] = -1, 40
    d2[::7], d2[3] = 2.0, np.nan
    nrm[11], nrm[12, 1], nrm[13, 2] = 0.0, np.nan, np.inf
    T = RR.similarity(RR.rotation((1, -2, 0.5), 33.0), (0.3, -0.2, 0.1), 1.25, (10.0, -20.0, 3.0))
    R, p, trim = PR.rotation_of(T), (10.25, -19.5, 3.125), 1.2
    sums, count = [[] for _ in range(37)], 0
    for i in range(300):
        j = int(idx[i])
        if j < 0 or j >= 40 or not float(d2[i]) <= trim * trim:
            continue
        nx, ny, nz = (float(v) for v in nrm[i])
        if not (math.isfinite(nx) and math.isfinite(ny) and math.isfinite(nz)) or not (nx * nx + ny * ny) + nz * nz > 0.0:
            continue
        x, y, z = (float(v) for v in src[i])
        q = [(((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * z) + T[k, 3]) - p[k] for k in range(3)]
        g = [float(dst[j, k]) - p[k] for k in range(3)]
        n = [(R[k, 0] * nx + R[k, 1] * ny) + R[k, 2] * nz for k in range(3)]
        r = ((q[0] - g[0]) * n[0] + (q[1] - g[1]) * n[1]) + (q[2] - g[2]) * n[2]
        J = [g[1] * n[2] - g[2] * n[1], g[2] * n[0] - g[0] * n[2], g[0] * n[1] - g[1] * n[0], n[0], n[1], n[2],
             (q[0] * n[0] + q[1] * n[1]) + q[2] * n[2]]
        terms = [J[a] * J[b] for a in range(7) for b in range(a, 7)] + [J[a] * r for a in range(7)] + [r * r, float(d2[i])]
        for k in range(37):
            sums[k].append(terms[k])
        count += 1
    got_count, got, mags = PR.plane_moments(src, nrm, T, dst, idx, d2, trim, p)
    assert got_count == count and 100 < count < 250
    assert got.tolist() == [math.fsum(s) for s in sums] and mags.tolist() == [math.fsum(abs(v) for v in s) for s in sums]
    # by hand: one pair, q = (1, 2, 3), g = (1, 0, 0), n = (0, 0, 1) -> r = 3, J = [0, -1, 0, 0, 0, 1, 3]
    count, got, _ = PR.plane_moments([[1, 2, 3]], [[0, 0, 1]], np.eye(4), [[1, 0, 0]], [0], [0.5])
    A = np.zeros((7, 7))
    A[np.triu_indices(7)] = got[:28]
    assert count == 1 and np.array_equal(A, np.triu(np.outer([0, -1, 0, 0, 0, 1, 3], [0, -1, 0, 0, 0, 1, 3])))
    assert got[28:].tolist() == [0, -3, 0, 0, 0, 3, 9, 9, 0.5]


@pytest.mark.parametrize('shift', [(0.0, 0.0, 0.0), (1000.0, -1000.0, 3.0)])
@pytest.mark.parametrize('with_scale', [False, True])
def test_motion_from_plane_moments_equals_the_fit_from_rows(shift, with_scale):
    """The restatement's exact sums through the product's normal equations against numpy.linalg.lstsq on the explicit rows of the
    same pairs.  The pairs are a shape's points against a moved copy, so the system is as well conditioned as ICP's (condition ~1e2
    after the extent scaling): normal equations square it, 1e-16 * 1e4 leaves 1e-11 with room."""
    p, n = PR.shape_with_normals(600, 9)
    M = RR.similarity(RR.rotation((1, 2, 3), 2.0), (0.02, -0.01, 0.015), 1.01 if with_scale else 1.0, (1.0, 0.6, 0.4))
    src, nrm = (p + shift).astype(np.float32), n.astype(np.float32)
    dst = (RC.apply(M, p) + shift).astype(np.float32)
    idx, d2 = np.arange(600, dtype=np.int32), np.zeros(600, np.float32)
    idx[::11] = -1
    T = RR.similarity(RR.rotation((0, 1, 0), 1.0), (0.01, 0.0, 0.0), 1.0, shift)
    pivot = np.array(shift) + (1.0, 0.6, 0.4)
    count, sums, _ = PR.plane_moments(src, nrm, T, dst, idx, d2, np.inf, pivot)
    _, _, _, r, J, _ = PR.plane_pairs(src, nrm, T, dst, idx, d2, np.inf, pivot)
    want = PR.motion_from_points(J, r, pivot, with_scale)
    got = RC.motion_from_plane_moments(count, sums, pivot, with_scale, extent=1.2)
    print('max |difference| %.3e' % np.abs(got - want).max())
    assert count == len(r) and np.abs(got - want).max() <= 1e-11
    assert np.abs(got - np.eye(4)).max() > 1e-3                                      # a real step, not the identity
    # the extent only conditions the solve
    assert np.abs(RC.motion_from_plane_moments(count, sums, pivot, with_scale, extent=100.0) - got).max() <= 1e-9
    # one exact step from the truth's neighbourhood lands on it: the pairs are exact and the motion small
    step = got @ T
    moved = RC.apply(step, src.astype(np.float64))
    assert np.abs(((moved - dst.astype(np.float64)) * (n @ step[:3, :3].T))[idx >= 0].sum(axis=1)).max() < 2e-3


def test_the_increment_is_a_proper_similarity():
    rng = np.random.default_rng(4)
    src, nrm, dst, idx, d2 = _random_pairs(400, 400, 4)
    for with_scale in (False, True):
        T = np.eye(4)
        for k in range(20):                                # twenty LARGE increments composed: random pairs never settle
            count, sums, _ = PR.plane_moments(src, nrm, T, dst, rng.integers(0, 400, 400).astype(np.int32), d2)
            try:
                D = RC.motion_from_plane_moments(count, sums, None, with_scale)
            except ValueError:                             # a step that would turn the scale negative
                continue
            s = np.cbrt(np.linalg.det(D[:3, :3]))
            R = D[:3, :3] / s
            assert s > 0 and np.abs(R.T @ R - np.eye(3)).max() <= 1e-15 and np.linalg.det(R) > 0
            assert np.array_equal(D[3], [0, 0, 0, 1]) and (with_scale or abs(s - 1.0) <= 1e-15)
            T = D @ T
        R = T[:3, :3] / np.cbrt(np.linalg.det(T[:3, :3]))
        assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-14 and np.linalg.det(T[:3, :3]) > 0
    # about the pivot: the pivot moves by t alone
    count, sums, _ = PR.plane_moments(src, nrm, np.eye(4), dst, idx, d2, np.inf, (3, 4, 5))
    D = RC.motion_from_plane_moments(count, sums, (3, 4, 5), True)
    A = np.zeros((7, 7))
    A[np.triu_indices(7)] = sums[:28]
    x = np.linalg.solve(A + np.triu(A, 1).T, -sums[28:35])
    assert np.abs(RC.apply(D, np.array([[3.0, 4.0, 5.0]]))[0] - (np.array([3, 4, 5]) + x[3:6])).max() <= 1e-12


def test_a_single_plane_and_too_few_pairs_are_refused():
    rng = np.random.default_rng(6)
    flat = np.concatenate([rng.uniform(0, 1, (300, 2)), np.zeros((300, 1))], 1).astype(np.float32)
    up = np.tile(np.array([[0, 0, 1]], np.float32), (300, 1))
    idx, d2 = np.arange(300, dtype=np.int32), np.zeros(300, np.float32)
    count, sums, _ = PR.plane_moments(flat, up, np.eye(4), flat + np.float32([0, 0, 0.01]), idx, d2, np.inf, (0.5, 0.5, 0))
    for with_scale in (False, True):
        with pytest.raises(ValueError, match="do not constrain the motion.*single plane.*icp='point'"):
            RC.motion_from_plane_moments(count, sums, (0.5, 0.5, 0), with_scale)
    # two planes still leave sliding along their common line free; the shape's three walls do not
    p, n = PR.shape_with_normals(400, 3)
    two = (n[:, 2] == 1.0) | (n[:, 1] == 1.0)
    args = (np.eye(4), p.astype(np.float32) + np.float32(0.001))
    count, sums, _ = PR.plane_moments(p[two].astype(np.float32), n[two].astype(np.float32), args[0], args[1][two],
                                      np.arange(two.sum(), dtype=np.int32), np.zeros(two.sum(), np.float32))
    with pytest.raises(ValueError, match='do not constrain'):
        RC.motion_from_plane_moments(count, sums)
    count, sums, _ = PR.plane_moments(p.astype(np.float32), n.astype(np.float32), args[0], args[1], np.arange(400, dtype=np.int32),
                                      np.zeros(400, np.float32))
    assert RC.motion_from_plane_moments(count, sums).shape == (4, 4)
    with pytest.raises(ValueError, match='5 pairs.*at least 6'):
        RC.motion_from_plane_moments(5, sums)
    with pytest.raises(ValueError, match='6 pairs.*at least 7'):
        RC.motion_from_plane_moments(6, sums, with_scale=True)
    with pytest.raises(ValueError, match='37 sums'):
        RC.motion_from_plane_moments(100, sums[:18])
    with pytest.raises(ValueError, match='extent'):
        RC.motion_from_plane_moments(count, sums, extent=0.0)


def test_plane_icp_needs_at_most_half_the_iterations_and_is_no_worse():
    """The comparison of DESIGN.md section 12.1a, restated loops only: independent samples of the shape (8000 target, 4000 source
    points, exact positions, analytic normals), moved by 4 degrees / (0.06, -0.04, 0.05), stages 0.2 / 0.1 / 0.05, both loops
    stopped when the box corners move by at most 1e-6.  Measured: point-to-point 50 + 1 + 1 iterations, corner error 2.35e-3;
    point-to-plane 5 + 1 + 1, 2.67e-4."""
    _, src, _, M = PR.comparison_pair()
    (T_point, st_point), (T_plane, st_plane) = PR.comparison_point(), PR.comparison_plane()
    e_point, e_plane = PR.corner_error(T_point, M, src), PR.corner_error(T_plane, M, src)
    print('point-to-point: stages %s, corner error %.3e; point-to-plane: stages %s, corner error %.3e' % (st_point, e_point, st_plane, e_plane))
    assert PR.corner_error(np.eye(4), M, src) > 0.1                                  # where both started
    assert all(s[0] < 100 for s in st_point + st_plane)                              # both stopped by their rule
    assert 2 * sum(s[0] for s in st_plane) <= sum(s[0] for s in st_point)
    assert e_plane <= e_point


def test_ops_and_register_refuse_bad_arguments_no_fallback():
    P = torch.zeros(5, 3)
    idx, d2 = torch.zeros(5, dtype=torch.int32), torch.zeros(5)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.cloud_plane_moments(P, P, np.eye(4), P, idx, d2)
    with pytest.raises(TypeError, match='src'):
        ops.cloud_plane_moments(P.double(), P, np.eye(4), P, idx, d2)
    with pytest.raises(ValueError, match='src'):
        ops.cloud_plane_moments(torch.zeros(5, 2), P, np.eye(4), P, idx, d2)
    with pytest.raises(TypeError, match='src'):
        ops.cloud_plane_moments(np.zeros((5, 3), np.float32), P, np.eye(4), P, idx, d2)
    with pytest.raises(ValueError, match='trim'):
        ops.cloud_plane_moments(P, P, np.eye(4), P, idx, d2, trim=float('nan'))
    with pytest.raises(ValueError, match='pivot'):
        ops.cloud_plane_moments(P, P, np.eye(4), P, idx, d2, pivot=(0, 0))
    with pytest.raises(ValueError, match='pivot'):
        ops.cloud_plane_moments(P, P, np.eye(4), P, idx, d2, pivot=(0, np.inf, 0))
    for bad in (np.eye(3), np.full((4, 4), np.nan), np.diag([1.0, 1.0, -1.0, 1.0]), np.zeros((4, 4))):
        with pytest.raises(ValueError, match='T: '):
            ops.cloud_plane_moments(P, P, bad, P, idx, d2)
    pts = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="icp='plane' needs the reconstruction's normals"):
        RC.register(pts, pts, icp='plane')
    with pytest.raises(ValueError, match="icp must be 'point' or 'plane'"):
        RC.register(pts, pts, icp='symmetric')
    with pytest.raises(ValueError, match="icp='plane' only"):
        RC.register(pts, pts, normals=pts)
    with pytest.raises(ValueError, match='go together'):
        eval_cloud.evaluate(pts, pts, register=True, register_icp='plane')
    with pytest.raises(ValueError, match='needs register=True'):
        eval_cloud.evaluate(pts, pts, register_icp='plane', recon_normals=pts)
    with pytest.raises(ValueError, match='normals: 3 rows for 4 points'):
        clean_cloud.clean(pts, voxel=0.1, normals=pts[:3])
    import inspect
    assert inspect.signature(RC.register).parameters['icp'].default == 'point'
    assert inspect.signature(eval_cloud.evaluate).parameters['register_icp'].default == 'point'


def test_library_exports_the_plane_moments_and_checks_arguments_on_the_host():
    names = _lib.declared_symbols()
    L = _lib.lib()
    for n in ('atvs_cloud_plane_moments_scratch_size', 'atvs_cloud_plane_moments'):
        assert n in names and hasattr(L, n), n
    assert _lib.header_abi_version() >= 55 and L.atvs_abi_version() == _lib.header_abi_version()
    with open(_lib.HEADER) as f:
        run = int(f.read().split('#define ATVS_CLOUD_MOMENT_RUN')[1].split()[0])
    lng, dbl = ctypes.c_long, ctypes.c_double
    nbytes = ctypes.c_long(0)
    assert L.atvs_cloud_plane_moments_scratch_size(lng(1050000), ctypes.byref(nbytes)) == 0
    rows = -(-1050000 // (256 * run))
    assert rows > 256 and 304 * (rows + 2) < nbytes.value <= 304 * (rows + 3) + 256        # two levels of rows of 38 words
    assert L.atvs_cloud_plane_moments_scratch_size(lng(-1), ctypes.byref(nbytes)) == -2
    assert L.atvs_cloud_plane_moments_scratch_size(lng((1 << 30) + 1), ctypes.byref(nbytes)) == -2
    assert L.atvs_cloud_plane_moments_scratch_size(lng(5), None) == -1
    fake = ctypes.c_void_p(256)                     # never dereferenced: every call below is refused before a launch
    three = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    bad3 = (ctypes.c_double * 3)(0.0, float('inf'), 0.0)
    eye12 = (ctypes.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    eye9 = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    nan12 = (ctypes.c_double * 12)(*([1.0] * 11 + [float('nan')]))
    inf9 = (ctypes.c_double * 9)(*([float('inf')] + [0.0] * 8))

    def call(m12=eye12, r9=eye9, n=5, m=5, trim=1.0, pivot=three, scratch=fake, scratch_bytes=1 << 20, out=fake, normals=fake):
        return L.atvs_cloud_plane_moments(fake, normals, m12, r9, fake, lng(n), fake, fake, lng(m), dbl(trim), pivot, scratch,
                                          lng(scratch_bytes), out, None)
    assert call(trim=-1.0) == -3 and call(trim=float('nan')) == -3
    assert call(pivot=bad3) == -3 and call(m12=nan12) == -3 and call(r9=inf9) == -3
    assert call(scratch_bytes=8) == -2 and call(m=-1) == -2 and call(n=(1 << 30) + 1) == -2
    assert call(out=None) == -1 and call(normals=None) == -1 and call(pivot=None) == -1 and call(m12=None) == -1 and call(r9=None) == -1
    src = os.path.join(_lib.CSRC, 'cloud_register.hip')
    with open(src) as f:
        text = f.read()
    assert 'moment_row<kPlaneSums>' in text and 'moment_fold<kPlaneSums>' in text                # the shared tree, not a copy


def _plys(tmp_path):
    pts = np.random.default_rng(0).uniform(0, 1, (50, 3)).astype(np.float32)
    cols = np.full((50, 3), 200, np.uint8)
    plain, with_n = str(tmp_path / 'plain.ply'), str(tmp_path / 'normals.ply')
    ply.write_ply(plain, pts, cols)
    ply.write_ply(with_n, pts, cols, np.tile(np.array([[0, 0, 1]], np.float32), (50, 1)))
    return plain, with_n


def test_command_lines_refuse(capsys, tmp_path):
    plain, with_n = _plys(tmp_path)
    assert ply.has_normals(with_n) and not ply.has_normals(plain)
    p = eval_cloud.make_parser()
    o = eval_cloud.register_options(p, p.parse_args(['--recon', with_n, '--gt', plain, '--register', '--register_icp', 'plane']))
    assert o == {'register': True, 'with_scale': False, 'register_icp': 'plane'}
    o = eval_cloud.register_options(p, p.parse_args(['--recon', plain, '--gt', plain, '--register', '--register_icp', 'point']))
    assert o == {'register': True, 'with_scale': False}                         # point is the default: nothing new is passed on
    for argv, message in ((['--recon', with_n, '--gt', plain, '--register_icp', 'plane'], '--register_icp needs --register'),
                          (['--recon', with_n, '--gt', plain, '--register_icp', 'point'], '--register_icp needs --register'),
                          (['--recon', plain, '--gt', plain, '--register', '--register_icp', 'plane'], 'depth_fusion --normals depth'),
                          (['--recon', str(tmp_path / 'none.ply'), '--gt', plain, '--register', '--register_icp', 'plane'], 'cannot read'),
                          (['--recon', with_n, '--gt', plain, '--register', '--register_icp', 'symmetric'], 'invalid choice')):
        with pytest.raises(SystemExit) as e:
            eval_cloud.cli(argv)                                   # refused before a device is touched
        assert e.value.code == 2 and message in ' '.join(capsys.readouterr().err.split()), argv
    with pytest.raises(ValueError, match='depth_fusion --normals depth'):
        eval_cloud.evaluate_files(plain, [plain], register=True, register_icp='plane')
    fused = ['--fuse', '--scene_cache', '--gt_ply', 'g.ply']
    for argv, message in ((fused + ['--register', '--register_icp', 'plane'], '--register_icp plane needs --fuse_normals depth'),
                          (fused + ['--register', '--register_icp', 'plane', '--fuse_normals', 'fake'],
                           '--register_icp plane needs --fuse_normals depth'),
                          (fused + ['--register_icp', 'plane', '--fuse_normals', 'depth'], '--register_icp needs --register'),
                          (fused + ['--clean_voxel', '0.1', '--clean_keep_normals'], '--clean_keep_normals needs --fuse_normals depth'),
                          (fused + ['--fuse_normals', 'depth', '--clean_keep_normals'], '--clean_keep_normals needs --clean_voxel')):
        with pytest.raises(SystemExit) as e:
            eval_pointcloud.cli(argv)
        assert e.value.code == 2 and message in ' '.join(capsys.readouterr().err.split()), argv
    with pytest.raises(ValueError, match='register icp=plane needs fuse_normals'):
        eval_pointcloud.run_eval_pc('out', [], fuse=dict(prob_threshold=0.8), gt_ply=['g.ply'], register=dict(icp='plane'))
    with pytest.raises(ValueError, match='clean_keep_normals needs clean'):
        eval_pointcloud.run_eval_pc('out', [], fuse=dict(prob_threshold=0.8), fuse_normals=dict(normals='depth'), clean_keep_normals=True)
    # given consistently, the new rows refuse nothing; not given, they are not listed
    ok = dict(fuse=dict(prob_threshold=0.8), gt_ply=['g.ply'], fuse_normals=dict(normals='depth'), clean=dict(voxel=0.1))
    rules = eval_pointcloud._option_rules(register=dict(icp='plane'), clean_keep_normals=True, **ok)
    assert not any(b for b, _ in rules) and len(rules) == len(eval_pointcloud._option_rules(**ok)) + 3
    for argv, message in ((['--in', plain, '--out', str(tmp_path / 'o.ply'), '--voxel', '0.1', '--keep_normals'], 'carries no normals'),
                          (['--in', str(tmp_path / 'none.ply'), '--out', str(tmp_path / 'o.ply'), '--voxel', '0.1', '--keep_normals'],
                           'cannot read')):
        with pytest.raises(SystemExit) as e:
            clean_cloud.cli(argv)
        assert e.value.code == 2 and message in ' '.join(capsys.readouterr().err.split()), argv
    assert not os.path.exists(str(tmp_path / 'o.ply'))


def test_restated_clean_carries_the_normals_of_the_rows_that_stay():
    """What clean(normals=) is held to on the device (tests/test_gpu_cloud_plane.py): the restated clean's surviving rows index the
    normals -- after a voxel step the row of each voxel's FIRST point, after a filter the rows its mask keeps."""
    rng = np.random.default_rng(2)
    pts = np.concatenate([rng.uniform(0, 1, (400, 2)), rng.normal(0, 0.002, (400, 1))], 1).astype(np.float32)
    pts[100] = (0.5, 0.5, 0.4)                                              # a floater
    nrm = rng.normal(0, 1, (400, 3)).astype(np.float32)
    _, _, rows = KR.clean(pts, None, voxel=0.1)
    means, first = RR.voxel_downsample(pts, 0.1, np.floor(pts.astype(np.float64).min(axis=0)))
    assert np.array_equal(rows, first) and len(rows) < 400 and np.array_equal(nrm[rows], nrm[first])
    seen = {}
    for i, cell in enumerate(map(tuple, np.floor((pts.astype(np.float64) - np.floor(pts.astype(np.float64).min(axis=0))) / 0.1).astype(int))):
        seen.setdefault(cell, i)
    assert sorted(seen.values()) == rows.tolist()                            # the first row of every voxel, by hand
    _, _, rows = KR.clean(pts, None, voxel=0.1, sor=(4, 2.0, 0.8), radius_filter=(0.3, 3))
    assert 100 not in rows and set(rows) < set(first.tolist()) and (np.diff(rows) > 0).all()
