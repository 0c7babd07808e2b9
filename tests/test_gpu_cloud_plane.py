"""-m gpu: point-to-plane registration over the source's normals (csrc/cloud_register.hip: atvs_cloud_plane_moments, ops/cloud.py,
atvsnet/register_cloud.py icp='plane', eval_cloud --register_icp plane, clean_cloud --keep_normals).

cloud_plane_moments is held to the restatement (tests/cloud_plane_restated.py): its count exactly, its 37 sums within the bound
that the reduction's stated shape gives; the loop to the restated loop."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd                                   # noqa: F401
from atvsnet_amd import _lib, ops
from atvsnet_amd.atvsnet import clean_cloud, eval_cloud, register_cloud as RC
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_knn_restated as KR  # noqa: E402
import cloud_plane_restated as PR  # noqa: E402
import cloud_register_restated as RR  # noqa: E402

pytestmark = pytest.mark.gpu

SHIFT = (1000.0, -1000.0, 3.0)
STAGES = PR.STAGES


def _up(dev, a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _moment_run():
    with open(_lib.HEADER) as f:
        return int(f.read().split('#define ATVS_CLOUD_MOMENT_RUN')[1].split()[0])


@pytest.mark.parametrize('m', [1, 255, 257, 4097, 1050000])
def test_plane_moments_within_the_bound_of_the_stated_reduction(cuda, m):
    """Each sum within (L + ceil(log2 m) + 2) * 2^-53 * sum |term| of math.fsum of the restated terms: the bound of
    tests/test_gpu_cloud_register.py for the same tree, derived from its shape.  1 050 000 pairs are 257 rows of 4096: the fold runs
    two levels.  Cloud at the origin and at (1000, -1000, 3), pivot 0 and the target's box centre (the largest m: the shifted
    cloud about its box centre only -- math.fsum over 74 columns of 600 000 terms is what takes its seconds)."""
    L = _moment_run()
    assert L <= 64 and (m < 1050000 or -(-m // (256 * L)) > 256)
    rng = np.random.default_rng(m)
    n = max(3, m // 2)
    bound = (L + math.ceil(math.log2(m)) + 2) * 2.0 ** -53
    for shift in ((0.0, 0.0, 0.0), SHIFT)[int(m == 1050000):]:
        shift = np.array(shift)
        src = (rng.normal(0, 1, (m, 3)) + shift).astype(np.float32)
        dst = (rng.normal(0, 1, (n, 3)) + shift).astype(np.float32)
        nrm = rng.normal(0, 1, (m, 3))
        nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
        idx = rng.integers(0, n, m).astype(np.int32)
        d2 = rng.uniform(0, 1, m).astype(np.float32)
        trim = np.inf
        if m >= 255:                                                                 # every way a pair can drop out
            idx[rng.uniform(size=m) < 0.15] = -1
            idx[7], trim = n, math.sqrt(0.75)
            d2[11] = np.nan
            nrm[rng.uniform(size=m) < 0.1] = 0.0
            nrm[13, 0], nrm[17, 1], nrm[19, 2] = np.nan, np.inf, -np.inf
        T = RR.similarity(RR.rotation((1, -2, 0.5), 33.0), (0.3, -0.2, 0.1), 1.25, shift)
        lo, hi = PR.box(dst)
        for pivot in ((0.0, 0.0, 0.0), (lo + hi) / 2.0)[int(m == 1050000):]:
            count, sums, mags = PR.plane_moments(src, nrm, T, dst, idx, d2, trim, pivot)
            args = (_up(cuda, src), _up(cuda, nrm), T, _up(cuda, dst), _up(cuda, idx, np.int32), _up(cuda, d2))
            got_count, got = ops.cloud_plane_moments(*args, trim=trim, pivot=pivot)
            again = ops.cloud_plane_moments(*args, trim=trim, pivot=pivot)
            assert got.dtype == np.float64 and got.shape == (37,)
            assert got_count == count == again[0] and _bits(got) == _bits(again[1])              # two runs: bitwise equal
            if m >= 255:
                assert 0.3 <= count / float(m) <= 0.7                                            # neither branch is vacuous
            else:
                assert count == 1
            excess = np.abs(got - sums) / np.maximum(bound * mags, 1e-300)
            print('m %d, shift %s, pivot %s: %d pairs, worst |error| / bound %.3f' % (m, shift.tolist(), np.asarray(pivot).tolist(), count,
                                                                                     excess.max()))
            assert (np.abs(got - sums) <= bound * mags).all()
            assert mags[:28].min() > 0 and mags[35] > 0
    # nothing takes part; m = 0; rows that do not match
    args = (_up(cuda, src), _up(cuda, nrm), T, _up(cuda, dst))
    none = ops.cloud_plane_moments(*args, _up(cuda, np.full(m, -1), np.int32), _up(cuda, d2))
    assert none[0] == 0 and not none[1].any() and none[1].shape == (37,)
    none = ops.cloud_plane_moments(args[0], torch.zeros_like(args[1]), T, args[3], _up(cuda, np.zeros(m), np.int32), _up(cuda, d2))
    assert none[0] == 0 and not none[1].any()
    none = ops.cloud_plane_moments(*args, _up(cuda, idx, np.int32), _up(cuda, np.full(m, 1.0)), trim=0.5)          # all beyond the trim
    assert none[0] == 0 and not none[1].any()
    z3, z1 = torch.zeros((0, 3), device=cuda), torch.zeros(0, device=cuda)
    none = ops.cloud_plane_moments(z3, z3, T, _up(cuda, dst), z1.int(), z1)
    assert none[0] == 0 and not none[1].any() and none[1].shape == (37,)
    with pytest.raises(ValueError, match='one entry per row'):
        ops.cloud_plane_moments(args[0], z3, T, args[3], _up(cuda, idx, np.int32), _up(cuda, d2))


@pytest.mark.parametrize('with_scale', [False, True])
def test_register_plane_equals_the_restated_loop_on_a_noisy_pair(cuda, with_scale):
    """The noisy pair of tests/test_gpu_cloud_register.py (independent samples, sigma = 0.003, 4000 ground-truth x 2000 source
    points) with unit normals about 5 degrees off (sigma 0.06 per component), the default stop rule: the same iterations per
    stage, and the matrices agree to 1e-9 max-abs -- the bar of that test for the same comparison, for the same reason (search
    exact on both sides, moments ~1e-16 relative apart; the product solves normal equations, the restatement least squares)."""
    gt, src, nrm, M = PR.sampled_pair(4000, 2000, 11, 12, 1.03 if with_scale else 1.0, noise=0.003, normal_noise=0.06)
    want, stages = PR.register_plane(src, nrm, gt, with_scale=with_scale, distances=STAGES, max_iterations=100, min_move=None)
    reg = RC.register(src, gt, with_scale=with_scale, distances=STAGES, voxel=0, max_iterations=100, icp='plane', normals=nrm)
    got = np.array(reg['matrix'])
    diff = np.abs(got - want).max()
    print('GPU vs restated loop: max |difference| %.3e; iterations %s vs %s; corner error %.3e; stages %s' % (
        diff, [s['iterations'] for s in reg['stages']], [s[0] for s in stages], PR.corner_error(got, M, src), reg['stages']))
    assert [(s['iterations'], s['pairs']) for s in reg['stages']] == stages and all(s['converged'] for s in reg['stages'])
    assert PR.corner_error(got, M, src) < 0.05 * PR.corner_error(np.eye(4), M, src)          # it did register
    assert diff <= 1e-9
    assert reg['icp'] == 'plane' and reg['with_scale'] == with_scale
    assert all(0.0 < s['plane_rmse'] <= s['rmse'] for s in reg['stages'])                    # |r| = |e . n| <= |e| per pair


def test_register_plane_recovers_the_motion_no_worse_than_point(cuda):
    """The comparison of DESIGN.md section 12.1a on the device: the iterations of the restated point-to-plane loop, stage by stage,
    and a corner error against the true motion no larger than the device's own point-to-point result on the same input."""
    gt, src, nrm, M = PR.comparison_pair()
    _, stages = PR.comparison_plane()
    common = dict(distances=STAGES, voxel=0, max_iterations=100, min_move=PR.MIN_MOVE)
    plane = RC.register(src, gt, icp='plane', normals=nrm, **common)
    point = RC.register(src, gt, **common)
    e_plane, e_point = PR.corner_error(np.array(plane['matrix']), M, src), PR.corner_error(np.array(point['matrix']), M, src)
    its = lambda reg: [s['iterations'] for s in reg['stages']]          # noqa: E731
    print('plane: iterations %s, corner error %.3e; point: iterations %s, corner error %.3e' % (its(plane), e_plane, its(point), e_point))
    assert its(plane) == [s[0] for s in stages]
    assert 2 * sum(its(plane)) <= sum(its(point))
    assert e_plane <= e_point
    # the default is the point path: the same dict, and no new key in it
    assert RC.register(src, gt, icp='point', **common) == point and 'icp' not in point and 'plane_rmse' not in point['stages'][0]


def test_register_plane_recovers_a_scale(cuda):
    gt, src, nrm, M = PR.sampled_pair(4000, 2000, 21, 22, scale=1.03)
    want, stages = PR.register_plane(src, nrm, gt, with_scale=True, distances=STAGES, max_iterations=100, min_move=PR.MIN_MOVE)
    reg = RC.register(src, gt, with_scale=True, distances=STAGES, voxel=0, max_iterations=100, min_move=PR.MIN_MOVE, icp='plane', normals=nrm)
    scale = float(np.cbrt(np.linalg.det(want[:3, :3])))
    print('scale %.12f, restated %.12f, true 1.03; stages %s' % (reg['scale'], scale, reg['stages']))
    assert [s['iterations'] for s in reg['stages']] == [s[0] for s in stages]
    assert abs(reg['scale'] - scale) <= 1e-9 and abs(reg['scale'] - 1.03) < 2e-3
    # down-sampled first: the normals follow their points (a voxel keeps its first row's), and it still registers
    easy = RC.register(src, gt, with_scale=True, distances=STAGES, icp='plane', normals=nrm)
    assert easy['voxel'] == 0.025 and easy['n_recon'] < len(src) and easy['n_gt'] < len(gt)
    assert PR.corner_error(np.array(easy['matrix']), M, src) < 0.1 * PR.corner_error(np.eye(4), M, src)
    with pytest.raises(ValueError, match='normals: 5 rows'):
        RC.register(src, gt, icp='plane', normals=nrm[:5])


def _scores(result):
    return {k: result[k] for k in ('n_recon', 'n_gt', 'radius', 'tolerances', 'mean_recon', 'median_recon', 'mean_gt', 'median_gt',
                                   'not_found_recon', 'not_found_gt')}


def test_command_line_registers_by_planes_saves_and_reloads(cuda, tmp_path):
    gt, src, nrm, M = PR.comparison_pair()
    recon_ply, gt_ply = str(tmp_path / 'recon.ply'), str(tmp_path / 'gt.ply')
    ply.write_ply(recon_ply, src, np.full((len(src), 3), 255, np.uint8), nrm)
    ply.write_ply(gt_ply, gt, np.full((len(gt), 3), 255, np.uint8))
    base = ['--recon', recon_ply, '--gt', gt_ply, '--tolerances', '0.01,0.02,0.05']
    reg = ['--register', '--register_distances', '0.2,0.1,0.05', '--register_voxel', '0']
    out, saved = str(tmp_path / 'reg.json'), str(tmp_path / 'T.txt')
    before = eval_cloud.cli(base + ['--out', str(tmp_path / 'plain.json')])
    after = eval_cloud.cli(base + reg + ['--register_icp', 'plane', '--save_transform', saved, '--out', out])
    print('before %s, after %s, %s' % (before['tolerances'][0], after['tolerances'][0], after['registration']['stages']))
    assert after['registration']['icp'] == 'plane' and 'plane_rmse' in after['registration']['stages'][0]
    assert after['tolerances'][2]['accuracy'] > 0.99 > before['tolerances'][2]['accuracy']
    assert all(a['f1'] > b['f1'] for a, b in zip(after['tolerances'], before['tolerances']))
    with open(out) as f:
        assert json.load(f) == json.loads(json.dumps(after))
    T = eval_cloud.load_matrix(saved)
    assert np.array_equal(T, np.array(after['registration']['matrix'])) and PR.corner_error(T, M, src) < 2e-3
    again = eval_cloud.cli(base + ['--init_transform', saved, '--out', str(tmp_path / 'again.json')])
    assert 'registration' not in again and _scores(again) == _scores(after)
    # without the new option, on the same file with normals: the point path's result, with no new key anywhere
    point = eval_cloud.cli(base + reg + ['--out', str(tmp_path / 'point.json')])
    want = eval_cloud.evaluate(src, gt, [0.01, 0.02, 0.05], register=True, register_distances=[0.2, 0.1, 0.05], register_voxel=0)
    assert point == want and 'icp' not in point['registration']
    assert sum(s['iterations'] for s in after['registration']['stages']) < sum(s['iterations'] for s in point['registration']['stages'])


def test_clean_keeps_the_normals_of_the_rows_that_stay(cuda, tmp_path):
    rng = np.random.default_rng(2)
    pts = np.concatenate([rng.uniform(0, 1, (4000, 2)), rng.normal(0, 0.002, (4000, 1))], 1).astype(np.float32)
    pts[100] = (0.5, 0.5, 0.4)                                              # a floater
    pts[200] = np.nan
    cols = rng.integers(0, 256, (4000, 3)).astype(np.uint8)
    nrm = rng.normal(0, 1, (4000, 3)).astype(np.float32)
    for steps in (dict(voxel=0.05), dict(sor=(4, 2.0, 0.3)), dict(voxel=0.05, sor=(4, 2.0, 0.4), radius_filter=(0.12, 3))):
        want_p, want_c, rows = KR.clean(pts, cols, **steps)
        got_p, got_c, got_n, report = clean_cloud.clean(pts, cols, normals=nrm, **steps)
        assert 0 < len(rows) < 4000 and 200 not in rows and ('sor' not in steps or 100 not in rows)
        assert _bits(got_p) == _bits(want_p) and np.array_equal(got_c, want_c)
        assert got_n.dtype == np.float32 and _bits(got_n) == _bits(nrm[rows])
        plain = clean_cloud.clean(pts, cols, **steps)                        # without normals: the three-tuple it was
        assert len(plain) == 3 and _bits(plain[0]) == _bits(got_p) and np.array_equal(plain[1], got_c) and plain[2] == report
    # the command line: --keep_normals writes them; without it the file is the cleaned cloud without normals, byte for byte
    src_ply, kept, dropped, want_ply = (str(tmp_path / n) for n in ('in.ply', 'kept.ply', 'dropped.ply', 'want.ply'))
    finite = np.isfinite(pts).all(axis=1)
    ply.write_ply(src_ply, pts[finite], cols[finite], nrm[finite])
    argv = ['--in', src_ply, '--voxel', '0.05', '--sor', '4,2.0', '--report', str(tmp_path / 'r.json')]
    clean_cloud.cli(argv + ['--out', kept, '--keep_normals'])
    clean_cloud.cli(argv + ['--out', dropped])
    want_p, want_c, rows = KR.clean(pts[finite], cols[finite], voxel=0.05, sor=(4, 2.0, 0.4))
    p, c, n = ply.read_ply_normals(kept)
    assert _bits(p) == _bits(want_p) and np.array_equal(c, want_c) and _bits(n) == _bits(nrm[finite][rows])
    ply.write_ply(want_ply, want_p, want_c)
    with open(dropped, 'rb') as f, open(want_ply, 'rb') as g:
        assert f.read() == g.read()
    assert ply.read_ply_normals(dropped)[2] is None
