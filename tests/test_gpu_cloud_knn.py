"""-m gpu: point-cloud neighbourhoods (csrc/cloud_knn.hip, ops.cloud_knn / cloud_radius_count / cloud_knn_mean / cloud_sor_stats /
cloud_bounds, atvsnet/clean_cloud.py, eval_pointcloud --fuse --clean_*).

Every comparison of d2, idx and counts with the brute-force restatement (tests/cloud_knn_restated.py) is exact: np.array_equal."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd                                   # noqa: F401
from atvsnet_amd import ops
from atvsnet_amd.atvsnet import clean_cloud
from atvsnet_amd.atvsnet import eval_pointcloud as E
from atvsnet_amd.flags import FLAGS
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_knn_restated as KR  # noqa: E402

pytestmark = pytest.mark.gpu

KS = (1, 3, 4, 8, 13, 16, 32)
_cache = {}


def _up(dev, a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def _same(dev, Q, Pts, R, ks, exclude=False, want=None):
    """cloud_knn for every k of ks against the restatement at max(ks) (its first k columns are the restatement at k)."""
    want = KR.knn(Q, Pts, R, max(ks), exclude) if want is None else want
    g = ops.cloud_grid(_up(dev, Pts).reshape(-1, 3), R)
    q = _up(dev, Q).reshape(-1, 3)
    for k in ks:
        d2, idx = ops.cloud_knn(g, q, k, exclude_same_index=exclude)
        assert d2.dtype == torch.float32 and idx.dtype == torch.int32 and d2.shape == idx.shape == (len(q), k)
        assert np.array_equal(d2.cpu().numpy(), want[0][:, :k]), k
        assert np.array_equal(idx.cpu().numpy(), want[1][:, :k]), k
    return want, g, q


def _random():
    """The inputs of case 1 and their restated answers at k = 32, computed once."""
    if 'random' not in _cache:
        rng = np.random.default_rng(21)
        Pts = rng.uniform(0, 4, (12000, 3)).astype(np.float32)
        J = (Pts + rng.normal(0, 0.05, Pts.shape)).astype(np.float32)
        R = 0.25
        _cache['random'] = (Pts, J, R, KR.knn(Pts, Pts, R, 32, True), KR.knn(J, Pts, R, 32, False))
    return _cache['random']


def _lattice2():
    a = np.arange(8, dtype=np.float32)
    lattice = np.stack(np.meshgrid(a, a, a, indexing='ij'), -1).reshape(-1, 3)
    return lattice, np.concatenate([lattice, lattice], 0)                  # every point again at a higher index


def test_random_cloud_equals_the_restatement(cuda):
    Pts, J, R, want_self, want_jit = _random()
    for k in (8, 16):
        for want in (want_self, want_jit):
            full = np.isfinite(want[0][:, k - 1]).mean()
            print('k = %d: share of fully found rows %.3f' % (k, full))
            assert 0.05 < full < 0.95                   # neither the padding nor the full branch is vacuous
    _same(cuda, Pts, Pts, R, KS, exclude=True, want=want_self)
    _same(cuda, J, Pts, R, KS, exclude=False, want=want_jit)


def test_k1_is_cloud_nearest_bit_for_bit(cuda):
    Pts, J, R, _, _ = _random()
    g = ops.cloud_grid(_up(cuda, Pts), R)
    for Q in (J, Pts):
        q = _up(cuda, Q)
        d2, idx = ops.cloud_knn(g, q, 1)
        nd2, nidx = ops.cloud_nearest(g, q)
        assert d2[:, 0].cpu().numpy().tobytes() == nd2.cpu().numpy().tobytes() and torch.equal(idx[:, 0], nidx)


def test_order_and_ties(cuda):
    lattice, Pts = _lattice2()
    n = len(lattice)
    for k in (4, 32):
        (d2, idx), _, _ = _same(cuda, Pts, Pts, 1.0, (k,), exclude=True)
        rows = np.arange(2 * n)
        assert np.array_equal(idx[:, 0], (rows + n) % (2 * n)) and (d2[:, 0] == 0).all()      # the duplicate, at distance 0
    d2, idx = KR.knn(Pts, Pts, 1.0, 4, True)
    inner = np.flatnonzero(((lattice > 0) & (lattice < 7)).all(axis=1))                      # six lattice neighbours, twelve with duplicates
    assert (d2[inner, 1:] == 1).all() and (idx[inner, 1:] < n).all() and (np.diff(idx[inner, 1:], axis=1) > 0).all()
    d2, idx = KR.knn(Pts, Pts, 1.0, 32, True)
    assert ((idx >= 0).sum(axis=1) <= 13).all() and ((idx >= 0).sum(axis=1)[inner] == 13).all()      # padding from column 13 on


@pytest.mark.parametrize('shift', [(0.0, 0.0, 0.0), (1000.0, -1000.0, 3.0)])
def test_trap_pairs(cuda, shift):
    """test_gpu_cloud.py::test_trap_pairs through cloud_knn: the pair at reference x = 0.5 (float32 d2 = R * R exactly: found) and the
    pair at 0.5 + 2^-20 (not found), alone and among other points."""
    s = np.array(shift, np.float32)
    qx = np.float32(0.25 - 2.0 ** -26)
    for px in (0.5, 0.5 + 2.0 ** -20):
        Q = np.array([[qx, 0, 0]], np.float32) + s
        Pts = np.array([[px, 0, 0]], np.float32) + s
        (d2, idx), _, _ = _same(cuda, Q, Pts, 0.25, (2,))
        if shift == (0.0, 0.0, 0.0):
            assert (idx[0, 0] == 0) == (px == 0.5) and idx[0, 1] == -1
        more = np.array([[0, 0, 0], [2, 2, 2], [px, 0, 0], [0.75 + 2.0 ** -20, 0, 0]], np.float32) + s
        _same(cuda, np.array([[qx, 0, 0], [0.25, 0, 0], [1.25, 2, 2]], np.float32) + s, more, 0.25, (2,))
        _same(cuda, more, np.array([[qx, 0, 0], [0.25, 0, 0]], np.float32) + s, 0.25, (2,))


@pytest.mark.parametrize('nearer_later', [True, False])
def test_adversarial_arrival(cuda, nearer_later):
    """3000 reference points in one cell, all within 0.2 R of the query; by index ever nearer (every candidate enters the k best) or
    ever further (only the first ones do)."""
    R = 1.0
    rng = np.random.default_rng(6)
    dist = np.sort(rng.uniform(0.01, 0.2, 3000))
    if nearer_later:
        dist = dist[::-1]
    v = rng.normal(size=(3000, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    centre = np.array([0.5, 0.5, 0.5])
    Pts = (centre + v * dist[:, None]).astype(np.float32)
    Q = np.array([centre, centre + 0.01], np.float32)
    (d2, idx), g, _ = _same(cuda, Q, Pts, R, (32, 5))
    order = np.argsort(idx[0]) if nearer_later else np.argsort(-idx[0])
    assert (idx >= 0).all() and np.array_equal(order, np.arange(32)[::-1])          # the arrival order really is adversarial
    # the reference points as queries of their own cloud: every lane of many wavefronts walks the same 3000 records
    _same(cuda, Pts[:300], Pts, R, (32,))


def test_edges(cuda):
    rng = np.random.default_rng(11)
    Pts = rng.uniform(-1, 1, (3000, 3)).astype(np.float32)
    Q = rng.uniform(-1.2, 1.2, (2500, 3)).astype(np.float32)
    Pts[::7, 0], Pts[3::11, 1], Pts[5::13, 2] = np.nan, np.inf, -np.inf
    Q[::9, 2], Q[4::10, 0], Q[1::17, 1] = np.nan, -np.inf, np.inf
    (d2, idx), _, _ = _same(cuda, Q, Pts, 0.15, (6, 32))
    assert np.isfinite(d2[:, 5]).any() and np.isinf(d2[::9]).all() and np.isinf(d2).any()
    _same(cuda, Pts, Pts, 0.15, (6,), exclude=True)
    empty = np.zeros((0, 3), np.float32)
    _same(cuda, Q, empty, 0.15, (3,))                                      # n = 0
    _same(cuda, empty, empty, 0.15, (3,), exclude=True)
    d2, idx = ops.cloud_knn(ops.cloud_grid(_up(cuda, Pts), 0.15), _up(cuda, empty), 5)       # m = 0
    assert d2.shape == idx.shape == (0, 5)
    assert ops.cloud_radius_count(ops.cloud_grid(_up(cuda, Pts), 0.15), _up(cuda, empty)).shape == (0,)
    _same(cuda, Q, np.full((5, 3), np.nan, np.float32), 0.15, (3,))        # no finite reference point
    few = rng.uniform(0, 0.1, (6, 3)).astype(np.float32)
    (d2, idx), _, _ = _same(cuda, few[:3] + np.float32(0.01), few[:5], 1.0, (5,))               # n = k: every row full
    assert (idx >= 0).all()
    (d2, idx), _, _ = _same(cuda, few, few, 1.0, (5,), exclude=True)                            # n = k + 1 with exclusion: full
    assert (idx >= 0).all() and (idx != np.arange(6)[:, None]).all()
    (d2, idx), _, _ = _same(cuda, few[:5], few[:5], 1.0, (5,), exclude=True)                    # n = k with exclusion: one padded
    assert ((idx >= 0).sum(axis=1) == 4).all()
    far = (Pts + np.array([1000, -1000, 3], np.float32)).astype(np.float32)
    (d2, idx), _, _ = _same(cuda, far, far, 0.15, (8,), exclude=True)
    assert np.isfinite(d2[:, 0]).mean() > 0.3


def test_radius_count(cuda):
    Pts, J, R, want_self, want_jit = _random()
    lattice, twice = _lattice2()
    cases = [(Pts, Pts, R, True, want_self), (J, Pts, R, False, want_jit), (twice, twice, 1.0, True, KR.knn(twice, twice, 1.0, 32, True))]
    for Q, P_, r, exclude, knn in cases:
        want = KR.radius_count(Q, P_, r, exclude)
        g, q = ops.cloud_grid(_up(cuda, P_), r), _up(cuda, Q)
        got = ops.cloud_radius_count(g, q, exclude_same_index=exclude)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
        for k in (8, 32):
            idx = ops.cloud_knn(g, q, k, exclude_same_index=exclude)[1].cpu().numpy()
            assert np.array_equal(idx, knn[1][:, :k])
            low = want <= k
            assert low.any() and np.array_equal((idx >= 0).sum(axis=1)[low], want[low])
            assert ((idx >= 0).sum(axis=1)[~low] == k).all()
    assert want.max() == 13 and want.min() == 7                            # the doubled lattice: corner 2 * 3 + 1, inner 2 * 6 + 1


def _stat_bar(m, L=16):
    return (L + math.ceil(math.log2(max(m, 2))) + 2) * 2.0 ** -53


def test_knn_mean_and_sor_stats(cuda):
    Pts, J, R, want_self, _ = _random()
    g, q = ops.cloud_grid(_up(cuda, Pts), R), _up(cuda, Pts)
    last = None
    for k in (1, 5, 8, 16, 32):
        d2 = ops.cloud_knn(g, q, k, exclude_same_index=True)[0]
        s = ops.cloud_knn_mean(d2)
        assert s.dtype == torch.float64 and s.shape == (len(Pts),)
        got, want = s.cpu().numpy(), KR.knn_mean(want_self[0][:, :k])
        inf = np.isinf(want)
        assert np.array_equal(np.isinf(got), inf) and not np.isnan(got).any()
        # one rounding per square root, per addition and for the division
        rel = np.abs(got[~inf] - want[~inf]) / want[~inf]
        print('k = %d: knn_mean worst relative difference %.3g, bar %.3g' % (k, rel.max() if rel.size else 0.0, (k + 2) * 2.0 ** -52))
        assert (rel <= (k + 2) * 2.0 ** -52).all()
        if k == 8:
            last = s
    # the statistics of the k = 8 column (a mix of finite and +inf entries), and of inputs that take one, two and three fold passes
    rng = np.random.default_rng(4)
    big = rng.uniform(0.5, 1.5, 1100000)
    big[::5] = np.inf
    for name, s in (('k8', last), ('tiny', _up(cuda, [np.inf, 2.5], np.float64)), ('one', _up(cuda, [1.0, 2.0, 4.0], np.float64)),
                    ('rows2', _up(cuda, big[:5000], np.float64)), ('rows269', _up(cuda, big, np.float64))):
        host = s.cpu().numpy()
        c, mean, std = ops.cloud_sor_stats(s)
        again = ops.cloud_sor_stats(s)
        assert (c, mean, std) == again and isinstance(c, int) and isinstance(mean, float)       # bit-equal
        f = host[np.isfinite(host)]
        wc, wmean, wstd, (mag, _) = KR.sor_stats(host)
        assert c == wc == len(f)
        bar = _stat_bar(len(host))
        # the mean: the sum within bar * sum |s| of math.fsum, one more rounding for each side's division
        print('%s: mean %.17g (fsum %.17g), std %.17g (fsum %.17g)' % (name, mean, wmean, std, wstd))
        assert abs(mean - wmean) <= (bar * mag + 2 * 2.0 ** -53 * abs(math.fsum(f.tolist()))) / c
        if c < 2:
            assert std == 0.0
            continue
        # the deviations about the DEVICE's mean, the terms formed as the kernel forms them; their sum within bar * sum |term| of
        # math.fsum; then a division, a root (which halves a relative error) and this test's own squaring and product: 4 roundings
        terms = ((f - mean) * (f - mean)).tolist()
        dev = math.fsum(terms)
        assert abs(std * std * (c - 1) - dev) <= (bar + 6 * 2.0 ** -53) * dev
    assert ops.cloud_sor_stats(torch.zeros(0, dtype=torch.float64, device=cuda)) == (0, 0.0, 0.0)
    assert ops.cloud_sor_stats(_up(cuda, [np.inf, 2.5], np.float64)) == (1, 2.5, 0.0)
    assert ops.cloud_sor_stats(_up(cuda, [1.0, 2.0, 4.0], np.float64))[:2] == (3, 7.0 / 3.0)


def _patch():
    """A noisy plane patch of 6000 points (sigma 0.002) and 120 floaters at least 0.1 above it, shuffled, with colours."""
    rng = np.random.default_rng(1)
    plane = np.concatenate([rng.uniform(0, 1, (6000, 2)), rng.normal(0, 0.002, (6000, 1))], 1)
    floaters = np.concatenate([rng.uniform(0, 1, (120, 2)), rng.uniform(0.1, 0.6, (120, 1))], 1)
    pts = np.concatenate([plane, floaters], 0).astype(np.float32)
    perm = rng.permutation(len(pts))
    cols = rng.integers(0, 256, (len(pts), 3)).astype(np.uint8)
    return pts[perm], cols, perm >= 6000


@pytest.mark.parametrize('steps', [dict(sor=(8, 2.0, 0.05)), dict(voxel=0.01, sor=(8, 2.0, 0.05)), dict(radius_filter=(0.05, 4))],
                         ids=['sor', 'voxel_sor', 'radius_filter'])
def test_clean_on_a_plane_patch_with_floaters(cuda, steps):
    pts, cols, is_floater = _patch()
    detail = {}
    want_p, want_c, rows = KR.clean(pts, cols, detail=detail, **steps)
    # conditions of the test, properties of the restatement alone: every floater goes, and no row's s lies within 1e-9 relative of
    # the threshold -- which is what lets the device's mask be compared exactly
    assert not is_floater[rows].any() and len(rows) > 4900
    if 'sor' in steps:
        s, thr = detail['s'], detail['threshold']
        assert np.abs(s[np.isfinite(s)] - thr).min() > 1e-9 * thr
    got_p, got_c, report = clean_cloud.clean(pts, cols, device=cuda, **steps)
    assert got_p.dtype == np.float32 and got_c.dtype == np.uint8
    assert np.array_equal(got_p, want_p) and np.array_equal(got_c, want_c)
    assert (report['n_in'], report['n_out']) == (len(pts), len(want_p)) and [s['step'] for s in report['steps']] == list(steps)
    assert report['steps'][0]['rows_in'] == len(pts) and report['steps'][-1]['rows_out'] == len(want_p)
    for a, b in zip(report['steps'], report['steps'][1:]):
        assert a['rows_out'] == b['rows_in']
    if 'sor' in steps:
        r = report['steps'][-1]
        assert r['count'] == detail['count'] and r['threshold'] == r['mean'] + 2.0 * r['std']
        assert abs(r['threshold'] - detail['threshold']) <= 1e-12 * detail['threshold']
    json.dumps(report)
    if 'voxel' not in steps:
        assert np.array_equal(got_p, pts[rows])
    none_p, none_c, _ = clean_cloud.clean(pts, None, device=cuda, **steps)
    assert none_c is None and np.array_equal(none_p, want_p)


def test_clean_command_line(cuda, tmp_path):
    pts, cols, _ = _patch()
    src, out, rep = str(tmp_path / 'in.ply'), str(tmp_path / 'o' / 'out.ply'), str(tmp_path / 'o' / 'clean.json')
    ply.write_ply(src, pts, cols)
    clean_cloud.cli(['--in', src, '--out', out, '--voxel', '0.01', '--sor', '8,2.0', '--radius_filter', '0.05,4', '--report', rep])
    want_p, want_c, _ = clean_cloud.clean(pts, cols, voxel=0.01, sor=(8, 2.0, 0.08), radius_filter=(0.05, 4), device=cuda)
    got_p, got_c = ply.read_ply(out)
    assert np.array_equal(got_p, want_p) and np.array_equal(got_c, want_c)
    with open(rep) as f:
        report = json.load(f)
    assert report['steps'][1]['radius'] == 0.08 and report['n_out'] == len(want_p)


def test_bounds(cuda):
    rng = np.random.default_rng(11)
    Pts = rng.uniform(-1, 1, (3000, 3)).astype(np.float32)
    Pts[::7, 0], Pts[3::11, 1], Pts[5::13, 2] = np.nan, np.inf, -np.inf
    far = (Pts + np.array([1000, -1000, 3], np.float32)).astype(np.float32)
    big = rng.normal(0, 50, (700001, 3)).astype(np.float32)                # more points than one pass of 2048 workgroups covers
    for cloud in (Pts, far, big, Pts[1:2], np.array([[-0.0, 0.0, 5.0], [np.nan, 1, 1]], np.float32)):
        lo, hi = ops.cloud_bounds(_up(cuda, cloud))
        ok = cloud[np.isfinite(cloud).all(axis=1)].astype(np.float64)
        assert lo.dtype == hi.dtype == np.float64 and lo.shape == hi.shape == (3,)
        assert np.array_equal(lo, ok.min(axis=0)) and np.array_equal(hi, ok.max(axis=0))
    for cloud in (np.zeros((0, 3), np.float32), np.full((5, 3), np.nan, np.float32), np.array([[1, np.inf, 2]], np.float32)):
        assert ops.cloud_bounds(_up(cuda, cloud).reshape(-1, 3)) == (None, None)


def test_driver_cleans_the_fused_cloud(cuda, tmp_path, weights):
    """eval_pointcloud --fuse --clean_* on the tiny synthetic scene of test_gpu_fusion_scene.py."""
    from test_gpu_fusion_scene import _write_scene_dir
    root = str(tmp_path)
    _write_scene_dir(root)
    base = ['--data_root', root, '--view_num', '3', '--max_d', '16', '--max_w', '160', '--max_h', '128', '--synthetic_weights',
            '--scenes', 'toy', '--scene_cache', '--fuse', '--no_map_files', '--prob_threshold', '0.5', '--disp_threshold', '0.5',
            '--num_consistent', '1']
    out = {}
    try:
        for name in ('plain', 'clean'):
            FLAGS.reset()
            out[name] = os.path.join(root, 'out_' + name, 'toy')
            extra = []
            if name == 'clean':
                pts, cols = ply.read_ply(os.path.join(out['plain'], 'final3d_model.ply'))
                assert len(pts) >= 100
                # a horizon from the cloud itself: four times the median nearest-neighbour spacing
                d2 = np.concatenate([np.where(np.arange(len(pts))[None, :] == np.arange(a, min(a + 512, len(pts)))[:, None], np.inf,
                                              KR._d2_block(pts[a:a + 512], pts)).min(axis=1) for a in range(0, len(pts), 512)])
                radius = 4.0 * float(np.sqrt(np.median(d2.astype(np.float64))))
                steps = dict(sor=(4, 1.0, radius), radius_filter=(radius, 2))
                ply.write_ply(os.path.join(root, 'gt.ply'), pts[::2], cols[::2])
                extra = ['--clean_sor', '4,1.0', '--clean_sor_radius', repr(radius), '--clean_radius_filter', '%r,2' % radius,
                         '--gt_ply', os.path.join(root, 'gt.ply')]
            E.cli(base + ['--savepath', os.path.dirname(out[name])] + extra)
    finally:
        FLAGS.reset()
        E._Pipelines.CO_RESIDENT = False
    for f in ('final3d_model_clean.ply', 'cloud_clean.json', 'cloud_eval_clean.json', 'cloud_eval.json'):
        assert not os.path.exists(os.path.join(out['plain'], f)) and os.path.exists(os.path.join(out['clean'], f)), f
    with open(os.path.join(out['plain'], 'final3d_model.ply'), 'rb') as f, open(os.path.join(out['clean'], 'final3d_model.ply'), 'rb') as g:
        assert f.read() == g.read()
    got_p, got_c = ply.read_ply(os.path.join(out['clean'], 'final3d_model_clean.ply'))
    want_p, want_c, want_report = clean_cloud.clean(pts, cols, device=cuda, **steps)
    assert np.array_equal(got_p, want_p) and np.array_equal(got_c, want_c) and 0 < len(got_p) < len(pts)
    # an in-order subsequence of the fused rows, with their colours
    fused = np.concatenate([np.ascontiguousarray(pts).view(np.uint32), cols.astype(np.uint32)], 1)
    mine = np.concatenate([np.ascontiguousarray(got_p).view(np.uint32), got_c.astype(np.uint32)], 1)
    at = 0
    for row in mine:
        while not np.array_equal(fused[at], row):
            at += 1
        at += 1
    with open(os.path.join(out['clean'], 'cloud_clean.json')) as f:
        report = json.load(f)
    assert report == json.loads(json.dumps(want_report))
    assert report['n_in'] == len(pts) and report['n_out'] == len(got_p)
    assert report['steps'][0]['rows_in'] == len(pts) and report['steps'][0]['rows_out'] == report['steps'][1]['rows_in']
    assert report['steps'][1]['rows_out'] == len(got_p)
    with open(os.path.join(out['clean'], 'cloud_eval_clean.json')) as f:
        score = json.load(f)
    assert score['n_recon'] == len(got_p) and score['n_gt'] == len(pts[::2])
