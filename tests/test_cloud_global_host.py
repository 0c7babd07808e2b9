"""CPU: the restatement of the global registration (tests/cloud_global_restated.py) held to independent ground truth -- the
descriptor's invariance, the bin rules against numpy.arctan2, the three-point similarity against a known one, the whole of
global_init on the moved room -- and the header, the sources, the argument checks and the command lines of what it restates."""
import ctypes
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd                                   # noqa: F401
from atvsnet_amd import _lib, ops
from atvsnet_amd.atvsnet import eval_cloud, eval_pointcloud, register_cloud as RC
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_global_restated as GR  # noqa: E402
import cloud_knn_restated as KR  # noqa: E402
import cloud_register_restated as RR  # noqa: E402

DISTANCES = (0.2, 0.1, 0.05)            # the ICP stages of the end-to-end tests (the room is 2 x 1.2 x 0.8)
VOXEL = DISTANCES[-1] / 2.0             # register's default voxel


def _inputs(case):
    pts, k, radius = GR.fpfh_case(case)
    idx = KR.knn(pts, pts, radius, k, exclude_same_index=True)[1]
    return (pts,) + GR.fpfh_edits(case, idx, GR.normals_pca(pts, idx))


@pytest.mark.parametrize('case', ['plane', 'room', 'sphere', 'sparse', 'edited'])
def test_descriptor_by_a_plain_loop_and_the_cap_on_rows_near_an_edge(case):
    """The vectorised restatement against a loop over single pairs written from the header (every 16th row), the parts' sums, and
    the cap: at most 1 % of the rows of each cloud the GPU test uses have a pair within 1e-9 of a bin edge."""
    pts, idx, nrm = _inputs(case)
    got, near = GR.fpfh(pts, idx, nrm)
    hist, pairs, _ = GR.spfh(pts, idx, nrm)
    zero = ~got.any(axis=1)
    assert near.sum() <= 0.01 * len(pts) and np.array_equal(zero, pairs == 0)
    assert np.abs(got[~zero].astype(np.float64).reshape(-1, 3, 11).sum(axis=2) - 1.0).max() <= GR.PART_SUM_BAR
    P, N, n = pts.astype(np.float64), nrm.astype(np.float64), len(pts)
    for j in range(0, n, 16):
        valid = [int(i) for i in idx[j] if 0 <= i < n and np.isfinite(P[i]).all()]
        c = np.zeros(3)
        for i in valid:
            c = c + (P[i] - P[j])
        u = -N[j] if (N[j, 0] * c[0] + N[j, 1] * c[1]) + N[j, 2] * c[2] < 0 else N[j]
        h = np.zeros(33, np.int64)
        for i in valid:
            m, d = N[i], P[i] - P[j]
            if not (np.isfinite(N[j]).all() and N[j].any() and np.isfinite(m).all() and m.any() and np.isfinite(P[j]).all() and d.any()):
                continue
            g = np.cross(u, d)
            if not g.any():
                continue
            m = -m if u @ m < 0 else m
            v = g / np.linalg.norm(g)
            w = np.cross(u, v)
            alpha, phi, theta = v @ m, (u @ d) / np.linalg.norm(d), math.atan2(w @ m, u @ m)
            h[min(10, int(math.floor((alpha + 1.0) * 5.5)))] += 1
            h[11 + min(10, int(math.floor((phi + 1.0) * 5.5)))] += 1
            h[22 + min(10, int(math.floor((theta + math.pi / 2) / (math.pi / 11))))] += 1
        if not near[j]:
            assert h.tolist() == hist[j].tolist() and h.sum() == 3 * pairs[j], (case, j)


def test_descriptor_does_not_change_with_the_frame_the_scale_or_the_normals_sign():
    """The sign rule's whole purpose: the room and the same room under a rotation, a translation and the factor 1.7 (float64, not
    rounded again) have the same descriptors to the output's rounding, with the given normals and with every one of them negated
    -- and negating only some.  Rows with a pair near a bin edge are left out (the moved features differ by roundings)."""
    pts = RR.shape(1500, 2, 0.002)
    idx = KR.knn(pts.astype(np.float32), pts.astype(np.float32), 0.2, 16, exclude_same_index=True)[1]
    nrm = GR.normals_pca(pts, idx).astype(np.float64)
    rng = np.random.default_rng(0)
    R = RR.rotation(rng.normal(size=3), 131.0)
    moved, turned = 1.7 * pts @ R.T + rng.normal(size=3) * 5.0, nrm @ R.T
    base, near = GR.fpfh(pts, idx, nrm, storage=np.float64)
    some = np.where(rng.uniform(size=len(pts)) < 0.5, -1.0, 1.0)[:, None]
    assert base.any(axis=1).sum() > 1400
    for p, n in ((moved, turned), (moved, -turned), (pts, -nrm), (moved, turned * some)):
        other, near_other = GR.fpfh(p, idx, n, storage=np.float64)
        held = ~(near | near_other)
        assert held.sum() >= 0.99 * len(pts)
        assert np.abs(other[held].astype(np.float64) - base[held]).max() <= GR.FPFH_BAR
    # and it is a descriptor: it tells the ball from the floor (their descriptors differ by far more than two floor rows do)
    ball = np.linalg.norm(pts - [1.3, 0.4, 0.0], axis=1) < 0.26
    floor = (np.abs(pts[:, 2]) < 0.01) & (pts[:, 0] > 0.3) & (pts[:, 1] > 0.3) & ~ball
    f = base.astype(np.float64)
    assert np.linalg.norm(f[ball].mean(axis=0) - f[floor].mean(axis=0)) > 4 * np.linalg.norm(f[floor] - f[floor].mean(axis=0), axis=1).mean()


def test_bin_rules_agree_with_arctan2_and_floor_away_from_the_edges():
    rng = np.random.default_rng(1)
    theta = np.linspace(-math.pi / 2, math.pi / 2, 200001)[1:-1]
    radius = rng.uniform(1e-3, 2.0, len(theta))
    x, y = radius * np.cos(theta), radius * np.sin(theta)
    got, near = GR.theta_bin(x, y)
    angle = np.arctan2(y, x)
    want = np.floor((angle + math.pi / 2) / (math.pi / 11)).astype(int)
    edge_gap = np.abs((angle + math.pi / 2) / (math.pi / 11) - np.round((angle + math.pi / 2) / (math.pi / 11)))
    away = edge_gap > 1e-6
    assert away.sum() > 0.99 * len(theta) and np.array_equal(got[away], want[away]) and not near[away].any()
    assert set(got.tolist()) == set(range(11)) and np.bincount(got).min() > 18000
    # a tie goes to the upper bin; the direction (0, 0) is a tie with every edge
    C, S = GR.THETA_COS, GR.THETA_SIN
    assert GR.theta_bin(C[4], S[4])[0] == 5 and GR.theta_bin(C[4], np.nextafter(S[4], -1))[0] == 4 and GR.theta_bin(0.0, 0.0)[0] == 10
    assert GR.theta_bin(1.0, 0.0)[0] == 5 and GR.theta_bin(0.0, 1.0)[0] == 10 and GR.theta_bin(0.0, -1.0)[0] == 0
    v = np.linspace(-1, 1, 200001)
    got, near = GR.linear_bin(v)
    away = np.abs((v + 1.0) * 5.5 - np.round((v + 1.0) * 5.5)) > 1e-6
    assert np.array_equal(got[away], np.minimum(10, np.floor((v[away] + 1.0) * 5.5).astype(int))) and not near[away].any()
    assert GR.linear_bin(np.array([-1.0, -9.0 / 11, np.nextafter(-9.0 / 11, -1), 0.0, 1.0]))[0].tolist() == [0, 1, 0, 5, 10]
    assert GR.linear_bin(np.array([1.0 / 11]))[1][0] and not GR.linear_bin(np.array([0.0]))[1][0]


def test_header_tables_limits_and_sources():
    """The edge table is cos / sin of (2 e - 11) pi / 22 to the last digit, the limits come from the header, the kernels use the
    header's names and no transcendental function, and the build does not contract."""
    with open(_lib.HEADER) as f:
        text = f.read()
    for e in range(1, 11):
        angle = (2 * e - 11) * math.pi / 22
        assert GR.THETA_COS[e - 1] == math.cos(angle) and GR.THETA_SIN[e - 1] == math.sin(angle), e
        assert '%.17g' % math.cos(angle) in GR.header_value('ATVS_CLOUD_FPFH_THETA_COS', text)
        assert '%.17g' % math.sin(angle) in GR.header_value('ATVS_CLOUD_FPFH_THETA_SIN', text)
    assert (GR.BINS, GR.MAX_K, GR.MAX_BEST, GR.MIN_EDGE2) == (11, 32, 8, 1e-60)
    assert ops.cloud.CLOUD_FPFH_BINS == GR.BINS and ops.cloud.CLOUD_RANSAC_MAX_BEST == GR.MAX_BEST and ops.cloud.CLOUD_MAX_K == GR.MAX_K
    assert '-ffp-contract=off' in _lib.FLAGS
    sources = {}
    for name in ('cloud_features.hip', 'cloud_ransac.hip'):
        with open(os.path.join(_lib.CSRC, name)) as f:
            sources[name] = f.read()
        code = re.sub(r'//[^\n]*', '', sources[name])
        assert not re.search(r'\b(atan2?f?|sincosf?|sinf?|cosf?|acosf?|asinf?|tanf?|expf?|logf?|powf?|atomic\w*)\s*\(', code), name
        assert 'fma' not in code
    for token in ('ATVS_CLOUD_FPFH_THETA_COS', 'ATVS_CLOUD_FPFH_THETA_SIN', 'ATVS_CLOUD_FPFH_BINS', 'ATVS_CLOUD_FEATURE_TILE', 'ATVS_CLOUD_MAX_K'):
        assert token in sources['cloud_features.hip'], token
    for token in ('ATVS_CLOUD_RANSAC_MAX_BEST', 'ATVS_CLOUD_RANSAC_MIN_EDGE2'):
        assert token in sources['cloud_ransac.hip'], token
    assert int(GR.header_value('ATVS_CLOUD_FEATURE_TILE', text)) == 128


def test_three_points_give_back_a_known_similarity_and_every_degenerate_case_is_flagged():
    rng = np.random.default_rng(2)
    src = rng.integers(-8, 9, (40, 3)).astype(np.float64) / 4.0
    src[:3] = [[0, 0, 0], [2, 0, 0], [0, 1, 0]]
    # exact in float32: a quarter turn about z, the factor 2, an integer translation
    M = RR.similarity([[0, -1, 0], [1, 0, 0], [0, 0, 1]], (3, -2, 5), 2.0)
    dst = src @ M[:3, :3].T + M[:3, 3]
    got, valid, reason = GR.hypotheses(src, dst, [[0, 1, 2], [2, 0, 1]], with_scale=True)
    assert valid.all() and np.abs(got - M[:3]).max() <= 1e-15
    rigid, valid, reason = GR.hypotheses(src, dst, [[0, 1, 2]], with_scale=False)
    assert not valid[0] and reason[0] == 'ratio'                                      # lengths doubled: no rigid motion fits
    # a general similarity, through float32 storage: to its rounding
    for with_scale in (False, True):
        M = RR.similarity(RR.rotation((1, -2, 0.5), 150.0), (7.0, -5.0, 9.0), 1.7 if with_scale else 1.0, (0.3, 0.2, 0.1))
        dst = src @ M[:3, :3].T + M[:3, 3]
        triples = np.array([[0, 1, 2], [5, 9, 20], [0, 0, 1], [1, 2, 40], [-1, 2, 3]])
        got, valid, reason = GR.hypotheses(src, dst, triples, with_scale)
        assert valid.tolist() == [True, True, False, False, False] and reason.tolist() == ['', '', 'index', 'index', 'index']
        assert np.abs(got[:2] - M[:3]).max() <= 1e-5 and not got[2:].any()
        for T in got[:2]:                                                             # a rotation times the scale, never a reflection
            A = T[:, :3] / (1.7 if with_scale else 1.0)
            assert np.abs(A @ A.T - np.eye(3)).max() <= 1e-6 and np.linalg.det(A) > 0.99
        best, counts, sums = GR.ransac(src, dst, triples, 1e-4, with_scale, best=3)
        assert [b['count'] for b in best] == [40, 40, -1] and counts.tolist() == [40, 40, -1, -1, -1]
        assert best[0]['sum'] <= best[1]['sum'] and best[2]['index'] == -1 and sums[best[0]['index']] == best[0]['sum']
    # the degenerate triangles: a repeated point at two indices, three points on a line, a sliver below the sine floor
    s = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [1, 1e-7, 0], [0, 2, 0]], np.float64)
    _, valid, reason = GR.hypotheses(s, s, [[0, 1, 4], [0, 2, 3], [0, 2, 5], [0, 2, 4], [0, 2, 6]], False)
    assert valid.tolist() == [False, False, False, True, True] and reason.tolist() == ['edge', 'area', 'area', '', '']
    # the edge-length ratio after the scale: one stretched edge fails it, and passes a looser ratio
    d = s.copy()
    d[4] = [0, 1.5, 0]
    assert GR.hypotheses(s, d, [[0, 2, 4]], False)[2][0] == 'ratio' and GR.hypotheses(s, d, [[0, 2, 4]], False, edge_ratio=0.6)[1][0]
    assert GR.hypotheses(s, d, [[0, 2, 4]], True)[2][0] == 'ratio'


def test_feature_nearest_by_a_plain_loop():
    ref, query = GR.features(40, 1), GR.features(30, 2)
    query[8] = ref[20]
    d2, idx = GR.feature_nearest(ref, query)
    for j in range(30):
        best, at = np.float32(np.inf), -1
        for i in range(40):
            if not ref[i].any():
                continue
            acc = np.float32(0)
            for b in range(33):
                e = np.float32(query[j, b] - ref[i, b])
                acc = np.float32(acc + np.float32(e * e))
            if acc < best:
                best, at = acc, i
        if not query[j].any():
            best, at = np.float32(np.inf), -1
        assert (d2[j], idx[j]) == (best, at), j
    assert idx[8] == 3 and d2[8] == 0                                                 # rows 3 and 20 are equal: the lower index


@pytest.fixture(scope='module')
def matched():
    """`match` of the moved room, once per (cloud seed, with_scale): the descriptors do not depend on the triples' seed."""
    cache = {}

    def get(seed, with_scale):
        if (seed, with_scale) not in cache:
            gt, src, M = GR.moved_room(seed, with_scale)
            cache[seed, with_scale] = (GR.match(src, gt, with_scale=with_scale, voxel=VOXEL), src, M)
        return cache[seed, with_scale]
    return get


@pytest.mark.parametrize('with_scale', [False, True])
@pytest.mark.parametrize('cloud_seed', [0, 1, 2])
def test_global_init_brings_the_moved_room_within_reach_of_icp(matched, cloud_seed, with_scale):
    """The room of 4097 points (noise 0.002) turned by 150 degrees about a skew axis, moved by several room sizes and, with_scale,
    scaled by 1.7: the restated global_init, at its defaults, brings every corner of the source's box within HALF THE FIRST ICP
    DISTANCE of where the true motion puts it -- what ICP needs: a point then finds a partner within the first distance (derived,
    not fitted).  Three clouds, two seeds of the triples, rigid and with_scale."""
    m, src, M = matched(cloud_seed, with_scale)
    assert RR.corners_of(src).shape == (8, 3) and np.linalg.norm(M[:3, 3]) > 5.0
    for seed in (0, 1):
        found = GR.solve(m, seed=seed)
        err = GR.corner_error(found['matrix'], M, src)
        print('cloud %d, with_scale %s, seed %d: corner error %.4f (bar %.3f), fitness %.3f, %d of %d matches mutual, %d valid hypotheses' % (
            cloud_seed, with_scale, seed, err, DISTANCES[0] / 2.0, found['fitness'], found['n_mutual'], found['n_matches'], found['n_valid']))
        assert err <= DISTANCES[0] / 2.0
        assert found['fitness'] > 0.9 and found['n_valid'] > 0
    assert np.array_equal(GR.solve(m, seed=1)['matrix'], found['matrix'])               # the seed fixes the run


def test_ops_and_register_refuse_bad_arguments_no_fallback():
    P, idx, F = torch.zeros(5, 3), torch.zeros((5, 4), dtype=torch.int32), torch.zeros(5, 33)
    tri = torch.zeros((2, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.cloud_fpfh(P, idx, P)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.cloud_feature_nearest(F, F)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.cloud_ransac(P, P, tri, 0.1, False)
    for bad in (torch.zeros(5, dtype=torch.int32), torch.zeros((5, 33), dtype=torch.int32), torch.zeros((5, 0), dtype=torch.int32)):
        with pytest.raises(ValueError, match='idx: expected shape'):
            ops.cloud_fpfh(P, bad, P)
    with pytest.raises(TypeError, match='idx'):
        ops.cloud_fpfh(P, idx.numpy(), P)
    with pytest.raises(TypeError, match='points'):
        ops.cloud_fpfh(P.double(), idx, P)
    with pytest.raises(ValueError, match='feat_ref'):
        ops.cloud_feature_nearest(torch.zeros(5, 32), F)
    with pytest.raises(TypeError, match='feat_ref'):
        ops.cloud_feature_nearest(F.double(), F)
    for kwargs, message in ((dict(tau=0.0), 'tau'), (dict(tau=float('nan')), 'tau'), (dict(edge_ratio=0.0), 'edge_ratio'),
                            (dict(edge_ratio=1.5), 'edge_ratio'), (dict(best=0), 'best'), (dict(best=9), 'best')):
        args = dict(dict(tau=0.1, with_scale=False), **kwargs)
        with pytest.raises(ValueError, match=message):
            ops.cloud_ransac(P, P, tri, **args)
    with pytest.raises(TypeError, match='with_scale'):
        ops.cloud_ransac(P, P, tri, 0.1, 1)
    with pytest.raises(TypeError, match='src'):
        ops.cloud_ransac(P.double(), P, tri, 0.1, False)
    pts = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="init: a 4x4 matrix, None or 'global'"):
        RC.register(pts, pts, init='cameras')
    with pytest.raises(ValueError, match="global_options are used by init='global' only"):
        RC.register(pts, pts, global_options=dict(seed=1))
    for kwargs, message in ((dict(normal_k=1), 'normal_k'), (dict(feature_k=33), 'feature_k'), (dict(hypotheses=0), 'hypotheses'),
                            (dict(best=9), 'best'), (dict(seed=-1), 'seed'), (dict(edge_ratio=0.0), 'edge_ratio'), (dict(tau=0.0), 'tau'),
                            (dict(feature_voxel=0.0), 'feature_voxel'), (dict(feature_voxel=(1.0, 2.0, 3.0)), 'feature_voxel'),
                            (dict(feature_radius=-1.0), 'feature_radius'), (dict(voxel=None), 'give voxel')):
        with pytest.raises(ValueError, match=message):
            RC.global_init(pts, pts, **dict(dict(voxel=0.1), **kwargs))
    with pytest.raises(ValueError, match='need register=True'):
        eval_cloud.evaluate(pts, pts, register_global=True)
    with pytest.raises(ValueError, match='need register_global=True'):
        eval_cloud.evaluate(pts, pts, register=True, global_options=dict(seed=1))
    with pytest.raises(ValueError, match='init_transform is not used'):
        eval_cloud.evaluate(pts, pts, register=True, register_global=True, init_transform=np.eye(4))
    sig = inspect.signature(RC.global_init).parameters
    assert {k: sig[k].default for k in ('normal_k', 'feature_k', 'hypotheses', 'seed', 'mutual', 'edge_ratio', 'best')} == dict(
        normal_k=16, feature_k=32, hypotheses=65536, seed=0, mutual=True, edge_ratio=0.9, best=4)
    assert all(sig[k].default is None for k in ('feature_voxel', 'feature_radius', 'tau', 'voxel'))
    assert inspect.signature(RC.register).parameters['global_options'].default is None
    assert '--register_global' in inspect.getsource(RC.register)                       # the hint of the "too far off" message


def test_library_exports_the_new_entry_points_and_checks_arguments_on_the_host():
    names = _lib.declared_symbols()
    L = _lib.lib()
    for n in ('atvs_cloud_fpfh_scratch_size', 'atvs_cloud_fpfh', 'atvs_cloud_feature_nearest', 'atvs_cloud_ransac_scratch_size',
              'atvs_cloud_ransac_score'):
        assert n in names and hasattr(L, n), n
    assert _lib.header_abi_version() >= 57 and L.atvs_abi_version() == _lib.header_abi_version()
    lng, dbl, integer = ctypes.c_long, ctypes.c_double, ctypes.c_int
    size = ctypes.c_long(0)
    assert L.atvs_cloud_fpfh_scratch_size(lng(1000), ctypes.byref(size)) == 0 and size.value >= 36000 and size.value % 256 == 0
    assert L.atvs_cloud_fpfh_scratch_size(lng(-1), ctypes.byref(size)) == -2 and L.atvs_cloud_fpfh_scratch_size(lng(5), None) == -1
    assert L.atvs_cloud_ransac_scratch_size(lng(65536), ctypes.byref(size)) == 0 and size.value == 12 * 65536
    assert L.atvs_cloud_ransac_scratch_size(lng(0), ctypes.byref(size)) == -2
    assert L.atvs_cloud_ransac_scratch_size(lng((1 << 24) + 1), ctypes.byref(size)) == -2
    fake = ctypes.c_void_p(256)                     # never dereferenced: every call below is refused before a launch

    def fpfh(n=5, k=4, points=fake, idx=fake, normals=fake, scratch=fake, scratch_bytes=1 << 20, out=fake):
        return L.atvs_cloud_fpfh(points, lng(n), idx, integer(k), normals, scratch, lng(scratch_bytes), out, None)
    assert fpfh(k=0) == -2 and fpfh(k=33) == -2 and fpfh(n=-1) == -2 and fpfh(n=(1 << 30) + 1) == -2 and fpfh(scratch_bytes=8) == -2
    assert fpfh(points=None) == -1 and fpfh(idx=None) == -1 and fpfh(normals=None) == -1 and fpfh(out=None) == -1 and fpfh(scratch=None) == -1
    assert fpfh(n=0, points=None, idx=None, normals=None, out=None) == 0                        # nothing to do, nothing read

    def nearest(n=5, m=5, ref=fake, query=fake, d2=fake, idx=fake):
        return L.atvs_cloud_feature_nearest(ref, lng(n), query, lng(m), d2, idx, None)
    assert nearest(n=-1) == -2 and nearest(m=-1) == -2 and nearest(m=(1 << 30) + 1) == -2
    assert nearest(ref=None) == -1 and nearest(query=None) == -1 and nearest(d2=None) == -1 and nearest(idx=None) == -1
    assert nearest(m=0, query=None, d2=None, idx=None) == 0

    def ransac(c=5, h=4, tau=0.1, with_scale=0, ratio=0.9, best=4, src=fake, triples=fake, scratch=fake, scratch_bytes=1 << 20, out=fake):
        return L.atvs_cloud_ransac_score(src, fake, lng(c), triples, lng(h), dbl(tau), integer(with_scale), dbl(ratio), integer(best),
                                         scratch, lng(scratch_bytes), out, None)
    assert ransac(c=2) == -2 and ransac(h=0) == -2 and ransac(h=(1 << 24) + 1) == -2 and ransac(scratch_bytes=8) == -2
    assert ransac(tau=0.0) == -3 and ransac(tau=float('nan')) == -3 and ransac(tau=float('inf')) == -3
    assert ransac(ratio=0.0) == -3 and ransac(ratio=1.01) == -3 and ransac(ratio=float('nan')) == -3
    assert ransac(with_scale=2) == -3 and ransac(best=0) == -3 and ransac(best=9) == -3
    assert ransac(src=None) == -1 and ransac(triples=None) == -1 and ransac(scratch=None) == -1 and ransac(out=None) == -1
    assert ops.cloud_fpfh.__doc__ and ops.cloud_feature_nearest.__doc__ and ops.cloud_ransac.__doc__ and RC.global_init.__doc__


def test_command_lines_parse_and_refuse(capsys, tmp_path):
    pts = np.random.default_rng(0).uniform(0, 1, (50, 3)).astype(np.float32)
    plain = str(tmp_path / 'plain.ply')
    ply.write_ply(plain, pts, np.full((50, 3), 200, np.uint8))
    p = eval_cloud.make_parser()
    base = ['--recon', plain, '--gt', plain]
    assert eval_cloud.register_options(p, p.parse_args(base + ['--register'])) == {'register': True, 'with_scale': False}     # as it was
    o = eval_cloud.register_options(p, p.parse_args(base + ['--register', '--register_global']))
    assert o == {'register': True, 'with_scale': False, 'register_global': True}
    o = eval_cloud.register_options(p, p.parse_args(base + ['--register', '--with_scale', '--register_global', '--global_voxel', '0.05',
                                                           '--global_hypotheses', '1000', '--global_seed', '7', '--global_tau', '0.1',
                                                           '--global_no_mutual']))
    assert o == {'register': True, 'with_scale': True, 'register_global': True,
                 'global_options': {'feature_voxel': 0.05, 'hypotheses': 1000, 'seed': 7, 'tau': 0.1, 'mutual': False}}
    for argv, message in ((base + ['--register_global'], '--register_global needs --register'),
                          (base + ['--register', '--global_seed', '1'], '--global_seed needs --register_global'),
                          (base + ['--register', '--global_no_mutual'], '--global_no_mutual needs --register_global'),
                          (base + ['--register', '--register_global', '--init_transform', plain], 'from the clouds alone'),
                          (base + ['--register', '--register_global', '--init_cameras', 'a', 'b'], 'from the clouds alone'),
                          (base + ['--register', '--register_global', '--global_voxel', '0'], '--global_voxel must be positive'),
                          (base + ['--register', '--register_global', '--global_tau', '-1'], '--global_tau must be positive'),
                          (base + ['--register', '--register_global', '--global_hypotheses', '0'], '--global_hypotheses must be in'),
                          (base + ['--register', '--register_global', '--global_seed', '-2'], '--global_seed must be >= 0')):
        with pytest.raises(SystemExit) as e:
            eval_cloud.cli(argv)                                   # refused before a device is touched
        assert e.value.code == 2 and message in ' '.join(capsys.readouterr().err.split()), argv
    fused = ['--fuse', '--scene_cache', '--gt_ply', 'g.ply']
    for argv, message in ((fused + ['--register_global'], '--register_global needs --register'),
                          (fused + ['--register', '--global_tau', '1'], '--global_tau needs --register_global'),
                          (fused + ['--register', '--register_global', '--init_cameras', 'a', 'b'], 'from the clouds alone'),
                          (fused + ['--register', '--register_global', '--global_hypotheses', '0'], '--global_hypotheses must be in')):
        with pytest.raises(SystemExit) as e:
            eval_pointcloud.cli(argv)
        assert e.value.code == 2 and message in ' '.join(capsys.readouterr().err.split()), argv
    ok = dict(fuse=dict(prob_threshold=0.8), gt_ply=['g.ply'])
    rules = eval_pointcloud._option_rules(register={'global': {}}, **ok)
    assert not any(b for b, _ in rules) and len(rules) == len(eval_pointcloud._option_rules(**ok)) + 1
    assert len(eval_pointcloud._option_rules(register={}, **ok)) == len(eval_pointcloud._option_rules(**ok))               # as it was
    with pytest.raises(ValueError, match='from the clouds alone'):
        eval_pointcloud.run_eval_pc('out', [], register={'global': {}, 'init_cameras': ('a', 'b')}, **ok)
    flags = p.parse_args(base + ['--register', '--register_global', '--global_seed', '3', '--global_no_mutual'])
    assert eval_pointcloud._global_options(flags) == {'global': {'seed': 3, 'mutual': False}}
    assert eval_pointcloud._global_options(p.parse_args(base + ['--register'])) == {}
