"""The host side of the ETH3D-style score (atvsnet/eval_eth3d.py, eval_cloud's scans= and --eth3d) and the restatement the GPU
tests hold the kernels to (tests/cloud_eth3d_restated.py), without a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd                                   # noqa: F401
from atvsnet_amd import _lib, ops
from atvsnet_amd.atvsnet import eval_cloud, eval_eth3d

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_eth3d_restated as ER  # noqa: E402
import scan_render_restated as SR  # noqa: E402


def _room(n_scan=4000, size=16, seed=3):
    """Two scanners in a box room of half-edge 2, their cube maps by the restated renderer, 300 queries in and around it."""
    rng = np.random.default_rng(seed)
    origins = np.array([[0.25, -0.25, 0.125], [-1.0, 0.75, -0.5]])            # exact in float32
    cams = np.concatenate([eval_eth3d.cube_cameras(o, size) for o in origins], 0)
    maps = np.concatenate([SR.scan_render(ER.box_walls(n_scan, 2.0, rng), cams[6 * s:6 * s + 6], size, size, 0.5, 0)
                           for s in range(2)], 0)
    q = rng.uniform(-3.0, 3.0, (300, 3)).astype(np.float32)
    q[0] = origins[0]
    q[1] = [np.nan, 0, 0]
    q[2] = [np.inf, 0, 1]
    q[3] = origins[0] + [1.0, -1.0, 0.0]                       # on a cube edge of scanner 0
    return cams, maps, q


@pytest.mark.parametrize('window', [0, 1, 2])
def test_scan_excess_restatement_is_the_literal_loop(window):
    cams, maps, q = _room()
    e, s = ER.scan_excess(q, cams, maps, 0.5, window)
    e2, s2 = ER.scan_excess_loop(q, cams, maps, 0.5, window)
    assert e.dtype == np.float32 and s.dtype == np.int32
    assert np.array_equal(e.view(np.uint32), e2.view(np.uint32)) and np.array_equal(s, s2)
    assert (s[1:3] == -1).all() and np.isposinf(e[1:3]).all() and s[0] == 1     # scanner 0's origin: seen by scanner 1 alone
    assert (s >= 0).sum() > 200 and (e[s >= 0] < 0).any() and (e[s >= 0] > 0).any()
    assert set(np.unique(s)) == {-1, 0, 1}


def test_scan_excess_restatement_one_scanner_sees_nothing_at_its_origin():
    cams, maps, q = _room()
    e, s = ER.scan_excess(q[:1], cams[:6], maps[:6], 0.5, 1)
    assert s.tolist() == [-1] and np.isposinf(e).all()


@pytest.mark.parametrize('with_excess', [False, True])
def test_voxel_shares_restatement_is_the_literal_loop(with_excess):
    rng = np.random.default_rng(5)
    p = rng.uniform(0.0, 0.05, (300, 3)).astype(np.float32)
    p[7] = np.nan
    d2 = (rng.uniform(0.0, 0.02, 300) ** 2).astype(np.float32)
    d2[::9] = np.inf
    ex = rng.uniform(-0.1, 0.1, 300).astype(np.float32)
    ex[::7] = np.inf
    tol = [0.005, 0.01, 0.02]
    got = ER.voxel_shares(p, d2, ex if with_excess else None, 0.01, (0, 0, 0), tol, 0.01)
    want = ER.voxel_shares_loop(p, d2, ex if with_excess else None, 0.01, (0, 0, 0), tol, 0.01)
    assert got == want
    assert all(isinstance(v, int) for row in got for v in row)
    if not with_excess:
        assert [row[3] for row in got] == [299] * 3              # every finite point counts
    else:
        assert got[0][3] < 299                                   # some points are unobserved
    with pytest.raises(ValueError, match='2\\^21'):
        ER.voxel_shares(p, d2, None, 0.01, (1, 0, 0), tol)


def test_cube_cameras_are_six_rotations_that_tile_the_sphere():
    N = 64
    o = np.array([0.25, -1.5, 3.0])
    cams = eval_eth3d.cube_cameras(o, N)
    assert cams.shape == (6, 16) and cams.dtype == np.float64
    fwd = []
    for row in cams:
        R = row[:9].reshape(3, 3)
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-15 and np.linalg.det(R) == pytest.approx(1.0, abs=1e-15)
        assert np.array_equal(row[9:12], -(R @ o)) and row[12:].tolist() == [N / 2.0] * 4
        fwd.append(R[2].tolist())
    assert fwd == [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    rng = np.random.default_rng(0)
    d = rng.normal(size=(10000, 3))
    pts = (o + d * rng.uniform(0.1, 10.0, (10000, 1))).astype(np.float32)
    count = np.zeros(10000, int)
    for row in cams:
        c2, xs, ys = SR.project(pts, row, 0.5)
        count += (c2 > 0) & (xs >= 0) & (xs < N) & (ys >= 0) & (ys < N)
    assert (count == 1).all()
    for bad in ([0, 0], [0, 0, np.nan]):
        with pytest.raises(ValueError, match='origin'):
            eval_eth3d.cube_cameras(bad, N)
    with pytest.raises(ValueError, match='size'):
        eval_eth3d.cube_cameras(o, 0)


_MLP = '''<!DOCTYPE MeshLabDocument>
<MeshLabProject>
 <MeshGroup>
  <MLMesh label="a" filename="scans/a.ply">
   <MLMatrix44>
%s
</MLMatrix44>
  </MLMesh>
  <MLMesh label="b" filename="b.ply"/>
 </MeshGroup>
 <RasterGroup/>
</MeshLabProject>
'''


def test_read_mlp(tmp_path):
    T = np.array([[0.0, -1.0, 0.0, 1.5], [1.0, 0.0, 0.0, -2.25], [0.0, 0.0, 1.0, 0.125], [0.0, 0.0, 0.0, 1.0]])
    path = tmp_path / 'scan_alignment.mlp'
    path.write_text(_MLP % '\n'.join(' '.join(repr(float(v)) for v in row) for row in T))
    got = eval_eth3d.read_mlp(str(path))
    assert [p for p, _ in got] == [str(tmp_path / 'scans' / 'a.ply'), str(tmp_path / 'b.ply')]
    assert np.array_equal(got[0][1], T) and got[0][1].dtype == np.float64
    assert np.array_equal(got[1][1], np.eye(4))
    for text in ('1 2 3', ' '.join(['1'] * 15 + ['nan']), ' '.join(['1'] * 15 + ['x'])):
        path.write_text(_MLP % text)
        with pytest.raises(ValueError, match='16 finite numbers'):
            eval_eth3d.read_mlp(str(path))
    path.write_text('<MeshLabProject><MeshGroup/></MeshLabProject>')
    with pytest.raises(ValueError, match='no MLMesh'):
        eval_eth3d.read_mlp(str(path))


def test_metrics_forms_the_shares_from_the_integer_words():
    wr = [[3 << 31, 2, 10, 12], [0, 0, 0, 0]]
    wg = [[1 << 32, 4, 7, 9], [5 << 32, 5, 9, 9]]
    out = eval_eth3d.metrics(wr, wg, 20, [0.01, 0.02], {'voxel': 0.01})
    a = out['tolerances'][0]
    assert (a['accuracy'], a['completeness'], a['f1']) == (0.75, 0.25, 2 * 0.75 * 0.25 / 1.0)
    assert (a['n_accurate'], a['n_inaccurate'], a['n_unobserved'], a['voxels_recon'], a['voxels_gt']) == (10, 2, 8, 2, 4)
    b = out['tolerances'][1]
    assert (b['accuracy'], b['completeness'], b['f1'], b['n_unobserved']) == (0.0, 1.0, 0.0, 20)
    assert out['voxel'] == 0.01 and [t['tolerance'] for t in out['tolerances']] == [0.01, 0.02]


def test_evaluate_refuses_contradictory_scans():
    a = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match='voxel'):
        eval_cloud.evaluate(a, None, scans=[a], scanner_origins=[[0, 0, 0]], voxel=0.05)
    with pytest.raises(ValueError, match='2 scans but 1 scanner origins'):
        eval_cloud.evaluate(a, None, scans=[a, a], scanner_origins=[[0, 0, 0]])
    with pytest.raises(ValueError, match='scanner_origins'):
        eval_cloud.evaluate(a, None, scans=[a])
    with pytest.raises(ValueError, match='gt must be None'):
        eval_cloud.evaluate(a, a, scans=[a], scanner_origins=[[0, 0, 0]])
    with pytest.raises(ValueError, match='needs scans'):
        eval_cloud.evaluate(a, a, scanner_origins=[[0, 0, 0]])
    for kw, text in ((dict(vis_window=3), 'vis_window'), (dict(cube_size=0), 'cube_size'), (dict(eth3d_voxel=0.0), 'eth3d_voxel'),
                     (dict(free_space_margin=float('nan')), 'free_space_margin')):
        with pytest.raises(ValueError, match=text):
            eval_cloud.evaluate(a, None, scans=[a], scanner_origins=[[0, 0, 0]], **kw)


def test_cli_refuses_eth3d_without_origins(capsys):
    for argv, text in ((['--recon', 'r.ply', '--gt', 'a.ply', '--eth3d'], '--gt_mlp'),
                       (['--recon', 'r.ply', '--gt', 'a.ply', '--eth3d'], '--scanner_origins'),
                       (['--recon', 'r.ply', '--eth3d'], '--scanner_origins'),
                       (['--recon', 'r.ply', '--gt', 'a.ply', '--eth3d', '--gt_mlp', 'p.mlp'], 'replaces --gt'),
                       (['--recon', 'r.ply', '--eth3d', '--scanner_origins', 'o.txt'], 'needs --gt'),
                       (['--recon', 'r.ply', '--gt', 'a.ply', '--gt_mlp', 'p.mlp'], 'needs --eth3d'),
                       (['--recon', 'r.ply', '--gt', 'a.ply', '--cube_size', '64'], 'needs --eth3d'),
                       (['--recon', 'r.ply', '--eth3d', '--gt_mlp', 'p.mlp', '--voxel', '0.1'], '--voxel'),
                       (['--recon', 'r.ply', '--eth3d', '--gt_mlp', 'p.mlp', '--vis_window', '3'], 'vis_window'),
                       (['--recon', 'r.ply'], '--gt is required')):
        with pytest.raises(SystemExit) as e:
            eval_cloud.cli(argv)
        assert e.value.code == 2
        assert text in capsys.readouterr().err, argv


def test_ops_refuse_bad_arguments_no_fallback():
    P, C, M = torch.zeros(5, 3), torch.zeros(6, 16, dtype=torch.float64), torch.zeros(6, 4, 4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.cloud_scan_excess(P, C, M)
    for kw, text in ((dict(window=3), 'window'), (dict(window=-1), 'window'), (dict(window=1.0), 'window'),
                     (dict(pixel_centre=float('inf')), 'pixel_centre')):
        with pytest.raises(ValueError, match=text):
            ops.cloud_scan_excess(P, C, M, **kw)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.cloud_voxel_shares(P, torch.zeros(5), None, 0.01, (0, 0, 0), [0.01])
    for args, text in (((0.0, (0, 0, 0), [0.01]), 'voxel'), ((0.01, (0, 0, 0), []), 'tolerances'),
                       ((0.01, (0, 0, 0), [0.01] * 17), 'tolerances'), ((0.01, (0, 0, 0), [-1.0]), 'tolerances'),
                       ((0.01, (0, 0, np.inf), [0.01]), 'origin')):
        with pytest.raises(ValueError, match=text):
            ops.cloud_voxel_shares(P, torch.zeros(5), None, *args)
    with pytest.raises(ValueError, match='margin'):
        ops.cloud_voxel_shares(P, torch.zeros(5), None, 0.01, (0, 0, 0), [0.01], float('nan'))
    assert ops.CLOUD_SCAN_MAX_WINDOW == 2


def test_library_exports_both_entry_points_and_checks_arguments_on_the_host():
    names = _lib.declared_symbols()
    L = _lib.lib()
    for n in ('atvs_cloud_scan_excess', 'atvs_cloud_voxel_shares', 'atvs_cloud_voxel_shares_scratch_size'):
        assert n in names and hasattr(L, n), n
    assert _lib.header_abi_version() >= 52 and L.atvs_abi_version() == _lib.header_abi_version()
    assert 'cloud_visibility' not in _lib.OWNS_ITS_SIMD
    flags = _lib.flags_for(os.path.join(_lib.CSRC, 'cloud_visibility.hip'))
    assert '-ffp-contract=off' in flags and '-fno-slp-vectorize' in flags
    fake, lng, dbl = ctypes.c_void_p(256), ctypes.c_long, ctypes.c_double       # never dereferenced: refused before a launch
    excess = lambda m=10, S=1, N=8, centre=0.5, w=1, pts=fake: L.atvs_cloud_scan_excess(  # noqa: E731
        pts, lng(m), fake, fake, S, N, dbl(centre), w, fake, fake, None)
    for kw in (dict(w=-1), dict(w=3), dict(centre=float('nan')), dict(centre=float('inf'))):
        assert excess(**kw) == -3, kw                                                    # ATVS_ERR_ARG
    for kw in (dict(N=0), dict(S=0), dict(S=10923), dict(S=2, N=13378), dict(m=-1), dict(m=(1 << 30) + 1)):
        assert excess(**kw) == -2, kw                                                    # ATVS_ERR_SHAPE
    assert excess(pts=None) == -1
    assert excess(m=0, pts=None) == 0
    nbytes = lng(0)
    assert L.atvs_cloud_voxel_shares_scratch_size(lng(1000), ctypes.byref(nbytes)) == 0
    assert nbytes.value == 256 + 2048 * 8 + 2048 * 32 + 4096                             # header, keys, counters, slot_of
    assert L.atvs_cloud_voxel_shares_scratch_size(lng(-1), ctypes.byref(nbytes)) == -2
    assert L.atvs_cloud_voxel_shares_scratch_size(lng(1), None) == -1
    one, org = (dbl * 1)(0.01), (dbl * 3)(0.0, 0.0, 0.0)
    shares = lambda n=10, voxel=0.01, tol=one, T=1, margin=0.0, sb=1 << 20, origin=org: L.atvs_cloud_voxel_shares(  # noqa: E731
        fake, fake, None, lng(n), dbl(voxel), origin, tol, T, dbl(margin), fake, lng(sb), fake, None)
    for kw in (dict(voxel=0.0), dict(voxel=float('inf')), dict(margin=float('nan')), dict(tol=(dbl * 1)(-1.0)),
               dict(tol=(dbl * 1)(float('nan'))), dict(origin=(dbl * 3)(0.0, float('inf'), 0.0))):
        assert shares(**kw) == -3, kw
    for kw in (dict(n=-1), dict(T=0), dict(T=17)):
        assert shares(**kw) == -2, kw
    assert shares(origin=None) == -1
