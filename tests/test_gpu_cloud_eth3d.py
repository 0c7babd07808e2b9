"""-m gpu: the ETH3D-style score on the device -- ops.cloud_scan_excess and ops.cloud_voxel_shares against their restatement
(tests/cloud_eth3d_restated.py) bit for bit, known answers, and eval_cloud's scans= / --eth3d end to end."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd                                   # noqa: F401
from atvsnet_amd import ops
from atvsnet_amd.atvsnet import eval_cloud, eval_eth3d
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_eth3d_restated as ER  # noqa: E402
import scan_render_restated as SR  # noqa: E402

pytestmark = pytest.mark.gpu

ORIGINS = np.array([[0.25, -0.25, 0.125], [-1.0, 0.75, -0.5]])            # exact in float32


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _excess(dev, pts, cams, maps, centre=0.5, window=1):
    p = torch.from_numpy(np.array(pts, np.float32).reshape(-1, 3)).to(dev)              # copies: the shared inputs are read-only
    c = torch.from_numpy(np.array(cams, np.float64)).to(dev)
    m = torch.from_numpy(np.array(maps, np.float32)).to(dev)
    e, s = ops.cloud_scan_excess(p, c, m, centre, window)
    assert e.dtype == torch.float32 and s.dtype == torch.int32 and tuple(e.shape) == tuple(s.shape) == (len(p),)
    return e.cpu().numpy(), s.cpu().numpy()


def _same(got, want):
    return np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])


@functools.lru_cache(maxsize=None)
def _room(n_scan=20000, size=64, n_query=5000):
    """Two scanners inside a box room of half-edge 2, each with its own n_scan wall points rendered into its cube map by the
    RESTATED renderer, and queries spread inside and outside the room."""
    rng = np.random.default_rng(17)
    cams = np.concatenate([eval_eth3d.cube_cameras(o, size) for o in ORIGINS], 0)
    maps = np.concatenate([SR.scan_render(ER.box_walls(n_scan, 2.0, rng), cams[6 * s:6 * s + 6], size, size, 0.5, 0)
                           for s in range(2)], 0)
    q = rng.uniform(-3.0, 3.0, (n_query, 3)).astype(np.float32)
    return _frozen(cams, maps, q)


@functools.lru_cache(maxsize=None)
def _room_want(window):
    cams, maps, q = _room()
    return _frozen(*ER.scan_excess(q, cams, maps, 0.5, window))


@pytest.mark.parametrize('window', [0, 1, 2])
def test_excess_is_the_restatement(cuda, window):
    cams, maps, q = _room()
    want = _room_want(window)
    got = _excess(cuda, q, cams, maps, 0.5, window)
    assert _same(got, want)
    seen = want[1] >= 0
    assert {0, 1} <= set(np.unique(want[1])) and (want[0][seen] < 0).sum() > 500 and (want[0][seen] > 0).sum() > 500
    assert (~seen).any() == (window == 0)                      # 20 000 points leave pixels empty, but no 3 x 3 window
    assert np.isposinf(want[0][~seen]).all()
    assert _same(_excess(cuda, q, cams, maps, 0.5, window), got)                        # the same bits on every run


@functools.lru_cache(maxsize=None)
def _edge_cases():
    """One scanner with a SPARSE scan (most pixels empty) and 257 queries: the scanner's origin, NaN and +-inf rows, both sides
    of a cube edge (|c_0| = c_2), the rest random."""
    rng = np.random.default_rng(23)
    o = ORIGINS[0]
    cams = eval_eth3d.cube_cameras(o, 16)
    maps = SR.scan_render(ER.box_walls(150, 2.0, rng), cams, 16, 16, 0.5, 0)
    q = rng.uniform(-3.0, 3.0, (257, 3)).astype(np.float32)
    q[0] = o
    q[1] = [np.nan, 0.0, 0.0]
    q[2] = [0.0, np.inf, 0.0]
    q[3] = [0.0, 0.0, -np.inf]
    q[4] = o + [1.0, -1.0, 0.0]                                 # c_0 = c_2 on +x: xs = size, not in view there; -y takes it
    q[5] = o + [1.0, 1.0, 0.0]                                  # c_0 = -c_2 on +x: xs = 0, in view
    q[6] = o + [0.5, 0.0, 0.5]
    q[256] = o + [-0.5, 0.25, 0.125]
    return _frozen(cams, maps, q)


@pytest.mark.parametrize('m', [0, 1, 257])
@pytest.mark.parametrize('window', [0, 2])
def test_excess_edge_cases_one_scanner(cuda, window, m):
    cams, maps, q = _edge_cases()
    want = ER.scan_excess(q[:m], cams, maps, 0.5, window)
    got = _excess(cuda, q[:m], cams, maps, 0.5, window)
    assert got[0].shape == (m,) and _same(got, want)
    if m == 257:
        assert want[1][:4].tolist() == [-1] * 4 and np.isposinf(want[0][:4]).all()     # its own origin, NaN, +inf, -inf
        finite = np.isfinite(q).all(axis=1)
        finite[0] = False
        empty = finite & (want[1] < 0)                          # in view of a face (the faces tile the sphere), nothing in the window
        assert empty.sum() > (60 if window == 0 else 5) and (want[1] == 0).sum() > 10     # 150 points fill a tenth of the pixels
        lone = _excess(cuda, q[256:], cams, maps, 0.5, window)
        assert _same(lone, (want[0][256:], want[1][256:]))


def test_excess_cube_edge_takes_the_first_face_in_view(cuda):
    o = ORIGINS[0]
    cams = eval_eth3d.cube_cameras(o, 16)
    maps = np.zeros((6, 16, 16), np.float32)
    maps[0, 8, 0] = 4.0                                        # +x face, leftmost column: where c_0 = -c_2 lands
    maps[3, 8, 0] = 0.5                                        # -y face, leftmost column: where +x's other edge lands
    q = np.array([o + [1.0, 1.0, 0.0], o + [1.0, -1.0, 0.0]], np.float32)
    e, s = _excess(cuda, q, cams, maps, 0.5, 0)
    r = np.sqrt(2.0)
    assert s.tolist() == [0, 0]
    assert e.tolist() == [float(np.float32(r * (1.0 - 4.0 / 1.0))), float(np.float32(r * (1.0 - 0.5 / 1.0)))]
    assert _same((e, s), ER.scan_excess(q, cams, maps, 0.5, 0))


def test_excess_known_answers_behind_a_wall(cuda):
    """A scanner at the origin, a wall at x = 2 sampled so densely that it fills every pixel of the +x face: one unit in front of
    it is -1, two behind it +2, and nothing is known on the other side of the scanner."""
    N = 16
    g = np.linspace(-2.0, 2.0, 201)
    yy, zz = np.meshgrid(g, g, indexing='ij')
    wall = np.stack([np.full(yy.size, 2.0), yy.reshape(-1), zz.reshape(-1)], 1).astype(np.float32)
    cams = torch.from_numpy(eval_eth3d.cube_cameras([0.0, 0.0, 0.0], N)).to(cuda)
    maps = ops.scan_render(torch.from_numpy(wall).to(cuda), cams, N, N, 0.5, 0)
    assert bool((maps[0] == 2.0).all()) and bool((maps[1] == 0).all())
    q = torch.tensor([[1.0, 0.0, 0.0], [4.0, 0.0, 0.0], [-1.0, 0.0, 0.0]], device=cuda)
    e, s = ops.cloud_scan_excess(q, cams, maps, 0.5, 0)
    assert e.cpu().tolist() == [-1.0, 2.0, float('inf')] and s.cpu().tolist() == [0, 0, -1]


# ---- shares ----------------------------------------------------------------------------------------------------------------

def _shares(dev, pts, d2, excess, voxel, origin, tol, margin=0.0):
    up = lambda a: None if a is None else torch.from_numpy(np.array(a, np.float32)).to(dev)  # noqa: E731
    out = ops.cloud_voxel_shares(up(pts), up(d2), up(excess), voxel, origin, tol, margin)
    assert out.dtype == torch.int64 and tuple(out.shape) == (len(tol), 4) and out.device.type == 'cuda'
    return out.cpu().tolist()


@functools.lru_cache(maxsize=None)
def _share_cloud():
    rng = np.random.default_rng(29)
    n = 30000
    p = rng.uniform(0.0, 0.2, (n, 3)).astype(np.float32)
    p[rng.integers(0, n, 40), rng.integers(0, 3, 40)] = np.nan
    d2 = (rng.uniform(0.0, 0.03, n) ** 2).astype(np.float32)
    d2[rng.integers(0, n, 3000)] = np.inf
    ex = rng.uniform(-0.05, 0.05, n).astype(np.float32)
    ex[rng.integers(0, n, 3000)] = np.inf
    return _frozen(p, d2, ex)


TOL16 = tuple(0.002 * (k + 1) for k in range(16))


@functools.lru_cache(maxsize=None)
def _share_want(with_excess, tol):
    p, d2, ex = _share_cloud()
    return ER.voxel_shares(p, d2, ex if with_excess else None, 0.01, (0.0, 0.0, 0.0), tol, 0.01)


@pytest.mark.parametrize('tol', [(0.01,), TOL16], ids=['T1', 'T16'])
@pytest.mark.parametrize('with_excess', [False, True])
def test_shares_are_the_restatement(cuda, with_excess, tol):
    p, d2, ex = _share_cloud()
    want = _share_want(with_excess, tol)
    got = _shares(cuda, p, d2, ex if with_excess else None, 0.01, (0.0, 0.0, 0.0), tol, 0.01)
    assert got == want
    assert 6000 <= want[0][1] <= 21 ** 3 and want[0][2] > 0                  # about 20^3 voxels, most of them counted
    if with_excess:
        assert want[0][3] < _share_want(False, tol)[0][3]                    # some points are unobserved
    assert _shares(cuda, p, d2, ex if with_excess else None, 0.01, (0.0, 0.0, 0.0), tol, 0.01) == got


def test_shares_known_answer_does_not_depend_on_density(cuda):
    """One voxel of 1000 points, all within tau, and one voxel with a single miss: half the voxels are accurate, whatever the
    plain share of points says."""
    rng = np.random.default_rng(31)
    dense = rng.uniform(0.101, 0.109, (1000, 3)).astype(np.float32)
    p = np.concatenate([dense, np.array([[0.505, 0.505, 0.505]], np.float32)], 0)
    d2 = np.concatenate([np.full(1000, 1e-6, np.float32), np.array([1.0], np.float32)])
    for excess in (None, np.zeros(1001, np.float32)):
        (sq, voxels, hit, den), = _shares(cuda, p, d2, excess, 0.01, (0.0, 0.0, 0.0), [0.01])
        assert (sq, voxels, hit, den) == (1 << 32, 2, 1000, 1001)
        assert sq / (voxels * 4294967296) == 0.5 and hit / den == 1000 / 1001
    behind = np.zeros(1001, np.float32)
    behind[1000] = 0.5                                          # the miss lies behind the scan: unobserved, its voxel is left out
    assert _shares(cuda, p, d2, behind, 0.01, (0.0, 0.0, 0.0), [0.01]) == [[1 << 32, 1, 1000, 1000]]
    assert _shares(cuda, p, d2, behind, 0.01, (0.0, 0.0, 0.0), [0.01], margin=0.5) == [[1 << 32, 2, 1000, 1001]]
    assert _shares(cuda, p[:0], d2[:0], None, 0.01, (0.0, 0.0, 0.0), [0.01, 0.02]) == [[0] * 4] * 2


def test_shares_refuse_a_point_beyond_the_cells(cuda):
    p = np.array([[0.005, 0.005, 0.005], [0.01 * (1 << 21) + 1.0, 0.0, 0.0]], np.float32)
    d2 = np.zeros(2, np.float32)
    with pytest.raises(ValueError, match='more than 2\\^21 voxels from the origin'):
        _shares(cuda, p, d2, None, 0.01, (0.0, 0.0, 0.0), [0.01])
    with pytest.raises(ValueError, match='below the origin'):
        _shares(cuda, p, d2, None, 0.01, (0.004, 0.006, 0.0), TOL16)
    assert _shares(cuda, p, d2, None, 0.02, (0.0, 0.0, 0.0), [0.01]) == [[2 << 32, 2, 2, 2]]


# ---- end to end ------------------------------------------------------------------------------------------------------------

def _blob(n, centre, radius, rng):
    d = rng.normal(size=(n, 3))
    d *= (radius * rng.random(n) ** (1.0 / 3.0) / np.linalg.norm(d, axis=1))[:, None]
    return (d + np.asarray(centre)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _scene():
    """A scanner at the origin of a cube room with sampled walls; the reconstruction is a third of the wall samples, a blob floating
    in the room (free space: inaccurate) and a blob outside the walls (behind the scan: unobserved)."""
    rng = np.random.default_rng(37)
    walls = ER.box_walls(60000, 2.0, rng)
    inner, outer = _blob(2000, (0.5, 0.5, 0.5), 0.2, rng), _blob(1500, (3.0, 0.3, 0.2), 0.2, rng)
    recon = np.concatenate([walls[::3], inner, outer], 0)
    return _frozen(walls, recon) + (len(inner), len(outer))


OPTIONS = dict(eth3d_voxel=0.05, cube_size=64, vis_window=1, free_space_margin=0.0)


def test_evaluate_with_scans_end_to_end(cuda):
    walls, recon, n_inner, n_outer = _scene()
    tol = [0.02, 0.05]
    plain = eval_cloud.evaluate(recon, walls, tol, device=cuda)
    dist = {}
    got = eval_cloud.evaluate(recon, None, tol, device=cuda, distances=dist, scans=[walls], scanner_origins=[[0.0, 0.0, 0.0]],
                              **OPTIONS)
    assert {k: v for k, v in got.items() if k != 'eth3d'} == plain and set(got) == set(plain) | {'eth3d'}
    e = got['eth3d']
    first = e['tolerances'][0]
    assert first['n_inaccurate'] == n_inner and first['n_unobserved'] == n_outer and first['n_accurate'] == 20000
    assert first['accuracy'] > plain['tolerances'][0]['accuracy'] and first['accuracy'] < 1.0
    assert first['completeness'] < 1.0 and first['voxels_gt'] > first['voxels_recon'] > 0
    # the same through the restatement, from the distances the device found
    cams = eval_eth3d.cube_cameras([0.0, 0.0, 0.0], 64)
    maps = SR.scan_render(walls, cams, 64, 64, 0.5, 0)
    excess, _ = ER.scan_excess(recon, cams, maps, 0.5, 1)
    org = np.floor(np.minimum(recon.min(axis=0), walls.min(axis=0)).astype(np.float64))
    wr = ER.voxel_shares(recon, dist['d2_recon'], excess, 0.05, org, tol, 0.0)
    wg = ER.voxel_shares(walls, dist['d2_gt'], None, 0.05, org, tol, 0.0)
    params = {'voxel': 0.05, 'cube_size': 64, 'vis_window': 1, 'free_space_margin': 0.0, 'n_scanners': 1,
              'scanner_origins': [[0.0, 0.0, 0.0]]}
    assert e == eval_eth3d.metrics(wr, wg, len(recon), tol, params)
    json.dumps(got)                                             # plain Python numbers


def _mlp(path, meshes):
    rows = []
    for name, T in meshes:
        matrix = '' if T is None else '<MLMatrix44>\n%s\n</MLMatrix44>' % '\n'.join(' '.join(repr(float(v)) for v in r) for r in T)
        rows.append('<MLMesh label="%s" filename="%s">%s</MLMesh>' % (name, name, matrix))
    with open(path, 'w') as f:
        f.write('<!DOCTYPE MeshLabDocument>\n<MeshLabProject><MeshGroup>%s</MeshGroup><RasterGroup/></MeshLabProject>\n' % ''.join(rows))


def test_cli_eth3d_from_a_meshlab_project(cuda, tmp_path):
    rng = np.random.default_rng(41)
    a, b = ER.box_walls(9000, 2.0, rng), ER.box_walls(7000, 2.0, rng, centre=(0.5, 0.0, 0.0))
    T = np.eye(4)
    T[:3, 3] = [0.5, 0.25, -0.125]
    recon = np.concatenate([eval_cloud.transform_points(a, T)[::2], _blob(500, (0.5, 0.5, 0.5), 0.2, rng)], 0)
    white = lambda x: np.full((len(x), 3), 255, np.uint8)  # noqa: E731
    for name, pts in (('recon.ply', recon), ('a.ply', a), ('b.ply', b)):
        ply.write_ply(str(tmp_path / name), pts, white(pts))
    _mlp(str(tmp_path / 'scan_alignment.mlp'), [('a.ply', T), ('b.ply', None)])
    base = ['--recon', str(tmp_path / 'recon.ply'), '--tolerances', '0.05,0.1']
    out = str(tmp_path / 'eth3d.json')
    eval_cloud.cli(base + ['--eth3d', '--gt_mlp', str(tmp_path / 'scan_alignment.mlp'), '--cube_size', '32', '--eth3d_voxel', '0.05',
                           '--out', out])
    moved = [eval_cloud.transform_points(a, T), b]
    want = eval_cloud.evaluate(recon, None, [0.05, 0.1], device=cuda, scans=moved, scanner_origins=[T[:3, 3], [0.0, 0.0, 0.0]],
                               eth3d_voxel=0.05, cube_size=32)
    with open(out) as f:
        assert json.load(f) == json.loads(json.dumps(want))
    assert want['eth3d']['n_scanners'] == 2 and want['eth3d']['tolerances'][0]['n_inaccurate'] == 500
    # the same scans by --gt and --scanner_origins, in the frame they are in
    for name, pts in (('a_moved.ply', moved[0]),):
        ply.write_ply(str(tmp_path / name), pts, white(pts))
    np.savetxt(str(tmp_path / 'origins.txt'), np.array([T[:3, 3], [0.0, 0.0, 0.0]]), fmt='%.17g')
    eval_cloud.cli(base + ['--eth3d', '--gt', str(tmp_path / 'a_moved.ply'), str(tmp_path / 'b.ply'), '--scanner_origins',
                           str(tmp_path / 'origins.txt'), '--cube_size', '32', '--eth3d_voxel', '0.05', '--out', out])
    with open(out) as f:
        assert json.load(f) == json.loads(json.dumps(want))
    # without --eth3d the file keeps its bytes
    plain = str(tmp_path / 'plain.json')
    eval_cloud.cli(base + ['--gt', str(tmp_path / 'a_moved.ply'), str(tmp_path / 'b.ply'), '--out', plain])
    expect = eval_cloud.evaluate(recon, np.concatenate(moved, 0), [0.05, 0.1], device=cuda)
    with open(plain) as f:
        assert f.read() == json.dumps(expect, indent=1, sort_keys=True) + '\n'
    assert 'eth3d' not in expect and {k: v for k, v in want.items() if k != 'eth3d'} == expect
