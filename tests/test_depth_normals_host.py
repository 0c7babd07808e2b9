"""CPU: normals from depth maps -- the float64 restatement of the estimator (tests/depth_normals_restated.py) against the analytic
plane normal and on planted cases, the PLY with normals, and every refusal that comes before a launch (SceneFusion, ops, the
driver's option rule, the C entry points)."""
import ctypes

import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
import depth_normals_restated as R
from atvsnet_amd import _lib, ops
from atvsnet_amd.atvsnet import depth_fusion as DF
from atvsnet_amd.atvsnet import eval_pointcloud as E
from atvsnet_amd.tools import ply


# ---------------------------------------------------------------------------------------------------------- the restatement

@pytest.fixture(scope='module')
def plane():
    Ps, depths, _, _, n, _ = R.plane_scene()
    cams = DF.pack_cameras(Ps)
    return cams, depths, n, R.depth_normals(cams, depths)


def _points(cams, depths):
    rows, cols = depths.shape[1:]
    ys, xs = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing='ij')
    return np.stack([R._back_project(cams[v].astype(np.float64), xs, ys, depths[v].astype(np.float64)) for v in range(len(cams))])


def test_plane_normals_are_the_analytic_normal(plane):
    """Every pixel within 1e-3 rad of the plane's normal: four times the residue float32 depth rounding leaves (2.5e-4 measured
    with this restatement), so a formula wrong by degrees fails and rounding does not."""
    cams, depths, n, est = plane
    est = est.astype(np.float64)
    assert np.abs(np.linalg.norm(est, axis=-1) - 1.0).max() < 1e-6           # every pixel has a normal, corners included
    cos = np.abs((est * n).sum(-1)) / np.linalg.norm(est, axis=-1)
    sin = np.linalg.norm(np.cross(est, n), axis=-1)
    angle = np.arctan2(sin, cos)                                              # accurate near 0, unlike arccos
    print('largest angle to the analytic normal: %.3e rad' % angle.max())
    assert angle.max() < 1e-3


def test_plane_normals_face_their_camera(plane):
    cams, depths, n, est = plane
    X = _points(cams, depths)
    C = cams[:, None, None, 21:24].astype(np.float64)
    assert ((est.astype(np.float64) * (C - X)).sum(-1) > 0).all()


def test_corners_use_their_one_quadrant(plane):
    """A corner has one valid quadrant: its normal is that quadrant's cross product alone."""
    cams, depths, n, est = plane
    X = _points(cams, depths)
    for v in range(len(cams)):
        for (y, x), (a, b) in {(0, 0): ((0, 1), (1, 0)), (0, 63): ((1, 63), (0, 62)), (47, 63): ((47, 62), (46, 63)),
                                (47, 0): ((46, 0), (47, 1))}.items():          # (R,D), (D,L), (L,U), (U,R)
            c = np.cross(X[v][a] - X[v, y, x], X[v][b] - X[v, y, x])
            c /= np.linalg.norm(c)
            if c @ (cams[v, 21:24] - X[v, y, x]) < 0:
                c = -c
            assert np.abs(est[v, y, x] - c).max() <= 2.0 ** -23


def test_planted_holes_and_steps_cut_their_quadrants():
    n, rows, cols = 2, 48, 64
    cams = DF.pack_cameras(R.cameras(n, rows, cols))
    depths = R.planted_depths(n, rows, cols)
    X = _points(cams, depths)
    for step in (1, 2):
        est = R.depth_normals(cams, depths, step, 0.02)
        zero = (est == 0).all(-1)
        assert zero[:, 2:5, 5:9].all() and zero[:, rows - 3, 1].all()         # no depth: no normal
        y0, x0 = rows // 4 + 3, cols // 4 + 3
        assert zero[:, y0, x0].all()                                          # depth, but no valid neighbour: (0,0,0)
        if step == 1:
            assert zero[:, rows - 3, 0].all()                                 # R is the hole, L is outside: no quadrant
        assert np.array_equal(zero, _no_quadrant(depths, step, 0.02))         # and nowhere else
        # left of the zero-depth block only the quadrants (D,L) and (L,U) remain; R is cut
        y, x = 3, 5 - step
        c = sum(_unit(np.cross(X[0][a] - X[0, y, x], X[0][b] - X[0, y, x]))
                for a, b in (((y + step, x), (y, x - step)), ((y, x - step), (y - step, x))))
        assert np.abs(est[0, y, x] - _oriented(_unit(c), cams[0], X[0, y, x])).max() <= 2.0 ** -23
        # just above the depth step (rows // 2): D is cut, only (L,U) and (U,R) remain
        y, x = rows // 2 - 1, cols // 2 + 5
        c = sum(_unit(np.cross(X[0][a] - X[0, y, x], X[0][b] - X[0, y, x]))
                for a, b in (((y, x - step), (y - step, x)), ((y - step, x), (y, x + step))))
        assert np.abs(est[0, y, x] - _oriented(_unit(c), cams[0], X[0, y, x])).max() <= 2.0 ** -23
    # a gate wide enough for the 30 % step: the lone pixel (50 %) stays cut, the step no longer is
    wide = R.depth_normals(cams, depths, 1, 0.4)
    assert not np.array_equal(wide[0, rows // 2 - 1, cols // 2 + 5], R.depth_normals(cams, depths, 1, 0.02)[0, rows // 2 - 1, cols // 2 + 5])


def _no_quadrant(depths, step, gate):
    """Pixel by pixel: no depth, or no two cyclically adjacent neighbours of R, D, L, U that are both valid."""
    n, rows, cols = depths.shape
    out = np.zeros(depths.shape, bool)
    d64, gate = depths.astype(np.float64), np.float64(np.float32(gate))
    for v, y, x in np.ndindex(n, rows, cols):
        d = d64[v, y, x]
        ok = []
        for yy, xx in ((y, x + step), (y + step, x), (y, x - step), (y - step, x)):
            inside = 0 <= yy < rows and 0 <= xx < cols
            ok.append(inside and d64[v, yy, xx] > 0 and abs(d64[v, yy, xx] - d) <= gate * d)
        out[v, y, x] = not (d > 0 and any(ok[k] and ok[(k + 1) % 4] for k in range(4)))
    return out


def _unit(v):
    return v / np.linalg.norm(v)


def _oriented(n, cam, X):
    return -n if n @ (cam[21:24].astype(np.float64) - X) < 0 else n


def test_step_two_reads_the_second_neighbours():
    cams = DF.pack_cameras(R.cameras(1, 9, 11))
    depths = R.planted_depths(1, 9, 11, seed=3)
    base = R.depth_normals(cams, depths, 2, 0.02)
    touched = depths.copy()
    touched[0, 4, 6] *= 1.001                          # the first neighbour R of (4, 5): step 2 does not read it
    assert np.array_equal(R.depth_normals(cams, touched, 2, 0.02)[0, 4, 5], base[0, 4, 5])
    assert not np.array_equal(R.depth_normals(cams, touched, 1, 0.02)[0, 4, 5], R.depth_normals(cams, depths, 1, 0.02)[0, 4, 5])
    touched = depths.copy()
    touched[0, 4, 7] *= 1.001                          # the second neighbour
    assert not np.array_equal(R.depth_normals(cams, touched, 2, 0.02)[0, 4, 5], base[0, 4, 5])
    assert (base[0, 0, 0] == 0).sum() == 0             # a corner at step 2 still has its quadrant (R,D)


def test_unit_normals():
    n = np.array([[3, 0, 4], [0, 0, 0], [1e-30, 0, 0], [0.2, 0.2, 0.2]], np.float32)
    got = DF.unit_normals(n)
    assert got.dtype == np.float32 and got.shape == (4, 3)
    assert got[0].tolist() == [np.float32(0.6), 0.0, np.float32(0.8)] and got[1].tolist() == [0, 0, 0] and got[2].tolist() == [1, 0, 0]
    assert np.abs(np.linalg.norm(got[[0, 2, 3]].astype(np.float64), axis=-1) - 1).max() <= 2.0 ** -23


# ------------------------------------------------------------------------------------------------------------------- the PLY

def test_ply_with_normals_round_trips(tmp_path):
    rng = np.random.default_rng(0)
    pts = rng.normal(size=(37, 3)).astype(np.float32)
    cols = rng.integers(0, 256, (37, 3)).astype(np.uint8)
    nrm = DF.unit_normals(rng.normal(size=(37, 3)).astype(np.float32))
    nrm[5] = 0
    nrm[7, 1] = np.nan
    pts[9, 0] = np.inf
    path = str(tmp_path / 'n.ply')
    ply.write_ply(path, pts, cols, nrm)
    want_p, want_n = pts.copy(), nrm.copy()
    want_p[9], want_n[7] = 0, 0
    got_p, got_c, got_n = ply.read_ply_normals(path)
    assert got_p.tobytes() == want_p.tobytes() and got_c.tobytes() == cols.tobytes() and got_n.tobytes() == want_n.tobytes()
    p2, c2 = ply.read_ply(path)
    assert p2.tobytes() == want_p.tobytes() and c2.tobytes() == cols.tobytes()
    assert ply.read_ply_points(path).tobytes() == want_p.tobytes()
    with open(path, 'rb') as f:
        head = f.read().split(b'end_header\n')[0].decode().split('\n')
    assert [h.split()[-1] for h in head if h.startswith('property')] == ['x', 'y', 'z', 'nx', 'ny', 'nz', 'red', 'green', 'blue']
    with pytest.raises(ValueError):
        ply.write_ply(path, pts, cols, nrm[:5])


def test_ply_without_normals_keeps_its_bytes(tmp_path):
    rng = np.random.default_rng(1)
    pts = rng.normal(size=(5, 3)).astype(np.float32)
    cols = rng.integers(0, 256, (5, 3)).astype(np.uint8)
    path = str(tmp_path / 'p.ply')
    ply.write_ply(path, pts, cols)
    vertex = np.dtype([('p', '<f4', 3), ('c', 'u1', 3)])
    body = np.zeros(5, vertex)
    body['p'], body['c'] = pts, cols
    want = (b'ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty float x\nproperty float y\nproperty float z\n'
            b'property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n') + body.tobytes()
    with open(path, 'rb') as f:
        assert f.read() == want
    got = ply.read_ply_normals(path)
    assert got[0].tobytes() == pts.tobytes() and got[1].tobytes() == cols.tobytes() and got[2] is None


# --------------------------------------------------------------------------------------------------- refusals before a launch

def test_scene_fusion_rejects_bad_normal_options():
    for bad in (dict(normals='knn'), dict(normals=None), dict(normals='depth', normal_step=0), dict(normal_step=1.5),
                dict(normals='depth', normal_depth_gate=-0.1), dict(normal_depth_gate=float('nan')),
                dict(normal_depth_gate=float('inf')), dict(normals='depth', normal_threshold=0), dict(normal_threshold=float('nan')),
                dict(normal_threshold=400)):
        with pytest.raises(ValueError):
            DF.SceneFusion(2, 6, 7, device='meta', **bad)
    f = DF.SceneFusion(2, 6, 7, device='meta')
    assert (f.normal_source, f.normal_threshold, f.normal_step, f.normal_depth_gate) == ('fake', 360.0, 1, 0.02)
    assert DF.normal_threshold_radians(f.normal_threshold) == DF.NORMAL_THRESHOLD
    with pytest.raises(RuntimeError):
        f.normals()                                                 # fake normals: nothing to return
    f = DF.SceneFusion(2, 6, 7, device='meta', normals='depth')
    assert f.normal_threshold == DF.DEPTH_NORMAL_THRESHOLD_DEG == 30.0
    assert DF.SceneFusion(2, 6, 7, device='meta', normals='depth', normal_threshold=45, normal_step=2).normal_threshold == 45.0


def test_depth_fusion_main_rejects_bad_normal_options(capsys):
    for argv in (['--normals', 'knn'], ['--normals', 'depth', '--normal_step', '0'], ['--normal_depth_gate', '-1'],
                 ['--normal_threshold', '0']):
        with pytest.raises(SystemExit) as e:
            DF.main(['--dense_folder', '/nonexistent'] + argv)
        assert e.value.code == 2
    capsys.readouterr()


def test_ops_depth_normals_validates_before_launch(monkeypatch):
    from atvsnet_amd.ops import aanet
    calls = []
    monkeypatch.setattr(aanet, '_call', lambda *a: calls.append(a))
    n, r, c = 3, 6, 7
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32)        # noqa: E731
    with pytest.raises(RuntimeError):
        ops.depth_normals(f32(n, 28), f32(n, r, c, 4))              # CPU tensors: no fallback
    for cams, nd, kw, exc in [(f32(n, 27), f32(n, r, c, 4), {}, ValueError), (f32(n + 1, 28), f32(n, r, c, 4), {}, ValueError),
                              (f32(n, 28), f32(n, r, c, 3), {}, ValueError), (f32(n, 28), f32(r, c, 4), {}, ValueError),
                              (f32(n, 28).double(), f32(n, r, c, 4), {}, TypeError), (f32(n, 28), f32(n, r, c, 8)[..., ::2], {}, ValueError),
                              (f32(n, 28), f32(n, r, c, 4), dict(step=0), ValueError),
                              (f32(n, 28), f32(n, r, c, 4), dict(step=1.5), ValueError),
                              (f32(n, 28), f32(n, r, c, 4), dict(depth_gate=-1.0), ValueError),
                              (f32(n, 28), f32(n, r, c, 4), dict(depth_gate=float('nan')), ValueError)]:
        with pytest.raises(exc):
            ops.depth_normals(cams, nd, **kw)
    meta = f32(n, r, c, 4).to('meta')
    assert ops.depth_normals(f32(n, 28).to('meta'), meta, step=2) is meta          # meta: shapes only, no launch
    with pytest.raises(RuntimeError):
        ops.depth_normals(f32(n, 28), meta)                         # meta mixed with another device
    with pytest.raises(RuntimeError):
        ops.fusibile_scene(f32(n, 28), f32(n, r, c, 4), f32(n, r, c, 4), 0.01, 0.5, 2, with_normals=True)
    assert calls == []


def test_option_rule_names_fuse(capsys):
    normals = dict(normals='depth')
    rules = E._option_rules(fuse_normals=normals)
    broken = [message for b, message in rules if b]
    assert len(broken) == 1 and '--fuse_normals' in broken[0] and 'need --fuse' in broken[0]
    assert len(rules) == len(E._option_rules()) + 1
    assert not any(b for b, _ in E._option_rules(fuse=dict(prob_threshold=0.8), fuse_normals=normals))
    with pytest.raises(ValueError, match='need --fuse'):
        E.run_eval_pc('out', [], fuse_normals=normals)
    for argv in (['--fuse_normals', 'depth'], ['--fuse_normal_threshold', '20'], ['--fuse_normal_step', '2'],
                 ['--fuse_normal_depth_gate', '0.1']):
        with pytest.raises(SystemExit) as e:
            E.cli(argv)
        assert e.value.code == 2 and 'need --fuse' in ' '.join(capsys.readouterr().err.split())
    with pytest.raises(SystemExit) as e:
        E.cli(['--fuse', '--fuse_normals', 'depth', '--fuse_normal_step', '0'])
    assert e.value.code == 2 and 'normal_step' in capsys.readouterr().err
    assert E._normal_options(type('A', (), dict(fuse_normals=None, fuse_normal_step=2))()) == dict(normal_step=2)
    assert E._normal_options(type('A', (), {})()) is None


def test_c_entry_points_refuse_before_any_launch():
    names = _lib.declared_symbols()
    for name in ('atvs_depth_normals_f32', 'atvs_fusibile_scene_normals', 'atvs_fusibile_scene_normals_scratch_size'):
        assert name in names
    L = _lib.lib()
    assert _lib.header_abi_version() >= 54 and L.atvs_abi_version() == _lib.header_abi_version()
    buf = (ctypes.c_double * 16)()                                   # a stand-in pointer: refusals come before any launch
    ptr = ctypes.c_void_p(ctypes.addressof(buf))
    NULL, SHAPE, ARG = -1, -2, -3                                    # ATVS_ERR_NULL, ATVS_ERR_SHAPE, ATVS_ERR_ARG
    dn = L.atvs_depth_normals_f32
    assert dn(None, ptr, 2, 6, 7, 1, 0.02, None) == NULL and dn(ptr, None, 2, 6, 7, 1, 0.02, None) == NULL
    for shape in ((0, 6, 7), (2, 0, 7), (2, 6, -1), (2, 32768, 32768), (3, 1, 0x7fffffff)):
        assert dn(ptr, ptr, shape[0], shape[1], shape[2], 1, 0.02, None) == SHAPE, shape
    for step, gate in ((0, 0.02), (-1, 0.02), (1, -0.5), (1, float('nan')), (1, float('inf'))):
        assert dn(ptr, ptr, 2, 6, 7, step, gate, None) == ARG, (step, gate)
    small, large = ctypes.c_long(0), ctypes.c_long(0)
    assert L.atvs_fusibile_scene_scratch_size(3, 37, 53, ctypes.byref(small)) == 0
    assert L.atvs_fusibile_scene_normals_scratch_size(3, 37, 53, ctypes.byref(large)) == 0
    blocks = 3 * ((37 * 53 + 255) // 256)
    assert large.value == small.value + blocks * 256 * 16            # one more float4 region; the plain size is unchanged
    assert small.value == 2 * ((blocks * 4 + 255) // 256 * 256) + blocks * 256 * 16
    assert L.atvs_fusibile_scene_normals_scratch_size(3, 37, 53, None) == NULL
    assert L.atvs_fusibile_scene_normals_scratch_size(0, 37, 53, ctypes.byref(large)) == SHAPE
    fn = L.atvs_fusibile_scene_normals
    cap = 3 * 37 * 53
    good = [ptr, ptr, ptr, 3, 37, 53, 0.01, 0.5, 2, ptr, large.value, ptr, ptr, ptr, cap, ptr, None]
    for k in (0, 1, 2, 9, 11, 12, 13, 15):                            # every pointer, the normals' among them
        assert fn(*[None if i == k else a for i, a in enumerate(good)]) == NULL, k
    assert fn(*[small.value if i == 10 else a for i, a in enumerate(good)]) == SHAPE       # the plain scratch is too short
    assert fn(*[cap - 1 if i == 14 else a for i, a in enumerate(good)]) == SHAPE
    assert fn(*[0 if i == 3 else a for i, a in enumerate(good)]) == SHAPE
