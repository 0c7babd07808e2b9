"""The mesh renderer's definition on the host (no GPU): the known answers of tests/mesh_render_restated.py, the occlusion rule,
ply.read_mesh_any, the ABI version, the wrappers' argument checks on the `meta` device and the new parser errors."""
import os
import struct
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd                                   # noqa: F401
from atvsnet_amd import _lib, ops
from atvsnet_amd.atvsnet import eval_depth, eval_pointcloud, mesh_fusion
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_render_restated as MR  # noqa: E402


def test_known_answer_lattice_square():
    MR.check_lattice(MR.mesh_render)


def test_watertight_sphere():
    MR.check_watertight_sphere(MR.mesh_render)


def test_a_ground_plane_crossing_the_camera_plane():
    rows, cols = 48, 64
    cam = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 50, 50, 32, 23.5], np.float64)
    v = np.array([[-4000, 1, -50], [4000, 1, -50], [0, 1, 4000]], np.float32)         # y points down: the plane one unit below
    depth, face = MR.mesh_render(v, np.array([[0, 1, 2]], np.int32), cam[None], rows, cols, 0.0)
    ry = (np.arange(rows) - 23.5) / 50.0
    assert not depth[0][ry <= 0].any()                               # nothing above the horizon although two vertices lie behind
    below = depth[0][ry > 0]
    assert (below > 0).all() and (face[0][ry > 0] == 0).all()
    want = (1.0 / ry[ry > 0])[:, None]
    assert np.abs(below / want - 1.0).max() <= 1.4e-7


def test_reversed_winding_gives_the_same_maps():
    rows, cols = 37, 53
    cams = MR.ring_cameras(3, rows, cols)
    v, f = MR.triangle_soup(300, cams, rows, cols, seed=3)
    a = MR.mesh_render(v, f, cams, rows, cols, 0.5)
    b = MR.mesh_render(v, f[:, ::-1].copy(), cams, rows, cols, 0.5)
    assert (a[0] > 0).sum() > 1000
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_the_soup_has_what_it_promises():
    rows, cols = 37, 53
    cams = MR.ring_cameras(9, rows, cols)
    v, f = MR.triangle_soup(3000, cams, rows, cols, seed=5)
    C = np.stack([MR.camera_space(v, c)[:, 2] for c in cams])        # (cams, vertices)
    z = C[:, f.reshape(-1)].reshape(len(cams), -1, 3)
    with np.errstate(invalid='ignore'):
        crossing = ((z > 0).any(2) & (z < 0).any(2)).sum()
        behind_all = (z < 0).all(2).all(0).sum()
        behind_some = (z < 0).all(2).any(0).sum()
        near = ((z > 0) & (z < 0.05)).any(2).sum()
    assert crossing > 100 and behind_some > 100 and near > 20
    assert behind_all >= 0 and np.isnan(v).any() and np.isinf(v).any() and (f[:, 0] == f[:, 2]).any()


def test_depth_occlude_rule_on_a_table():
    tol = 0.25                                                       # 1 + tol and 4 * 1.25 = 5 are exact
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    table = [  # depth, occluder, out
        (0.0, 0.0, 0.0), (3.0, 0.0, 3.0), (0.0, 2.0, 0.0), (3.0, 4.0, 3.0), (4.0, 4.0, 4.0), (5.0, 4.0, 5.0),      # equality at 1 + tol
        (np.nextafter(np.float32(5.0), np.float32(6.0)), 4.0, 0.0), (6.0, 4.0, 0.0), (nan, 4.0, nan), (6.0, nan, 6.0),
        (inf, 4.0, 0.0), (6.0, inf, 6.0), (inf, inf, inf), (-1.0, 4.0, -1.0), (6.0, -4.0, 6.0)]
    d, o, want = (np.array(c, np.float32) for c in zip(*table))
    assert np.array_equal(MR.depth_occlude(d, o, tol), want, equal_nan=True)
    assert np.array_equal(MR.depth_occlude(d, o, 0.0)[3:6], np.float32([3.0, 4.0, 0.0]))


def _ply_bytes(fmt, with_extras, quad=False, name='vertex_indices'):
    v = np.array([[0, 0, 0], [1, 0, 0.5], [0, 1, 0.25], [1, 1, -2]], np.float64)
    faces = [[0, 1, 2, 3]] if quad else [[0, 1, 2], [2, 1, 3]]
    head = ['ply', 'format %s 1.0' % fmt, 'comment a third-party file', 'element vertex 4', 'property double x', 'property float y']
    head += ['property uchar red'] if with_extras else []
    head += ['property float z', 'element face %d' % len(faces)]
    head += ['property uchar flags'] if with_extras else []
    head += ['property list ushort uint %s' % name, 'end_header']
    out = ('\n'.join(head) + '\n').encode('ascii')
    if fmt == 'ascii':
        for p in v:
            out += ('%r %r %s%r\n' % (float(p[0]), float(p[1]), '7 ' if with_extras else '', float(p[2]))).encode('ascii')
        for f in faces:
            out += ('%s%d %s\n' % ('1 ' if with_extras else '', len(f), ' '.join(str(i) for i in f))).encode('ascii')
        return out, v, faces
    e = '<' if fmt == 'binary_little_endian' else '>'
    for p in v:
        out += struct.pack(e + 'df', p[0], p[1]) + (b'\x07' if with_extras else b'') + struct.pack(e + 'f', p[2])
    for f in faces:
        out += (b'\x01' if with_extras else b'') + struct.pack(e + 'H%dI' % len(f), len(f), *f)
    return out, v, faces


@pytest.mark.parametrize('fmt', ['ascii', 'binary_little_endian', 'binary_big_endian'])
def test_read_mesh_any(tmp_path, fmt):
    for extras, name in ((False, 'vertex_indices'), (True, 'vertex_index')):
        data, v, faces = _ply_bytes(fmt, extras, name=name)
        path = tmp_path / ('m_%s_%d.ply' % (fmt, extras))
        path.write_bytes(data)
        gv, gf = ply.read_mesh_any(str(path))
        assert gv.dtype == np.float32 and gf.dtype == np.int32
        assert np.array_equal(gv, v.astype(np.float32)) and np.array_equal(gf, np.array(faces, np.int32))
    data, _, _ = _ply_bytes(fmt, True, quad=True)
    path = tmp_path / 'quad.ply'
    path.write_bytes(data)
    with pytest.raises(ValueError, match='quad.ply.*4 corners'):
        ply.read_mesh_any(str(path))
    path.write_bytes(_ply_bytes(fmt, False)[0][:-3])
    with pytest.raises(ValueError, match='quad.ply'):
        ply.read_mesh_any(str(path))


def test_load_meshes_reads_both_kinds_and_offsets_the_faces(tmp_path):
    data, v, faces = _ply_bytes('ascii', False)
    (tmp_path / 'a.ply').write_bytes(data)
    ply.write_mesh(str(tmp_path / 'b.ply'), v.astype(np.float32), None, np.array(faces, np.int32))
    gv, gf = eval_depth.load_meshes([str(tmp_path / 'a.ply'), str(tmp_path / 'b.ply')])
    assert np.array_equal(gv, np.concatenate([v, v]).astype(np.float32))
    assert np.array_equal(gf, np.concatenate([np.array(faces), np.array(faces) + 4]).astype(np.int32)) and gf.dtype == np.int32


def test_abi_version_and_symbols():
    L = _lib.lib()
    assert _lib.header_abi_version() >= 59 and L.atvs_abi_version() == _lib.header_abi_version()
    for name in ('atvs_mesh_render_scratch_size', 'atvs_mesh_render', 'atvs_depth_occlude'):
        assert name in _lib.declared_symbols() and hasattr(L, name)
    assert ops.MESH_RENDER_SMALL_PIXELS == _lib.header_macro('ATVS_MESH_RENDER_SMALL_PIXELS') >= 16


def test_the_c_abi_refuses_bad_arguments_without_a_launch():
    import ctypes
    L = _lib.lib()
    n = ctypes.c_long(0)
    assert L.atvs_mesh_render_scratch_size(2, 37, 53, 10, ctypes.byref(n)) == 0 and n.value >= 2 * 37 * 53 * 8
    assert L.atvs_mesh_render_scratch_size(2, 37, 53, 10, None) == -1
    assert L.atvs_mesh_render_scratch_size(0, 37, 53, 10, ctypes.byref(n)) == -2
    assert L.atvs_mesh_render_scratch_size(2, 1 << 15, 1 << 15, 10, ctypes.byref(n)) == -2
    assert L.atvs_mesh_render_scratch_size(2, 37, 53, 1 << 31, ctypes.byref(n)) == -2
    assert L.atvs_mesh_render(None, 0, None, 0, None, 1, 4, 4, 0.0, None, 0, None, None, None, None) == -1
    assert L.atvs_mesh_render(8, 1, 8, 1, 8, 1, 4, 4, float('nan'), 8, 1 << 30, 8, 8, 8, None) == -3
    assert L.atvs_mesh_render(8, 1, 8, 1, 8, 1, 4, 4, 0.0, 8, 16, 8, 8, 8, None) == -2          # a short scratch
    assert L.atvs_mesh_render(8, 1, 8, 1, 8, 0, 4, 4, 0.0, 8, 1 << 30, 8, 8, 8, None) == -2
    assert L.atvs_depth_occlude(8, 8, 4, -1.0, 8, None) == -3
    assert L.atvs_depth_occlude(None, 8, 4, 0.0, 8, None) == -1
    assert L.atvs_depth_occlude(8, 8, -1, 0.0, 8, None) == -2
    assert L.atvs_depth_occlude(None, None, 0, 0.0, None, None) == 0


def _meta(shape, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device='meta')


def test_the_wrappers_argument_errors():
    v, f, c = _meta((5, 3)), _meta((2, 3), torch.int32), _meta((2, 16), torch.float64)
    depth, face = ops.mesh_render(v, f, c, 4, 6)                     # the host checks alone run on `meta`
    assert tuple(depth.shape) == (2, 4, 6) and depth.dtype == torch.float32 and face.dtype == torch.int32
    with pytest.raises(TypeError, match='vertices'):
        ops.mesh_render(v.double(), f, c, 4, 6)
    with pytest.raises(TypeError, match='faces'):
        ops.mesh_render(v, f.long(), c, 4, 6)
    with pytest.raises(TypeError, match='cams'):
        ops.mesh_render(v, f, c.float(), 4, 6)
    with pytest.raises(ValueError, match='faces'):
        ops.mesh_render(v, _meta((2, 4), torch.int32), c, 4, 6)
    with pytest.raises(ValueError, match='vertices'):
        ops.mesh_render(_meta((5, 2)), f, c, 4, 6)
    with pytest.raises(ValueError, match='cams'):
        ops.mesh_render(v, f, _meta((2, 18), torch.float64), 4, 6)
    with pytest.raises(ValueError, match='cameras'):
        ops.mesh_render(v, f, c[:0], 4, 6)
    with pytest.raises(ValueError, match='2\\^31'):
        ops.mesh_render(v, f, c, 1 << 15, 1 << 15)
    with pytest.raises(ValueError, match='rows'):
        ops.mesh_render(v, f, c, 0, 6)
    with pytest.raises(ValueError, match='pixel_centre'):
        ops.mesh_render(v, f, c, 4, 6, pixel_centre=float('inf'))
    with pytest.raises(RuntimeError, match='faces'):
        ops.mesh_render(v, torch.zeros((2, 3), dtype=torch.int32), c, 4, 6)
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.mesh_render(torch.zeros(5, 3), torch.zeros((2, 3), dtype=torch.int32), torch.zeros((2, 16), dtype=torch.float64), 4, 6)
    d = _meta((2, 4, 6))
    assert tuple(ops.depth_occlude(d, d.clone()).shape) == (2, 4, 6)
    with pytest.raises(ValueError, match='tol'):
        ops.depth_occlude(d, d, tol=-0.1)
    with pytest.raises(ValueError, match='occluder'):
        ops.depth_occlude(d, _meta((2, 4, 5)))
    with pytest.raises(TypeError, match='occluder'):
        ops.depth_occlude(d, d.double())
    with pytest.raises(ValueError, match='out'):
        ops.depth_occlude(d, d, out=_meta((2, 4, 5)))
    with pytest.raises(RuntimeError, match='occluder'):
        ops.depth_occlude(d, torch.zeros(2, 4, 6))


def test_report_gains_its_keys_only_when_asked():
    pred = np.ones((1, 12, 12), np.float32)
    plain = eval_depth.report(pred, pred)
    assert not {'occlusion_mesh_tol', 'occlusion_faces', 'gt_mesh'} & set(plain)
    used = eval_depth.report(pred, pred, occlusion_mesh_tol=0.02, occlusion_faces=7, gt_mesh=2)
    assert used['occlusion_mesh_tol'] == 0.02 and used['occlusion_faces'] == 7 and used['gt_mesh'] == 2
    assert repr(dict((k, v) for k, v in sorted(used.items()) if k in plain)) == repr(dict(sorted(plain.items())))    # NaNs and all
    assert eval_depth.DEFAULT_OCCLUDER_TOL == 0.01


def test_command_lines_refuse(capsys, tmp_path):
    def refused(cli, argv, text):
        with pytest.raises(SystemExit) as e:
            cli(argv)
        assert e.value.code == 2 and text in ' '.join(capsys.readouterr().err.split())

    maps, scan = tmp_path / 'maps', tmp_path / 'scan.ply'
    maps.mkdir()
    scan.write_bytes(b'')
    refused(eval_depth.cli, ['--maps', str(maps)], 'exactly one of --gt and --gt_mesh')
    refused(eval_depth.cli, ['--maps', str(maps), '--gt', str(scan), '--gt_mesh', str(scan)], 'exactly one of --gt and --gt_mesh')
    refused(eval_depth.cli, ['--maps', str(maps), '--gt', str(scan), '--occlusion_mesh_tol', '0.1'], 'needs --occlusion_mesh')
    refused(eval_depth.cli, ['--maps', str(maps), '--gt', str(scan), '--occlusion_mesh', str(scan), '--occlusion_mesh_tol', '-1'],
            '--occlusion_mesh_tol must be >= 0')
    refused(eval_depth.cli, ['--maps', str(maps), '--gt', str(scan), '--occlusion_mesh', str(tmp_path / 'none.ply')], 'no such file')
    refused(eval_depth.cli, ['--maps', str(maps), '--gt_mesh', ','], '--gt_mesh names no file')
    refused(eval_pointcloud.cli, ['--fuse', '--gt_ply', 'a.ply', '--map_occlusion_mesh', 'm.ply'], 'need --score_maps')
    refused(eval_pointcloud.cli, ['--fuse', '--gt_ply', 'a.ply', '--map_occlusion_mesh_tol', '0.1'], 'need --score_maps')
    refused(eval_pointcloud.cli, ['--fuse', '--gt_ply', 'a.ply', '--score_maps', '--map_occlusion_mesh_tol', '0.1'],
            '--map_occlusion_mesh_tol needs --map_occlusion_mesh')
    refused(eval_pointcloud.cli, ['--fuse', '--gt_ply', 'a.ply', '--score_maps', '--map_occlusion_mesh', 'm.ply',
                                  '--map_occlusion_mesh_tol', '-1'], '--map_occlusion_mesh_tol')
    refused(eval_pointcloud.cli, ['--fuse', '--mesh_render'], '--mesh_render needs --mesh_voxel')
    assert '--render' in mesh_fusion.make_parser().format_help()
