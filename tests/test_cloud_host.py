"""CPU: the host side of the point-cloud scoring -- tools/ply.read_ply_points, eval_cloud.metrics, the argument checks of
ops.cloud_* (no CPU fallback), the command lines' refusals, and the library's new entry points."""
import os
import struct
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd                                   # noqa: F401
from atvsnet_amd import _lib, ops
from atvsnet_amd.atvsnet import eval_cloud
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_restated as CR  # noqa: E402

PTS = np.array([[0.5, -1.25, 3.0], [1e-3, 2.0, -7.5], [100.0, 0.0, 0.125]], np.float64)


def _write(path, header, body):
    with open(path, 'wb') as f:
        f.write(('ply\n' + header + 'end_header\n').encode('ascii'))
        f.write(body)


def test_read_ply_points_ascii_with_extra_properties_and_faces(tmp_path):
    p = str(tmp_path / 'a.ply')
    body = ''.join('7 %r %r 200 %r 0.5\n' % (x, y, z) for x, y, z in PTS.tolist()) + '3 0 1 2\n'
    _write(p, 'format ascii 1.0\ncomment made by hand\nelement vertex 3\nproperty int id\nproperty float x\nproperty float y\n'
              'property uchar red\nproperty float z\nproperty float quality\nelement face 1\nproperty list uchar int vertex_indices\n',
           body.encode('ascii'))
    got = ply.read_ply_points(p)
    assert got.dtype == np.float32 and got.shape == (3, 3) and np.array_equal(got, PTS.astype(np.float32))


@pytest.mark.parametrize('fmt,order', [('binary_little_endian', '<'), ('binary_big_endian', '>')])
def test_read_ply_points_binary_float_and_double(tmp_path, fmt, order):
    # doubles that are not float32 values: rounded once
    pts = PTS + 1e-9
    p = str(tmp_path / 'd.ply')
    body = b''.join(struct.pack(order + 'hdBdd', 5, x, 9, y, z) for x, y, z in pts) + struct.pack(order + 'Biii', 3, 0, 1, 2)
    _write(p, 'format %s 1.0\nelement vertex 3\nproperty short s\nproperty double x\nproperty uchar c\nproperty double y\n'
              'property double z\nelement face 1\nproperty list uchar int vertex_indices\n' % fmt, body)
    assert np.array_equal(ply.read_ply_points(p), pts.astype(np.float32))
    p = str(tmp_path / 'f.ply')
    body = b''.join(struct.pack(order + 'fffi', z, y, x, 1) for x, y, z in PTS)
    _write(p, 'format %s 1.0\nelement vertex 3\nproperty float z\nproperty float y\nproperty float x\nproperty int n\n' % fmt, body)
    assert np.array_equal(ply.read_ply_points(p), PTS.astype(np.float32))


def test_read_ply_points_of_a_write_ply_file(tmp_path):
    p = str(tmp_path / 'w.ply')
    pts = np.array([[1, 2, 3], [np.nan, 0, 1], [4, 5, np.inf], [-1, -2, -3]], np.float32)
    ply.write_ply(p, pts, np.arange(12, dtype=np.uint8).reshape(4, 3))
    want, _ = ply.read_ply(p)
    got = ply.read_ply_points(p)
    assert np.array_equal(got, want) and np.array_equal(got[1], [0, 0, 0]) and np.array_equal(got[2], [0, 0, 0])


def test_read_ply_points_errors_name_the_file(tmp_path):
    p = str(tmp_path / 'list.ply')
    _write(p, 'format ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n'
              'property list uchar int seen\n', b'0 0 0 0\n')
    with pytest.raises(ValueError, match='list.ply.*list property'):
        ply.read_ply_points(p)
    p = str(tmp_path / 'noz.ply')
    _write(p, 'format ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\n', b'0 0\n')
    with pytest.raises(ValueError, match="noz.ply.*'z'"):
        ply.read_ply_points(p)
    p = str(tmp_path / 'short.ply')
    _write(p, 'format binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n',
           struct.pack('<8f', *range(8)))
    with pytest.raises(ValueError, match='short.ply.*truncated'):
        ply.read_ply_points(p)
    p = str(tmp_path / 'short_ascii.ply')
    _write(p, 'format ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n', b'0 0 0\n')
    with pytest.raises(ValueError, match='short_ascii.ply.*truncated'):
        ply.read_ply_points(p)


def test_metrics_by_hand():
    inf = np.float32(np.inf)
    # distances 0, 0.5 (d2 = 0.25 exactly), 1, 2, not found  |  0.5, 0.5, 3, not found, not found, not found, 0
    d2_recon = np.array([0.0, 0.25, 1.0, 4.0, inf], np.float32)
    d2_gt = np.array([0.25, 0.25, 9.0, inf, inf, inf, 0.0], np.float32)
    m = eval_cloud.metrics(d2_recon, d2_gt, [0.5, 1.0, 4.0], 4.0)
    assert (m['n_recon'], m['n_gt'], m['radius']) == (5, 7, 4.0)
    assert (m['not_found_recon'], m['not_found_gt']) == (1, 3)
    assert m['mean_recon'] == (0 + 0.5 + 1 + 2 + 4) / 5.0 and m['median_recon'] == 1.0
    assert m['mean_gt'] == (0.5 + 0.5 + 3 + 4 + 4 + 4 + 0) / 7.0 and m['median_gt'] == 3.0
    t = m['tolerances']
    assert [x['tolerance'] for x in t] == [0.5, 1.0, 4.0]
    # tau = 0.5 equals a distance exactly: counted
    assert (t[0]['accuracy'], t[0]['completeness']) == (2 / 5.0, 3 / 7.0)
    assert t[0]['f1'] == 2 * (2 / 5.0) * (3 / 7.0) / (2 / 5.0 + 3 / 7.0)
    assert (t[1]['accuracy'], t[1]['completeness']) == (3 / 5.0, 3 / 7.0)
    assert (t[2]['accuracy'], t[2]['completeness']) == (4 / 5.0, 4 / 7.0)
    assert (t[2]['n_recon_within'], t[2]['n_gt_within']) == (4, 4)
    # both shares 0 -> f1 0
    z = eval_cloud.metrics(np.array([inf, 4.0], np.float32), np.array([inf], np.float32), [1.0], 2.0)['tolerances'][0]
    assert (z['accuracy'], z['completeness'], z['f1']) == (0.0, 0.0, 0.0)
    # empty clouds
    e = eval_cloud.metrics(np.zeros(0, np.float32), np.array([inf, inf], np.float32), [1.0], 1.0)
    assert (e['n_recon'], e['mean_recon'], e['median_recon'], e['not_found_recon']) == (0, None, None, 0)
    assert (e['mean_gt'], e['not_found_gt']) == (1.0, 2) and e['tolerances'][0]['f1'] == 0.0
    e = eval_cloud.metrics(np.zeros(0, np.float32), np.zeros(0, np.float32), [1.0], 1.0)
    assert e['tolerances'][0] == {'tolerance': 1.0, 'accuracy': 0.0, 'completeness': 0.0, 'f1': 0.0, 'n_recon_within': 0,
                                  'n_gt_within': 0}
    with pytest.raises(ValueError, match='outside'):
        eval_cloud.metrics(d2_recon, d2_gt, [0.5, 5.0], 4.0)
    # the counts of the device path are taken as given
    c = eval_cloud.metrics(d2_recon, d2_gt, [0.5], 4.0, counts=([2], [3]))
    assert c['tolerances'][0] == t[0]


def test_default_radius_is_the_largest_tolerance_rounded_up_to_float32():
    tol, r = eval_cloud._check_tolerances([0.01, 0.1], None)
    assert r >= 0.1 and np.float32(r) == r and r - 0.1 < 1e-8
    tol, r = eval_cloud._check_tolerances([0.01], None)           # float32(0.01) < 0.01: the next float32 up
    assert r >= 0.01 and np.float32(r) == r and r - 0.01 < 1e-9


def test_restatement_of_the_trap_pair():
    """With a cell edge of exactly R a neighbour two cells away can pass the float32 test: R = 0.25, query x = 0.25 - 2^-26 (cell 0),
    reference x = 0.5 (cell 2) are further than R apart, yet dx rounds to 0.25 and d2 = 0.0625 = R * R exactly: found.  (The same
    query with the reference at 0.5 + 2^-20 has dx = 0.25 + 2^-20 after rounding and d2 > R * R: not found.  Both pairs are in the
    GPU tests.)"""
    q = np.array([[0.25 - 2.0 ** -26, 0, 0]], np.float32)
    assert float(q[0, 0]) == 0.25 - 2.0 ** -26
    p = np.array([[0.5, 0, 0]], np.float32)
    d2, idx = CR.nearest(q, p, 0.25)
    assert d2[0] == np.float32(0.0625) and idx[0] == 0 and float(p[0, 0]) - float(q[0, 0]) > 0.25
    p = np.array([[0.5 + 2.0 ** -20, 0, 0]], np.float32)
    assert float(p[0, 0]) == 0.5 + 2.0 ** -20
    d2, idx = CR.nearest(q, p, 0.25)
    assert np.isinf(d2[0]) and idx[0] == -1


def test_ops_cloud_refuse_bad_arguments_no_fallback():
    P = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.cloud_grid(P, 0.5)
    with pytest.raises(TypeError):
        ops.cloud_grid(torch.empty(5, 3, dtype=torch.float64, device='meta'), 0.5)
    with pytest.raises(TypeError):
        ops.cloud_grid(np.zeros((5, 3), np.float32), 0.5)
    with pytest.raises(ValueError, match='shape'):
        ops.cloud_grid(torch.empty(5, 4, device='meta'), 0.5)
    with pytest.raises(ValueError, match='contiguous'):
        ops.cloud_grid(torch.empty(3, 5, device='meta').t(), 0.5)
    for r in (0.0, -1.0, float('nan'), float('inf'), 1e39):
        with pytest.raises(ValueError, match='radius'):
            ops.cloud_grid(torch.empty(5, 3, device='meta'), r)
    with pytest.raises(TypeError, match='CloudGrid'):
        ops.cloud_nearest(P, P)
    g = ops.CloudGrid(torch.empty(0, dtype=torch.uint8), 0, 1.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.cloud_nearest(g, P)
    with pytest.raises(TypeError):
        ops.cloud_nearest(g, P.double())
    with pytest.raises(ValueError, match='shape'):
        ops.cloud_nearest(g, torch.zeros(5, 2))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.cloud_counts(torch.zeros(4), [0.5], 1.0)
    with pytest.raises(ValueError, match='tolerance'):
        ops.cloud_counts(torch.empty(4, device='meta'), [0.5, 1.5], 1.0)
    with pytest.raises(ValueError, match='tolerances'):
        ops.cloud_counts(torch.empty(4, device='meta'), [0.1] * 17, 1.0)


def test_library_exports_the_cloud_entry_points_and_checks_arguments_on_the_host():
    import ctypes
    names = _lib.declared_symbols()
    new = ['atvs_cloud_grid_scratch_size', 'atvs_cloud_grid_build', 'atvs_cloud_nearest_scratch_size', 'atvs_cloud_nearest',
           'atvs_cloud_counts']
    L = _lib.lib()
    for n in new:
        assert n in names and hasattr(L, n), n
    assert _lib.header_abi_version() >= 48
    assert 'cloud' not in _lib.OWNS_ITS_SIMD and '-ffp-contract=off' in _lib.flags_for(os.path.join(_lib.CSRC, 'cloud.hip'))
    nbytes = ctypes.c_long(0)
    lng, flt = ctypes.c_long, ctypes.c_float
    assert L.atvs_cloud_grid_scratch_size(lng(1000), ctypes.byref(nbytes)) == 0
    # O(n + cells): 16 + 4 bytes per point, 4 bytes per cell of at most max(4096, 8 n) cells, the header and alignment
    assert 0 < nbytes.value <= 1000 * 20 + 4 * (8 * 1000 + 2) + 4096
    assert L.atvs_cloud_grid_scratch_size(lng((1 << 30) + 1), ctypes.byref(nbytes)) == -2
    assert L.atvs_cloud_grid_scratch_size(lng(-1), ctypes.byref(nbytes)) == -2
    assert L.atvs_cloud_nearest_scratch_size(lng(10), lng((1 << 30) + 1), ctypes.byref(nbytes)) == -2
    fake = ctypes.c_void_p(256)                     # never dereferenced: every call below is refused before a launch
    for r in (0.0, -1.0, float('nan'), float('inf')):
        assert L.atvs_cloud_grid_build(fake, lng(10), flt(r), fake, lng(1 << 30), None) == -3, r
    assert L.atvs_cloud_grid_build(fake, lng(10), flt(1.0), fake, lng(64), None) == -2          # short grid buffer
    assert L.atvs_cloud_grid_build(fake, lng((1 << 30) + 1), flt(1.0), fake, lng(1 << 30), None) == -2
    assert L.atvs_cloud_nearest(fake, lng(64), lng(10), fake, lng(10), fake, lng(1 << 30), fake, fake, None) == -2
    assert L.atvs_cloud_nearest(fake, lng(1 << 30), lng(10), fake, lng(10), fake, lng(64), fake, fake, None) == -2
    tol = (ctypes.c_double * 2)(0.5, 1.5)
    assert L.atvs_cloud_counts(fake, lng(10), tol, 2, flt(1.0), fake, None) == -3               # a tolerance above R
    assert L.atvs_cloud_counts(fake, lng(10), tol, 17, flt(2.0), fake, None) == -2
    assert L.atvs_cloud_counts(fake, lng(10), tol, 2, flt(0.0), fake, None) == -3


def test_command_lines_refuse(tmp_path, capsys):
    from atvsnet_amd.atvsnet import eval_pointcloud
    with pytest.raises(SystemExit) as e:
        eval_pointcloud.cli(['--scene_cache', '--gt_ply', 'gt.ply'])
    assert e.value.code == 2 and '--gt_ply needs --fuse' in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        eval_cloud.cli(['--recon', 'a.ply', '--gt', 'b.ply', '--tolerances', '0.1,0.5', '--radius', '0.2'])
    assert e.value.code == 2 and 'outside [0, radius' in capsys.readouterr().err
