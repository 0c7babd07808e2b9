"""The mesh smoothing on the host (no GPU): the numpy restatement's own properties (tests/mesh_smooth_restated.py on the cases of
tests/mesh_smooth_cases.py: what Taubin's filter does to a noisy sphere and what Laplacian smoothing does, the pinned sheet, the dirty
mesh by hand, independence of the faces' order, the normals), the header's symbols and the C entry points' refusals, the argument
errors of ops, of atvsnet/smooth_mesh.py and of mesh_fusion.check_smooth, the driver's rules with and without smooth=, the PLY
layout with vertex normals, and the rows of the buffer contract."""
import argparse
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
from atvsnet_amd import _lib, ops
from atvsnet_amd.atvsnet import eval_pointcloud, mesh_fusion, smooth_mesh
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buffer_contract_rows as BR  # noqa: E402
import mesh_smooth_cases as C  # noqa: E402
import mesh_smooth_contract_rows as MR  # noqa: E402
import mesh_smooth_restated as R  # noqa: E402

NAMES = ('atvs_mesh_adjacency_scratch_size', 'atvs_mesh_adjacency', 'atvs_mesh_quantize', 'atvs_mesh_smooth_pass', 'atvs_mesh_dequantize',
         'atvs_mesh_face_extent', 'atvs_mesh_vertex_normal_sums', 'atvs_mesh_vertex_normals')


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _radii(v):
    return np.linalg.norm(np.asarray(v, np.float64), axis=1)


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_taubin_smooths_the_noisy_sphere_without_shrinking_it_and_laplacian_shrinks_it():
    """Measured with the restatement on the committed icosphere (642 vertices, 1280 faces):

                                      std of radii            mean radius
        input                         0.018555                0.997517
        10 Taubin iterations          0.007845 (ratio 0.4228) 1.000508 (moved by 0.002991)
        10 Laplacian iterations       0.004700                0.942512

    inside the bars the issue sets (ratio <= 0.5, move <= 0.005, Laplacian mean radius < 0.95): the bars stand as stated."""
    v, f = C.mesh('noisy_sphere')
    assert v.shape == (642, 3) and f.shape == (1280, 3)
    before = _radii(v)
    taubin, info = R.smooth(v, f, 10)
    after = _radii(taubin)
    laplacian = _radii(R.smooth(v, f, 10, 0.5, None)[0])
    print('radii: std %.6f -> %.6f (ratio %.4f), mean %.6f -> %.6f (moved by %.6f); Laplacian: std %.6f, mean %.6f' % (
        before.std(), after.std(), after.std() / before.std(), before.mean(), after.mean(), abs(after.mean() - before.mean()),
        laplacian.std(), laplacian.mean()))
    assert after.std() <= 0.5 * before.std()
    assert abs(after.mean() - before.mean()) <= 0.005
    assert laplacian.mean() < 0.95
    assert info['clamped'] == 0 and info['passes'] == 20 and info['boundary_pairs'] == 0 and info['pairs'] == 1920


def test_the_pinned_sheet_returns_its_input_bits_and_the_free_one_pulls_its_corners_in():
    v, f = C.mesh('sheet')
    for iterations in (1, 3, 10):
        out, info = R.smooth(v, f, iterations, pin_boundary=True)
        assert np.array_equal(_bits(out), _bits(v))
    assert info['boundary_pairs'] == 24 and info['pairs'] == 2 * 6 * 7 + 36
    out, _ = R.smooth(v, f, 3)
    centre = v.astype(np.float64).mean(0)
    corners = [0, 6, 42, 48]
    assert (np.linalg.norm(out[corners] - centre, axis=1) < np.linalg.norm(v[corners] - centre, axis=1)).all()
    assert np.array_equal(_bits(out[:, 2]), _bits(v[:, 2]))                      # a flat sheet stays in its plane, bit for bit
    noisy, _ = C.mesh('noisy_sheet')
    smoothed, _ = R.smooth(noisy, f, 5, pin_boundary=True)
    inner = np.ones(49, bool).reshape(7, 7)
    inner[0], inner[-1], inner[:, 0], inner[:, -1] = False, False, False, False
    inner = inner.reshape(-1)
    assert np.array_equal(_bits(smoothed[~inner]), _bits(noisy[~inner])) and smoothed[inner, 2].std() < noisy[inner, 2].std()


def test_the_dirty_mesh_is_what_the_case_says_by_hand():
    v, f = C.mesh('dirty')
    got = R.adjacency(v, f)
    assert got['degree'].tolist() == C.DIRTY['degree'] and got['flags'].tolist() == C.DIRTY['flags'] and got['info'] == C.DIRTY['info']
    assert got['offsets'].tolist() == np.concatenate([[0], np.cumsum(C.DIRTY['degree'])]).tolist()
    rows = [got['neighbours'][got['offsets'][k]:got['offsets'][k + 1]].tolist() for k in range(len(v))]
    assert rows == [[1, 2, 4], [0, 2, 3, 9], [0, 1, 3], [1, 2, 9, 10], [0], [], [], [], [], [1, 3, 10], [3, 9]]
    out, info = R.smooth(v, f, 3)
    stay = [5, 6, 7, 8]                                                 # isolated, unnamed, NaN, inf: the input bits
    assert np.array_equal(_bits(out[stay]), _bits(v[stay])) and info['nonfinite_vertices'] == 2
    assert np.isfinite(out[[0, 1, 2, 3, 4, 9, 10]]).all() and (_bits(out[:5]) != _bits(v[:5])).any(1).all()
    one_bad, _ = R.adjacency(v, np.concatenate([f, [[0, 1, 11]]]).astype(np.int32)), None
    assert one_bad['info'] == dict(C.DIRTY['info'], skipped_index_faces=1)


@pytest.mark.parametrize('name', ['noisy_sphere', 'fan', 'dirty', 'noisy_sheet'])
def test_any_order_of_the_faces_and_any_rotation_of_a_face_give_the_same_q_after_every_pass(name):
    v, f = C.mesh(name)
    want = C.restated(name)
    rng = np.random.default_rng(17)
    for _ in range(2):
        g = f[rng.permutation(len(f))]
        g = np.take_along_axis(g, (np.arange(3)[None, :] + rng.integers(0, 3, len(g))[:, None]) % 3, 1)
        trace = []
        out, _ = R.smooth(v, g, C.ITERATIONS, C.TAUBIN[0], C.TAUBIN[1], trace=trace)
        assert len(trace) == 7 and all(np.array_equal(a, b) for a, b in zip(trace, want['trace']))
        assert np.array_equal(_bits(out), _bits(want['out']))
        sums, incidences = R.vertex_normal_sums(v, g, want['extent']['max_extent'] or 1.0)
        assert np.array_equal(sums, want['sums']) and np.array_equal(incidences, want['incidences'])


def test_normals_of_the_sphere_are_radial_and_point_outward_and_dirty_vertices_get_zeros():
    """Measured with the restatement on sphere4 (2562 vertices, 5120 faces): the largest angle between a vertex normal and the radial
    direction is 0.0059068 rad; the bar is 1.5 times that."""
    v, f = C.mesh('sphere4')
    assert v.shape == (2562, 3) and f.shape == (5120, 3)
    n = C.restated('sphere4')['normals'].astype(np.float64)
    radial = v.astype(np.float64) / _radii(v)[:, None]
    cosine = (n * radial).sum(1)
    angle = np.arccos(np.clip(cosine, -1.0, 1.0))
    print('sphere4: the largest angle to the radial direction is %.7f rad' % angle.max())
    assert (cosine > 0.0).all() and angle.max() <= 1.5 * 0.0059068
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-6
    assert (C.restated('sphere4')['incidences'] >= 5).all()
    d = C.restated('dirty')
    assert not d['normals'][[4, 5, 6, 7, 8]].any() and d['incidences'][[4, 5, 6, 7, 8]].tolist() == [0, 0, 0, 0, 0]
    assert np.abs(np.linalg.norm(d['normals'][[0, 1, 2, 3, 9, 10]].astype(np.float64), axis=1) - 1.0).max() < 1e-6
    assert d['extent'] == dict(max_extent=d['extent']['max_extent'], usable_faces=7, skipped_index_faces=0, nonfinite_faces=2)
    # a saturating unit: with area_unit far below every face, every face votes 1
    flat, g = C.mesh('sheet')
    assert np.array_equal(R.vertex_normals(flat, g, 1e-6), np.tile(np.float32([0, 0, 1]), (49, 1)))
    assert np.array_equal(R.vertex_normals(flat, g), np.tile(np.float32([0, 0, 1]), (49, 1)))


def test_the_lattice_holds_the_box_in_two_to_the_31_steps():
    for name in C.NAMES:
        v, f = C.mesh(name)
        origin, step = R.lattice(v)
        o, s = ops.mesh_smooth_lattice(*((v[np.isfinite(v).all(1)].min(0), v[np.isfinite(v).all(1)].max(0)) if len(v) else (np.zeros(3), np.zeros(3))))
        assert s == step and np.array_equal(o, origin) and np.frexp(step)[0] == 0.5
        q, info = R.quantize(v, origin, step)
        assert info['far_coordinates'] == 0 and np.abs(q).max(initial=0) <= 1 << 31
        back = R.dequantize(q + 1, q, v, origin, step)                         # every coordinate moved by one step
        fin = np.isfinite(v).all(1)                                            # (a vertex that is not finite has the row 0, 0, 0)
        # half a step of quantisation, the step itself, and one rounding to float32 of a value at most two steps from v
        assert (np.abs(back[fin].astype(np.float64) - v[fin]) <= 1.5 * step + np.spacing(np.abs(v[fin]) + np.float32(2 * step)).astype(np.float64)).all()
    assert R.lattice(np.float32([[0, 0, 0], [3, 1, 0]]))[1] == 2.0 ** -30 and R.lattice(np.float32([[1, 1, 1]]))[1] == 2.0 ** -32


# ------------------------------------------------------------------------------------------------------------------------- the ABI
def test_abi_version_constants_and_symbols():
    L = _lib.lib()
    assert _lib.header_abi_version() >= 66 and L.atvs_abi_version() == _lib.header_abi_version()
    for name in NAMES:
        assert name in _lib.declared_symbols() and hasattr(L, name)
    assert ops.MESH_ADJACENCY_MIN_SLOTS == _lib.header_macro('ATVS_MESH_ADJACENCY_MIN_SLOTS') == 1024 == 6 * BR.CENSUS_MIN_FACES + 4
    assert ops.MESH_ADJACENCY_INFO == R.ADJACENCY_INFO
    assert (ops.MESH_FLAG_FINITE, ops.MESH_FLAG_BOUNDARY, ops.MESH_FLAG_NONMANIFOLD) == (R.FINITE, R.BOUNDARY, R.NONMANIFOLD)
    assert 'mesh_smooth' not in _lib.OWNS_ITS_SIMD and '-ffp-contract=off' in _lib.flags_for(os.path.join(_lib.CSRC, 'mesh_smooth.hip'))
    with open(_lib.HEADER) as f:
        text = f.read()
    assert text.index('atvs_mesh_nearest(') < text.index('atvs_mesh_adjacency_scratch_size(')          # appended behind the last section


def test_the_c_abi_refuses_bad_arguments_without_a_launch():
    L = _lib.lib()
    buf = (ctypes.c_double * 16)(*([0.0] * 16))                      # a stand-in pointer: refusals come before any launch
    ptr = ctypes.c_void_p(ctypes.addressof(buf))
    other = ctypes.c_void_p(ctypes.addressof(buf) + 64)
    n = ctypes.c_long(0)
    size = L.atvs_mesh_adjacency_scratch_size
    assert size(-1, 1, ctypes.byref(n)) == -2 and size(1, -1, ctypes.byref(n)) == -2 and size((1 << 30) + 1, 1, ctypes.byref(n)) == -2
    assert size(1, (1 << 28) + 1, ctypes.byref(n)) == -2 and size(1, 1, None) == -1
    assert size(5, 0, ctypes.byref(n)) == 0 and n.value == 1024 * 8 + 1024 * 4 + 256 + 256
    assert size(4096, 171, ctypes.byref(n)) == 0 and n.value == 2048 * 12 + 16640 + 256
    adj = lambda nv=3, nf=1, scratch=ptr, bytes_=1 << 20, degree=ptr, offsets=ptr, neighbours=ptr, info=ptr: L.atvs_mesh_adjacency(      # noqa: E731
        ptr, nv, ptr, nf, scratch, bytes_, degree, ptr, offsets, neighbours, info, None)
    assert adj(nv=-1) == -2 and adj(nf=-1) == -2 and adj(nv=(1 << 30) + 1) == -2 and adj(nf=(1 << 28) + 1) == -2 and adj(bytes_=1000) == -2
    assert adj(scratch=None) == -1 and adj(degree=None) == -1 and adj(offsets=None) == -1 and adj(neighbours=None) == -1 and adj(info=None) == -1
    quant = lambda nv=3, origin=ptr, step=0.5, q=ptr, info=ptr: L.atvs_mesh_quantize(ptr, nv, origin, step, q, info, None)      # noqa: E731
    assert quant(nv=-1) == -2 and quant(origin=None) == -1 and quant(q=None) == -1 and quant(info=None) == -1
    assert [quant(step=s) for s in (0.0, -0.5, 0.75, 3.0, float('inf'), float('nan'))] == [-3] * 6
    bad_origin = (ctypes.c_double * 3)(0.0, float('nan'), 0.0)
    assert quant(origin=bad_origin) == -3
    step = lambda q_in=ptr, q_out=other, nv=3, nn=6, factor=0.5, info=ptr: L.atvs_mesh_smooth_pass(      # noqa: E731
        q_in, nv, ptr, ptr, ptr, ptr, nn, factor, 0, q_out, info, None)
    assert step(nv=-1) == -2 and step(nn=-1) == -2 and step(nn=6 * (1 << 28) + 1) == -2
    assert [step(factor=x) for x in (1.5, -1.0000001, float('nan'), float('inf'))] == [-3] * 4
    assert step(q_out=ptr) == -3 and step(info=None) == -1 and step(q_out=None) == -1
    deq = lambda nv=3, step=0.5, origin=ptr, out=ptr: L.atvs_mesh_dequantize(ptr, ptr, ptr, nv, origin, step, out, None)      # noqa: E731
    assert deq(nv=-1) == -2 and deq(step=0.3) == -3 and deq(origin=None) == -1 and deq(out=None) == -1 and deq(origin=bad_origin) == -3
    assert L.atvs_mesh_face_extent(ptr, -1, ptr, 1, ptr, None) == -2 and L.atvs_mesh_face_extent(ptr, 3, ptr, 1, None, None) == -1
    assert L.atvs_mesh_face_extent(ptr, 3, None, 1, ptr, None) == -1
    sums = lambda nv=3, nf=1, unit=1.0, s=ptr, info=ptr: L.atvs_mesh_vertex_normal_sums(ptr, nv, ptr, nf, unit, s, ptr, info, None)      # noqa: E731
    assert sums(nv=-1) == -2 and sums(nf=(1 << 28) + 1) == -2 and sums(s=None) == -1 and sums(info=None) == -1
    assert [sums(unit=u) for u in (0.0, -1.0, float('inf'), float('nan'))] == [-3] * 4
    assert L.atvs_mesh_vertex_normals(ptr, -1, ptr, None) == -2 and L.atvs_mesh_vertex_normals(ptr, 3, None, None) == -1
    assert L.atvs_mesh_vertex_normals(None, 0, None, None) == 0                      # nothing to do


def test_every_new_entry_point_is_in_a_row_of_the_buffer_contract():
    named = set()
    for name in MR.NAMES:
        row = BR.ROWS[name]
        named.update(row.entries)
        reached = set()
        for size in row.sizes:
            reached.update(row.required(size))
        assert set(row.entries) <= reached and row.names and row.constants
    assert named == set(NAMES) and BR.ROWS['mesh_adjacency'].scratch and BR.ROWS['mesh_smooth'].scratch


@pytest.mark.parametrize('name,size', MR.cases(), ids=['%s[%s]' % c for c in MR.cases()])
def test_the_rows_build_what_they_state(name, size):
    row = BR.ROWS[name]
    p = row.sizes[size]
    d, again, stated = row.build(p), row.build(p), row.shapes(p)
    tensors = {k: v for k, v in d.items() if isinstance(v, torch.Tensor)}
    assert sorted(tensors) == sorted(stated)
    for k, (shape, dtype) in stated.items():
        t = tensors[k]
        assert t.device.type == 'cpu' and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape), k
        assert int(t.shape[0]) <= 5000 and (t.numel() == 0 or torch.equal(t.view(torch.uint8), again[k].view(torch.uint8))), k


# ---------------------------------------------------------------------------------------------------------------------------- ops
def _meta(shape, dtype):
    return torch.empty(shape, dtype=dtype, device='meta')


def test_ops_refuse_bad_arguments_and_plan_shapes_on_meta():
    v, f = _meta((5, 3), torch.float32), _meta((4, 3), torch.int32)
    a = ops.mesh_adjacency(v, f)
    assert isinstance(a, ops.MeshAdjacency) and tuple(a.degree.shape) == (5,) and tuple(a.offsets.shape) == (6,) and a.offsets.dtype == torch.int32
    assert tuple(a.neighbours.shape) == (0,) and a.info == dict.fromkeys(ops.MESH_ADJACENCY_INFO, 0)
    q, info = ops.mesh_quantize(v, (0, 0, 0), 0.25)
    assert tuple(q.shape) == (5, 3) and q.dtype == torch.int64 and info == {'nonfinite_vertices': 0}
    q2, tallies = ops.mesh_smooth_pass(q, a, 0.5)
    assert tuple(q2.shape) == (5, 3) and tuple(tallies.shape) == (2,) and tallies.dtype == torch.int32
    assert ops.mesh_dequantize(q2, q, v, (0, 0, 0), 0.25).dtype == torch.float32
    out, info = ops.mesh_smooth(v, f, 3, mu=None)
    assert tuple(out.shape) == (5, 3) and info['passes'] == 3 and ops.mesh_smooth(v, f, 3)[1]['passes'] == 6
    assert tuple(ops.mesh_vertex_normals(v, f).shape) == (5, 3) and ops.mesh_face_extent(v, f)['max_extent'] == 0.0
    sums, inc = ops.mesh_vertex_normal_sums(v, f, 2.0)
    assert sums.dtype == torch.int64 and tuple(sums.shape) == (5, 3) and inc.dtype == torch.int32
    assert ops.mesh_normals_from_sums(sums).dtype == torch.float32
    for step in (0, -0.25, 0.3, 3, float('inf'), float('nan'), '1', None, True):
        with pytest.raises(ValueError, match='step'):
            ops.mesh_quantize(v, (0, 0, 0), step)
        with pytest.raises(ValueError, match='step'):
            ops.mesh_dequantize(q, q, v, (0, 0, 0), step)
    for origin in ((0, 0), (0, float('nan'), 0), 'abc', None, 3.0):
        with pytest.raises(ValueError, match='origin'):
            ops.mesh_quantize(v, origin, 0.5)
    for factor in (1.5, -1.01, float('nan'), '0.5', None, True):
        with pytest.raises(ValueError, match='factor'):
            ops.mesh_smooth_pass(q, a, factor)
    for mask in (-1, 1 << 31, 1.0, True):
        with pytest.raises(ValueError, match='pin_mask'):
            ops.mesh_smooth_pass(q, a, 0.5, mask)
    for unit in (0, -1.0, float('inf'), float('nan'), '1', True):
        with pytest.raises(ValueError, match='area_unit'):
            ops.mesh_vertex_normal_sums(v, f, unit)
        with pytest.raises(ValueError, match='area_unit'):
            ops.mesh_vertex_normals(v, f, unit)
    for kw, what in ((dict(iterations=-1), 'iterations'), (dict(iterations=1001), 'iterations'), (dict(iterations=2.0), 'iterations'),
                     (dict(iterations=True), 'iterations'), (dict(iterations=1, lam=0.0), 'lam'), (dict(iterations=1, lam=1.0), 'lam'),
                     (dict(iterations=1, lam='x'), 'lam'), (dict(iterations=1, mu=-0.5), 'mu'), (dict(iterations=1, mu=0.6), 'mu'),
                     (dict(iterations=1, mu=-1.01), 'mu'), (dict(iterations=1, lam=0.6, mu=-0.55), 'mu')):
        with pytest.raises(ValueError, match=what):
            ops.mesh_smooth(v, f, **kw)
    assert ops.mesh_smooth(v, f, 1000, 0.6, -1.0)[1]['passes'] == 2000
    with pytest.raises(ValueError, match='vertices'):
        ops.mesh_adjacency(_meta((5, 3), torch.float64), f)
    with pytest.raises(ValueError, match='faces'):
        ops.mesh_smooth(v, _meta((4, 3), torch.int64), 1)
    with pytest.raises(ValueError, match='q_in'):
        ops.mesh_smooth_pass(_meta((5, 3), torch.int32), a, 0.5)
    with pytest.raises(ValueError, match='degree: 5 rows, expected 4'):
        ops.mesh_smooth_pass(_meta((4, 3), torch.int64), a, 0.5)
    with pytest.raises(ValueError, match='q0: 4 rows, expected 5'):
        ops.mesh_dequantize(q, _meta((4, 3), torch.int64), v, (0, 0, 0), 0.5)
    with pytest.raises(ValueError, match='sums'):
        ops.mesh_normals_from_sums(_meta((5, 3), torch.int32))
    with pytest.raises(ValueError, match='faces on cpu, vertices on meta'):
        ops.mesh_adjacency(v, torch.zeros((4, 3), dtype=torch.int32))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.mesh_adjacency(torch.zeros((5, 3)), torch.zeros((4, 3), dtype=torch.int32))


# ----------------------------------------------------------------------------------------------------------------------- the tool
def test_the_tool_checks_its_options(tmp_path, capsys):
    assert smooth_mesh.check_options(10) == (10, 0.5, -0.53, False, False, None)
    assert smooth_mesh.check_options(0, 0.3, None, True, True, 2.0) == (0, 0.3, None, True, True, 2.0)
    for kw, what in ((dict(iterations=None), 'iterations'), (dict(iterations=-1), 'iterations'), (dict(iterations=1001), 'iterations'),
                     (dict(iterations=1.0), 'iterations'), (dict(iterations=True), 'iterations'), (dict(iterations=1, lam=0), 'lam'),
                     (dict(iterations=1, lam=1), 'lam'), (dict(iterations=1, lam=None), 'lam'), (dict(iterations=1, mu=-0.5), 'mu'),
                     (dict(iterations=1, mu=-2), 'mu'), (dict(iterations=1, mu='x'), 'mu'), (dict(iterations=1, pin_boundary=1), 'pin_boundary'),
                     (dict(iterations=1, normals='yes'), 'normals'), (dict(iterations=1, normals=True, area_unit=0), 'area_unit'),
                     (dict(iterations=1, normals=True, area_unit=float('nan')), 'area_unit'), (dict(iterations=1, area_unit=1.0), 'needs normals')):
        with pytest.raises(ValueError, match=what):
            smooth_mesh.check_options(**kw)
    assert {'step', 'origin', 'boundary_vertices', 'pinned', 'isolated_vertices', 'nonfinite_vertices', 'moved', 'max_move', 'seconds',
            'iterations', 'lam', 'mu', 'pin_boundary'} | set(ops.MESH_ADJACENCY_INFO) <= set(smooth_mesh.REPORT_KEYS)
    parser = smooth_mesh.make_parser()
    assert {s for a in parser._actions for s in a.option_strings} == {
        '-h', '--help', '--in', '--out', '--iterations', '--lam', '--mu', '--laplacian', '--pin_boundary', '--normals', '--normal_area_unit',
        '--report', '--gpu_id'}
    args = parser.parse_args(['--in', 'a', '--out', 'b', '--iterations', '3'])
    assert smooth_mesh.options(parser, args) == dict(iterations=3, lam=0.5, mu=-0.53, pin_boundary=False, normals=False, area_unit=None)
    args = parser.parse_args(['--in', 'a', '--out', 'b', '--iterations', '0', '--laplacian', '--normals', '--normal_area_unit', '0.01', '--pin_boundary'])
    assert smooth_mesh.options(parser, args) == dict(iterations=0, lam=0.5, mu=None, pin_boundary=True, normals=True, area_unit=0.01)
    assert smooth_mesh.options(parser, parser.parse_args(['--in', 'a', '--out', 'b', '--iterations', '1', '--mu', '-0.9']))['mu'] == -0.9
    mesh = str(tmp_path / 'mesh.ply')
    v, f = C.mesh('tetra')
    ply.write_mesh(mesh, v, None, f)
    out = str(tmp_path / 'out.ply')
    for argv, message in ((['--in', mesh, '--out', out], 'the following arguments are required: --iterations'),
                          (['--in', mesh, '--out', out, '--iterations', '-1'], 'iterations must be an integer in 0..1000'),
                          (['--in', mesh, '--out', out, '--iterations', '1', '--lam', '1.5'], 'lam must be a number with 0 < lam < 1'),
                          (['--in', mesh, '--out', out, '--iterations', '1', '--mu', '-0.4'], 'mu must be None or a number with -1 <= mu < -lam'),
                          (['--in', mesh, '--out', out, '--iterations', '1', '--laplacian', '--mu', '-0.6'], '--laplacian has no mu pass'),
                          (['--in', mesh, '--out', out, '--iterations', '1', '--normal_area_unit', '1'], '--normal_area_unit needs --normals'),
                          (['--in', mesh, '--out', out, '--iterations', '1', '--normals', '--normal_area_unit', '0'], '--normal_area_unit must be'),
                          (['--in', mesh + '.no', '--out', out, '--iterations', '1'], 'no such file'),
                          (['--in', __file__, '--out', out, '--iterations', '1'], '--in:')):
        with pytest.raises(SystemExit) as e:
            smooth_mesh.cli(argv)
        assert e.value.code == 2 and message in ' '.join(capsys.readouterr().err.split()), argv
    assert not os.path.exists(out)
    assert [np.array_equal(a, b) for a, b in zip(smooth_mesh.read_mesh(mesh), (v, np.full((4, 3), 255, np.uint8), f))] == [True] * 3


# ------------------------------------------------------------------------------------------------------------------------ the driver
def test_check_smooth_and_the_drivers_rules_with_and_without_smooth():
    assert mesh_fusion.check_smooth(None) is None
    assert mesh_fusion.check_smooth(dict(iterations=5)) == dict(iterations=5, lam=0.5, mu=-0.53, pin_boundary=False, normals=False)
    assert mesh_fusion.check_smooth(dict(iterations=0, lam=0.3, mu=None, pin_boundary=True, normals=True)) == dict(
        iterations=0, lam=0.3, mu=None, pin_boundary=True, normals=True)
    for bad in (5, {}, dict(lam=0.5), dict(iterations=1, area_unit=1.0), dict(iterations=1, cell=2), [('iterations', 1)]):
        with pytest.raises(ValueError, match='mesh smooth must be a dict\\(iterations=N'):
            mesh_fusion.check_smooth(bad)
    for bad, what in ((dict(iterations=-1), 'iterations'), (dict(iterations='3'), 'iterations'), (dict(iterations=1, lam=2), 'lam'),
                      (dict(iterations=1, mu=0.1), 'mu'), (dict(iterations=1, pin_boundary='no'), 'pin_boundary'),
                      (dict(iterations=1, normals=1), 'normals')):
        with pytest.raises(ValueError, match='mesh smooth: .*%s' % what):
            mesh_fusion.check_smooth(bad)
    with pytest.raises(ValueError, match='mesh smooth'):
        mesh_fusion.check_options(0.1, smooth=dict(iterations=-1))
    mesh_fusion.check_options(0.1, smooth=dict(iterations=2))
    assert inspect.signature(mesh_fusion.SceneMesh.__init__).parameters['smooth'].default is None
    assert inspect.signature(mesh_fusion.check_options).parameters['smooth'].default is None
    fuse = dict(prob_threshold=0.5)
    plain = mesh_fusion.rules(dict(voxel=0.1, simplify=dict(cell_voxels=3)), fuse)
    smooth = mesh_fusion.rules(dict(voxel=0.1, simplify=dict(cell_voxels=3), smooth=dict(iterations=2)), fuse)
    assert len(smooth) == len(plain) + 1 and [r for r in smooth if r not in plain] == [(False, smooth[1][1])] and 'mesh smooth= needs voxel=' in smooth[1][1]
    assert [b for b, _ in mesh_fusion.rules(dict(smooth=dict(iterations=2)), fuse)] == [False, True, True]
    without = eval_pointcloud._option_rules(fuse=fuse, mesh=dict(voxel=0.1))
    given = eval_pointcloud._option_rules(fuse=fuse, mesh=dict(voxel=0.1, smooth=dict(iterations=2)))
    assert len(given) == len(without) + 1 and all(r in given for r in without) and not any(b for b, _ in given)
    assert not any('smooth' in m for _, m in without)
    with pytest.raises(ValueError, match='mesh smooth= needs voxel='):
        eval_pointcloud._check_options(fuse=fuse, mesh=dict(smooth=dict(iterations=2)))
    with pytest.raises(ValueError, match='mesh smooth: iterations'):
        eval_pointcloud._check_options(fuse=fuse, mesh=dict(voxel=0.1, smooth=dict(iterations=2000)))
    eval_pointcloud._check_options(fuse=fuse, mesh=dict(voxel=0.1, smooth=dict(iterations=2, normals=True)))
    # the command line has no option for it, and what it gives carries no key of it
    assert not any('smooth' in s for a in eval_pointcloud.make_parser()._actions for s in a.option_strings)
    flags = argparse.Namespace(prob_threshold=0.8, disp_threshold=0.01, num_consistent=2, fuse=True, mesh_voxel=0.1)
    assert eval_pointcloud._run_options(flags)['mesh'] == dict(voxel=0.1)


# --------------------------------------------------------------------------------------------------------------------------- the PLY
def test_write_mesh_with_normals_round_trips_and_the_old_layout_keeps_its_bytes(tmp_path):
    v, f = C.mesh('dirty')
    n = C.restated('dirty')['normals'].copy()
    n[6] = np.nan                                                     # a non-finite normal is written as zeros
    colors = (np.arange(3 * len(v)) % 251).astype(np.uint8).reshape(-1, 3)
    finite = np.where(np.isfinite(v), v, np.float32(0.0))               # (write_mesh keeps the vertices' bits; compare what is comparable)
    plain, with_n = str(tmp_path / 'plain.ply'), str(tmp_path / 'normals.ply')
    ply.write_mesh(plain, finite, colors, f)
    ply.write_mesh(with_n, finite, colors, f, n)
    header = ('ply\nformat binary_little_endian 1.0\nelement vertex 11\nproperty float x\nproperty float y\nproperty float z\n'
              'property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 9\nproperty list uchar int vertex_indices\nend_header\n')
    body = b''.join(finite[k].tobytes() + colors[k].tobytes() for k in range(len(v))) + b''.join(b'\x03' + r.astype('<i4').tobytes() for r in f)
    with open(plain, 'rb') as fh:
        assert fh.read() == header.encode('ascii') + body          # the bytes of the layout without normals, spelled out
    with open(with_n, 'rb') as fh:
        assert fh.read().startswith(header.replace('property uchar red', 'property float nx\nproperty float ny\nproperty float nz\nproperty uchar red').encode('ascii'))
    assert os.path.getsize(with_n) == os.path.getsize(plain) + 12 * len(v) + len('property float nx\n') * 3
    for path, normals in ((plain, None), (with_n, np.where(np.isfinite(n), n, np.float32(0.0)))):
        got = ply.read_mesh(path)
        assert len(got) == 3 and np.array_equal(_bits(got[0]), _bits(finite)) and np.array_equal(got[1], colors) and np.array_equal(got[2], f)
        assert got[2].dtype == np.int32 and got[0].dtype == np.float32
        four = ply.read_mesh_normals(path)
        assert len(four) == 4 and all(np.array_equal(a, b) for a, b in zip(four[:3], got))
        assert four[3] is None if normals is None else np.array_equal(_bits(four[3]), _bits(normals))
        any_v, any_f = ply.read_mesh_any(path)
        assert np.array_equal(_bits(any_v), _bits(finite)) and np.array_equal(any_f, f)
        assert np.array_equal(_bits(ply.read_ply_points(path)), _bits(finite))
    with pytest.raises(ValueError, match='3 normals for 11 vertices'):
        ply.write_mesh(plain, finite, colors, f, n[:3])
    with open(with_n, 'rb') as fh:
        data = fh.read()
    with open(with_n, 'wb') as fh:
        fh.write(data[:-5])
    with pytest.raises(ValueError, match='truncated body'):
        ply.read_mesh_normals(with_n)
    with open(with_n, 'wb') as fh:
        fh.write(data.replace(b'property float nz\n', b'property float nw\n'))
    with pytest.raises(ValueError, match='not a mesh layout write_mesh writes'):
        ply.read_mesh(with_n)
