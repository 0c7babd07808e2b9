"""The mesh smoothing kernels (csrc/mesh_smooth.hip) against their numpy restatement on every case of tests/mesh_smooth_cases.py,
every op twice with the same bits both times: the adjacency (degree, flags, offsets, info; the rows of neighbours as sorted rows), the
quantisation, q after each of the six passes of 3 Taubin iterations (pinned and not), the dequantised vertices, mesh_smooth and
smooth_device as a whole, the same bits with the faces permuted and rotated on the device, the normal sums to one unit per incidence
(equality is expected) and the normals of the restatement's sums bit for bit, the errors and the empty meshes."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
from atvsnet_amd import _lib, ops
from atvsnet_amd.atvsnet import smooth_mesh

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_smooth_cases as C  # noqa: E402
import mesh_smooth_restated as R  # noqa: E402

pytestmark = pytest.mark.gpu

case = pytest.mark.parametrize('name', C.NAMES)
pinned = pytest.mark.parametrize('pin', [False, True], ids=['free', 'pinned'])


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                       # (a copy: the cases' arrays are read-only)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    g = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert g.shape == want.shape and g.dtype == want.dtype, (what, g.dtype, want.dtype, g.shape, want.shape)
    ne = np.nonzero(_bits(g).reshape(-1) != _bits(want).reshape(-1))[0]
    assert len(ne) == 0, '%s: %d of %d elements differ, first at %d: %r against %r' % (
        what, len(ne), g.size, ne[0], g.reshape(-1)[ne[0]], want.reshape(-1)[ne[0]])


def _mesh_on(name, dev):
    v, f = C.mesh(name)
    return _dev(v, dev), _dev(f, dev)


@case
def test_adjacency_is_the_restatement_twice(cuda, name):
    v, f = _mesh_on(name, cuda)
    want = C.restated(name)['adjacency']
    for _ in range(2):
        got = ops.mesh_adjacency(v, f)
        assert got.info == want['info']
        for key in ('degree', 'flags', 'offsets'):
            _same(getattr(got, key), want[key], key)
        assert tuple(got.neighbours.shape) == (2 * want['info']['pairs'],) == (int(want['offsets'][-1]),)
        _same(R.sorted_rows(want['offsets'], got.neighbours.cpu().numpy()), want['neighbours'], 'the sorted rows of neighbours')


@case
@pinned
def test_quantisation_every_pass_and_dequantisation_are_the_restatement_twice(cuda, name, pin):
    v, f = _mesh_on(name, cuda)
    want = C.restated(name, pin)
    adjacency = ops.mesh_adjacency(v, f)
    for _ in range(2):
        q0, info = ops.mesh_quantize(v, want['origin'], want['step'])
        _same(q0, want['trace'][0], 'q0')
        assert info == {'nonfinite_vertices': want['info']['nonfinite_vertices']}
        q, tallies = q0, None
        for k, factor in enumerate(C.TAUBIN * C.ITERATIONS):
            q, tallies = ops.mesh_smooth_pass(q, adjacency, factor, ops.MESH_FLAG_BOUNDARY if pin else 0, tallies)
            _same(q, want['trace'][k + 1], 'q after pass %d' % (k + 1))
        assert tallies.cpu().tolist() == [0, 0]
        _same(ops.mesh_dequantize(q, q0, v, want['origin'], want['step']), want['out'], 'the dequantised vertices')
        _same(ops.mesh_dequantize(q0, q0, v, want['origin'], want['step']), C.mesh(name)[0], 'no pass: the input bits')


@case
@pinned
def test_the_whole_run_is_the_restatement_twice(cuda, name, pin):
    v, f = _mesh_on(name, cuda)
    want = C.restated(name, pin)
    colors = torch.arange(3 * len(v), dtype=torch.int64, device=cuda).remainder(251).to(torch.uint8).reshape(-1, 3)
    for _ in range(2):
        out, info = ops.mesh_smooth(v, f, C.ITERATIONS, C.TAUBIN[0], C.TAUBIN[1], pin)
        _same(out, want['out'], 'mesh_smooth')
        assert info == {k: want['info'][k] for k in info}
        sv, sc, sf, sn, report = smooth_mesh.smooth_device(v, colors, f, C.ITERATIONS, C.TAUBIN[0], C.TAUBIN[1], pin, normals=True)
        _same(sv, want['out'], 'smooth_device')
        assert sc is colors and sf is f and tuple(sn.shape) == tuple(v.shape)
        assert set(report) == set(smooth_mesh.REPORT_KEYS)
        flags, degree = want['adjacency']['flags'], want['adjacency']['degree']
        hv = C.mesh(name)[0]
        moved = (_bits(want['out']) != _bits(hv)).any(1)
        assert report['boundary_vertices'] == int(((flags & R.BOUNDARY) != 0).sum()) and report['pinned'] == (report['boundary_vertices'] if pin else 0)
        assert report['isolated_vertices'] == int((((flags & R.FINITE) != 0) & (degree == 0)).sum())
        assert report['nonfinite_vertices'] == int(((flags & R.FINITE) == 0).sum()) and report['moved'] == int(moved.sum())
        e = want['out'][moved].astype(np.float64) - hv[moved].astype(np.float64)
        largest = math.sqrt(float(np.float32(((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]).max(initial=0.0))))
        assert report['max_move'] == largest and report['step'] == want['step'] and report['origin'] == want['info']['origin']


@pytest.mark.parametrize('name', ['noisy_sphere', 'sphere4', 'fan', 'dirty'])
def test_permuted_and_rotated_faces_give_the_same_bits(cuda, name):
    v, f = _mesh_on(name, cuda)
    want = C.restated(name)
    rng = np.random.default_rng(5)
    order = _dev(rng.permutation(len(f)), cuda)
    shift = _dev(rng.integers(0, 3, len(f)), cuda)
    columns = (torch.arange(3, device=cuda)[None, :] + shift[:, None]).remainder(3)
    permuted = torch.gather(f.index_select(0, order).to(torch.int64), 1, columns).to(torch.int32).contiguous()
    out, info = ops.mesh_smooth(v, permuted, C.ITERATIONS, C.TAUBIN[0], C.TAUBIN[1])
    _same(out, want['out'], 'mesh_smooth of the permuted faces')
    sums, incidences = ops.mesh_vertex_normal_sums(v, permuted, want['extent']['max_extent'])
    plain = ops.mesh_vertex_normal_sums(v, f, want['extent']['max_extent'])
    assert torch.equal(sums, plain[0]) and torch.equal(incidences, plain[1])


@case
def test_normal_sums_are_the_restatement_to_a_unit_per_incidence_and_the_normals_of_its_sums_bit_for_bit(cuda, name):
    v, f = _mesh_on(name, cuda)
    want = C.restated(name)
    extent = ops.mesh_face_extent(v, f)
    assert {k: extent[k] for k in extent if k != 'max_extent'} == {k: want['extent'][k] for k in extent if k != 'max_extent'}
    # the largest s is one double square root: the device's may differ from numpy's in the last place, nothing else is rounded twice
    assert abs(extent['max_extent'] - want['extent']['max_extent']) <= np.spacing(want['extent']['max_extent'])
    unit = want['extent']['max_extent'] or 1.0
    first = None
    for _ in range(2):
        sums, incidences = ops.mesh_vertex_normal_sums(v, f, unit)
        s, inc = sums.cpu().numpy(), incidences.cpu().numpy()
        assert s.dtype == np.int64 and s.shape == want['sums'].shape and np.array_equal(inc, want['incidences'])
        diff = np.abs(s - want['sums'])
        print('%s: %d of %d normal-sum words differ from the restatement, by at most %d' % (name, int((diff != 0).sum()), diff.size,
                                                                                          int(diff.max(initial=0))))
        # a term on a rint tie or a last-bit difference in sqrt moves a term by one unit: at most one unit per incidence
        assert (diff <= want['incidences'][:, None]).all()
        assert first is None or np.array_equal(s, first)
        first = s
    _same(ops.mesh_normals_from_sums(_dev(want['sums'], cuda)), want['normals'], 'the normals of the restatement\'s sums')
    own, _ = ops.mesh_vertex_normal_sums(v, f, extent['max_extent'] or 1.0)
    _same(ops.mesh_vertex_normals(v, f), R.normals_from_sums(own.cpu().numpy()), 'mesh_vertex_normals')


def test_errors(cuda):
    v, f = _mesh_on('tetra', cuda)
    bad = f.clone()
    bad[2, 1] = 4
    assert ops.mesh_adjacency(v, bad).info['skipped_index_faces'] == 1
    with pytest.raises(ValueError, match='mesh_smooth: 1 of 4 faces have a vertex index outside 0..3'):
        ops.mesh_smooth(v, bad, 1)
    with pytest.raises(ValueError, match='mesh_vertex_normal_sums: 1 of 4 faces'):
        ops.mesh_vertex_normal_sums(v, bad, 1.0)
    assert ops.mesh_face_extent(v, bad)['skipped_index_faces'] == 1
    adjacency = ops.mesh_adjacency(v, f)
    q0, _ = ops.mesh_quantize(v, (0.0, 0.0, 0.0), 2.0 ** -31)
    lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    tallies = torch.zeros(2, dtype=torch.int32, device=cuda)

    def one_pass(q_in, q_out, factor):
        return lib.atvs_mesh_smooth_pass(q_in.data_ptr(), 4, adjacency.degree.data_ptr(), adjacency.flags.data_ptr(), adjacency.offsets.data_ptr(),
                                         adjacency.neighbours.data_ptr(), int(adjacency.neighbours.shape[0]), factor, 0, q_out.data_ptr(),
                                         tallies.data_ptr(), stream)
    other = torch.empty_like(q0)
    assert one_pass(q0, q0, 0.5) == -3 and one_pass(q0, other, 1.5) == -3 and one_pass(q0, other, float('nan')) == -3       # ATVS_ERR_ARG
    assert one_pass(q0, other, 0.5) == 0
    origin = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    words = torch.empty(2, dtype=torch.int64, device=cuda)
    for step in (0.0, -0.5, 0.3, float('inf'), float('nan')):
        assert lib.atvs_mesh_quantize(v.data_ptr(), 4, origin, step, other.data_ptr(), words.data_ptr(), stream) == -3
        assert lib.atvs_mesh_dequantize(q0.data_ptr(), q0.data_ptr(), v.data_ptr(), 4, origin, step, torch.empty_like(v).data_ptr(), stream) == -3
        with pytest.raises(ValueError, match='step must be a positive power of two'):
            ops.mesh_quantize(v, (0.0, 0.0, 0.0), step)
    sums, inc, word = torch.empty((4, 3), dtype=torch.int64, device=cuda), torch.empty(4, dtype=torch.int32, device=cuda), torch.empty(1, dtype=torch.int32, device=cuda)
    for unit in (0.0, -1.0, float('inf'), float('nan')):
        assert lib.atvs_mesh_vertex_normal_sums(v.data_ptr(), 4, f.data_ptr(), 4, unit, sums.data_ptr(), inc.data_ptr(), word.data_ptr(), stream) == -3
        with pytest.raises(ValueError, match='area_unit must be a positive finite number'):
            ops.mesh_vertex_normal_sums(v, f, unit)
    with pytest.raises(ValueError, match='2 coordinates lie more than 2\\^31 steps'):
        ops.mesh_quantize(v, (0.0, 0.0, 3.0), 2.0 ** -30)                 # z = -1 is 2^32 steps below the origin's 3
    with pytest.raises(ValueError, match='factor must be'):
        ops.mesh_smooth_pass(q0, adjacency, 1.5)
    torch.cuda.synchronize()


def test_a_q_buffer_at_the_clamp_diverges_and_says_so(cuda):
    """q handed in at 2^32 on one vertex of the tetrahedron: the inflating pass (mu < 0) moves it outward, past the clamp."""
    v, f = _mesh_on('tetra', cuda)
    adjacency = ops.mesh_adjacency(v, f)
    host = np.zeros((4, 3), np.int64)
    host[0] = 1 << 32
    want, clamped = R.smooth_pass(host, C.restated('tetra')['adjacency'], -0.53)
    assert clamped == 3 and (want[0] == 1 << 32).all()
    q, tallies = ops.mesh_smooth_pass(_dev(host, cuda), adjacency, -0.53)
    _same(q, want, 'the clamped pass')
    assert tallies.cpu().tolist() == [3, 0]
    q, tallies = ops.mesh_smooth_pass(q, adjacency, -0.53, 0, tallies)           # the tallies run on
    assert tallies.cpu().tolist()[0] > 3
    # a row that leaves the arrays, and a neighbour outside the vertices: the lanes keep q_in and say so
    short = ops.MeshAdjacency(adjacency.degree, adjacency.flags, adjacency.offsets, adjacency.neighbours[:10].contiguous(), adjacency.info)
    q, tallies = ops.mesh_smooth_pass(_dev(host, cuda), short, 0.5)
    assert tallies.cpu().tolist() == [0, 1] and torch.equal(q[3], _dev(host, cuda)[3])
    wrong = adjacency.neighbours.clone()
    wrong[0] = 4
    q, tallies = ops.mesh_smooth_pass(_dev(host, cuda), ops.MeshAdjacency(adjacency.degree, adjacency.flags, adjacency.offsets, wrong, adjacency.info), 0.5)
    assert tallies.cpu().tolist() == [0, 1] and torch.equal(q[0], _dev(host, cuda)[0])


def test_mesh_smooth_raises_when_a_coordinate_was_clamped(cuda, monkeypatch):
    v, f = _mesh_on('tetra', cuda)
    real = ops.mesh_smooth_pass

    def pass_at_the_clamp(q_in, adjacency, factor, pin_mask=0, info=None):
        q = q_in.clone()
        q[0] = 1 << 32                                                  # the q buffer handed in at 2^32
        return real(q, adjacency, factor, pin_mask, info)
    monkeypatch.setitem(ops.mesh_smooth.__globals__, 'mesh_smooth_pass', pass_at_the_clamp)
    with pytest.raises(RuntimeError, match='the filter has diverged: [0-9]+ coordinates'):
        ops.mesh_smooth(v, f, 1)


def test_empty_meshes(cuda):
    for name in ('no_vertices', 'no_faces'):
        v, f = _mesh_on(name, cuda)
        hv = C.mesh(name)[0]
        n = len(hv)
        got = ops.mesh_adjacency(v, f)
        assert got.info == dict.fromkeys(ops.MESH_ADJACENCY_INFO, 0) and tuple(got.neighbours.shape) == (0,)
        assert got.offsets.cpu().tolist() == [0] * (n + 1) and got.degree.cpu().tolist() == [0] * n and got.flags.cpu().tolist() == [1] * n
        out, info = ops.mesh_smooth(v, f, 5)
        _same(out, hv, 'mesh_smooth of %s' % name)
        assert info['passes'] == 10 and info['pairs'] == 0
        normals = ops.mesh_vertex_normals(v, f)
        assert tuple(normals.shape) == (n, 3) and not normals.any()
        assert ops.mesh_face_extent(v, f) == {'max_extent': 0.0, 'usable_faces': 0, 'skipped_index_faces': 0, 'nonfinite_faces': 0}
        sv, sc, sf, sn, report = smooth_mesh.smooth_device(v, None, f, 2, normals=True)
        _same(sv, hv, 'smooth_device of %s' % name)
        assert sc is None and report['moved'] == 0 and report['max_move'] == 0.0 and report['isolated_vertices'] == n
    torch.cuda.synchronize()
