"""The mesh simplification kernels (csrc/mesh_simplify.hip) against their numpy restatement on every case of
tests/mesh_simplify_cases.py, every op twice: the clusters, the rewritten faces, the mean placement and the largest move bit for
bit; the quadrics to one unit per incidence (equality is expected); the quadric placement, handed the restatement's own sums, to
the header's allowance for the solve plus one float32 spacing; the whole simplify_device; the errors; the empty meshes."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
from atvsnet_amd import ops
from atvsnet_amd.atvsnet import simplify_mesh

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_simplify_cases as K  # noqa: E402
import mesh_simplify_restated as S  # noqa: E402
import mesh_topology_restated as T  # noqa: E402

pytestmark = pytest.mark.gpu

RANK_EPSILON = 1e-3
LOW_MARGIN = 1e-6
REPORT_KEYS = {'cell', 'placement', 'origin', 'rank_epsilon', 'clusters', 'vertices_in', 'vertices_out', 'faces_in', 'faces_out',
               'degenerate_faces', 'duplicate_faces', 'nonfinite_faces', 'placed_by_quadric', 'fell_back', 'max_move', 'max_move_bound',
               'census_in', 'census_out', 'seconds'}


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    return a.view(np.int64) if a.dtype == np.uint64 else a


def _same(got, want):
    """A device tensor (or None) against a numpy array (or None): shape and bits (uint64 sums travel as int64)."""
    if want is None:
        assert got is None
        return
    g = got.cpu().numpy()
    assert g.shape == want.shape and g.dtype.itemsize == want.dtype.itemsize, (g.dtype, want.dtype, g.shape, want.shape)
    assert np.array_equal(_bits(g), _bits(want))


def _solve_allowance(cell):
    """The header's allowance for the solve, in the mesh's unit: ATVS_MESH_SIMPLIFY_SOLVE_UNITS units of 2^-53 / rank_epsilon cells."""
    return cell * ops.MESH_SIMPLIFY_SOLVE_UNITS * 2.0 ** -53 / RANK_EPSILON


def _positions_close(got, want, cell, rows):
    """|got - want| <= the solve's allowance + one float32 spacing of the coordinate, on `rows`."""
    got, want = got[rows].astype(np.float64), want[rows]
    bound = _solve_allowance(cell) + np.spacing(np.abs(want)).astype(np.float64)
    err = np.abs(got - want.astype(np.float64))
    print('quadric positions: %d rows, largest error %.3g, allowance %.3g + a spacing' % (len(want), err.max(initial=0.0), _solve_allowance(cell)))
    assert (err <= bound).all()


@pytest.mark.parametrize('name', K.NAMES)
def test_clusters_are_the_restatement_twice(cuda, name):
    c, want = K.case(name), K.restated(name)['cluster']
    v, col = _dev(c['vertices'], cuda), _dev(c['colors'], cuda)
    for _ in range(2):
        got = ops.mesh_cluster(v, col, c['cell'], c['origin'])
        assert int(got.counts.shape[0]) == len(want['counts'])
        for key in ('vertex_cluster', 'cells', 'counts', 'position_sums', 'color_sums'):
            _same(getattr(got, key), want[key])


@pytest.mark.parametrize('name', K.NAMES)
def test_quadrics_are_the_restatement_to_a_unit_per_incidence_twice(cuda, name):
    c, r = K.case(name), K.restated(name)
    v, f, vc = _dev(c['vertices'], cuda), _dev(c['faces'], cuda), _dev(r['cluster']['vertex_cluster'], cuda)
    C = len(r['cluster']['counts'])
    first = None
    for _ in range(2):
        q, inc = ops.mesh_cluster_quadrics(v, f, vc, C, c['cell'], c['origin'])
        q, inc = q.cpu().numpy(), inc.cpu().numpy()
        assert q.dtype == np.int64 and q.shape == (C, 10) and np.array_equal(inc, r['incidences'])
        diff = np.abs(q - r['quadrics'])
        print('%s: %d of %d quadric words differ from the restatement, by at most %d' % (name, int((diff != 0).sum()), diff.size, int(diff.max(initial=0))))
        # a term on a rint tie or a last-bit difference in sqrt moves a term by one unit: at most one unit per incidence
        assert (diff <= r['incidences'][:, None]).all()
        assert first is None or np.array_equal(q, first)                 # integer sums: the same bits on every run
        first = q


@pytest.mark.parametrize('name', K.NAMES)
def test_mean_placement_is_the_restatement_twice(cuda, name):
    c, r = K.case(name), K.restated(name, 'mean')
    cl = r['cluster']
    args = [_dev(cl[k], cuda) for k in ('cells', 'counts')] + [_dev(cl['position_sums'].view(np.int64), cuda), _dev(cl['color_sums'], cuda)]
    for quadrics in (None, _dev(r['quadrics'], cuda)):                   # with the mean the quadrics are not read
        pos, col, placed = ops.mesh_cluster_place(*args, quadrics, c['cell'], c['origin'], 'mean')
        _same(pos, r['place']['positions'])
        _same(col, r['place']['colors'])
        assert not placed.any().item() and placed.dtype == torch.uint8


@pytest.mark.parametrize('name', K.NAMES)
def test_quadric_placement_solves_the_restatements_sums_twice(cuda, name):
    c, r = K.case(name), K.restated(name, 'quadric')
    cl, want = r['cluster'], r['place']
    sure = want['margin'] >= LOW_MARGIN
    assert (~sure).sum() <= 0.01 * len(sure)
    args = [_dev(cl[k], cuda) for k in ('cells', 'counts')] + [_dev(cl['position_sums'].view(np.int64), cuda), _dev(cl['color_sums'], cuda),
                                                                _dev(r['quadrics'], cuda)]
    for _ in range(2):
        pos, col, placed = ops.mesh_cluster_place(*args, c['cell'], c['origin'], 'quadric', RANK_EPSILON)
        assert np.array_equal(placed.cpu().numpy()[sure], want['placed'][sure])
        _positions_close(pos.cpu().numpy(), want['positions'], c['cell'], sure)
        _same(col, want['colors'])


@pytest.mark.parametrize('name', K.NAMES)
def test_faces_and_the_largest_move_are_the_restatement_twice(cuda, name):
    c, r = K.case(name), K.restated(name)
    f, vc = _dev(c['faces'], cuda), _dev(r['cluster']['vertex_cluster'], cuda)
    v, pos = _dev(c['vertices'], cuda), _dev(r['place']['positions'], cuda)
    for _ in range(2):
        faces, keep, drops = ops.mesh_cluster_faces(f, vc)
        _same(faces, r['rewrite']['faces'])
        _same(keep, r['rewrite']['keep'])
        assert drops == {k: r['rewrite'][k] for k in ('nonfinite_faces', 'degenerate_faces', 'duplicate_faces')}
        assert ops.mesh_cluster_max_move(v, vc, pos) == r['max_move']


@pytest.mark.parametrize('placement', S.PLACEMENTS)
@pytest.mark.parametrize('name', K.NAMES)
def test_simplify_device_is_the_restatement(cuda, name, placement):
    c, r = K.case(name), K.restated(name, placement)
    out_v, out_c, out_f, report = simplify_mesh.simplify_device(_dev(c['vertices'], cuda), _dev(c['colors'], cuda), _dev(c['faces'], cuda),
                                                                c['cell'], placement, c['origin'], RANK_EPSILON)
    want_v, want_c, want_f = r['out']
    assert set(report) == REPORT_KEYS
    for key, n in r['counts'].items():
        if key not in ('placed_by_quadric', 'fell_back'):
            assert report[key] == n, key
    _same(out_f, want_f)
    _same(out_c, want_c)
    assert report['census_in'] == T.edge_census(c['faces'], len(c['vertices']))
    assert report['census_out'] == T.edge_census(want_f, len(want_v))
    assert report['max_move_bound'] == c['cell'] * math.sqrt(3.0) and 0.0 <= report['max_move'] <= report['max_move_bound']
    assert report['placed_by_quadric'] + report['fell_back'] == (report['clusters'] if placement == 'quadric' else 0)
    assert (report['cell'], report['placement'], report['origin'], report['rank_epsilon']) == (c['cell'], placement, list(c['origin']), RANK_EPSILON)
    if placement == 'mean':
        _same(out_v, want_v)
        assert report['max_move'] == r['max_move']
        return
    margin = r['place']['margin']
    unsure = int((margin < LOW_MARGIN).sum())
    assert unsure <= 0.01 * len(margin) and abs(report['placed_by_quadric'] - r['counts']['placed_by_quadric']) <= unsure
    rows = margin[r['cluster_map'] >= 0] >= LOW_MARGIN                     # the output's rows are the surviving clusters in their order
    # the device's own quadrics may differ from the restatement's by a unit per incidence of 2^-30: on a cluster whose quadric is
    # well conditioned that moves the minimiser by about as much, far below a float32 spacing of these coordinates
    _positions_close(out_v.cpu().numpy(), want_v, c['cell'], rows)


def test_a_mesh_without_an_origin_starts_at_its_lower_bound(cuda):
    c = K.case('plane')
    lo = c['vertices'].min(0).astype(np.float64)
    out_v, _, out_f, report = simplify_mesh.simplify_device(_dev(c['vertices'], cuda), None, _dev(c['faces'], cuda), c['cell'], 'mean')
    want = S.simplify(c['vertices'], None, c['faces'], c['cell'], tuple(lo), 'mean')
    assert report['origin'] == lo.tolist()
    _same(out_v, want['out'][0])
    _same(out_f, want['out'][2])
    host = simplify_mesh.simplify(c['vertices'], None, c['faces'], c['cell'], 'mean')
    assert np.array_equal(_bits(host[0]), _bits(want['out'][0])) and np.array_equal(host[2], want['out'][2]) and host[1] is None
    assert {'upload', 'download'} <= set(host[3]['seconds'])


def test_errors(cuda):
    c = K.case('single_face')
    v, f = _dev(c['vertices'], cuda), _dev(c['faces'], cuda)
    vc = ops.mesh_cluster(v, None, c['cell'], c['origin']).vertex_cluster
    for bad in ([[0, 1, 3]], [[0, -1, 2]]):
        bad = torch.tensor(bad, dtype=torch.int32, device=cuda)
        with pytest.raises(ValueError, match='1 of 1 faces have a vertex index outside 0..2'):
            ops.mesh_cluster_quadrics(v, bad, vc, 3, c['cell'], c['origin'])
        with pytest.raises(ValueError, match='1 of 1 faces have a vertex index outside 0..2'):
            ops.mesh_cluster_faces(bad, vc)
        with pytest.raises(ValueError, match='vertex index outside'):
            simplify_mesh.simplify_device(v, None, bad, c['cell'], origin=c['origin'])
    # a cell coordinate beyond 2^21, and one below the origin
    with pytest.raises(ValueError, match='2\\^21'):
        ops.mesh_cluster(v, None, 1e-7, c['origin'])
    with pytest.raises(ValueError, match='below the origin'):
        ops.mesh_cluster(v, None, c['cell'], (0.5, 0.0, 0.0))
    with pytest.raises(ValueError, match='2\\^21'):
        simplify_mesh.simplify_device(v, None, f, 1e-7, origin=c['origin'])


@pytest.mark.parametrize('shape', ['no_vertices', 'no_faces', 'only_nonfinite'])
def test_empty_meshes_give_empty_outputs(cuda, shape):
    c = K.case('single_face')
    vertices = {'no_vertices': np.zeros((0, 3), np.float32), 'no_faces': c['vertices'],
                'only_nonfinite': np.full((3, 3), np.nan, np.float32)}[shape]
    faces = c['faces'] if shape == 'only_nonfinite' else np.zeros((0, 3), np.int32)
    colors = None if shape == 'no_vertices' else np.full((len(vertices), 3), 9, np.uint8)
    for placement in S.PLACEMENTS:
        out_v, out_c, out_f, report = simplify_mesh.simplify_device(_dev(vertices, cuda), _dev(colors, cuda), _dev(faces, cuda), 0.35, placement,
                                                                    (0.0, 0.0, 0.0))
        torch.cuda.synchronize()
        assert tuple(out_v.shape) == (0, 3) and tuple(out_f.shape) == (0, 3) and (out_c is None) == (colors is None)
        assert (report['vertices_out'], report['faces_out'], report['max_move']) == (0, 0, 0.0)
        assert report['clusters'] == (3 if shape == 'no_faces' else 0) and report['nonfinite_faces'] == (1 if shape == 'only_nonfinite' else 0)
        assert report['census_out'] == T.edge_census(np.zeros((0, 3), np.int32), 0)
