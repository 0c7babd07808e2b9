"""The point-to-triangle kernels (csrc/mesh_distance.hip) against their numpy restatement on every case of
tests/mesh_distance_cases.py: d2, face and closest bit for bit, computed twice with the same bits both times (no query is left out
of the face comparison); the same bits under reference budgets that force one, two and more coarsenings, with the queries permuted,
and through a larger radius wherever the distance is within the smaller one; the properties (a usable face's corners are at
distance 0, a surface sample within the rounding of its float32 coordinates, the surface never further than the nearest sample);
the empty shapes."""
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
from atvsnet_amd import ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_distance_cases as C  # noqa: E402
import mesh_distance_restated as R  # noqa: E402

pytestmark = pytest.mark.gpu

case = pytest.mark.parametrize('name', C.NAMES)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    g = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert g.shape == want.shape and g.dtype == want.dtype, (what, g.dtype, want.dtype, g.shape, want.shape)
    ne = np.nonzero(_bits(g).reshape(-1) != _bits(want).reshape(-1))[0]
    assert len(ne) == 0, '%s: %d of %d elements differ, first at %d: %r against %r' % (
        what, len(ne), g.size, ne[0], g.reshape(-1)[ne[0]], want.reshape(-1)[ne[0]])


def _search(c, dev, radius=None, max_refs=None, queries=None):
    grid = ops.mesh_grid(_dev(c['vertices'], dev), _dev(c['faces'], dev), c['radius'] if radius is None else radius, max_refs)
    q = _dev(c['queries'] if queries is None else queries, dev)
    return grid, [t.cpu().numpy() for t in ops.mesh_nearest(grid, q, closest=True)]


@case
def test_d2_face_and_closest_are_the_restatement_twice(cuda, name):
    c = C.case(name)
    want = C.restated(name)
    usable = int(R.usable_faces(c['vertices'], c['faces']).sum())
    for _ in range(2):
        grid, got = _search(c, cuda)
        print('%s: %d faces (%d usable), %d queries, %d found, cell %g, %d references, %d build(s)' % (
            name, len(c['faces']), grid.usable_faces, len(c['queries']), int((got[1] >= 0).sum()), grid.cell, grid.refs, grid.rounds))
        assert grid.usable_faces == usable and grid.n_faces == len(c['faces']) and grid.refs <= grid.max_refs
        assert grid.cell >= c['radius'] * (1.0 + 2.0 ** -20)
        for g, w, what in zip(got, want, ('d2', 'face', 'closest')):
            _same(g, w, '%s of %s' % (what, name))
        d2, face = ops.mesh_nearest(grid, _dev(c['queries'], cuda))              # without the third output: the same two
        _same(d2, want[0], 'd2 alone')
        _same(face, want[1], 'face alone')


@pytest.mark.parametrize('name', ['big_triangles', 'cube', 'zero_area', 'debris_bad_index'])
def test_the_reference_budget_and_its_coarsenings_cannot_be_seen(cuda, name):
    """Budgets chosen from the restatement's count of the references at the free grid's cell edge doubled k times: each makes the
    device build exactly as often as the restated loop, and reach its cell edge and its count; the results keep their bits."""
    c = C.case(name)
    want = C.restated(name)
    free, _ = _search(c, cuda)
    least = 8 * len(c['faces'])
    assert free.rounds == 1 and free.refs == R.grid_refs(c['vertices'], c['faces'], free.cell)
    ladder = R.coarsening(c['vertices'], c['faces'], free.cell, least)            # [(cell edge, references)] down to 8 per face
    seen = set()
    for budget in sorted({least, max(least, free.refs - 1)} | {refs for _, refs in ladder[1:] if refs >= least}):
        steps = R.coarsening(c['vertices'], c['faces'], free.cell, budget)
        grid, got = _search(c, cuda, max_refs=budget)
        seen.add(grid.rounds)
        print('%s: budget %d -> %d build(s), cell %g, %d references (free: %d at %g)' % (name, budget, grid.rounds, grid.cell, grid.refs,
                                                                                         free.refs, free.cell))
        assert (grid.rounds, grid.cell, grid.refs) == (len(steps),) + steps[-1] and grid.refs <= budget
        for g, w, what in zip(got, want, ('d2', 'face', 'closest')):
            _same(g, w, '%s of %s under a budget of %d' % (what, name, budget))
    if name == 'big_triangles':
        assert {2, 3, 4} <= seen, seen                                # one, two and more coarsenings ran
    assert free.refs <= least or max(seen) >= 2


@pytest.mark.parametrize('name', ['cube', 'sheets', 'twice'])
def test_the_order_of_the_queries_cannot_be_seen(cuda, name):
    c = C.case(name)
    want = C.restated(name)
    perm = np.random.RandomState(5).permutation(len(c['queries']))
    _, got = _search(c, cuda, queries=c['queries'][perm])
    for g, w, what in zip(got, want, ('d2', 'face', 'closest')):
        _same(g, w[perm], '%s of %s, permuted' % (what, name))


@pytest.mark.parametrize('name', ['cube', 'sheets', 'big_triangles', 'zero_area'])
def test_a_larger_radius_gives_the_same_results_within_the_smaller(cuda, name):
    c = C.case(name)
    want = C.restated(name)
    for factor in (1.37, 3.0):
        _, got = _search(c, cuda, radius=c['radius'] * factor)
        within = want[1] >= 0
        assert within.sum() > 100
        for g, w, what in zip(got, want, ('d2', 'face', 'closest')):
            _same(g[within], w[within], '%s of %s through %g radii' % (what, name, factor))
        r2 = float(np.float32(c['radius'])) ** 2
        assert (got[0][~within].astype(np.float64) > r2).all()                    # what the smaller radius did not find is further


@pytest.mark.parametrize('name', ['cube', 'big_triangles', 'debris_bad_index', 'zero_area'])
def test_the_corners_of_usable_faces_are_at_distance_zero(cuda, name):
    c = C.case(name)
    usable = R.usable_faces(c['vertices'], c['faces'])
    corners = np.ascontiguousarray(c['vertices'][np.unique(c['faces'][usable])])
    _, (d2, face, closest) = _search(c, cuda, queries=corners)
    assert (d2 == 0.0).all() and (face >= 0).all() and usable[face].all()
    _same(closest, corners, 'the closest point of a corner')


@pytest.mark.parametrize('name', ['cube', 'sheets', 'big_triangles'])
def test_samples_lie_on_the_surface_and_the_surface_is_never_further_than_a_sample(cuda, name):
    """A sample is (a + u e1) + v e2 in double rounded to float32: each coordinate moves by at most half a unit in the last place,
    2^-24 |coordinate|, so its distance to its own face is at most sqrt(3) 2^-24 M with M the largest |coordinate| of the mesh, and
    d2 <= 3 (2^-24 M)^2, times (1 + 2^-20) for the roundings of the distance itself.  For any query the exact distance is at most
    the distance to any point of the surface, a sample included: d_surface <= d_sample + sqrt(3) 2^-24 M (the sample's own offset),
    compared in double on the square roots with 2^-20 relative for the float32 roundings of both d2."""
    c = C.case(name)
    v, f = _dev(c['vertices'], cuda), _dev(c['faces'], cuda)
    M = float(np.abs(c['vertices'][np.unique(c['faces'])]).max())
    spacing = c['radius'] / 2.0
    samples, info = ops.mesh_sample(v, None, f, 1.0 / spacing ** 2, 3)
    assert info['samples'] > 200
    grid = ops.mesh_grid(v, f, c['radius'])
    d2, face = ops.mesh_nearest(grid, samples.points)
    off = np.sqrt(3.0) * 2.0 ** -24 * M
    print('%s: %d samples, largest d2 %.3g (bar %.3g)' % (name, info['samples'], float(d2.max()), off * off * (1 + 2.0 ** -20)))
    assert (face >= 0).all() and float(d2.max()) <= off * off * (1.0 + 2.0 ** -20)
    q = _dev(c['queries'], cuda)
    s2, _ = ops.cloud_nearest(ops.cloud_grid(samples.points, c['radius']), q)
    e2, _ = ops.mesh_nearest(grid, q)
    s, e = np.sqrt(s2.cpu().numpy().astype(np.float64)), np.sqrt(e2.cpu().numpy().astype(np.float64))
    near = np.isfinite(s)
    assert near.sum() > 100 and np.isfinite(e[near]).all()
    assert (e[near] <= s[near] * (1.0 + 2.0 ** -20) + off).all()


def test_empty_shapes(cuda):
    c = C.case('cube')
    v, f, q = _dev(c['vertices'], cuda), _dev(c['faces'], cuda), _dev(c['queries'][:50], cuda)
    none = ops.mesh_grid(v, f[:0], 0.1)
    assert none.usable_faces == 0 and none.refs == 0 and none.rounds == 1
    d2, face, closest = ops.mesh_nearest(none, q, closest=True)
    assert torch.isinf(d2).all() and (face == -1).all() and torch.isnan(closest).all()
    d2, face, closest = ops.mesh_nearest(ops.mesh_grid(v, f, 0.1), q[:0], closest=True)
    assert tuple(d2.shape) == (0,) and tuple(face.shape) == (0,) and tuple(closest.shape) == (0, 3)
    bad = f.clone()
    bad[:, 1] = -1
    unusable = ops.mesh_grid(v, bad, 0.1)
    assert unusable.usable_faces == 0
    d2, face = ops.mesh_nearest(unusable, q)
    assert torch.isinf(d2).all() and (face == -1).all()
    nothing = ops.mesh_grid(v[:0], f[:0], 0.1)
    d2, face = ops.mesh_nearest(nothing, q)
    assert torch.isinf(d2).all() and (face == -1).all()
