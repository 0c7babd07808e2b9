"""The mesh topology kernels (csrc/mesh_topology.hip) against their numpy restatement, bit for bit: every case of
tests/mesh_topology_cases.py through ops.mesh_components, ops.mesh_select and ops.mesh_edge_census; every op twice; bad indices;
mesh_fusion.mesh_report on device tensors against the same tensors on the host."""
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
from atvsnet_amd import ops
from atvsnet_amd.atvsnet import clean_mesh, mesh_fusion

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_topology_cases as MC  # noqa: E402
import mesh_topology_restated as T  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def cuda():
    assert torch.cuda.is_available()
    return torch.device('cuda', torch.cuda.current_device())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want):
    """Device tensors (or None) against numpy arrays (or None): dtype, shape and bits."""
    for g, w in zip(got, want):
        if w is None:
            assert g is None
            continue
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(_bits(g), _bits(w))


def _census(faces, V, dev):
    return ops.mesh_edge_census(torch.from_numpy(faces).to(dev), V)


@pytest.mark.parametrize('name', MC.NAMES)
def test_census_is_the_restatement_twice(cuda, name):
    c = MC.case(name)
    want = T.edge_census(c['faces'], c['V'])
    got = _census(c['faces'], c['V'], cuda)
    print(name, got)
    assert set(got) == set(T.CENSUS_WORDS) and all(type(n) is int for n in got.values())
    assert got == want
    assert _census(c['faces'], c['V'], cuda) == got


@pytest.mark.parametrize('name', [n for n in MC.NAMES if n != 'high_bits'])
def test_components_are_the_restatement_twice(cuda, name):
    c = MC.case(name)
    want = T.components(c['faces'], c['V'])
    faces = torch.from_numpy(c['faces']).to(cuda)
    got = ops.mesh_components(faces, c['V'])
    print(name, 'C =', len(want[2]), 'largest', sorted(want[2].tolist())[-3:])
    _same(got, want)
    again = ops.mesh_components(faces, c['V'])
    assert all(torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize('colored', [False, True])
@pytest.mark.parametrize('name', [n for n in MC.NAMES if n != 'high_bits'])
def test_select_is_the_restatement_twice(cuda, name, colored):
    c = MC.case(name)
    vertices = MC.poisoned(c['vertices'])
    colors = c['colors'] if colored else None
    dv, df = torch.from_numpy(vertices).to(cuda), torch.from_numpy(c['faces']).to(cuda)
    dc = None if colors is None else torch.from_numpy(colors).to(cuda)
    for kind, keep in MC.select_keeps(c).items():
        want = T.select(vertices, colors, c['faces'], keep)
        dk = torch.from_numpy(keep).to(cuda)
        got = ops.mesh_select(dv, dc, df, dk)
        _same(got, want)
        again = ops.mesh_select(dv, dc, df, dk)
        assert all(a is None and b is None or torch.equal(a, b) for a, b in zip(got[2:], again[2:]))
        assert np.array_equal(_bits(got[0].cpu().numpy()), _bits(again[0].cpu().numpy()))


@pytest.mark.parametrize('criterion', [dict(min_faces=9), dict(min_ratio='1/100'), dict(keep_largest=1)])
def test_each_criterion_leaves_exactly_the_sphere(cuda, criterion):
    vertices, faces, of_sphere = MC.sphere_and_shells()
    vertices = MC.poisoned(vertices)
    colors = MC.case('sphere_and_shells')['colors']
    _, face_component, face_count, _ = T.components(faces, len(vertices))
    keep = clean_mesh.keep_components(face_count, **criterion)
    assert keep.sum() == 1 and np.array_equal(keep[face_component], of_sphere)
    want = T.select(vertices, colors, faces, of_sphere.astype(np.uint8))          # exactly the faces of the components dropped
    got = ops.mesh_select(torch.from_numpy(vertices).to(cuda), torch.from_numpy(colors).to(cuda), torch.from_numpy(faces).to(cuda),
                          torch.from_numpy(of_sphere.astype(np.uint8)).to(cuda))
    _same(got, want)
    out_v, out_c, out_f, report = clean_mesh.clean(vertices, colors, faces, **criterion)
    assert np.array_equal(_bits(out_v), _bits(want[0])) and np.array_equal(out_c, want[1]) and np.array_equal(out_f, want[2])
    census = report['census_out']
    assert census == T.edge_census(want[2], len(want[0])) and report['census_in'] == T.edge_census(faces, len(vertices))
    assert len(out_v) - census['edges'] + len(out_f) == 2 and census['boundary'] == 0 and census['misoriented'] == 0
    assert (want[3] >= 0).sum() == len(out_v) == len(np.unique(out_f))            # no unreferenced vertex
    assert report['components'] == MC.SHELLS + 1 and report['components_removed'] == MC.SHELLS
    assert report['largest_components'] == [11888] + [8] * 15
    assert (report['faces_in'], report['faces_out'], report['vertices_in']) == (len(faces), 11888, len(vertices))


def test_bad_indices_raise_naming_the_count(cuda):
    faces, V, bad = MC.bad_index_cases()
    df = torch.from_numpy(faces).to(cuda)
    with pytest.raises(ValueError, match='mesh_components: %d of %d faces' % (bad, len(faces))):
        ops.mesh_components(df, V)
    with pytest.raises(ValueError, match='mesh_edge_census: %d of %d faces' % (bad, len(faces))):
        ops.mesh_edge_census(df, V)
    dv = torch.zeros((V, 3), device=cuda)
    with pytest.raises(ValueError, match='mesh_select: %d of %d faces' % (bad, len(faces))):
        ops.mesh_select(dv, None, df, torch.ones(len(faces), dtype=torch.uint8, device=cuda))
    keep = torch.tensor([1, 0, 1, 1, 1], dtype=torch.uint8, device=cuda)          # only kept faces count
    with pytest.raises(ValueError, match='mesh_select: 1 of'):
        ops.mesh_select(dv, None, df, keep)
    keep[3] = 0
    got = ops.mesh_select(dv, None, df, keep)
    _same(got, T.select(np.zeros((V, 3), np.float32), None, faces, keep.cpu().numpy()))


class _Volume(object):
    origin, voxel, trunc, dims, num_blocks = (0.0, 0.0, 0.0), 1.0, 4.0, (4, 4, 4), 0


@pytest.mark.parametrize('name', ['clipped_sphere', 'sphere_and_shells', 'self_edges', 'empty_v7'])
def test_mesh_report_on_the_device_is_mesh_report_on_the_host(cuda, name):
    c = MC.case(name)
    v, f = torch.from_numpy(c['vertices']), torch.from_numpy(c['faces'])
    host = mesh_fusion.mesh_report(_Volume(), (v, None, f), 1.0, {'extract': 0.5})
    device = mesh_fusion.mesh_report(_Volume(), (v.to(cuda), None, f.to(cuda)), 1.0, {'extract': 0.5})
    assert host == device and host['boundary_edges'] == T.edge_census(c['faces'], c['V'])['boundary']
