"""Every case of tests/mesh_topology_cases.py has what it promises, on the restatement alone (no GPU): the component counts and
sizes, the census words, the unreferenced vertices -- so that a pass of tests/test_gpu_mesh_topology.py means something."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_topology_cases as MC  # noqa: E402
import mesh_topology_restated as T  # noqa: E402


@pytest.mark.parametrize('name', MC.NAMES)
def test_the_case_has_what_it_promises(name):
    MC.check_promise(MC.case(name))


def test_the_strips_are_one_path_in_three_numberings():
    a, b, c = (MC.case('strip_' + k)['faces'] for k in ('ascending', 'descending', 'shuffled'))
    assert (np.diff(a[:, 0]) == 1).all() and (np.diff(b[:, 0]) == -1).all() and not (np.diff(c[:, 0]) == 1).all()
    assert len(a) == len(b) == len(c) == 20000


def test_the_stars_share_the_highest_and_the_lowest_vertex():
    for name, hub in (('star_highest', 2 * 8192), ('star_lowest', 0)):
        faces = MC.case(name)['faces']
        assert len(faces) == 8192 and (faces == hub).any(axis=1).all()


def test_the_sphere_with_shells_cleans_to_the_sphere():
    vertices, faces, of_sphere = MC.sphere_and_shells()
    _, face_component, face_count, _ = T.components(faces, len(vertices))
    giant = int(np.argmax(face_count))
    assert np.array_equal(face_component == giant, of_sphere) and of_sphere.sum() == 11888
    v, _, f, vertex_map = T.select(vertices, None, faces, of_sphere.astype(np.uint8))
    census = T.edge_census(f, len(v))
    assert len(v) - census['edges'] + len(f) == 2 and census['boundary'] == 0 and census['misoriented'] == 0
    assert len(np.unique(f)) == len(v) == (vertex_map >= 0).sum() == 5946
    centre = np.array(MC.CENTRE)
    removed = vertices[vertex_map < 0].astype(np.float64)
    assert len(removed) == 6 * MC.SHELLS and (np.linalg.norm(removed - centre, axis=1) > MC.RADIUS + 2.0).all()       # outside it


def test_select_on_the_restatement_keeps_order_and_bits():
    c = MC.case('sphere_and_shells')
    vertices = MC.poisoned(c['vertices'])
    assert np.isnan(vertices).any() and np.signbit(vertices[vertices == 0]).any()
    for kind, keep in MC.select_keeps(c).items():
        v, col, f, vertex_map = T.select(vertices, c['colors'], c['faces'], keep)
        kept = np.flatnonzero(vertex_map >= 0)
        assert np.array_equal(vertex_map[kept], np.arange(len(kept)))                   # in their order
        assert np.array_equal(v.view(np.uint32), vertices.view(np.uint32)[kept]) and np.array_equal(col, c['colors'][kept])
        assert np.array_equal(kept[f], c['faces'][keep != 0])                           # renumbered, in their order
        assert len(f) == {'all': len(c['faces']), 'none': 0, 'third': (len(c['faces']) + 2) // 3}[kind]


def test_components_against_scipy():
    sparse = pytest.importorskip('scipy.sparse')
    csgraph = pytest.importorskip('scipy.sparse.csgraph')
    for name in ('two_tetrahedra', 'isolated', 'sphere_and_shells', 'strip_shuffled', 'self_edges'):
        c = MC.case(name)
        f, V = c['faces'].astype(np.int64), c['V']
        rows = np.concatenate([f[:, 0], f[:, 1]])
        cols = np.concatenate([f[:, 1], f[:, 2]])
        n, labels = csgraph.connected_components(sparse.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(V, V)), directed=False)
        vc, _, face_count, _ = T.components(f, V)
        referenced = vc >= 0
        assert n - int((~referenced).sum()) == len(face_count)
        pairs = set(zip(labels[referenced].tolist(), vc[referenced].tolist()))
        assert len(pairs) == len(face_count)                                            # the two labellings are one partition


def test_bad_indices_are_counted():
    faces, V, bad = MC.bad_index_cases()
    assert T.bad_faces(faces, V) == bad and (faces == -1).sum() == 1 and (faces == V).sum() == 1
    for fn in (lambda: T.components(faces, V), lambda: T.edge_census(faces, V),
               lambda: T.select(np.zeros((V, 3), np.float32), None, faces, np.ones(len(faces)))):
        with pytest.raises(ValueError, match='%d of %d faces' % (bad, len(faces))):
            fn()
