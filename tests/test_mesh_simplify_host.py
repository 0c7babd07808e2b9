"""The mesh simplification on the host (no GPU): the restatement's own invariants on every case, what quadric placement buys on the
cube, the margins, the ABI version and symbols, the build flags, the wrappers' and the module's argument checks, the command
lines' refusals, SceneMesh's option check, and the two pinned parsers' option strings."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd                                   # noqa: F401
from atvsnet_amd import _lib, ops
from atvsnet_amd.atvsnet import eval_pointcloud, mesh_fusion, simplify_mesh
from atvsnet_amd.tools import ply

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mesh_simplify_cases as K  # noqa: E402
import mesh_simplify_restated as S  # noqa: E402

SYMBOLS = ('atvs_mesh_cluster_scratch_size', 'atvs_mesh_cluster', 'atvs_mesh_cluster_quadrics', 'atvs_mesh_cluster_place',
           'atvs_mesh_cluster_max_move', 'atvs_mesh_cluster_faces_scratch_size', 'atvs_mesh_cluster_faces')
CLOSE = 2.0 ** -21          # four float32 spacings of the cube's largest coordinate, 1.2


@pytest.mark.parametrize('placement', S.PLACEMENTS)
@pytest.mark.parametrize('name', K.NAMES)
def test_the_restatement_keeps_its_invariants(name, placement):
    c, r = K.case(name), K.restated(name, placement)
    v, vc, pos = c['vertices'], r['cluster']['vertex_cluster'], r['place']['positions']
    finite = np.isfinite(v).all(1)
    assert np.array_equal(vc >= 0, finite)
    # every finite vertex within cell sqrt(3) of its representative
    d = np.sqrt(((pos[vc[finite]].astype(np.float64) - v[finite].astype(np.float64)) ** 2).sum(1))
    assert d.max() <= c['cell'] * np.sqrt(3.0) and r['max_move'] <= c['cell'] * np.sqrt(3.0)
    # ids in ascending order of the cluster's lowest vertex index, all of them used
    first = np.full(r['counts']['clusters'], len(v))
    np.minimum.at(first, vc[finite], np.nonzero(finite)[0])
    assert (np.diff(first) > 0).all() and r['cluster']['counts'].sum() == finite.sum()
    # the representative lies in its cell (the mean exactly; the quadric's by the fallback), up to the float32 rounding of the output
    x = r['place']['x']
    assert (np.abs(x) <= 0.5).all()
    if placement == 'mean':
        assert not r['place']['placed'].any()
        g = (pos.astype(np.float64) - np.asarray(c['origin'])) / c['cell'] - r['cluster']['cells']
        slack = 2.0 * np.spacing(np.abs(pos).max(initial=1.0).astype(np.float32)) / c['cell']
        assert (g >= -slack).all() and (g <= 1.0 + slack).all()
    # surviving faces: three distinct ids, distinct sets, in their order, with their own winding
    rw = r['rewrite']
    kept = rw['faces'][rw['keep'] != 0]
    assert (kept >= 0).all() and (kept[:, 0] != kept[:, 1]).all() and (kept[:, 1] != kept[:, 2]).all() and (kept[:, 0] != kept[:, 2]).all()
    assert len(np.unique(np.sort(kept, 1), axis=0)) == len(kept)
    assert np.array_equal(kept, vc[c['faces'][rw['keep'] != 0]])
    assert rw['nonfinite_faces'] + rw['degenerate_faces'] + rw['duplicate_faces'] + len(kept) == len(c['faces'])
    out_v, out_c, out_f = r['out']
    assert len(out_f) == len(kept) and (out_c is None) == (c['colors'] is None)
    if len(out_f):
        assert np.array_equal(out_v[out_f], pos[kept])                 # select keeps the order of faces and of clusters
        assert (np.diff(np.unique(kept, return_index=False)) > 0).all()


def test_the_cases_are_what_they_say():
    n = {name: K.restated(name)['counts'] for name in K.NAMES}
    assert (n['cube']['vertices_in'], n['cube']['faces_in'], n['cube']['vertices_out'], n['cube']['faces_out']) == (866, 1728, 98, 192)
    assert n['cube']['placed_by_quadric'] == 98 and n['cube']['duplicate_faces'] == 0 and n['cube_far'] == n['cube']
    assert (n['sphere']['vertices_in'], n['sphere']['faces_in']) == (1986, 3968)
    assert (n['plane']['vertices_in'], n['plane']['faces_in']) == (4900, 9522) and n['plane']['clusters'] > 256
    assert n['plane']['fell_back'] > 0 and n['plane']['duplicate_faces'] >= 1
    assert n['sheets']['faces_in'] == 3364 and n['sheets']['duplicate_faces'] == n['sheets']['faces_out'] > 0      # one copy stays
    assert (n['one_cell']['clusters'], n['one_cell']['vertices_out'], n['one_cell']['faces_out']) == (1, 0, 0)
    for name in ('big_triangles', 'single_face'):                                                                  # back as it went in
        c, r = K.case(name), K.restated(name)
        assert np.array_equal(r['out'][2], c['faces']) and np.array_equal(r['out'][0], c['vertices']) and r['max_move'] == 0.0
    d = K.restated('debris')
    assert (d['counts']['nonfinite_faces'], d['counts']['degenerate_faces'], d['counts']['duplicate_faces'], d['counts']['faces_out']) == (2, 4, 3, 3)
    assert d['cluster']['vertex_cluster'].tolist() == [0, 0, 1, 2, 3, 1, 2, 1, 4, -1, -1, 5, 5, 5, 6]
    assert d['place']['colors'][0].tolist() == [11, 255, 2] and d['place']['colors'][1].tolist() == [1, 3, 134]      # the rounding rule
    assert d['incidences'][5] == 2 and d['incidences'][4] == 0          # the zero-area face adds nothing; the unreferenced vertex has no face
    assert d['counts']['vertices_out'] == 6 and d['counts']['clusters'] == 7
    # saturated weights: each of the two big triangles adds w = 1, so the trace of A is 1 per incidence
    b = K.restated('big_triangles')
    assert np.array_equal(b['quadrics'][:, [0, 3, 5]].sum(1) // 4, (b['incidences'].astype(np.int64) << 30) // 4)


def _cube_distances(vertices):
    """-> (the farthest vertex from the cube's surface, the farthest corner from its nearest vertex)."""
    q = vertices.astype(np.float64) - np.asarray(K.CUBE_CORNER)
    outside = np.sqrt((np.maximum(np.maximum(-q, q - K.CUBE_EDGE), 0.0) ** 2).sum(1))
    inside = np.where((q >= 0).all(1) & (q <= K.CUBE_EDGE).all(1), np.minimum(q, K.CUBE_EDGE - q).min(1), 0.0)
    corners = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], np.float64) * K.CUBE_EDGE
    nearest = np.sqrt(((q[None] - corners[:, None]) ** 2).sum(2)).min(1)
    return float(np.maximum(outside, inside).max()), float(nearest.max())


def test_quadric_placement_keeps_the_cubes_faces_edges_and_corners():
    surface_q, corner_q = _cube_distances(K.restated('cube', 'quadric')['out'][0])
    surface_m, corner_m = _cube_distances(K.restated('cube', 'mean')['out'][0])
    print('cube: farthest output vertex from the surface: quadric %.3g, mean %.3g; farthest corner from a vertex: quadric %.3g, '
          'mean %.3g; 2^-21 = %.3g' % (surface_q, surface_m, corner_q, corner_m, CLOSE))
    assert surface_q <= CLOSE and corner_q <= CLOSE
    assert surface_m > 100.0 * CLOSE


@pytest.mark.parametrize('name', K.NAMES)
def test_few_clusters_sit_on_a_decision(name):
    margin = K.restated(name)['place']['margin']
    assert (margin < 1e-6).sum() <= 0.01 * len(margin)


def test_abi_version_symbols_and_flags():
    L = _lib.lib()
    assert _lib.header_abi_version() >= 63 and L.atvs_abi_version() == _lib.header_abi_version()
    for name in SYMBOLS:
        assert name in _lib.declared_symbols() and hasattr(L, name)
    src = os.path.join(_lib.CSRC, 'mesh_simplify.hip')
    assert src in _lib.sources()
    for flags in (_lib.flags_for(src), _lib.flags_for('mesh_simplify.hip')):
        assert '-ffp-contract=off' in flags and '-fno-slp-vectorize' in flags
    assert ops.MESH_SIMPLIFY_SOLVE_UNITS == _lib.header_macro('ATVS_MESH_SIMPLIFY_SOLVE_UNITS') == 512
    assert ops.MESH_SIMPLIFY_SOLVE_UNITS * 2.0 ** -53 / ops.MESH_RANK_EPSILON < 2.0 ** -30 / 8        # well below cell 2^-30
    assert list(ops.MESH_PLACEMENTS) == ['mean', 'quadric'] and set(S.PLACEMENTS) == set(simplify_mesh.PLACEMENTS) == set(ops.MESH_PLACEMENTS)
    # the solver is shared through a header, not copied
    with open(os.path.join(_lib.CSRC, 'cloud_normals.hip')) as f:
        normals = f.read()
    with open(src) as f:
        simplify = f.read()
    assert '#include "jacobi3.h"' in normals and '#include "jacobi3.h"' in simplify
    assert 'void jacobi_rotate' not in normals and 'void jacobi_rotate' not in simplify


def test_the_c_abi_refuses_bad_arguments_without_a_launch():
    L = _lib.lib()
    n = ctypes.c_long(0)
    org = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    bad_org = (ctypes.c_double * 3)(0.0, float('nan'), 0.0)
    big_f, big_v = (1 << 28) + 1, (1 << 30) + 1
    assert L.atvs_mesh_cluster_scratch_size(100, ctypes.byref(n)) == 0 and n.value >= 64 * 1024 + 8 * 100
    assert L.atvs_mesh_cluster_scratch_size(100, None) == -1
    assert L.atvs_mesh_cluster_scratch_size(-1, ctypes.byref(n)) == -2 and L.atvs_mesh_cluster_scratch_size(big_v, ctypes.byref(n)) == -2
    assert L.atvs_mesh_cluster(None, None, 3, 0.5, org, 8, 1 << 20, 8, 8, 8, 8, None, 8, None) == -1               # vertices
    assert L.atvs_mesh_cluster(8, 8, 3, 0.5, org, 8, 1 << 20, 8, 8, 8, 8, None, 8, None) == -1                     # colors without color_sums
    assert L.atvs_mesh_cluster(8, None, 3, 0.5, None, 8, 1 << 20, 8, 8, 8, 8, None, 8, None) == -1                 # origin
    assert L.atvs_mesh_cluster(8, None, big_v, 0.5, org, 8, 1 << 40, 8, 8, 8, 8, None, 8, None) == -2
    assert L.atvs_mesh_cluster(8, None, 3, 0.5, org, 8, 16, 8, 8, 8, 8, None, 8, None) == -2                       # a short scratch
    for cell in (0.0, -1.0, float('nan'), float('inf')):
        assert L.atvs_mesh_cluster(8, None, 3, cell, org, 8, 1 << 20, 8, 8, 8, 8, None, 8, None) == -3
    assert L.atvs_mesh_cluster(8, None, 3, 0.5, bad_org, 8, 1 << 20, 8, 8, 8, 8, None, 8, None) == -3
    assert L.atvs_mesh_cluster_quadrics(8, 3, None, 1, 8, 3, 0.5, org, 8, 8, 8, None) == -1                        # faces
    assert L.atvs_mesh_cluster_quadrics(8, 3, 8, 1, 8, 3, 0.5, org, 8, 8, None, None) == -1                        # info
    assert L.atvs_mesh_cluster_quadrics(8, 3, 8, 1, 8, 4, 0.5, org, 8, 8, 8, None) == -2                           # more clusters than vertices
    assert L.atvs_mesh_cluster_quadrics(8, 3, 8, big_f, 8, 3, 0.5, org, 8, 8, 8, None) == -2
    assert L.atvs_mesh_cluster_quadrics(8, 3, 8, 1, 8, 3, 0.0, org, 8, 8, 8, None) == -3
    assert L.atvs_mesh_cluster_place(8, 8, 8, None, None, 3, 0.5, org, 1, 1e-3, 8, None, 8, None) == -1            # quadric without quadrics
    assert L.atvs_mesh_cluster_place(8, 8, 8, 8, None, 3, 0.5, org, 0, 1e-3, 8, None, 8, None) == -1               # color_sums without colors_out
    assert L.atvs_mesh_cluster_place(8, 8, 8, None, 8, 3, 0.5, org, 2, 1e-3, 8, None, 8, None) == -3               # placement
    for eps in (0.0, 1.0, -1e-3, float('nan')):
        assert L.atvs_mesh_cluster_place(8, 8, 8, None, 8, 3, 0.5, org, 1, eps, 8, None, 8, None) == -3
    assert L.atvs_mesh_cluster_place(8, 8, 8, None, 8, -1, 0.5, org, 1, 1e-3, 8, None, 8, None) == -2
    assert L.atvs_mesh_cluster_max_move(8, 3, 8, 8, 3, None, None) == -1
    assert L.atvs_mesh_cluster_max_move(8, 3, 8, 8, 4, 8, None) == -2
    assert L.atvs_mesh_cluster_faces_scratch_size(0, ctypes.byref(n)) == 0 and n.value == 4 * ops.MESH_SIMPLIFY_MIN_SLOTS
    assert L.atvs_mesh_cluster_faces_scratch_size(1000, ctypes.byref(n)) == 0 and n.value == 4 * 2048 + 4096          # 2000 -> 2^11 slots
    assert L.atvs_mesh_cluster_faces_scratch_size(1000, None) == -1
    assert L.atvs_mesh_cluster_faces_scratch_size(big_f, ctypes.byref(n)) == -2
    assert L.atvs_mesh_cluster_faces(None, 1, 3, 8, 8, 1 << 20, 8, 8, 8, None) == -1
    assert L.atvs_mesh_cluster_faces(8, 1, 3, 8, 8, 1 << 20, 8, None, 8, None) == -1                               # keep
    assert L.atvs_mesh_cluster_faces(8, 1, 3, 8, 8, 16, 8, 8, 8, None) == -2                                       # a short scratch
    assert L.atvs_mesh_cluster_faces(8, big_f, 3, 8, 8, 1 << 40, 8, 8, 8, None) == -2


def _meta(shape, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device='meta')


def test_the_wrappers_argument_errors():
    v, c, f = _meta((5, 3)), _meta((5, 3), torch.uint8), _meta((2, 3), torch.int32)
    org = (0.0, 0.0, 0.0)
    cl = ops.mesh_cluster(v, c, 0.5, org)                              # the host checks alone run on `meta`
    assert tuple(cl.vertex_cluster.shape) == (5,) and cl.vertex_cluster.dtype == torch.int32 and cl.position_sums.dtype == torch.int64
    assert ops.mesh_cluster(v, None, 0.5, org).color_sums is None
    vc = _meta((5,), torch.int32)
    q, inc = ops.mesh_cluster_quadrics(v, f, vc, 4, 0.5, org)
    assert tuple(q.shape) == (4, 10) and q.dtype == torch.int64 and tuple(inc.shape) == (4,)
    cells, counts, sums = _meta((4, 3), torch.int32), _meta((4,), torch.int32), _meta((4, 3), torch.int64)
    p, pc, placed = ops.mesh_cluster_place(cells, counts, sums, sums, q, 0.5, org)
    assert tuple(p.shape) == (4, 3) and pc.dtype == torch.uint8 and placed.dtype == torch.uint8
    assert ops.mesh_cluster_place(cells, counts, sums, None, None, 0.5, org, 'mean')[1] is None
    fo, keep, drops = ops.mesh_cluster_faces(f, vc)
    assert tuple(fo.shape) == (2, 3) and keep.dtype == torch.uint8 and sorted(drops) == ['degenerate_faces', 'duplicate_faces', 'nonfinite_faces']
    assert ops.mesh_cluster_max_move(v, vc, p) == 0.0
    for cell in (0, -1.0, float('nan'), float('inf'), '0.5', True, None):
        with pytest.raises(ValueError, match='cell'):
            ops.mesh_cluster(v, c, cell, org)
    for origin in (None, (0.0, 1.0), (0.0, float('nan'), 0.0), 'abc'):
        with pytest.raises(ValueError, match='origin'):
            ops.mesh_cluster(v, c, 0.5, origin)
    with pytest.raises(TypeError, match='vertices'):
        ops.mesh_cluster(v.double(), c, 0.5, org)
    with pytest.raises(ValueError, match='colors'):
        ops.mesh_cluster(v, _meta((4, 3), torch.uint8), 0.5, org)
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.mesh_cluster(torch.zeros(5, 3), None, 0.5, org)
    with pytest.raises(TypeError, match='faces'):
        ops.mesh_cluster_quadrics(v, f.long(), vc, 4, 0.5, org)
    with pytest.raises(ValueError, match='vertex_cluster'):
        ops.mesh_cluster_quadrics(v, f, _meta((4,), torch.int32), 4, 0.5, org)
    with pytest.raises(ValueError, match='num_clusters'):
        ops.mesh_cluster_quadrics(v, f, vc, 6, 0.5, org)
    with pytest.raises(ValueError, match='placement'):
        ops.mesh_cluster_place(cells, counts, sums, None, q, 0.5, org, 'median')
    with pytest.raises(ValueError, match='quadrics'):
        ops.mesh_cluster_place(cells, counts, sums, None, None, 0.5, org, 'quadric')
    for eps in (0, 1, -0.5, float('nan'), 'small', None):
        with pytest.raises(ValueError, match='rank_epsilon'):
            ops.mesh_cluster_place(cells, counts, sums, None, q, 0.5, org, 'quadric', eps)
    with pytest.raises(ValueError, match='counts'):
        ops.mesh_cluster_place(cells, _meta((3,), torch.int32), sums, None, q, 0.5, org)
    with pytest.raises(TypeError, match='position_sums'):
        ops.mesh_cluster_place(cells, counts, sums.int(), None, q, 0.5, org)
    with pytest.raises(TypeError, match='vertex_cluster'):
        ops.mesh_cluster_faces(f, vc.long())


def test_the_module_checks_its_options_before_anything_touches_a_gpu():
    v, f = np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.int32)
    assert simplify_mesh.check_options(0.5) == (0.5, 'quadric', None, 1e-3)
    assert simplify_mesh.check_options(2, 'mean', [1, 2, 3], 0.01) == (2.0, 'mean', (1.0, 2.0, 3.0), 0.01)
    for bad, word in ((dict(cell=0), 'cell'), (dict(cell=-1), 'cell'), (dict(cell=float('nan')), 'cell'), (dict(cell='1'), 'cell'),
                      (dict(cell=None), 'cell'), (dict(cell=1, placement='median'), 'placement'), (dict(cell=1, placement=None), 'placement'),
                      (dict(cell=1, rank_epsilon=0), 'rank_epsilon'), (dict(cell=1, rank_epsilon=1.0), 'rank_epsilon'),
                      (dict(cell=1, rank_epsilon=float('nan')), 'rank_epsilon'), (dict(cell=1, origin=(0, 1)), 'origin'),
                      (dict(cell=1, origin=(0, 1, float('inf'))), 'origin'), (dict(cell=1, origin='here'), 'origin')):
        with pytest.raises(ValueError, match=word):
            simplify_mesh.simplify(v, None, f, **bad)
    with pytest.raises(ValueError, match='colors'):
        simplify_mesh.simplify(v, np.zeros((2, 3), np.uint8), f, cell=1.0)


def test_command_lines_refuse(capsys, tmp_path):
    def refused(argv, text):
        with pytest.raises(SystemExit) as e:
            simplify_mesh.cli(argv)
        assert e.value.code == 2 and text in ' '.join(capsys.readouterr().err.split())

    mesh = tmp_path / 'mesh.ply'
    ply.write_mesh(str(mesh), np.zeros((3, 3), np.float32), None, np.array([[0, 1, 2]], np.int32))
    io = ['--in', str(mesh), '--out', str(tmp_path / 'out.ply')]
    refused(io, '--cell')                                             # it has no default
    refused(io + ['--cell', '0'], '--cell must be a positive finite number')
    refused(io + ['--cell', 'nan'], '--cell must be a positive finite number')
    refused(io + ['--cell', '1', '--placement', 'median'], '--placement must be one of quadric, mean')
    refused(io + ['--cell', '1', '--rank_epsilon', '1'], '--rank_epsilon must be a number in (0, 1)')
    refused(io + ['--cell', '1', '--origin', '1,2'], 'expected x,y,z')
    refused(io + ['--cell', '1', '--origin', '1,2,inf'], '--origin must be 3 finite numbers')
    refused(['--in', str(tmp_path / 'none.ply'), '--out', 'x.ply', '--cell', '1'], 'no such file')
    (tmp_path / 'broken.ply').write_bytes(b'ply\nformat ascii 1.0\nelement vertex 1\n')
    refused(['--in', str(tmp_path / 'broken.ply'), '--out', 'x.ply', '--cell', '1'], 'broken.ply')
    text = ' '.join(simplify_mesh.make_parser().format_help().split())
    for option in ('--in', '--out', '--cell', '--placement', '--origin', '--rank_epsilon', '--report', '--gpu_id'):
        assert option in text
    assert 'no default' in text


def test_scene_mesh_checks_simplify_without_a_gpu():
    check = mesh_fusion.check_options
    assert check(0.1, simplify=dict(cell_voxels=3)) == check(0.1) == check(0.1, simplify=None)
    assert check(0.1, simplify=dict(cell_voxels=2.5, placement='mean', rank_epsilon=0.01)) == check(0.1)
    assert mesh_fusion.check_simplify(dict(cell_voxels=3)) == (3.0, 'quadric', 1e-3) and mesh_fusion.check_simplify(None) is None
    for bad, word in ((dict(cell_voxels=0), 'cell_voxels'), (dict(cell_voxels=-2), 'cell_voxels'), (dict(cell_voxels='3'), 'cell_voxels'),
                      (dict(), 'cell_voxels'), (dict(placement='mean'), 'cell_voxels'), (dict(cell_voxels=3, placement='x'), 'placement'),
                      (dict(cell_voxels=3, rank_epsilon=2), 'rank_epsilon'), (dict(cell_voxels=3, cell=0.1), 'simplify'), (3, 'simplify')):
        with pytest.raises(ValueError, match=word):
            check(0.1, simplify=bad)


def test_the_driver_gains_its_row_only_with_the_argument():
    E = eval_pointcloud
    fuse = dict(prob_threshold=0.8, disp_threshold=0.01, num_consistent=2)
    base = E._option_rules(fuse=fuse, mesh=dict(voxel=0.05))
    rules = E._option_rules(fuse=fuse, mesh=dict(voxel=0.05, simplify=dict(cell_voxels=3)))
    assert len(rules) == len(base) + 1 and not any(b for b, _ in rules)
    assert [m for _, m in rules if 'simplify' not in m] == [m for _, m in base]
    broken = [m for b, m in E._option_rules(fuse=fuse, mesh=dict(simplify=dict(cell_voxels=3))) if b]
    assert 'mesh simplify= needs voxel=' in broken[0]
    with pytest.raises(ValueError, match='simplify= needs voxel='):
        E.run_eval_pc('out', [], fuse=fuse, mesh=dict(simplify=dict(cell_voxels=3)))
    with pytest.raises(ValueError, match='cell_voxels'):
        E.run_eval_pc('out', [], fuse=fuse, mesh=dict(voxel=0.05, simplify=dict(cell_voxels=0)))


def test_the_pinned_parsers_have_exactly_the_option_strings_they_had():
    with open(os.path.join(HERE, 'golden', 'cli_surface.json')) as f:
        golden = json.load(f)['surface']
    for tool in (eval_pointcloud, mesh_fusion):
        got = sorted(list(a.option_strings) for a in tool.make_parser()._actions)
        assert got == [row[0] for row in golden[tool.__name__.rsplit('.', 1)[1]]]
        assert not any('simpl' in s for strings in got for s in strings)
