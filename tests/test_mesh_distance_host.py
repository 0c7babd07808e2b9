"""The point-to-triangle distance on the host (no GPU): the header's constants and symbols and the C entry points' refusals; the
argument errors of ops.mesh_grid / ops.mesh_nearest and their shapes on `meta`; the numpy restatement
(tests/mesh_distance_restated.py) against its second, independently written reference on every case, within the bar derived there;
the census of the regions the cases reach; the rows of the buffer contract."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
from atvsnet_amd import _lib, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buffer_contract_rows as BR  # noqa: E402
import mesh_distance_cases as C  # noqa: E402
import mesh_distance_contract_rows as MR  # noqa: E402
import mesh_distance_restated as R  # noqa: E402

NAMES = ('atvs_mesh_grid_scratch_size', 'atvs_mesh_grid_build', 'atvs_mesh_nearest_scratch_size', 'atvs_mesh_nearest')


# ------------------------------------------------------------------------------------------------------------------------- the ABI
def test_abi_version_constants_and_symbols():
    L = _lib.lib()
    assert _lib.header_abi_version() >= 65 and L.atvs_abi_version() == _lib.header_abi_version()
    for name in NAMES:
        assert name in _lib.declared_symbols() and hasattr(L, name)
    assert ops.MESH_GRID_MAX_REFS == _lib.header_macro('ATVS_MESH_GRID_MAX_REFS') == (1 << 31) - 1
    assert '-ffp-contract=off' in _lib.flags_for(os.path.join(_lib.CSRC, 'mesh_distance.hip'))
    with open(_lib.HEADER) as f:
        text = f.read()
    assert text.index('atvs_mesh_sample_place(') < text.index('atvs_mesh_grid_scratch_size(')       # appended behind the last declaration


def test_the_c_abi_refuses_bad_arguments_without_a_launch():
    L = _lib.lib()
    buf = (ctypes.c_double * 16)()                                   # a stand-in pointer: refusals come before any launch
    ptr = ctypes.c_void_p(ctypes.addressof(buf))
    n = ctypes.c_long(0)
    size = L.atvs_mesh_grid_scratch_size
    assert size(-1, 0, ctypes.byref(n)) == -2 and size((1 << 28) + 1, 1 << 31 - 1, ctypes.byref(n)) == -2
    assert size(1, -1, ctypes.byref(n)) == -2 and size(1, 1 << 31, ctypes.byref(n)) == -2 and size(1, 8, None) == -1
    assert size(0, 0, ctypes.byref(n)) == 0 and n.value > 256
    assert size(100, 800, ctypes.byref(n)) == 0
    grid_bytes = n.value
    build = lambda nv=3, nf=100, r=0.1, cell=0.0, refs=800, grid=ptr, nbytes=grid_bytes, info=ptr: L.atvs_mesh_grid_build(      # noqa: E731
        ptr, nv, ptr, nf, r, cell, refs, grid, nbytes, info, None)
    assert build(nv=-1) == -2 and build(nv=(1 << 30) + 1) == -2 and build(nf=-1) == -2 and build(nbytes=grid_bytes - 1) == -2
    assert build(r=0.0) == -3 and build(r=-1.0) == -3 and build(r=float('nan')) == -3 and build(r=float('inf')) == -3
    assert build(cell=-1.0) == -3 and build(cell=float('nan')) == -3 and build(cell=float('inf')) == -3
    assert build(refs=799) == -3                                     # fewer than 8 references per face: the coarsening could not end
    assert build(grid=None) == -1 and build(info=None) == -1
    qsize = L.atvs_mesh_nearest_scratch_size
    assert qsize(-1, 1, ctypes.byref(n)) == -2 and qsize(1, -1, ctypes.byref(n)) == -2 and qsize(1, (1 << 30) + 1, ctypes.byref(n)) == -2
    assert qsize(1, 1, None) == -1 and qsize(100, 10, ctypes.byref(n)) == 0
    near = lambda nf=100, refs=800, m=10, nbytes=grid_bytes, sbytes=n.value, d2=ptr, q=ptr: L.atvs_mesh_nearest(      # noqa: E731
        ptr, nbytes, nf, refs, q, m, ptr, sbytes, d2, ptr, None, None)
    assert near(nf=-1) == -2 and near(m=-1) == -2 and near(refs=-1) == -2 and near(nbytes=grid_bytes - 1) == -2 and near(sbytes=n.value - 1) == -2
    assert near(d2=None) == -1 and near(q=None) == -1 and near(m=0) == 0


# ---------------------------------------------------------------------------------------------------------------------------- ops
def _meta(shape, dtype):
    return torch.empty(shape, dtype=dtype, device='meta')


def test_ops_refuse_bad_arguments_and_plan_shapes_on_meta():
    v, f, q = _meta((5, 3), torch.float32), _meta((4, 3), torch.int32), _meta((7, 3), torch.float32)
    grid = ops.mesh_grid(v, f, 0.1)
    assert isinstance(grid, ops.MeshGrid) and (grid.n_vertices, grid.n_faces, grid.max_refs) == (5, 4, 1 << 20) and grid.radius == float(np.float32(0.1))
    assert ops.mesh_grid(v, f, 0.1, max_refs=32).max_refs == 32
    d2, face, closest = ops.mesh_nearest(grid, q, closest=True)
    assert tuple(d2.shape) == (7,) and d2.dtype == torch.float32 and face.dtype == torch.int32 and tuple(closest.shape) == (7, 3)
    assert len(ops.mesh_nearest(grid, q)) == 2
    for radius in (0, -1.0, float('nan'), float('inf'), 1e39):
        with pytest.raises(ValueError, match='radius'):
            ops.mesh_grid(v, f, radius)
    for refs in (31, -1, 1 << 31, 32.0, '32', True):
        with pytest.raises(ValueError, match='max_refs'):
            ops.mesh_grid(v, f, 0.1, max_refs=refs)
    with pytest.raises(ValueError, match='vertices'):
        ops.mesh_grid(_meta((5, 3), torch.float64), f, 0.1)
    with pytest.raises(ValueError, match='vertices'):
        ops.mesh_grid(_meta((5, 2), torch.float32), f, 0.1)
    with pytest.raises(ValueError, match='vertices'):
        ops.mesh_grid(np.zeros((5, 3), np.float32), f, 0.1)
    with pytest.raises(ValueError, match='faces'):
        ops.mesh_grid(v, _meta((4, 3), torch.int64), 0.1)
    with pytest.raises(ValueError, match='faces'):
        ops.mesh_grid(v, _meta((4, 4), torch.int32), 0.1)
    with pytest.raises(ValueError, match='faces on cpu, vertices on meta'):
        ops.mesh_grid(v, torch.zeros((4, 3), dtype=torch.int32), 0.1)
    with pytest.raises(ValueError, match='grid'):
        ops.mesh_nearest(None, q)
    with pytest.raises(ValueError, match='queries'):
        ops.mesh_nearest(grid, _meta((7, 3), torch.float64))
    with pytest.raises(ValueError, match='queries'):
        ops.mesh_nearest(grid, _meta((7, 4), torch.float32))
    with pytest.raises(ValueError, match='queries on cpu, the grid on meta'):
        ops.mesh_nearest(grid, torch.zeros((7, 3)))


# ------------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('name', C.NAMES)
def test_the_two_references_agree_within_the_derived_bar(name):
    c = C.case(name)
    far = 1e30                                                        # no radius: the bar is on the distances, not on who is inside
    d2 = R.nearest(c['vertices'], c['faces'], c['queries'], far)[0]
    other, extent = R.nearest_by_projection(c['vertices'], c['faces'], c['queries'], far)
    finite = np.isfinite(c['queries']).all(1)
    assert np.isfinite(d2[finite]).all() and np.isinf(d2[~finite]).all() and np.array_equal(np.isfinite(other), np.isfinite(d2))
    err = np.abs(d2[finite].astype(np.float64) - other[finite].astype(np.float64))
    bar = R.bar(d2[finite], other[finite], extent[finite])
    print('%s: %d queries, largest error / bar %.3g' % (name, int(finite.sum()), float((err / bar).max())))
    assert (err <= bar).all()
    want = C.restated(name)
    inside = want[1] >= 0
    assert np.array_equal(want[0][inside].view(np.uint32), d2[inside].view(np.uint32))           # the radius only cuts
    assert (d2[finite & ~inside].astype(np.float64) > float(np.float32(c['radius'])) ** 2).all()
    assert np.isnan(want[2][~inside]).all() and np.isfinite(want[2][inside]).all()


def test_every_region_and_both_degenerate_kinds_are_reached():
    total = np.zeros(len(R.REGIONS), np.int64)
    for name in C.NAMES:
        region = C.restated(name)[3]
        total += np.bincount(region[region >= 0], minlength=len(R.REGIONS))
    census = dict(zip(R.REGIONS, total.tolist()))
    print(census)
    assert all(census[k] >= 10 for k in R.REGIONS), census
    c = C.case('single_face')
    d2, face, _, region = C.restated('single_face')
    k = c['constructed']
    assert set(region[:k - 1].tolist()) == set(range(7))              # the constructed queries alone reach the seven regions
    assert (d2[:3] == 0.0).all() and (face[:3] == 0).all()            # on a vertex
    assert d2[k - 2] == np.float32(c['radius']) ** 2 and face[k - 2] == 0 and np.isinf(d2[k - 1]) and face[k - 1] == -1     # exactly R | beyond
    d2, face, _, region = C.restated('axis_face')
    assert (d2[:7] == 0.0).all() and region[:7].tolist() == [6, 2, 5, 4, 0, 1, 3]      # on the plane, on the edges, on the vertices
    assert d2[7] == d2[8] == np.float32(0.0625) and np.isinf(d2[9])
    d2, face, _, _ = C.restated('twice')
    assert (face[:C.case('twice')['constructed']] == 0).all() and d2[0] == np.float32(np.float64(np.float32(0.2)) ** 2)
    z = C.case('zero_area')
    region = C.restated('zero_area')[3]
    face = C.restated('zero_area')[1]
    assert set(region[face == 2].tolist()) == {8} and set(region[np.isin(face, (1, 3, 4))].tolist()) == {7} and len(z['faces']) == 5


def test_degenerate_faces_give_the_distance_to_their_point_or_segment():
    v, f = C.mesh('zero_area')
    rng = np.random.RandomState(2)
    q = rng.uniform(-1.0, 4.0, (400, 3))
    for face, (x, y) in ((1, (3, 4)), (3, (6, 8)), (2, (5, 5))):
        dd = R.closest_points(q, *(v[f[face, k]].astype(np.float64) for k in range(3)))[0]
        want = R._seg_d2(q, v[x].astype(np.float64), v[y].astype(np.float64))
        assert np.isfinite(dd).all() and np.allclose(dd, want, rtol=1e-12, atol=1e-28)


# --------------------------------------------------------------------------------------------------------------- the buffer contract
def test_every_new_entry_point_is_in_a_row_of_the_buffer_contract():
    named = set()
    for name in MR.NAMES:
        row = BR.ROWS[name]
        named.update(row.entries)
        reached = set()
        for size in row.sizes:
            reached.update(row.required(size))
        assert set(row.entries) <= reached and row.names and row.constants and row.scratch
    assert named == set(NAMES)


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


# ------------------------------------------------------------------------------------------------- eval_cloud, the driver, the tool
def test_the_exact_options_are_argument_checked_without_a_device(tmp_path, capsys):
    import inspect
    import mesh_simplify_cases as K
    from atvsnet_amd.atvsnet import eval_cloud, eval_pointcloud, mesh_distance, mesh_fusion
    from atvsnet_amd.tools import ply
    mesh, cloud = str(tmp_path / 'mesh.ply'), str(tmp_path / 'cloud.ply')
    c = K.case('single_face')
    ply.write_mesh(mesh, c['vertices'], c['colors'], c['faces'])
    ply.write_ply(cloud, c['vertices'], c['colors'])
    with pytest.raises(ValueError, match='exact_recon needs sample_recon'):
        eval_cloud.evaluate_files(mesh, [cloud], exact_recon=True)
    with pytest.raises(ValueError, match='exact_gt needs sample_gt'):
        eval_cloud.evaluate_files(cloud, [mesh], exact_gt=True)
    with pytest.raises(ValueError, match='exact_gt: every ground-truth file must be a triangle mesh, .*cloud.ply has no faces'):
        eval_cloud.evaluate_files(cloud, [mesh, cloud], sample_gt=0.1, exact_gt=True)
    with pytest.raises(ValueError, match='exact_gt with gt_mlp_path'):
        eval_cloud.evaluate_files(cloud, [], sample_gt=0.1, exact_gt=True, gt_mlp_path='x.mlp')
    for argv, message in ((['--recon', mesh, '--gt', cloud, '--exact_recon'], '--exact_recon needs --sample_recon'),
                          (['--recon', cloud, '--gt', mesh, '--exact_gt'], '--exact_gt needs --sample_gt'),
                          (['--recon', cloud, '--gt', mesh, cloud, '--sample_gt', '0.1', '--exact_gt'], 'cloud.ply has no faces'),
                          (['--recon', cloud, '--eth3d', '--gt_mlp', 'x.mlp', '--exact_gt'], '--exact_gt with --gt_mlp')):
        with pytest.raises(SystemExit) as e:
            eval_cloud.cli(argv)
        assert e.value.code == 2 and message in ' '.join(capsys.readouterr().err.split()), argv
    # make_parser declares what it declared; cli's own parser adds the two flags behind the three sample options
    shared = {s for a in eval_cloud.make_parser()._actions for s in a.option_strings}
    sampled = {s for a in eval_cloud.add_sample_arguments(eval_cloud.make_parser())._actions for s in a.option_strings}
    own = {s for a in eval_cloud.add_exact_arguments(eval_cloud.add_sample_arguments(eval_cloud.make_parser()))._actions for s in a.option_strings}
    assert own - sampled == {'--exact_recon', '--exact_gt'} and not {'--exact_recon', '--exact_gt'} & shared
    sig = inspect.signature(eval_cloud.evaluate_files).parameters
    assert sig['exact_recon'].default is False and sig['exact_gt'].default is False
    sig = inspect.signature(eval_cloud.evaluate).parameters
    assert sig['recon_surface'].default is None and sig['gt_surface'].default is None
    assert list(sig)[-2:] == ['recon_surface', 'gt_surface']                       # behind every argument there was
    v, f = eval_cloud.read_surfaces([mesh, mesh])
    assert v.dtype == np.float32 and f.dtype == np.int32 and np.array_equal(f, [[0, 1, 2], [3, 4, 5]]) and np.array_equal(v[3:], c['vertices'])
    # the driver's score dict
    assert mesh_fusion.check_score(dict(spacing=0.01, exact=True)) == (0.01, 0)
    assert mesh_fusion.check_score_exact(dict(spacing=0.01, exact=True)) is True
    assert mesh_fusion.check_score_exact(dict(spacing=0.01)) is False and mesh_fusion.check_score_exact(None) is False
    with pytest.raises(ValueError, match='mesh score: exact must be True or False'):
        mesh_fusion.check_score(dict(spacing=0.01, exact=1))
    with pytest.raises(ValueError, match='mesh score must be a dict'):
        mesh_fusion.check_score_exact(dict(spacing=0.01, exactly=True))
    eval_pointcloud._check_options(gt_ply=['gt.ply'], fuse=dict(prob_threshold=0.5), mesh=dict(voxel=0.1, score=dict(spacing=0.05, exact=True)))
    assert not {'--mesh_score', '--mesh_exact'} & {s for a in eval_pointcloud.make_parser()._actions for s in a.option_strings}
    # the tool
    assert mesh_distance.check_options(0.5) == 0.5 and mesh_distance.check_options(1, 64) == 1.0
    for radius in (0, -1.0, float('nan'), float('inf'), '1', True):
        with pytest.raises(ValueError, match='radius'):
            mesh_distance.check_options(radius)
    for refs in (-1, 1.5, True):
        with pytest.raises(ValueError, match='max_refs'):
            mesh_distance.check_options(1.0, refs)
    for argv, message in ((['--mesh', mesh, '--points', cloud, '--radius', '0'], '--radius must be a positive finite number'),
                          (['--mesh', 'nowhere.ply', '--points', cloud, '--radius', '1'], '--mesh nowhere.ply: no such file'),
                          (['--mesh', mesh, '--points', cloud], 'required')):
        with pytest.raises(SystemExit) as e:
            mesh_distance.cli(argv)
        assert e.value.code == 2 and message in ' '.join(capsys.readouterr().err.split()), argv
