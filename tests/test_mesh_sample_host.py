"""The surface sampling on the host (no GPU): the header's constants and symbols and the C entry points' refusals; the argument
errors of ops, of atvsnet/sample_mesh.py, of eval_cloud's --sample_* options and of mesh_fusion.check_score; and the numpy
restatement (tests/mesh_sample_restated.py) itself -- against a plain Python loop, for unbiased counts, for uniform samples inside
the triangle, on the cube's surface, and for the margin that makes its counts comparable with the device's."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
from atvsnet_amd import _lib, ops
from atvsnet_amd.atvsnet import eval_cloud, eval_pointcloud, mesh_fusion, sample_mesh
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buffer_contract_rows as BR  # noqa: E402
import mesh_sample_cases as C  # noqa: E402
import mesh_sample_contract_rows as MR  # noqa: E402
import mesh_sample_restated as R  # noqa: E402
import mesh_simplify_cases as K  # noqa: E402

NAMES = ('atvs_mesh_sample_counts', 'atvs_mesh_sample_scratch_size', 'atvs_mesh_sample_offsets', 'atvs_mesh_sample_place')
case = pytest.mark.parametrize('name,spacing', C.CASES, ids=C.IDS)


# ------------------------------------------------------------------------------------------------------------------------- the ABI
def test_abi_version_constants_and_symbols():
    L = _lib.lib()
    assert _lib.header_abi_version() >= 64 and L.atvs_abi_version() == _lib.header_abi_version()
    for name in NAMES:
        assert name in _lib.declared_symbols() and hasattr(L, name)
    assert ops.MESH_SAMPLE_MAX == _lib.header_macro('ATVS_MESH_SAMPLE_MAX') == R.SAMPLE_MAX == 1 << 28
    assert ops.MESH_SAMPLE_MAX <= ops.MESH_TOPOLOGY_MAX_FACES
    assert 'mesh_sample' not in _lib.OWNS_ITS_SIMD and '-ffp-contract=off' in _lib.flags_for(os.path.join(_lib.CSRC, 'mesh_sample.hip'))


def test_the_c_abi_refuses_bad_arguments_without_a_launch():
    import ctypes
    L = _lib.lib()
    buf = (ctypes.c_double * 16)()                                   # a stand-in pointer: refusals come before any launch
    ptr = ctypes.c_void_p(ctypes.addressof(buf))
    n = ctypes.c_long(0)
    counts = lambda nv=3, nf=1, density=1.0, seed=0, info=ptr, out=ptr: L.atvs_mesh_sample_counts(      # noqa: E731
        ptr, nv, ptr, nf, density, seed, out, out, info, None)
    assert counts(nv=-1) == -2 and counts(nv=(1 << 30) + 1) == -2 and counts(nf=-1) == -2 and counts(nf=(1 << 28) + 1) == -2
    assert counts(density=0.0) == -3 and counts(density=float('nan')) == -3 and counts(density=float('inf')) == -3 and counts(seed=-1) == -3
    assert counts(info=None) == -1 and counts(out=None) == -1
    assert L.atvs_mesh_sample_scratch_size(-1, ctypes.byref(n)) == -2 and L.atvs_mesh_sample_scratch_size(1, None) == -1
    assert L.atvs_mesh_sample_scratch_size((1 << 28) + 1, ctypes.byref(n)) == -2
    assert L.atvs_mesh_sample_scratch_size(5000, ctypes.byref(n)) == 0 and n.value == 256        # three tile sums, rounded up
    assert L.atvs_mesh_sample_offsets(ptr, -1, ptr, 256, ptr, None) == -2 and L.atvs_mesh_sample_offsets(ptr, 1, ptr, 255, ptr, None) == -2
    assert L.atvs_mesh_sample_offsets(None, 1, ptr, 256, ptr, None) == -1 and L.atvs_mesh_sample_offsets(ptr, 1, None, 256, ptr, None) == -1
    place = lambda nv=3, nf=1, s=1, seed=0, info=ptr, points=ptr, cout=ptr: L.atvs_mesh_sample_place(      # noqa: E731
        ptr, ptr, nv, ptr, nf, ptr, s, seed, points, ptr, cout, None, info, None)
    assert place(nv=-1) == -2 and place(nf=-1) == -2 and place(s=-1) == -2 and place(s=(1 << 28) + 1) == -2
    assert place(seed=-1) == -3 and place(info=None) == -1 and place(points=None) == -1 and place(cout=None) == -1


def test_every_new_entry_point_is_in_a_row_of_the_buffer_contract():
    named = set()
    for name in MR.NAMES:
        row = BR.ROWS[name]
        named.update(row.entries)
        reached = set()
        for size in row.sizes:
            reached.update(row.required(size))
        assert set(row.entries) <= reached and row.names and row.constants
    assert named == set(NAMES) and BR.ROWS['mesh_sample_points'].scratch


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
    v, f, c = _meta((5, 3), torch.float32), _meta((4, 3), torch.int32), _meta((5, 3), torch.uint8)
    counts, areas, info = ops.mesh_sample_counts(v, f, 10.0)
    assert tuple(counts.shape) == (4,) and counts.dtype == torch.int32 and areas.dtype == torch.float64 and info['samples'] == 0
    got, info = ops.mesh_sample(v, c, f, 10.0, normals=True)
    assert isinstance(got, ops.MeshSamples) and tuple(got.points.shape) == (0, 3) and got.colors.dtype == torch.uint8
    assert got.face.dtype == torch.int32 and tuple(got.normals.shape) == (0, 3) and info['area'] == 0.0
    assert ops.mesh_sample_points(v, None, f, _meta((4,), torch.int32)).colors is None
    for density in (0, -1.0, float('nan'), float('inf'), '1', None, True):
        with pytest.raises(ValueError, match='density'):
            ops.mesh_sample_counts(v, f, density)
    for seed in (-1, 1 << 63, 1.5, '0', True, None):
        with pytest.raises(ValueError, match='seed'):
            ops.mesh_sample_counts(v, f, 1.0, seed)
        with pytest.raises(ValueError, match='seed'):
            ops.mesh_sample_points(v, None, f, _meta((4,), torch.int32), seed)
        with pytest.raises(ValueError, match='seed'):
            ops.mesh_sample(v, None, f, 1.0, seed)
    assert ops.mesh_sample_counts(v, f, 1.0, (1 << 63) - 1)[2]['samples'] == 0
    with pytest.raises(ValueError, match='vertices'):
        ops.mesh_sample_counts(_meta((5, 3), torch.float64), f, 1.0)
    with pytest.raises(ValueError, match='vertices'):
        ops.mesh_sample_counts(_meta((5, 2), torch.float32), f, 1.0)
    with pytest.raises(ValueError, match='faces'):
        ops.mesh_sample_counts(v, _meta((4, 3), torch.int64), 1.0)
    with pytest.raises(ValueError, match='faces'):
        ops.mesh_sample(v, None, _meta((4, 4), torch.int32), 1.0)
    with pytest.raises(ValueError, match='vertices'):
        ops.mesh_sample_counts(np.zeros((5, 3), np.float32), f, 1.0)
    with pytest.raises(ValueError, match='colors'):
        ops.mesh_sample(v, _meta((5, 3), torch.float32), f, 1.0)
    with pytest.raises(ValueError, match='colors: 4 rows for 5 vertices'):
        ops.mesh_sample(v, _meta((4, 3), torch.uint8), f, 1.0)
    with pytest.raises(ValueError, match='counts'):
        ops.mesh_sample_points(v, None, f, _meta((4,), torch.int64))
    with pytest.raises(ValueError, match='counts: 3 rows for 4 faces'):
        ops.mesh_sample_points(v, None, f, _meta((3,), torch.int32))
    with pytest.raises(ValueError, match='faces on cpu, vertices on meta'):
        ops.mesh_sample_counts(v, torch.zeros((4, 3), dtype=torch.int32), 1.0)
    with pytest.raises(ValueError, match='must be contiguous'):
        ops.mesh_sample_counts(_meta((3, 5), torch.float32).t(), f, 1.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.mesh_sample_counts(torch.zeros((5, 3)), torch.zeros((4, 3), dtype=torch.int32), 1.0)


# ----------------------------------------------------------------------------------------------------------------------- the tool
def test_the_tool_checks_its_options(tmp_path, capsys):
    assert sample_mesh.check_options(spacing=0.1) == (1.0 / (0.1 * 0.1), None, 0)
    assert sample_mesh.check_options(density=4.0, seed=9) == (4.0, None, 9)
    assert sample_mesh.check_options(count=100) == (None, 100, 0)
    for kw in ({}, dict(spacing=0.1, density=1.0), dict(spacing=0.1, count=5), dict(spacing=0.1, density=1.0, count=5)):
        with pytest.raises(ValueError, match='exactly one of spacing, density and count'):
            sample_mesh.check_options(**kw)
    for kw, what in ((dict(spacing=0.0), 'spacing'), (dict(spacing=float('nan')), 'spacing'), (dict(spacing='1'), 'spacing'),
                     (dict(spacing=1e-200), 'spacing'), (dict(density=-1.0), 'density'), (dict(density=float('inf')), 'density'),
                     (dict(count=0), 'count'), (dict(count=1.5), 'count'), (dict(count=True), 'count'),
                     (dict(spacing=0.1, seed=-1), 'seed'), (dict(spacing=0.1, seed=1 << 63), 'seed'), (dict(spacing=0.1, seed=0.5), 'seed')):
        with pytest.raises(ValueError, match=what):
            sample_mesh.check_options(**kw)
    assert sample_mesh.REPORT_KEYS == ('vertices', 'faces', 'area', 'density', 'spacing', 'seed', 'samples', 'expected_samples',
                                       'skipped_index_faces', 'skipped_nonfinite_faces', 'max_per_face', 'seconds')
    mesh = str(tmp_path / 'mesh.ply')
    v, c, f = C.mesh('single_face')
    ply.write_mesh(mesh, v, c, f)
    out = str(tmp_path / 'out.ply')
    for argv, message in ((['--in', mesh, '--out', out], 'one of the arguments --spacing --density --count is required'),
                          (['--in', mesh, '--out', out, '--spacing', '0.1', '--count', '5'], 'not allowed with argument'),
                          (['--in', mesh, '--out', out, '--spacing', '-1'], 'spacing must be a positive finite number'),
                          (['--in', mesh, '--out', out, '--count', '0'], 'count must be a positive integer'),
                          (['--in', mesh, '--out', out, '--density', '1', '--seed', '-3'], 'seed must be an integer in 0..2^63-1'),
                          (['--in', mesh + '.no', '--out', out, '--density', '1'], 'no such file'),
                          (['--in', __file__, '--out', out, '--density', '1'], '--in:')):
        with pytest.raises(SystemExit) as e:
            sample_mesh.cli(argv)
        assert e.value.code == 2 and message in ' '.join(capsys.readouterr().err.split()), argv
    assert not os.path.exists(out)


# ----------------------------------------------------------------------------------------------------------------------- eval_cloud
def test_eval_cloud_refuses_sampling_options_without_their_mesh(tmp_path, capsys):
    v, c, f = C.mesh('single_face')
    mesh, cloud, quads = str(tmp_path / 'mesh.ply'), str(tmp_path / 'cloud.ply'), str(tmp_path / 'quads.ply')
    ply.write_mesh(mesh, v, c, f)
    ply.write_ply(cloud, v, c)
    with open(quads, 'w') as fh:
        fh.write('ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 1\n'
                 'property list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n')
    assert eval_cloud.mesh_faces(mesh) == 1 and eval_cloud.mesh_faces(cloud) == 0 and eval_cloud.mesh_faces(quads) == 1
    with pytest.raises(ValueError, match='not a PLY'):
        eval_cloud.mesh_faces(__file__)
    for argv, message in ((['--recon', cloud, '--gt', cloud, '--sample_seed', '3'], '--sample_seed needs --sample_recon or --sample_gt'),
                          (['--recon', mesh, '--gt', cloud, '--sample_recon', '0.1', '--sample_seed', '-1'], '--sample_seed must be in'),
                          (['--recon', cloud, '--gt', cloud, '--sample_recon', '0.1'], 'has no faces: the option needs a triangle mesh'),
                          (['--recon', mesh, '--gt', cloud, '--sample_recon', '0'], '--sample_recon must be a positive finite spacing'),
                          (['--recon', mesh, '--gt', cloud, '--sample_recon', 'nan'], '--sample_recon must be a positive finite spacing'),
                          (['--recon', mesh, '--gt', cloud, cloud, '--sample_gt', '0.1'], 'none of the --gt files has faces: the option needs a triangle mesh'),
                          (['--recon', mesh, '--gt', __file__, '--sample_gt', '0.1'], '--sample_gt:'),
                          (['--recon', mesh, '--eth3d', '--gt_mlp', 'x.mlp', '--sample_gt', '0.1'], '--sample_gt with --gt_mlp')):
        with pytest.raises(SystemExit) as e:
            eval_cloud.cli(argv)
        assert e.value.code == 2 and message in ' '.join(capsys.readouterr().err.split()), argv
    with pytest.raises(ValueError, match='sample_seed needs sample_recon or sample_gt'):
        eval_cloud.evaluate_files(cloud, [cloud], sample_seed=1)
    with pytest.raises(ValueError, match='sample_recon must be a positive finite spacing'):
        eval_cloud.evaluate_files(mesh, [cloud], sample_recon=-1.0)
    with pytest.raises(ValueError, match='sample_gt: none of the ground-truth files is a triangle mesh'):
        eval_cloud.evaluate_files(mesh, [cloud], sample_gt=0.1)
    with pytest.raises(ValueError, match='sample_gt with gt_mlp_path'):
        eval_cloud.evaluate_files(mesh, [], sample_gt=0.1, gt_mlp_path='x.mlp')
    # the parser the driver's option groups share declares what it declared; cli's own adds the three options
    shared = {s for a in eval_cloud.make_parser()._actions for s in a.option_strings}
    own = {s for a in eval_cloud.add_sample_arguments(eval_cloud.make_parser())._actions for s in a.option_strings}
    assert own - shared == {'--sample_recon', '--sample_gt', '--sample_seed'}
    import inspect
    sig = inspect.signature(eval_cloud.evaluate_files).parameters
    assert all(sig[k].default is None for k in ('sample_recon', 'sample_gt', 'sample_seed'))
    assert 'sample_recon' not in inspect.signature(eval_cloud.evaluate).parameters


# ------------------------------------------------------------------------------------------------------------------------ the driver
def test_check_score_and_the_drivers_rules():
    assert mesh_fusion.check_score(None) is None
    assert mesh_fusion.check_score(dict(spacing=0.01)) == (0.01, 0) and mesh_fusion.check_score(dict(spacing=1, seed=5)) == (1.0, 5)
    for bad in (0.01, {}, dict(seed=1), dict(spacing=0.01, density=3.0), [('spacing', 0.01)]):
        with pytest.raises(ValueError, match='mesh score must be a dict\\(spacing=S\\[, seed=K\\]\\)'):
            mesh_fusion.check_score(bad)
    for bad, what in ((dict(spacing=0), 'spacing'), (dict(spacing='x'), 'spacing'), (dict(spacing=float('inf')), 'spacing'),
                      (dict(spacing=0.01, seed=-1), 'seed'), (dict(spacing=0.01, seed=2.5), 'seed')):
        with pytest.raises(ValueError, match='mesh score: .*%s' % what):
            mesh_fusion.check_score(bad)
    with pytest.raises(ValueError, match='mesh score'):
        mesh_fusion.check_options(0.1, score=dict(spacing=-1))
    mesh_fusion.check_options(0.1, score=dict(spacing=0.05))
    fuse = dict(prob_threshold=0.5)
    plain = mesh_fusion.rules(dict(voxel=0.1, simplify=dict(cell_voxels=3)), fuse)
    assert mesh_fusion.rules(dict(voxel=0.1, simplify=dict(cell_voxels=3)), fuse, ['gt.ply']) == plain      # no row without score=
    scored = mesh_fusion.rules(dict(voxel=0.1, simplify=dict(cell_voxels=3), score=dict(spacing=0.05)), fuse, None)
    assert scored[:len(plain)] == plain and len(scored) == len(plain) + 2                    # behind the existing rows: their order stays
    assert [b for b, _ in scored[len(plain):]] == [False, True] and 'mesh score= needs gt_ply' in scored[-1][1]
    assert not any(b for b, _ in mesh_fusion.rules(dict(voxel=0.1, score=dict(spacing=0.05)), fuse, ['gt.ply']))
    options = dict(fuse=fuse, mesh=dict(voxel=0.1, score=dict(spacing=0.05)))
    with pytest.raises(ValueError, match='mesh score= needs gt_ply'):
        eval_pointcloud._check_options(**options)
    no_voxel = mesh_fusion.rules(dict(score=dict(spacing=0.05), trunc_voxels=4.0), fuse, ['gt.ply'])
    assert [b for b, _ in no_voxel[-2:]] == [True, False] and 'mesh score= needs voxel=' in no_voxel[-2][1]
    with pytest.raises(ValueError, match='need --mesh_voxel'):            # the first broken row speaks, as before
        eval_pointcloud._check_options(fuse=fuse, gt_ply=['gt.ply'], mesh=dict(score=dict(spacing=0.05), trunc_voxels=4.0))
    with pytest.raises(ValueError, match='mesh score must be a dict'):
        eval_pointcloud._check_options(gt_ply=['gt.ply'], **dict(options, mesh=dict(voxel=0.1, score=0.05)))
    eval_pointcloud._check_options(gt_ply=['gt.ply'], **options)
    assert '--mesh_score' not in {s for a in eval_pointcloud.make_parser()._actions for s in a.option_strings}


# ------------------------------------------------------------------------------------------------------------------ the restatement
MASK = (1 << 64) - 1


def _mix(z):
    z &= MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def _loop(vertices, colors, faces, density, seed):
    """The rule of include/atvsnet_hip.h as one plain loop over the faces and their samples, in Python ints and floats."""
    G = 0x9E3779B97F4A7C15
    counts, areas, points, face_of, cols = [], [], [], [], []
    for f, idx in enumerate(faces.tolist()):
        count, area = 0, 0.0
        if all(0 <= i < len(vertices) for i in idx):
            a, b, c = ([float(x) for x in vertices[i]] for i in idx)
            e1, e2 = [b[k] - a[k] for k in range(3)], [c[k] - a[k] for k in range(3)]
            n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
            L = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
            half = 0.5 * math.sqrt(L) if L == L else L
            if math.isfinite(half):
                area = half
                x = area * density
                key = _mix(seed + G * (f + 1))
                u_f = ((key >> 11) + 0.5) * 2.0 ** -53
                count = int(math.floor(x)) + (1 if u_f < x - math.floor(x) else 0)
                for j in range(count):
                    w = _mix(key + G * (j + 1))
                    u, v = ((w >> 32) + 0.5) * 2.0 ** -32, ((w & 0xffffffff) + 0.5) * 2.0 ** -32
                    if u + v > 1.0:
                        u, v = 1.0 - u, 1.0 - v
                    points.append([(a[k] + u * e1[k]) + v * e2[k] for k in range(3)])
                    face_of.append(f)
                    if colors is not None:
                        t = (1.0 - u) - v
                        cols.append([(t * float(colors[idx[0]][k]) + u * float(colors[idx[1]][k])) + v * float(colors[idx[2]][k]) for k in range(3)])
        counts.append(count)
        areas.append(area)
    return (np.array(counts), np.array(areas), np.array(points, np.float64).reshape(-1, 3).astype(np.float32), np.array(face_of, np.int32),
            np.rint(np.array(cols, np.float64).reshape(-1, 3)).astype(np.uint8))


@pytest.mark.parametrize('name', ['debris', 'debris_bad_index'])
def test_the_restatement_is_the_plain_loop_on_debris(name):
    v, c, f = C.mesh(name)
    for seed, spacing in ((0, 0.05), (7, 0.03)):
        want = _loop(v, c, f, C.density(spacing), seed)
        got = R.sample(v, c, f, C.density(spacing), seed)
        assert np.array_equal(got['counts']['counts'], want[0]) and np.array_equal(got['counts']['areas'].view(np.uint64), want[1].view(np.uint64))
        assert np.array_equal(got['samples']['points'].view(np.uint32), want[2].view(np.uint32))
        assert np.array_equal(got['samples']['face'], want[3]) and np.array_equal(got['samples']['colors'], want[4])
        assert got['counts']['info']['samples'] == len(want[2]) > 500
    assert R.counts(v, f, C.density(0.05))['info']['skipped_nonfinite_faces'] == 2
    assert int(R.mix(0)[0]) == _mix(0) == 0 and int(R.hash64(5, 11)[0]) == _mix(5 + 0x9E3779B97F4A7C15 * 12)


@case
def test_counts_are_unbiased_and_sure(name, spacing):
    c = C.restated(name, spacing)['counts']
    x = c['x']
    fr = x - np.floor(x)
    sigma = math.sqrt(float((fr * (1.0 - fr)).sum()))
    print('%s@%g: %d samples for an expected %.1f (%.2f sigma), smallest margin %.2g' % (
        name, spacing, c['info']['samples'], x.sum(), (c['info']['samples'] - x.sum()) / max(sigma, 1e-300), c['margin'].min()))
    assert abs(c['info']['samples'] - x.sum()) <= 5.0 * sigma
    assert (c['margin'] < R.SURE).sum() <= 0.01 * len(x)
    assert not c['over'] and ((c['counts'] == np.floor(x)) | (c['counts'] == np.floor(x) + 1)).all()


def test_the_plane_at_the_coarse_spacing_is_mostly_empty_faces():
    c = C.restated('plane', 0.05)['counts']
    assert len(c['counts']) == 9522 and (c['x'] < 1.0).all() and int((c['counts'] == 0).sum()) == 8667
    assert not c['counts'][:2].any() and not c['counts'][-3:].any()
    assert C.restated('debris', 0.01)['counts']['info']['max_per_face'] == 9729
    v, _, f = C.mesh('cube')
    assert R.counts(v, f, 1e-9)['info']['samples'] == 0


@pytest.mark.parametrize('seed', [0, 1, 7])
def test_samples_of_one_face_are_inside_it_and_uniform(seed):
    v, c, f = C.mesh('single_face')
    got = R.sample(v, c, f, C.density(0.01), seed)['samples']
    u, w = got['u'], got['v']
    t = (1.0 - u) - w
    N = len(u)
    assert N > 3000 and (u > 0).all() and (w > 0).all() and (t >= 0).all()
    a, b, cc = v.astype(np.float64)
    rebuilt = a + u[:, None] * (b - a) + w[:, None] * (cc - a)
    assert np.abs(rebuilt - got['points']).max() <= 1e-7                      # the barycentric point, rounded to float32
    parts = [int((t > 0.5).sum()), int((u > 0.5).sum()), int((w > 0.5).sum())]
    parts.append(N - sum(parts))                                              # the medial triangle in the middle
    print('seed %d: %d samples, medial quarters %s, each %.0f +- %.0f' % (seed, N, parts, N / 4.0, 5.0 * math.sqrt(3.0 * N / 16.0)))
    assert all(abs(p - N / 4.0) <= 5.0 * math.sqrt(3.0 * N / 16.0) for p in parts)
    assert ((got['colors'] >= c.min(0)) & (got['colors'] <= c.max(0))).all()            # a mix of the three corners' colours


def test_samples_of_the_cube_lie_on_its_surface():
    for spacing in (0.05, 0.01):
        p = C.restated('cube', spacing)['samples']['points'].astype(np.float64)
        q = p - np.asarray(K.CUBE_CORNER)
        outside = np.linalg.norm(np.maximum(0.0, np.maximum(q - K.CUBE_EDGE, -q)), axis=1)
        inside = np.minimum(np.abs(q), np.abs(K.CUBE_EDGE - q)).min(1)
        d = np.where(outside > 0.0, outside, inside)
        print('cube@%g: %d samples, farthest %.3g from the surface' % (spacing, len(p), d.max()))
        assert d.max() <= 1e-7
    n = C.restated('cube', 0.05)['samples']['normals']
    assert np.allclose(np.abs(n).max(1), 1.0) and np.allclose(np.abs(n).sum(1), 1.0)      # axis-aligned unit normals
