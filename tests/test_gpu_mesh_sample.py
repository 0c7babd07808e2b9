"""The surface-sampling kernels (csrc/mesh_sample.hip) against their numpy restatement on every case of tests/mesh_sample_cases.py,
every op twice with the same bits both times: the counts on the faces whose rounding is sure, the areas to one unit in the last
place, the info words; the placement, handed the restatement's counts, bit for bit (normals to a float32 spacing); the whole
mesh_sample; the empty shapes, the limit errors and the total they report, another seed; eval_cloud's --sample_recon on the
simplified cube, through evaluate_files and through the command line."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
from atvsnet_amd import ops
from atvsnet_amd.atvsnet import eval_cloud, sample_mesh
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_sample_cases as C  # noqa: E402
import mesh_sample_restated as R  # noqa: E402
import mesh_simplify_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu

case = pytest.mark.parametrize('name,spacing', C.CASES, ids=C.IDS)


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def _same(got, want, what):
    if want is None:
        assert got is None, what
        return
    g = got.cpu().numpy()
    assert g.shape == want.shape and g.dtype == want.dtype, (what, g.dtype, want.dtype, g.shape, want.shape)
    ne = np.nonzero(_bits(g).reshape(-1) != _bits(want).reshape(-1))[0]
    assert len(ne) == 0, '%s: %d of %d elements differ, first at %d: %r against %r' % (
        what, len(ne), g.size, ne[0], g.reshape(-1)[ne[0]], want.reshape(-1)[ne[0]])


def _mesh_on(name, dev):
    v, c, f = C.mesh(name)
    return _dev(v, dev), _dev(c, dev), _dev(f, dev)


def _all_sure(want):
    return bool((want['counts']['margin'] >= R.SURE).all())


@case
def test_counts_are_the_restatement_on_the_sure_faces_twice(cuda, name, spacing):
    v, _, f = _mesh_on(name, cuda)
    want = C.restated(name, spacing)['counts']
    sure = want['margin'] >= R.SURE
    assert (~sure).sum() <= 0.01 * len(sure)
    first = None
    for _ in range(2):
        counts, areas, info = ops.mesh_sample_counts(v, f, C.density(spacing), C.SEED)
        c, a = counts.cpu().numpy(), areas.cpu().numpy()
        assert c.dtype == np.int32 and a.dtype == np.float64 and c.shape == a.shape == (len(sure),)
        assert np.array_equal(c[sure], want['counts'][sure])
        ulp = np.abs(a - want['areas']) / np.spacing(want['areas'])
        print('%s@%g: %d faces, %d unsure, areas differ by at most %.0f ulp, info %s' % (name, spacing, len(sure), int((~sure).sum()),
                                                                                       ulp.max(initial=0.0), info))
        assert (ulp <= 1.0).all()
        assert not sure.all() or info == want['info']
        assert info['samples'] == int(c.sum()) and info['max_per_face'] == int(c.max(initial=0))
        if first is not None:
            assert np.array_equal(c, first[0]) and np.array_equal(_bits(a), _bits(first[1])) and info == first[2]
        first = (c, a, info)


@case
def test_placement_of_the_restatements_counts_is_the_restatement_twice(cuda, name, spacing):
    v, col, f = _mesh_on(name, cuda)
    r = C.restated(name, spacing)
    want = r['samples']
    counts = _dev(r['counts']['counts'].astype(np.int32), cuda)
    first = None
    for _ in range(2):
        got = ops.mesh_sample_points(v, col, f, counts, C.SEED, normals=True)
        _same(got.points, want['points'], 'points')
        _same(got.face, want['face'], 'sample_face')
        _same(got.colors, want['colors'], 'colors')
        n, wn = got.normals.cpu().numpy(), want['normals']
        assert n.dtype == np.float32 and n.shape == wn.shape
        assert (np.abs(n.astype(np.float64) - wn.astype(np.float64)) <= np.spacing(np.abs(wn)).astype(np.float64)).all()
        if first is not None:
            _same(got.normals, first, 'normals of the second run')
        first = n
    plain = ops.mesh_sample_points(v, None, f, counts, C.SEED)
    assert plain.colors is None and plain.normals is None
    _same(plain.points, want['points'], 'points without colours and normals')


@case
def test_mesh_sample_is_the_restatement_where_every_face_is_sure(cuda, name, spacing):
    v, col, f = _mesh_on(name, cuda)
    r = C.restated(name, spacing)
    assert _all_sure(r)                  # every case of the list, as measured on the restatement
    for _ in range(2):
        got, info = ops.mesh_sample(v, col, f, C.density(spacing), C.SEED)
        _same(got.points, r['samples']['points'], 'points')
        _same(got.face, r['samples']['face'], 'sample_face')
        _same(got.colors, r['samples']['colors'], 'colors')
        assert got.normals is None
        assert {k: info[k] for k in R.INFO} == r['counts']['info']
        assert abs(info['area'] - r['area']) <= 1e-12 * r['area']


def test_empty_shapes_launch_nothing_that_could_misbehave(cuda):
    v, col, f = _mesh_on('cube', cuda)
    none = torch.zeros((0, 3), dtype=torch.int32, device=cuda)
    counts, areas, info = ops.mesh_sample_counts(v, none, 100.0)
    assert tuple(counts.shape) == (0,) and tuple(areas.shape) == (0,) and info == dict.fromkeys(R.INFO, 0)
    for faces, density in ((none, 100.0), (f, 1e-9)):                  # no face; a density so small that the total is 0
        got, info = ops.mesh_sample(v, col, faces, density, normals=True)
        torch.cuda.synchronize()
        assert info['samples'] == 0 and info['max_per_face'] == 0
        assert tuple(got.points.shape) == (0, 3) and tuple(got.colors.shape) == (0, 3) and tuple(got.normals.shape) == (0, 3)
        assert tuple(got.face.shape) == (0,) and got.face.dtype == torch.int32
    want = R.counts(*[C.mesh('cube')[k] for k in (0, 2)], 1e-9)
    assert want['info']['samples'] == 0 and abs(info['area'] - 6.0) < 1e-6
    got = ops.mesh_sample_points(v, None, f, torch.zeros(len(f), dtype=torch.int32, device=cuda))
    assert tuple(got.points.shape) == (0, 3)
    empty = torch.zeros((0, 3), dtype=torch.float32, device=cuda)
    got, info = ops.mesh_sample(empty, None, none, 1.0)
    assert tuple(got.points.shape) == (0, 3) and info['area'] == 0.0


def test_the_limits_raise_with_the_total_needed(cuda):
    v, _, f = _mesh_on('big_triangles', cuda)
    hv, _, hf = C.mesh('big_triangles')
    for density in (3.0e6, 1.0e7, 1.0e300):          # a total above the limit with every face below it; one face above it; x = inf
        want = R.counts(hv, hf, density)
        assert want['over']
        with pytest.raises(ValueError, match='needs %d samples \\(%d on one face\\)' % (want['info']['samples'], want['info']['max_per_face'])):
            ops.mesh_sample_counts(v, f, density)
        with pytest.raises(ValueError, match='needs %d samples' % want['info']['samples']):
            ops.mesh_sample(v, None, f, density)
    assert R.counts(hv, hf, 3.0e6)['info']['max_per_face'] < R.SAMPLE_MAX <= R.counts(hv, hf, 1.0e7)['info']['max_per_face']
    counts = torch.tensor([1 << 28, 1], dtype=torch.int32, device=cuda)
    with pytest.raises(ValueError, match='needs %d samples' % ((1 << 28) + 1)):
        ops.mesh_sample_points(v, None, f, counts)
    with pytest.raises(ValueError, match='negative'):
        ops.mesh_sample_points(v, None, f, torch.tensor([1, -1], dtype=torch.int32, device=cuda))
    # samples asked for on a face whose index is out of range: the lanes write zeros and say so
    bv, _, bf = _mesh_on('debris_bad_index', cuda)
    counts = torch.zeros(len(bf), dtype=torch.int32, device=cuda)
    counts[5] = 300
    with pytest.raises(ValueError, match='300 of 300 samples lie on faces with a vertex index outside 0..14'):
        ops.mesh_sample_points(bv, None, bf, counts)


def test_another_seed_moves_the_points_and_keeps_the_expectation(cuda):
    v, col, f = _mesh_on('sphere', cuda)
    hv, hc, hf = C.mesh('sphere')
    base = C.restated('sphere', 0.01)
    want = R.sample(hv, hc, hf, C.density(0.01), 7)
    got, info = ops.mesh_sample(v, col, f, C.density(0.01), 7)
    assert (want['counts']['margin'] >= R.SURE).all()
    _same(got.points, want['samples']['points'], 'points at seed 7')
    assert not np.array_equal(want['counts']['counts'], base['counts']['counts'])
    x = base['counts']['x']
    fr = x - np.floor(x)
    assert abs(info['samples'] - x.sum()) <= 5.0 * np.sqrt((fr * (1.0 - fr)).sum())
    top = (1 << 63) - 1
    got, _ = ops.mesh_sample(v, col, f, C.density(0.05), top)
    _same(got.points, R.sample(hv, hc, hf, C.density(0.05), top)['samples']['points'], 'points at the largest seed')


# --------------------------------------------------------------------------------------------------------------------- eval_cloud
@pytest.fixture(scope='module')
def simplified_cube(tmp_path_factory):
    """The simplified cube as a mesh file, the unsimplified cube's own samples (spacing 0.004, seed 7) as the ground truth."""
    folder = tmp_path_factory.mktemp('mesh_sample')
    mesh, gt = str(folder / 'simple.ply'), str(folder / 'gt.ply')
    v, c, f = K.restated('cube')['out']
    ply.write_mesh(mesh, v, c, f)
    hv, hc, hf = C.mesh('cube')
    truth = R.sample(hv, hc, hf, C.density(0.004), 7)['samples']
    ply.write_ply(gt, truth['points'], truth['colors'])
    want = R.sample(v, c, f, C.density(0.01), 0)
    assert (want['counts']['margin'] >= R.SURE).all() and len(truth['points']) > 370000
    return mesh, gt, truth['points'], want


def _at(result, tolerance):
    return [t for t in result['tolerances'] if t['tolerance'] == tolerance][0]


def test_a_simplified_mesh_scores_by_its_surface_with_sample_recon(cuda, simplified_cube, tmp_path, capsys):
    mesh, gt, truth, want = simplified_cube
    torch.cuda.set_device(cuda)
    by_vertices = eval_cloud.evaluate_files(mesh, [gt])
    assert 'recon_mesh' not in by_vertices and by_vertices['n_recon'] == len(K.restated('cube')['out'][0])
    print('the simplified cube by its %d vertices: completeness %.3f at 0.02' % (by_vertices['n_recon'], _at(by_vertices, 0.02)['completeness']))
    assert _at(by_vertices, 0.02)['completeness'] <= 0.05
    first = None
    for _ in range(2):
        sampled = eval_cloud.evaluate_files(mesh, [gt], sample_recon=0.01)
        assert _at(sampled, 0.02)['completeness'] >= 0.99 and _at(sampled, 0.02)['accuracy'] == 1.0
        assert first is None or sampled == first
        first = sampled
    print('by %d samples of its surface: completeness %.3f at 0.01, %.3f at 0.02' % (
        sampled['n_recon'], _at(sampled, 0.01)['completeness'], _at(sampled, 0.02)['completeness']))
    report = sampled.pop('recon_mesh')
    assert sampled == eval_cloud.evaluate(want['samples']['points'], truth)               # the whole result, of the restatement's samples
    assert set(report) == set(sample_mesh.REPORT_KEYS) - {'seconds'}
    assert report['samples'] == sampled['n_recon'] == len(want['samples']['points']) and report['seed'] == 0
    assert report['density'] == C.density(0.01) and abs(report['spacing'] - 0.01) < 1e-15 and abs(report['area'] - want['area']) < 1e-9
    assert abs(report['expected_samples'] - report['area'] * report['density']) < 1e-6 and report['faces'] == len(K.restated('cube')['out'][2])
    other = eval_cloud.evaluate_files(mesh, [gt], sample_recon=0.01, sample_seed=7)
    assert other['recon_mesh']['seed'] == 7 and other['n_recon'] != sampled['n_recon'] and _at(other, 0.02)['completeness'] >= 0.99
    # point-to-plane registration over the source's normals: the samples' face normals serve, the file carries none
    moved = eval_cloud.evaluate_files(mesh, [gt], sample_recon=0.01, register=True, register_icp='plane')
    matrix = np.asarray(moved['registration']['matrix'])
    print('registered by the samples\' face normals: |matrix - I| <= %.2g' % np.abs(matrix - np.eye(4)).max())
    assert moved['recon_mesh'] == report and np.abs(matrix - np.eye(4)).max() < 2e-3 and _at(moved, 0.02)['completeness'] >= 0.99
    # the ground truth as a surface: the unsimplified cube's mesh file beside the cloud
    whole = str(tmp_path / 'cube.ply')
    ply.write_mesh(whole, *C.mesh('cube'))
    both = eval_cloud.evaluate_files(mesh, [whole, gt], sample_recon=0.01, sample_gt=0.01)
    assert [m['file'] for m in both['gt_mesh']] == [whole] and both['n_gt'] == len(truth) + both['gt_mesh'][0]['samples']
    assert both['gt_mesh'][0]['samples'] == C.restated('cube', 0.01)['counts']['info']['samples']
    # the command line writes the same result
    out = str(tmp_path / 'eval.json')
    capsys.readouterr()
    result = eval_cloud.cli(['--recon', mesh, '--gt', gt, '--sample_recon', '0.01', '--out', out])
    with open(out) as f:
        written = json.load(f)
    assert written == json.loads(json.dumps(result)) and written['recon_mesh'] == report
    assert {k: v for k, v in written.items() if k != 'recon_mesh'} == json.loads(json.dumps(sampled))


def test_the_tool_writes_the_restatements_samples(cuda, simplified_cube, tmp_path, capsys):
    mesh, _, _, want = simplified_cube
    out, report_path = str(tmp_path / 'tool' / 'samples.ply'), str(tmp_path / 'tool' / 'samples.json')
    report = sample_mesh.cli(['--in', mesh, '--out', out, '--spacing', '0.01', '--normals', '--report', report_path])
    points, colors, normals = ply.read_ply_normals(out)
    assert np.array_equal(_bits(points), _bits(want['samples']['points'])) and np.array_equal(colors, want['samples']['colors'])
    assert normals.shape == points.shape and np.abs(np.linalg.norm(normals.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    with open(report_path) as f:
        assert json.load(f) == json.loads(json.dumps(report))
    assert set(report) == set(sample_mesh.REPORT_KEYS) and report['samples'] == len(points) and {'sample', 'upload', 'download'} <= set(report['seconds'])
    counted = sample_mesh.cli(['--in', mesh, '--out', out, '--count', '20000', '--seed', '3', '--report', report_path])
    assert abs(counted['expected_samples'] - 20000.0) < 1e-6 and abs(counted['samples'] - 20000) <= 5 * np.sqrt(20000.0)
    assert counted['seed'] == 3 and 'area' in counted['seconds'] and len(ply.read_ply(out)[0]) == counted['samples']
    plain, grey = str(tmp_path / 'plain.ply'), str(tmp_path / 'grey.ply')              # a third-party mesh without colours: grey samples
    v, _, f = C.mesh('single_face')
    with open(plain, 'w') as fh:
        fh.write('ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nelement face 1\n'
                 'property list uchar int vertex_indices\nend_header\n%s\n3 0 1 2\n' % '\n'.join(' '.join(repr(float(x)) for x in r) for r in v))
    sample_mesh.cli(['--in', plain, '--out', grey, '--spacing', '0.01', '--report', report_path])
    got = ply.read_ply(grey)
    assert np.array_equal(_bits(got[0]), _bits(C.restated('single_face', 0.01)['samples']['points'])) and (got[1] == sample_mesh.GREY).all()
