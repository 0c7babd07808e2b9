"""The exact distances through eval_cloud and the ETH3D driver: on the simplified cube of tests/mesh_simplify_cases.py against points
of the same cube, --sample_recon S --exact_recon gives per tolerance a completeness at least the sampled run's, per ground-truth point
a d2_gt at most the sampled run's, and the same completeness at two spacings; evaluate_files and the command line agree; --exact_gt
with the mesh as ground truth; the argument errors; register=True and init_transform move recon_surface with the points; evaluate
without the new arguments returns what it returned; run_eval_pc's mesh=dict(score=dict(spacing=, exact=True)) writes `exact` into
every mesh_eval*.json and leaves their bytes alone without it."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
from atvsnet_amd import FLAGS, ops
from atvsnet_amd.atvsnet import eval_cloud, eval_pointcloud as E, mesh_distance, sample_mesh
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_distance_restated as R  # noqa: E402
import mesh_sample_cases as SC  # noqa: E402
import mesh_sample_restated as SR  # noqa: E402
import mesh_simplify_cases as K  # noqa: E402
from test_gpu_depth_normals import _write_scene_dir  # noqa: E402

pytestmark = pytest.mark.gpu

SPACING = 0.02


@pytest.fixture(scope='module')
def cube(tmp_path_factory):
    """The simplified cube and the cube itself as mesh files, 15,000 samples of the cube's surface (seed 7) as the ground-truth cloud."""
    folder = tmp_path_factory.mktemp('mesh_distance')
    simple, whole, gt = (str(folder / name) for name in ('simple.ply', 'cube.ply', 'gt.ply'))
    ply.write_mesh(simple, *K.restated('cube')['out'])
    hv, hc, hf = SC.mesh('cube')
    ply.write_mesh(whole, hv, hc, hf)
    truth = SR.sample(hv, hc, hf, 2500.0, 7)['samples']
    ply.write_ply(gt, truth['points'], truth['colors'])
    assert 14000 < len(truth['points']) < 16000
    return dict(simple=simple, whole=whole, gt=gt, truth=truth['points'])


def _complete(result):
    return [t['completeness'] for t in result['tolerances']]


def test_exact_recon_removes_the_spacing_from_completeness(cuda, cube, tmp_path, capsys):
    torch.cuda.set_device(cuda)
    by_samples, by_surface, coarser = {}, {}, {}
    sampled = eval_cloud.evaluate_files(cube['simple'], [cube['gt']], sample_recon=SPACING, distances=by_samples)
    exact = eval_cloud.evaluate_files(cube['simple'], [cube['gt']], sample_recon=SPACING, exact_recon=True, distances=by_surface)
    other = eval_cloud.evaluate_files(cube['simple'], [cube['gt']], sample_recon=1.5 * SPACING, exact_recon=True, distances=coarser)
    print('completeness by samples at %g: %s; by the surface: %s' % (SPACING, _complete(sampled), _complete(exact)))
    assert 'exact' not in sampled
    faces = len(K.restated('cube')['out'][2])
    assert exact['exact'] == {'accuracy': False, 'completeness': True, 'gt_surface_faces': None, 'recon_surface_faces': faces}
    assert all(e >= s for e, s in zip(_complete(exact), _complete(sampled))) and _complete(sampled)[0] < _complete(exact)[0]
    assert (by_surface['d2_gt'] <= by_samples['d2_gt']).all()
    assert _complete(exact)[0] == 1.0                                 # the simplified cube IS the cube's surface (within 5e-8)
    # accuracy and everything of the reconstruction's direction is the samples', untouched
    for key in ('n_recon', 'n_gt', 'not_found_recon', 'mean_recon', 'median_recon', 'recon_mesh'):
        assert exact[key] == sampled[key], key
    assert [t['accuracy'] for t in exact['tolerances']] == [t['accuracy'] for t in sampled['tolerances']]
    assert np.array_equal(by_surface['d2_recon'], by_samples['d2_recon']) and np.array_equal(by_surface['idx_recon'], by_samples['idx_recon'])
    # the other spacing: other samples, another accuracy, the SAME completeness down to every distance
    assert other['n_recon'] != exact['n_recon'] and _complete(other) == _complete(exact)
    assert np.array_equal(coarser['d2_gt'].view(np.uint32), by_surface['d2_gt'].view(np.uint32))
    assert np.array_equal(coarser['idx_gt'], by_surface['idx_gt']) and by_surface['idx_gt'].min() >= 0 and by_surface['idx_gt'].max() < faces
    for key in ('not_found_gt', 'mean_gt', 'median_gt'):
        assert other[key] == exact[key], key
    # the distances are the restatement's
    v, _, f = K.restated('cube')['out']
    want = R.nearest(v, f, cube['truth'], exact['radius'])
    assert np.array_equal(want[0].view(np.uint32), by_surface['d2_gt'].view(np.uint32)) and np.array_equal(want[1], by_surface['idx_gt'])
    # the command line writes the same result
    out = str(tmp_path / 'eval.json')
    capsys.readouterr()
    result = eval_cloud.cli(['--recon', cube['simple'], '--gt', cube['gt'], '--sample_recon', repr(SPACING), '--exact_recon', '--out', out])
    with open(out) as fh:
        written = json.load(fh)
    assert written == json.loads(json.dumps(result)) == json.loads(json.dumps(exact))


def test_exact_gt_scores_accuracy_against_the_ground_truth_surface(cuda, cube, tmp_path, capsys):
    torch.cuda.set_device(cuda)
    d = {}
    both = eval_cloud.evaluate_files(cube['simple'], [cube['whole']], sample_recon=SPACING, sample_gt=SPACING, exact_recon=True,
                                     exact_gt=True, distances=d)
    sampled = eval_cloud.evaluate_files(cube['simple'], [cube['whole']], sample_recon=SPACING, sample_gt=SPACING)
    assert both['exact'] == {'accuracy': True, 'completeness': True, 'gt_surface_faces': len(SC.mesh('cube')[2]),
                             'recon_surface_faces': len(K.restated('cube')['out'][2])}
    assert both['n_recon'] == sampled['n_recon'] and both['n_gt'] == sampled['n_gt'] and both['gt_mesh'] == sampled['gt_mesh']
    for t, s in zip(both['tolerances'], sampled['tolerances']):
        assert t['accuracy'] == t['completeness'] == 1.0 and t['accuracy'] >= s['accuracy'] and t['completeness'] >= s['completeness']
    assert sampled['tolerances'][0]['accuracy'] < 1.0                # at 0.01 the samples of a surface at spacing 0.02 miss
    assert float(d['d2_recon'].max()) < 1e-12 and float(d['d2_gt'].max()) < 1e-12
    # two ground-truth meshes are concatenated with offset indices: the second copy's faces come behind the first's
    twice = {}
    eval_cloud.evaluate_files(cube['gt'], [cube['whole'], cube['whole']], sample_gt=SPACING, exact_gt=True, distances=twice)
    single = {}
    one = eval_cloud.evaluate_files(cube['gt'], [cube['whole']], sample_gt=SPACING, exact_gt=True, distances=single)
    assert np.array_equal(twice['d2_recon'], single['d2_recon']) and np.array_equal(twice['idx_recon'], single['idx_recon'])
    assert one['exact']['accuracy'] and not one['exact']['completeness'] and one['n_recon'] == len(cube['truth'])
    capsys.readouterr()
    result = eval_cloud.cli(['--recon', cube['gt'], '--gt', cube['whole'], '--sample_gt', repr(SPACING), '--exact_gt'])
    assert json.loads(json.dumps(result)) == json.loads(json.dumps(one))


def test_the_argument_errors(cuda, cube, tmp_path, capsys):
    torch.cuda.set_device(cuda)
    with pytest.raises(ValueError, match='exact_recon needs sample_recon'):
        eval_cloud.evaluate_files(cube['simple'], [cube['gt']], exact_recon=True)
    with pytest.raises(ValueError, match='exact_gt needs sample_gt'):
        eval_cloud.evaluate_files(cube['simple'], [cube['whole']], exact_gt=True)
    with pytest.raises(ValueError, match='exact_gt: every ground-truth file must be a triangle mesh, .*gt.ply has no faces'):
        eval_cloud.evaluate_files(cube['simple'], [cube['whole'], cube['gt']], sample_gt=SPACING, exact_gt=True)
    with pytest.raises(ValueError, match='exact_gt with gt_mlp_path'):
        eval_cloud.evaluate_files(cube['simple'], [], exact_gt=True, gt_mlp_path='x.mlp')
    with pytest.raises(ValueError, match='recon_surface: expected'):
        eval_cloud.evaluate(cube['truth'], cube['truth'], recon_surface=cube['truth'])
    with pytest.raises(ValueError, match='gt_surface: faces: expected shape'):
        eval_cloud.evaluate(cube['truth'], cube['truth'], gt_surface=(cube['truth'], np.zeros((4, 4), np.int32)))
    base = ['--recon', cube['simple']]
    for argv, message in ((base + ['--gt', cube['gt'], '--exact_recon'], '--exact_recon needs --sample_recon'),
                          (base + ['--gt', cube['whole'], '--exact_gt'], '--exact_gt needs --sample_gt'),
                          (base + ['--gt', cube['whole'], cube['gt'], '--sample_gt', '0.02', '--exact_gt'], 'gt.ply has no faces'),
                          (base + ['--eth3d', '--gt_mlp', 'x.mlp', '--exact_gt'], '--exact_gt with --gt_mlp')):
        with pytest.raises(SystemExit) as e:
            eval_cloud.cli(argv)
        assert e.value.code == 2 and message in ' '.join(capsys.readouterr().err.split()), argv


def test_the_surface_moves_with_the_points(cuda, cube):
    torch.cuda.set_device(cuda)
    v, _, f = K.restated('cube')['out']
    samples = SR.sample(v, None, f, 1.0 / SPACING ** 2, 0)['samples']['points']
    angle = 0.02
    T = np.array([[np.cos(angle), -np.sin(angle), 0.0, 0.03], [np.sin(angle), np.cos(angle), 0.0, -0.02], [0.0, 0.0, 1.0, 0.025],
                  [0.0, 0.0, 0.0, 1.0]])
    back = np.linalg.inv(T)
    moved_points, moved_vertices = eval_cloud.transform_points(samples, back), eval_cloud.transform_points(v, back)
    straight, d_straight = {}, {}
    want = eval_cloud.evaluate(samples, cube['truth'], recon_surface=(v, f), distances=straight)
    assert _complete(want)[0] == 1.0
    # left where it is, the surface is off by up to 0.04: completeness at 0.01 collapses
    off = eval_cloud.evaluate(moved_points, cube['truth'], recon_surface=(moved_vertices, f))
    assert _complete(off)[0] < 0.5
    # init_transform moves both: the distances return to within the float32 rounding of a vertex moved there and back (3 roundings of
    # 2^-24 on coordinates of about 1, on distances of about 5e-8 themselves: everything stays far below the smallest tolerance)
    init = eval_cloud.evaluate(moved_points, cube['truth'], init_transform=T, recon_surface=(moved_vertices, f), distances=d_straight)
    assert _complete(init) == _complete(want) and init['exact'] == want['exact'] and float(d_straight['d2_gt'].max()) < (1e-6) ** 2
    # and so does the registration's matrix, through device tensors as well as host arrays: the registration is the one the points
    # alone get, and the ground truth's distances are those to the surface moved by ITS matrix
    dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to(cuda).to(t)      # noqa: E731
    plain = eval_cloud.evaluate(moved_points, cube['truth'], register=True, init_transform=np.eye(4))
    d = {}
    registered = eval_cloud.evaluate(moved_points, cube['truth'], register=True, init_transform=np.eye(4), distances=d,
                                     recon_surface=(dev(moved_vertices, torch.float32), dev(f, torch.int32)))
    assert registered['registration'] == plain['registration'] and registered['exact']['completeness']
    matrix = np.asarray(registered['registration']['matrix'])
    there = ops.cloud_transform(dev(moved_vertices, torch.float32), matrix)
    d2, face = ops.mesh_nearest(ops.mesh_grid(there, dev(f, torch.int32), registered['radius']), dev(cube['truth'], torch.float32))
    assert np.array_equal(d['d2_gt'].view(np.uint32), d2.cpu().numpy().view(np.uint32)) and np.array_equal(d['idx_gt'], face.cpu().numpy())
    print('registered: |matrix - T| <= %.2g, completeness %s (points alone: %s)' % (np.abs(matrix - T).max(), _complete(registered),
                                                                                 _complete(plain)))
    assert all(e >= s for e, s in zip(_complete(registered), _complete(plain)))     # the moved surface holds the moved samples


def test_evaluate_without_the_new_arguments_returns_what_it_returned(cuda, cube):
    torch.cuda.set_device(cuda)
    v, _, f = K.restated('cube')['out']
    recon = SR.sample(v, None, f, 1.0 / SPACING ** 2, 0)['samples']['points']
    d = {}
    before = ops.launches()
    got = eval_cloud.evaluate(recon, cube['truth'], distances=d)
    inside = ops.launches() - before
    tol, radius = eval_cloud._check_tolerances(eval_cloud.DEFAULT_TOLERANCES, None)
    r, g = torch.from_numpy(recon).to(cuda), torch.from_numpy(cube['truth']).to(cuda)
    before = ops.launches()
    d2_r, idx_r = ops.cloud_nearest(ops.cloud_grid(g, radius), r)
    d2_g, idx_g = ops.cloud_nearest(ops.cloud_grid(r, radius), g)
    counts = [ops.cloud_counts(x, tol, radius).cpu().tolist() for x in (d2_r, d2_g)]
    assert inside == ops.launches() - before == 6                     # two grids, two searches, two counts: the calls it made before
    assert got == eval_cloud.metrics(d2_r.cpu().numpy(), d2_g.cpu().numpy(), tol, radius, counts=counts)
    assert sorted(got) == ['mean_gt', 'mean_recon', 'median_gt', 'median_recon', 'n_gt', 'n_recon', 'not_found_gt', 'not_found_recon',
                           'radius', 'tolerances']
    assert sorted(d) == ['d2_gt', 'd2_recon', 'idx_gt', 'idx_recon'] and np.array_equal(d['idx_gt'], idx_g.cpu().numpy())


def test_the_tool_reports_the_distances(cuda, cube, tmp_path, capsys):
    out, closest, report_path = (str(tmp_path / 'tool' / name) for name in ('d.npy', 'closest.ply', 'report.json'))
    report = mesh_distance.cli(['--mesh', cube['simple'], '--points', cube['gt'], '--radius', '0.05', '--out', out, '--closest', closest,
                                '--report', report_path])
    v, _, f = K.restated('cube')['out']
    want = R.nearest(v, f, cube['truth'], 0.05, closest=True)
    d = np.load(out)
    assert d.dtype == np.float32 and np.array_equal(d, np.sqrt(want[0].astype(np.float64)).astype(np.float32))
    assert np.array_equal(ply.read_ply_points(closest).view(np.uint32), want[2][want[1] >= 0].view(np.uint32))
    with open(report_path) as fh:
        assert json.load(fh) == json.loads(json.dumps(report))
    assert set(report) == set(mesh_distance.REPORT_KEYS) and report['points'] == report['found'] == len(cube['truth'])
    found = np.sqrt(want[0].astype(np.float64))
    assert report['mean'] == float(found.mean()) and report['median'] == float(np.median(found)) and report['max'] == float(found.max())
    assert report['faces'] == report['usable_faces'] == len(f) and report['references'] > 0 and report['cell'] >= 0.05
    for argv, message in ((['--mesh', cube['simple'], '--points', cube['gt'], '--radius', '0'], '--radius must be a positive finite number'),
                          (['--mesh', 'nowhere.ply', '--points', cube['gt'], '--radius', '1'], 'no such file')):
        with pytest.raises(SystemExit) as e:
            mesh_distance.cli(argv)
        assert e.value.code == 2 and message in ' '.join(capsys.readouterr().err.split()), argv


# --------------------------------------------------------------------------------------------------------------------- the driver
def _drive(argv, gt_ply=None, **mesh):
    """eval_pointcloud.cli's own steps with entries added to the mesh dict: the command line has no option for them."""
    parser = E.make_parser()
    args = parser.parse_args(argv)
    args.gt_ply = args.clean = None
    options = E._run_options(args, parser)
    options['mesh'] = dict(options['mesh'], **mesh)
    options['gt_ply'] = gt_ply
    E._check_options(**options)
    for k, v in vars(args).items():
        if k not in ('scenes', 'maps_in_flight'):
            setattr(FLAGS, k, v)
    E.main(args.scenes.split(','), options=options)


def _read(path):
    with open(path, 'rb') as fh:
        return fh.read()


def test_driver_writes_exact_completeness_into_every_mesh_eval(cuda, tmp_path, weights):
    root = str(tmp_path)
    _write_scene_dir(root)
    base = ['--data_root', root, '--view_num', '3', '--max_d', '16', '--max_w', '160', '--max_h', '128', '--synthetic_weights',
            '--scenes', 'toy', '--fuse', '--no_map_files', '--prob_threshold', '0.5', '--disp_threshold', '0.5', '--num_consistent', '1',
            '--mesh_voxel', '0.05', '--mesh_min_weight', '1']
    first, plain, exact = (os.path.join(root, name) for name in ('out_first', 'out_plain', 'out_exact'))
    simplify = dict(cell_voxels=3)
    try:
        FLAGS.reset()
        _drive(base + ['--savepath', first], simplify=simplify, score=None)
        gt = os.path.join(first, 'toy', 'final3d_model.ply')
        FLAGS.reset()
        _drive(base + ['--savepath', plain], [gt], simplify=simplify, score=dict(spacing=0.02))
        FLAGS.reset()
        _drive(base + ['--savepath', exact], [gt], simplify=simplify, score=dict(spacing=0.02, exact=True))
    finally:
        FLAGS.reset()
        E._Pipelines.CO_RESIDENT = False
    assert sorted(os.listdir(os.path.join(plain, 'toy'))) == sorted(os.listdir(os.path.join(exact, 'toy')))
    gt_points = ply.read_ply_points(gt)
    torch.cuda.set_device(cuda)
    for name, mesh in (('mesh_eval.json', 'final3d_mesh.ply'), ('mesh_eval_simple.json', 'final3d_mesh_simple.ply')):
        with open(os.path.join(plain, 'toy', name)) as fh:
            a = json.load(fh)
        with open(os.path.join(exact, 'toy', name)) as fh:
            b = json.load(fh)
        assert _read(os.path.join(plain, 'toy', mesh)) == _read(os.path.join(exact, 'toy', mesh))
        v, _, f = ply.read_mesh(os.path.join(exact, 'toy', mesh))
        assert 'exact' not in a and b['exact'] == {'accuracy': False, 'completeness': True, 'gt_surface_faces': None,
                                                   'recon_surface_faces': int(R.usable_faces(v, f).sum())}
        # without the key the file is what the samples alone give, as it was: the whole dict of evaluate on the written mesh's samples
        samples = sample_mesh.sample_device(torch.from_numpy(v).to(cuda), None, torch.from_numpy(f).to(cuda), spacing=0.02, seed=0)[0].points
        again = eval_cloud.evaluate(samples, gt_points)
        assert {k: x for k, x in a.items() if k != 'recon_mesh'} == json.loads(json.dumps(again))
        # with it: the reconstruction's direction is the samples', completeness is at least theirs, and is the surface's own
        assert a['recon_mesh'] == b['recon_mesh'] and all(a[k] == b[k] for k in ('n_recon', 'n_gt', 'mean_recon', 'median_recon'))
        d = {}
        direct = eval_cloud.evaluate(samples, gt_points, recon_surface=(v, f), distances=d)
        assert {k: x for k, x in b.items() if k != 'recon_mesh'} == json.loads(json.dumps(direct))
        for ta, tb in zip(a['tolerances'], b['tolerances']):
            assert tb['accuracy'] == ta['accuracy'] and tb['completeness'] >= ta['completeness']
        print('%s: completeness %s by samples, %s by the surface' % (name, _complete(a), _complete(b)))
