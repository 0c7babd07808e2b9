"""Without a GPU: the host side of the consistency mask and the per-pixel view weights -- the ABI, the
argument checks of ops.fusion_support and ops.tsdf_integrate(weights=) on `meta` tensors, the option rules and parsers -- and what
the restatement (tests/tsdf_weighted_restated.py) alone shows on the floater and the biased ring: the mask removes the blob at its
cause, all-ones weights are the unweighted bits, a weight of 0 is a masked depth, and a down-weighted biased view moves the surface
less."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import tsdf_carve_restated as CR
import tsdf_weighted_restated as WR
from atvsnet_amd import _lib, ops
from atvsnet_amd.atvsnet import eval_pointcloud as E
from atvsnet_amd.atvsnet import mesh_consistent, mesh_fusion


def _meta(shape, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device='meta')


def _bits_equal(a, b):
    for name in ('tsdf', 'weight', 'color', 'free', 'blocks'):
        x, y = a.get(name), b.get(name)
        assert (x is None) == (y is None), name
        if x is not None:
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                                                         y.view(np.uint32) if y.dtype == np.float32 else y), name


# ------------------------------------------------------------------------------------------------------------------------- the ABI
def test_the_symbols_exist_and_the_c_abi_refuses_bad_arguments():
    L = _lib.lib()
    assert _lib.header_abi_version() >= 62 and L.atvs_abi_version() == _lib.header_abi_version()
    assert {'atvs_fusion_support', 'atvs_tsdf_integrate_weighted'} <= set(_lib.declared_symbols())
    sup = lambda n=2, rows=4, cols=4, nc=2, outs=(8, 8, 8), cams=8, nd=8: L.atvs_fusion_support(      # noqa: E731
        cams, nd, n, rows, cols, 0.01, 6.28, nc, outs[0], outs[1], outs[2], None)
    assert sup(outs=(None, None, None)) == -1 and sup(cams=None) == -1 and sup(nd=None) == -1
    assert sup(n=0) == -2 and sup(rows=0) == -2 and sup(n=4, rows=1 << 15, cols=1 << 15) == -2        # scene_grid's limits
    assert sup(nc=-1) == -3
    org = (ctypes.c_double * 3)(0, 0, 0)
    weighted = lambda weights=8, free_masks=8, free_out=8, cw=1.0, count=1: L.atvs_tsdf_integrate_weighted(      # noqa: E731
        8, weights, None, 0, 8, 1, 4, 4, 0.1, 0.4, org, 2, 2, 2, 0.0, 8, 8, free_masks, cw, count, 8, 8, None, free_out, 8, None)
    assert weighted(weights=None) == -1
    assert weighted(free_masks=None) == -1 and weighted(free_out=None) == -1                          # one of the two
    for cw in (0.0, -1.0, float('nan'), float('inf')):
        assert weighted(cw=cw) == -3
    assert weighted(count=9) == -2
    assert weighted(count=0) == 0 and weighted(free_masks=None, free_out=None, cw=0.0, count=0) == 0  # nothing launched
    assert 'fusion_support.hip' in [s.rsplit('/', 1)[-1] for s in _lib.sources()]
    assert '-ffp-contract=off' in _lib.flags_for('fusion_support.hip') and '-fno-slp-vectorize' in _lib.flags_for('fusion_support.hip')


# ------------------------------------------------------------------------------------------------------------------ argument checks
def test_fusion_support_checks_its_arguments_on_meta_tensors():
    cams, nd = _meta((3, 28)), _meta((3, 5, 7, 4))
    out = ops.fusion_support(cams, nd, 0.01, 6.28, 2)
    assert sorted(out) == ['count', 'depth', 'weight']
    assert out['count'].dtype == torch.int32 and out['depth'].dtype == out['weight'].dtype == torch.float32
    assert all(tuple(t.shape) == (3, 5, 7) and t.device.type == 'meta' for t in out.values())
    assert sorted(ops.fusion_support(cams, nd, 0.01, 6.28, 0, want=('weight',))) == ['weight']
    assert sorted(ops.fusion_support(cams, nd, 0.01, 6.28, 0, want='count')) == ['count']
    with pytest.raises(TypeError, match='normals_depths'):
        ops.fusion_support(cams, _meta((3, 5, 7, 4), torch.float64), 0.01, 6.28, 2)
    with pytest.raises(TypeError, match='cams'):
        ops.fusion_support(_meta((3, 28), torch.float64), nd, 0.01, 6.28, 2)
    with pytest.raises(ValueError, match='cams'):
        ops.fusion_support(_meta((2, 28)), nd, 0.01, 6.28, 2)
    with pytest.raises(ValueError, match='normals_depths'):
        ops.fusion_support(cams, _meta((3, 5, 7)), 0.01, 6.28, 2)
    with pytest.raises(ValueError, match='normals_depths'):
        ops.fusion_support(cams, _meta((3, 5, 7, 3)), 0.01, 6.28, 2)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match='num_consistent'):
            ops.fusion_support(cams, nd, 0.01, 6.28, bad)
    for bad in ((), ('count', 'count'), ('points',)):
        with pytest.raises(ValueError, match='want'):
            ops.fusion_support(cams, nd, 0.01, 6.28, 2, want=bad)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.fusion_support(torch.zeros((3, 28)), torch.zeros((3, 5, 7, 4)), 0.01, 6.28, 2)
    with pytest.raises(RuntimeError, match='mixing'):
        ops.fusion_support(torch.zeros((3, 28)), nd, 0.01, 6.28, 2)
    with pytest.raises(ValueError, match='2\\^31'):
        ops.fusion_support(_meta((4, 28)), _meta((4, 1 << 15, 1 << 15, 4)), 0.01, 6.28, 2)


def test_tsdf_integrate_checks_its_weights_on_meta_tensors():
    d, c, im = _meta((3, 5, 7)), _meta((3, 16), torch.float64), _meta((3, 5, 7, 3))
    ok = dict(voxel=0.1, trunc=0.4, origin=(0, 0, 0), dims=(2, 2, 2))
    vol = ops.tsdf_integrate(d, c, images=im, weights=_meta((3, 5, 7)), **ok)
    assert vol.num_blocks == 0 and vol.free is None
    assert ops.tsdf_integrate(d, c, images=im, weights=_meta((3, 5, 7)), carve_weight=0.5, **ok).free is not None
    for bad in (_meta((3, 5, 8)), _meta((2, 5, 7)), _meta((3, 5, 7, 1)), _meta((3, 35))):
        with pytest.raises(ValueError, match='weights'):
            ops.tsdf_integrate(d, c, images=im, weights=bad, **ok)
    with pytest.raises(TypeError, match='weights'):
        ops.tsdf_integrate(d, c, images=im, weights=_meta((3, 5, 7), torch.float64), **ok)
    with pytest.raises(TypeError, match='weights'):
        ops.tsdf_integrate(d, c, images=im, weights=np.ones((3, 5, 7), np.float32), **ok)
    with pytest.raises(RuntimeError, match='weights'):
        ops.tsdf_integrate(d, c, images=im, weights=torch.ones((3, 5, 7)), **ok)


# -------------------------------------------------------------------------------------------------------- options, rules, parsers
def test_check_options_and_the_rules():
    assert mesh_fusion.check_options(0.1, consistent=True, weights='agree') == mesh_fusion.check_options(0.1)
    assert mesh_fusion.check_support() == (False, None) and mesh_fusion.check_support(True, 'agree') == (True, 'agree')
    assert mesh_fusion.check_support(False, 'prob', mesh_fusion.TOOL_WEIGHT_MODES) == (False, 'prob')
    for bad in (1, 'yes', None):
        with pytest.raises(ValueError, match='consistent'):
            mesh_fusion.check_options(0.1, consistent=bad)
    for bad in ('prob', 'angle', True, 1.0):                     # prob is the tool's only
        with pytest.raises(ValueError, match='weights'):
            mesh_fusion.check_options(0.1, weights=bad)
    fuse = dict(prob_threshold=0.8, disp_threshold=0.01, num_consistent=2)
    assert mesh_fusion.rules(dict(voxel=0.1), fuse) == mesh_fusion.rules(dict(voxel=0.1, consistent=False, weights=None), fuse)
    broken = lambda mesh, f=fuse: [m for b, m in E._option_rules(fuse=f, mesh=mesh) if b]      # noqa: E731
    assert any('mesh consistent= needs voxel=' in m for m in broken(dict(consistent=True)))
    assert any('mesh weights= needs voxel=' in m for m in broken(dict(weights='agree')))
    assert broken(dict(voxel=0.1, consistent=True, weights='agree')) == []
    assert any('need --fuse' in m for m in broken(dict(voxel=0.1, consistent=True), None))
    with pytest.raises(ValueError, match='weights'):
        E.run_eval_pc('out', [], fuse=fuse, mesh=dict(voxel=0.05, weights='prob'))
    with pytest.raises(ValueError, match='consistent'):
        E.run_eval_pc('out', [], fuse=fuse, mesh=dict(voxel=0.05, consistent='yes'))


def test_the_command_lines(capsys, tmp_path):
    # mesh_fusion's own command line and the driver's keep the options they had: the new ones are mesh_consistent's
    base = ['--maps', 'm', '--voxel', '0.1', '--out', 'o.ply']
    a = mesh_fusion.make_parser().parse_args(base)
    assert not any(hasattr(a, name) for name in ('consistent', 'weights', 'disp_threshold', 'num_consistent'))
    d = E.make_parser().parse_args([])
    assert not hasattr(d, 'mesh_consistent') and not hasattr(d, 'mesh_weights')
    p = mesh_consistent.make_parser()
    assert {o for x in mesh_fusion.make_parser()._actions for o in x.option_strings} | {
        '--consistent', '--weights', '--disp_threshold', '--num_consistent'} == {o for x in p._actions for o in x.option_strings}
    a = p.parse_args(base)
    assert a.consistent is False and a.weights is None and a.disp_threshold is None and a.num_consistent is None
    a = p.parse_args(base + ['--consistent', '--disp_threshold', '0.02', '--num_consistent', '3', '--weights', 'prob', '--carve'])
    assert a.consistent is True and a.weights == 'prob' and a.disp_threshold == 0.02 and a.num_consistent == 3 and a.carve == 1.0
    assert p.parse_args(base + ['--weights', 'agree']).weights == 'agree'
    err = lambda: ' '.join(capsys.readouterr().err.split())      # noqa: E731
    with pytest.raises(SystemExit) as x:
        p.parse_args(base + ['--weights', 'angle'])
    assert x.value.code == 2 and 'invalid choice' in err()
    with pytest.raises(SystemExit) as x:
        mesh_fusion.cli(base + ['--consistent'])
    assert x.value.code == 2 and 'unrecognized arguments: --consistent' in err()
    with pytest.raises(SystemExit) as x:
        mesh_consistent.cli(base + ['--num_consistent', '3'])
    assert x.value.code == 2 and 'need --consistent or --weights agree' in err()
    with pytest.raises(SystemExit) as x:
        mesh_consistent.cli(base + ['--consistent', '--num_consistent', '-1'])
    assert x.value.code == 2 and '--num_consistent >= 0' in err()
    with pytest.raises(SystemExit) as x:
        mesh_consistent.cli(base + ['--consistent', '--carve', '0'])          # mesh_fusion's own checks still run
    assert x.value.code == 2 and 'carve_weight' in err()
    # --weights prob without probability files: one depth map and its camera, no _prob.pfm beside them
    from atvsnet_amd.atvsnet import preprocess
    folder = tmp_path / 'depths_atvsnet'
    folder.mkdir()
    preprocess.write_pfm(str(folder / '00000000.pfm'), np.ones((4, 6), np.float32))
    cam = np.zeros((2, 4, 4))
    cam[0] = np.eye(4)
    cam[1, :3, :3] = [[5, 0, 3], [0, 5, 2], [0, 0, 1]]
    cam[1, 3, :2] = (0.5, 0.01)
    with open(str(folder / '00000000.txt'), 'w') as f:
        f.write(preprocess.cam_text(cam))
    with pytest.raises(SystemExit) as x:
        mesh_consistent.cli(['--maps', str(tmp_path), '--voxel', '0.1', '--out', str(tmp_path / 'o.ply'), '--weights', 'prob'])
    assert x.value.code == 2 and '--weights prob needs the probability maps' in err()
    # the driver takes the two through run_eval_pc's mesh dict
    flags = dict(prob_threshold=0.8, disp_threshold=0.01, num_consistent=2, fuse=True, mesh_voxel=0.1)
    assert E._run_options(argparse.Namespace(**flags))['mesh'] == dict(voxel=0.1)


# ------------------------------------------------------------------------------------------------- the restatement alone: the floater
def test_the_mask_removes_the_floater_at_its_cause():
    scene = WR.floater()
    blob = WR.blob_pixels()
    assert blob.shape == scene.depths[:2].shape and blob.sum(axis=(1, 2)).min() >= 4
    valid = scene.depths > 0
    count = WR.scene_support('floater', 2)['count']
    assert count[~valid].max() == 0                              # a pixel without a depth agrees with nothing
    assert count[:2][blob].max() <= 1                            # two views agree on the blob: each pixel has at most the other
    kept = WR.scene_support('floater', 2)['depth'] > 0
    assert not kept[:2][blob].any()                              # every blob pixel is masked
    others = valid.copy()
    others[:2] &= ~blob
    share = kept[others].sum() / others.sum()
    print('floater, num_consistent 2: %.4f of the other valid samples kept' % share)
    assert share >= 0.95                                         # the oracle gives 98.0 %: not an empty mask
    assert not (kept & ~valid).any()
    one = WR.scene_support('floater', 1)['depth'] > 0
    assert 0 < one[:2][blob].sum() < blob.sum()                  # at 1 the blob's better half stays: 2 is what removes it


def test_the_masked_mesh_has_no_floater_and_keeps_the_sphere():
    plain, masked = WR.floater_plain_mesh(), WR.floater_masked_mesh()
    print('farthest vertex: %.4f without the mask, %.4f with it' % (WR.farthest(plain[0]), WR.farthest(masked[0])))
    assert WR.farthest(plain[0]) > 1.1
    assert WR.farthest(masked[0]) < 0.95
    largest_plain, _ = WR.largest_component_faces(plain[2], len(plain[0]))
    largest, _ = WR.largest_component_faces(masked[2], len(masked[0]))
    print('largest component: %d faces of %d without the mask, %d of %d with it' % (largest_plain, len(plain[2]), largest, len(masked[2])))
    assert largest >= 0.9 * largest_plain


@pytest.mark.parametrize('cw', (None, 0.5))
def test_all_ones_weights_are_the_unweighted_bits(cw):
    scene = WR.floater()
    got = WR.integrate_scene(scene, np.ones(scene.depths.shape, np.float32), cw)
    want = dict(scene.plain, free=None) if cw is None else scene.want(cw)
    _bits_equal(got, want)


@pytest.mark.parametrize('cw', (None, 0.5))
def test_a_mask_as_weights_is_the_masked_depths(cw):
    scene = WR.floater()
    masked = WR.scene_support('floater', 2)['depth']
    mask = WR.scene_support('floater', 2)['count'] >= 2
    assert (mask & (scene.depths > 0)).sum() < (scene.depths > 0).sum()
    got = WR.integrate_scene(scene, mask.astype(np.float32), cw)
    if cw is None:
        want = dict(WR.floater_masked()[1], free=None)
    else:
        want = CR.integrate(masked, scene.cams, *scene.args(), images=scene.images, pixel_centre=scene.pixel_centre, carve_weight=cw)
    _bits_equal(got, want)
    assert not np.array_equal(got['weight'], scene.plain['weight'])


def test_no_weight_is_no_sample_and_an_unweighted_block_is_absent():
    scene = WR.ring()
    w = WR.special_weights(scene.depths.shape, 11)
    with np.errstate(invalid='ignore'):
        sample = (w > 0) & np.isfinite(w)
    assert 0.3 < sample.mean() < 0.7 and np.isnan(w).any() and np.isinf(w).any() and (w < 0).any() and (w == 0).any()
    got = WR.integrate_scene(scene, w, 0.5)
    want = WR.integrate_scene(scene, np.where(sample, w, np.float32(1.0)), 0.5, depths=np.where(sample, scene.depths, np.float32(0.0)))
    _bits_equal(got, want)
    assert np.isfinite(got['tsdf']).all() and np.isfinite(got['weight']).all()
    # view 3's weights all 0 and the others' 0 on the left half of the image: the blocks only those samples reach are not in the volume
    w = np.ones(scene.depths.shape, np.float32)
    w[3] = 0
    w[:, :, :scene.depths.shape[2] // 2] = 0
    got = WR.integrate_scene(scene, w)
    assert 0 < len(got['blocks']) < len(scene.plain['blocks'])
    bx, by, bz = scene.dims
    has = (got['weight'] > 0).reshape(bz, 8, by, 8, bx, 8).any(axis=(1, 3, 5))
    assert has.sum() == len(got['blocks'])                       # exactly the blocks with a voxel of weight > 0


def test_a_down_weighted_biased_view_moves_the_surface_less():
    scene, weights = WR.biased_ring()
    equal = WR.mesh_of(scene, WR.integrate_scene(scene, np.ones_like(weights)))
    weighted = WR.mesh_of(scene, WR.integrate_scene(scene, weights))
    e, w = WR.mean_radius_error(equal[0]), WR.mean_radius_error(weighted[0])
    print('mean |radius - 0.9| over the vertices: %.6f with equal weights, %.6f with 0.05 on the biased view' % (e, w))
    assert w < e


def test_the_weight_plane_is_one_rounded_division():
    count = np.arange(0, 24, dtype=np.int32).reshape(1, 4, 6)
    for nc in (0, 1, 2, 6, 23):
        got = WR.planes(count, np.ones((1, 4, 6), np.float32), nc)['weight']
        exact = (1.0 + count.astype(np.float64)) / (1.0 + nc)
        assert got.dtype == np.float32 and np.array_equal(got, exact.astype(np.float32))        # one division, correctly rounded
        assert (got[count == nc] == 1.0).all() and (got[count > nc] > 1.0).all() and (got[count < nc] < 1.0).all()
