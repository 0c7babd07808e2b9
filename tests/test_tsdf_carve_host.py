"""Free-space carving on the host (no GPU): tests/tsdf_carve_restated.py alone on the clean sphere, the floater scene, a healed
invalid depth, the exact band edge and the narrow field; the free-view rule as a superset of the exact (block, view) pairs on every
input the GPU file uses; the wrappers' argument checks on the `meta` device and the two command lines' option rules."""
import numpy as np
import pytest
import torch

import tsdf_carve_restated as CR
import tsdf_cases as TC
from atvsnet_amd import _lib, ops
from atvsnet_amd.atvsnet import eval_pointcloud as E
from atvsnet_amd.atvsnet import mesh_fusion


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ----------------------------------------------------------------------------------------------------------------- the clean sphere
def test_carving_leaves_weight_alone_and_moves_tsdf_only_where_a_view_saw_past():
    ring = CR.ring()
    want, plain = ring.want(1.0), ring.plain
    assert np.array_equal(want['weight'], plain['weight']) and np.array_equal(want['blocks'], plain['blocks'])
    assert np.array_equal(_bits(want['color']), _bits(plain['color']))
    untouched = want['free'] == 0
    assert np.array_equal(_bits(want['tsdf'])[untouched], _bits(plain['tsdf'])[untouched])
    assert (_bits(want['tsdf']) != _bits(plain['tsdf'])).any()
    assert not ((want['tsdf'] < 0) != (plain['tsdf'] < 0)).any()                  # no sign flips on a clean scene
    assert want['free'].max() >= 2
    assert (want['free'][plain['weight'] == 0] == 0).all()                        # a voxel no view has in band is not carved
    assert ((want['free'] > 0).sum(), (plain['weight'] > 0).sum()) == (3225, 21197)


def test_24_clean_views_flip_no_sign_either():
    ring = CR.ring(24)
    want, plain = ring.want(1.0), ring.plain
    assert not ((want['tsdf'] < 0) != (plain['tsdf'] < 0)).any()
    assert ((want['free'] > 0).sum(), (plain['weight'] > 0).sum()) == (6621, 22457)


# ----------------------------------------------------------------------------------------------------------------------- the floater
def _radii(mesh):
    return np.linalg.norm(mesh[0].astype(np.float64), axis=1)


@pytest.mark.parametrize('min_weight', (1.0, 2.0))
def test_the_floater_is_meshed_without_carving_and_gone_with_it(min_weight):
    scene = CR.floater()
    plain, carved = scene.mesh(None, min_weight), scene.mesh(1.0, min_weight)
    assert _radii(plain).max() > 1.1
    assert _radii(carved).max() <= 1.0
    big_plain, big_carved = CR.largest_component_faces(plain[2], len(plain[0])), CR.largest_component_faces(carved[2], len(carved[0]))
    assert big_plain[0] == big_carved[0] > 30000 and big_carved[1] < big_plain[1]
    assert len(carved[2]) < len(plain[2])


def test_half_a_vote_carves_the_floater_too():
    scene = CR.floater()
    carved = scene.mesh(0.5, 1.0)
    assert _radii(carved).max() <= 1.0
    assert CR.largest_component_faces(carved[2], len(carved[0]))[0] == CR.largest_component_faces(scene.mesh(None, 1.0)[2],
                                                                                                len(scene.mesh(None, 1.0)[0]))[0]
    assert not np.array_equal(_bits(scene.want(0.5)['tsdf']), _bits(scene.want(1.0)['tsdf']))


# ------------------------------------------------------------------------------------------------------------------ invalid depths
def test_an_invalid_depth_healed_to_a_far_one_changes_free():
    case = TC.uneven(0.2)
    scene = CR.Scene.of(case)
    want = scene.want(1.0)
    assert want['free'].max() >= 1
    for k, value in enumerate(TC.INVALID):
        mine = case.notes['cls'] == k
        healed = np.where(mine, np.float32(9.0), case.depths)                     # far beyond the box: free for every voxel on the ray
        other = CR.integrate(healed, case.cams, *scene.args(), images=case.images, pixel_centre=case.pixel_centre)
        assert np.array_equal(other['weight'], want['weight']), value            # 9.0 is in no voxel's band
        assert not np.array_equal(other['free'], want['free']), value


# ---------------------------------------------------------------------------------------------------------------------- band edge
def test_the_band_edge_scene_has_voxels_exactly_on_both_edges():
    scene = CR.band_edge()
    plus, minus = CR.band_edge_counts(scene)
    assert plus > 0 and minus > 0
    want = scene.want(1.0)
    assert want['free'].max() >= 1 and want['weight'].max() == 2
    # sdf == +trunc is in band, not free (band_edge_counts asserts it per view): with the band a hair narrower those voxels turn free
    narrower = CR.integrate(scene.depths, scene.cams, scene.voxel, np.nextafter(scene.trunc, 0.0), scene.origin, scene.dims)
    assert (narrower['free'] > want['free']).sum() >= 1 and (narrower['weight'] < want['weight']).sum() >= plus


# ------------------------------------------------------------------------------------------------------------------ the free views
def _scenes():
    yield 'ring', CR.ring()
    yield 'floater', CR.floater()
    for trunc in TC.UNEVEN_TRUNCS:
        yield 'uneven-%g' % trunc, CR.Scene.of(TC.uneven(trunc))
    yield 'lone_pixels', CR.Scene.of(TC.lone_pixels())
    yield 'full_box', CR.Scene.of(TC.full_box())
    yield 'camera_inside', CR.Scene.of(TC.camera_inside())
    yield 'long_directory', CR.Scene.of(TC.long_directory())
    for live in TC.MASK_LIVE:
        yield 'mask_bits-%s' % (live,), CR.Scene.of(TC.mask_bits(live))
    yield 'views65', CR.views65()
    yield 'band_edge', CR.band_edge()
    yield 'narrow_field', CR.narrow_field()


@pytest.mark.parametrize('name', [name for name, _ in _scenes()])
def test_the_rule_is_a_superset_of_the_views_that_contribute_or_carve(name):
    scene = dict(_scenes())[name]
    rule, exact = scene.rule(), scene.exact()
    assert CR.bits_set(exact) > 0
    assert ((exact & ~rule) == 0).all()
    n = len(scene.cams)
    beyond = ~np.uint64(0) << np.uint64(n & 63) if n & 63 else np.uint64(0)
    assert (rule[:, -1] & beyond == 0).all()                                      # the lanes beyond the last view vote 0


def test_the_narrow_field_clears_a_bit_in_every_view_and_camera_inside_clears_blocks_behind():
    scene = CR.narrow_field()
    rule = scene.rule()
    n = len(scene.cams)
    per_view = [int(((rule[:, 0] >> np.uint64(k)) & np.uint64(1)).sum()) for k in range(n)]
    assert all(0 < s < len(rule) for s in per_view)
    assert CR.bits_set(scene.rule(padding=0.0)) < CR.bits_set(rule)               # the pixel of padding sets bits of its own
    inside = CR.Scene.of(TC.camera_inside())
    assert CR.bits_set(inside.rule()) < len(inside.rule()) * len(inside.cams)
    # and there a voxel behind a camera is not carved although its block is seen: free counts only views with c2 > 0
    want = inside.want(1.0)
    assert want['free'].max() >= 1


def test_the_free_mask_uses_both_halves_and_the_top_bit():
    rule = CR.Scene.of(TC.mask_bits((31,))).rule()
    for bit in (0, 31, 32, 63):
        assert ((rule[:, 0] >> np.uint64(bit)) & np.uint64(1)).any()
    assert CR.views65().rule().shape[1] == 2 and (CR.views65().rule()[:, 1] == 1).any()


# ------------------------------------------------------------------------------------------------------------------- argument checks
def _meta(shape, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device='meta')


def test_carve_weight_must_be_a_finite_positive_number():
    d, c, im = _meta((3, 5, 7)), _meta((3, 16), torch.float64), _meta((3, 5, 7, 3))
    ok = dict(voxel=0.1, trunc=0.4, origin=(0, 0, 0), dims=(2, 2, 2))
    for bad in (0, 0.0, -1.0, float('nan'), float('inf'), '1.0', True):
        with pytest.raises(ValueError, match='carve_weight'):
            ops.tsdf_integrate(d, c, images=im, carve_weight=bad, **ok)
        with pytest.raises(ValueError, match='carve_weight'):
            mesh_fusion.check_carve_weight(bad)
        with pytest.raises(ValueError, match='carve_weight'):
            mesh_fusion.check_options(0.1, carve_weight=bad)
    vol = ops.tsdf_integrate(d, c, images=im, carve_weight=0.5, **ok)
    assert vol.num_blocks == 0 and tuple(vol.free.shape) == (0, 8, 8, 8) and vol.free.device.type == 'meta'
    assert ops.tsdf_integrate(d, c, images=im, **ok).free is None
    assert mesh_fusion.check_options(0.1, carve_weight=2) == mesh_fusion.check_options(0.1) and len(mesh_fusion.check_options(0.1)) == 5
    assert mesh_fusion.check_carve_weight(None) is None and mesh_fusion.check_carve_weight(2) == 2.0
    masks = ops.tsdf_free_views(_meta((4, 3), torch.int32), _meta((65, 16), torch.float64), 5, 7, 0.1, (0, 0, 0), (2, 2, 2))
    assert tuple(masks.shape) == (4, 2) and masks.dtype == torch.int64
    with pytest.raises(ValueError, match='blocks'):
        ops.tsdf_free_views(_meta((9, 3), torch.int32), c, 5, 7, 0.1, (0, 0, 0), (2, 2, 2))
    with pytest.raises(TypeError, match='blocks'):
        ops.tsdf_free_views(_meta((4, 3), torch.int64), c, 5, 7, 0.1, (0, 0, 0), (2, 2, 2))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.tsdf_free_views(torch.zeros((4, 3), dtype=torch.int32), torch.zeros((3, 16), dtype=torch.float64), 5, 7, 0.1, (0, 0, 0), (2, 2, 2))
    host = ops.TsdfVolume.from_dense(np.ones((8, 8, 8)), np.ones((8, 8, 8)), None, (0, 0, 0), 1.0, 4.0)
    assert host.free is None
    with pytest.raises(ValueError, match='free'):
        ops.TsdfVolume((0, 0, 0), 1.0, 4.0, (1, 1, 1), host.blocks, host.tsdf, host.weight, None, host.tsdf.reshape(1, 512))
    carrying = ops.TsdfVolume((0, 0, 0), 1.0, 4.0, (1, 1, 1), host.blocks, host.tsdf, host.weight, None, host.weight)
    assert len(carrying.to_dense()) == 3                                          # to_dense ignores free


def test_the_symbols_exist_and_the_c_abi_refuses_bad_arguments():
    L = _lib.lib()
    assert _lib.header_abi_version() >= 61 and L.atvs_abi_version() == _lib.header_abi_version()
    assert {'atvs_tsdf_free_views', 'atvs_tsdf_integrate_carve'} <= set(_lib.declared_symbols())
    import ctypes
    org = (ctypes.c_double * 3)(0, 0, 0)
    assert L.atvs_tsdf_free_views(None, 1, None, 1, 4, 4, 0.1, org, 2, 2, 2, 0.0, None, None) == -1
    assert L.atvs_tsdf_free_views(8, 9, 8, 1, 4, 4, 0.1, org, 2, 2, 2, 0.0, 8, None) == -2            # 9 of 8 blocks
    assert L.atvs_tsdf_free_views(8, 1, 8, 0, 4, 4, 0.1, org, 2, 2, 2, 0.0, 8, None) == -2            # no view
    assert L.atvs_tsdf_free_views(8, 1, 8, 1, 4, 4, 0.0, org, 2, 2, 2, 0.0, 8, None) == -3
    assert L.atvs_tsdf_free_views(8, 0, 8, 1, 4, 4, 0.1, org, 2, 2, 2, 0.0, None, None) == 0          # nothing to do, nothing launched
    carve = lambda cw, count=1: L.atvs_tsdf_integrate_carve(8, None, 0, 8, 1, 4, 4, 0.1, 0.4, org, 2, 2, 2, 0.0, 8, 8, 8, cw, count,   # noqa: E731
                                                            8, 8, None, 8, 8, None)
    for cw in (0.0, -1.0, float('nan'), float('inf')):
        assert carve(cw) == -3
    assert carve(1.0, 9) == -2
    assert L.atvs_tsdf_integrate_carve(8, None, 0, 8, 1, 4, 4, 0.1, 0.4, org, 2, 2, 2, 0.0, 8, 8, None, 1.0, 1, 8, 8, None, 8, 8, None) == -1
    assert L.atvs_tsdf_gather(8, 8, 8, None, 8, 4, 2, 8, 8, 8, None, 8, None, None) == -1             # free in without free out


def test_the_command_lines(capsys):
    p = mesh_fusion.make_parser()
    base = ['--maps', 'm', '--voxel', '0.1', '--out', 'o.ply']
    assert p.parse_args(base).carve is None
    assert p.parse_args(base + ['--carve']).carve == mesh_fusion.DEFAULT_CARVE_WEIGHT == 1.0
    assert p.parse_args(base + ['--carve', '0.5']).carve == 0.5
    with pytest.raises(SystemExit) as x:
        mesh_fusion.cli(base + ['--carve', '0'])
    assert x.value.code == 2 and 'carve_weight' in capsys.readouterr().err
    with pytest.raises(SystemExit) as x:
        E.cli(['--fuse', '--mesh_carve'])
    assert x.value.code == 2 and '--mesh_carve needs --mesh_voxel' in ' '.join(capsys.readouterr().err.split())
    with pytest.raises(SystemExit) as x:
        E.cli(['--fuse', '--mesh_voxel', '0.05', '--mesh_carve', '-2'])
    assert x.value.code == 2 and 'carve_weight' in capsys.readouterr().err
    import argparse
    flags = dict(prob_threshold=0.8, disp_threshold=0.01, num_consistent=2, fuse=True, mesh_voxel=0.1)
    assert E._run_options(argparse.Namespace(**flags))['mesh'] == dict(voxel=0.1)
    assert E._run_options(argparse.Namespace(mesh_carve=1.0, **flags))['mesh'] == dict(voxel=0.1, carve_weight=1.0)
    fuse = dict(prob_threshold=0.8, disp_threshold=0.01, num_consistent=2)
    broken = [m for b, m in E._option_rules(fuse=fuse, mesh=dict(carve_weight=1.0)) if b]
    assert any('--mesh_carve needs --mesh_voxel' in m for m in broken)
    with pytest.raises(ValueError, match='carve_weight'):
        E.run_eval_pc('out', [], fuse=fuse, mesh=dict(voxel=0.05, carve_weight=0))
