"""ops.tsdf_integrate(carve_weight=) and ops.tsdf_free_views on the GPU against tests/tsdf_carve_restated.py, bit for bit
(np.array_equal everywhere, floats as bits): the dense restatement visits every voxel for every view, so an equal `free` shows that
no view the free mask leaves out could have carved.  What makes each input discriminate is asserted in
tests/test_tsdf_carve_host.py without a GPU."""
import numpy as np
import pytest
import torch

import tsdf_carve_restated as CR
import tsdf_cases as TC
import tsdf_restated as R
from tsdf_cases import _mesh_equal, _volume_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops(cuda):
    from atvsnet_amd import ops as o
    return o


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _integrate(ops, scene, cw, **kw):
    return ops.tsdf_integrate(_dev(scene.depths), _dev(scene.cams), scene.voxel, scene.trunc, scene.origin, scene.dims,
                              images=_dev(scene.images), pixel_centre=scene.pixel_centre, carve_weight=cw, **kw)


def _dense_free(vol):
    """vol.free over the whole box, [z][y][x], as TsdfVolume.to_dense lays tsdf out."""
    bx, by, bz = vol.dims
    b = vol.blocks.cpu().numpy().astype(np.int64)
    full = np.zeros((bz * by * bx, 8, 8, 8), np.float32)
    full[(b[:, 2] * by + b[:, 1]) * bx + b[:, 0]] = vol.free.cpu().numpy()
    return full.reshape(bz, by, bx, 8, 8, 8).transpose(0, 3, 1, 4, 2, 5).reshape(bz * 8, by * 8, bx * 8)


def _carved_equal(vol, want):
    _volume_equal(vol, want)
    assert vol.free is not None and vol.free.dtype == torch.float32 and tuple(vol.free.shape) == (vol.num_blocks, 8, 8, 8)
    assert np.array_equal(_dense_free(vol).view(np.uint32), want['free'].view(np.uint32))


def _same_bits(a, b):
    for name in ('blocks', 'tsdf', 'weight', 'color', 'free'):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), name
        if x is not None:
            assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)), name


def _check(ops, scene, cw=1.0, **kw):
    vol = _integrate(ops, scene, cw, **kw)
    _carved_equal(vol, scene.want(cw))
    return vol


# ----------------------------------------------------------------------------------------------------------------------- the ring
@pytest.mark.parametrize('cw', (1.0, 0.5, 0.1, 3.0))            # 0.1 is not dyadic: cw * Wf rounds
def test_the_clean_ring(ops, cw):
    scene = CR.ring()
    vol = _check(ops, scene, cw)
    assert float(vol.free.max()) >= 2
    _same_bits(vol, _integrate(ops, scene, cw))                  # the same bits again
    # blocks, weight and colour are those of the run without carving, tsdf too where no view saw past
    plain = _integrate(ops, scene, None)
    assert plain.free is None
    assert torch.equal(vol.blocks, plain.blocks) and torch.equal(vol.weight.view(torch.int32), plain.weight.view(torch.int32))
    assert torch.equal(vol.color.view(torch.int32), plain.color.view(torch.int32))
    untouched = vol.free == 0
    assert torch.equal(vol.tsdf.view(torch.int32)[untouched], plain.tsdf.view(torch.int32)[untouched])
    assert not torch.equal(vol.tsdf, plain.tsdf)


def test_without_carving_the_ring_keeps_its_bits_and_has_no_free(ops):
    scene = CR.ring()
    vol = _integrate(ops, scene, None)
    assert vol.free is None
    _volume_equal(vol, scene.plain)
    _same_bits(vol, ops.tsdf_integrate(_dev(scene.depths), _dev(scene.cams), scene.voxel, scene.trunc, scene.origin, scene.dims,
                                       images=_dev(scene.images)))


def test_without_images(ops):
    scene = CR.ring()
    bare = CR.Scene(scene.depths, scene.cams, None)
    vol = _check(ops, bare)
    assert vol.color is None


# -------------------------------------------------------------------------------------------------------------------- the floater
def test_the_floater_is_carved_away(ops):
    scene = CR.floater()
    vol = _check(ops, scene, 1.0)
    got = ops.tsdf_mesh(vol)
    _mesh_equal(got, scene.mesh(1.0, 1.0))
    assert np.linalg.norm(got[0].cpu().numpy().astype(np.float64), axis=1).max() <= 1.0
    plain = ops.tsdf_mesh(_integrate(ops, scene, None))
    assert np.linalg.norm(plain[0].cpu().numpy().astype(np.float64), axis=1).max() > 1.1
    assert len(got[2]) < len(plain[2])
    # at min_weight 2 as well: the restated radius, without a second host mesh
    got2 = ops.tsdf_mesh(vol, min_weight=2)
    assert np.linalg.norm(got2[0].cpu().numpy().astype(np.float64), axis=1).max() <= 1.0
    _check(ops, scene, 0.5)


# ------------------------------------------------------------------------------------------------------- the inputs of tsdf_cases
@pytest.mark.parametrize('trunc', TC.UNEVEN_TRUNCS)
def test_uneven_box_with_every_invalid_depth(ops, trunc):
    _check(ops, CR.Scene.of(TC.uneven(trunc)))


def test_lone_pixels(ops):
    _check(ops, CR.Scene.of(TC.lone_pixels()))


def test_full_box(ops):
    assert _check(ops, CR.Scene.of(TC.full_box())).num_blocks == 6


def test_cameras_inside_the_box_do_not_carve_behind_themselves(ops):
    _check(ops, CR.Scene.of(TC.camera_inside()))


def test_long_directory_and_the_gather_carries_free(ops):
    case = TC.long_directory()
    scene = CR.Scene.of(case)
    marked = TC.check_marking_is_a_strict_superset(case)          # slots without a weight: gather compacts free with the rest
    vol = _check(ops, scene, 1.0, max_blocks=marked)
    assert vol.num_blocks == len(scene.want(1.0)['blocks']) < marked and float(vol.free.max()) >= 1


@pytest.mark.parametrize('live', TC.MASK_LIVE)
def test_mask_bits(ops, live):
    # the band mask holds only `live`; the free mask has views in both word halves and the top bit
    _check(ops, CR.Scene.of(TC.mask_bits(live)))


def test_65_views_need_a_second_word(ops):
    scene = CR.views65()
    vol = _check(ops, scene)
    assert float(vol.free.max()) >= 2
    # the last view alone carries a depth that lies behind everything: it carves from the second word
    depths = scene.depths.copy()
    depths[64] = np.where(depths[64] > 0, np.float32(9.0), 0)
    far = CR.Scene(depths, scene.cams, scene.images)
    assert not np.array_equal(far.want(1.0)['free'], scene.want(1.0)['free'])
    _check(ops, far)


# ------------------------------------------------------------------------------------------------------------------ the new cases
def test_the_exact_band_edge_is_in_band(ops):
    scene = CR.band_edge()
    for cw in (1.0, 0.1):
        _check(ops, scene, cw)


def test_the_free_views_of_a_narrow_field(ops):
    scene = CR.narrow_field()
    blocks = CR.all_blocks(scene.dims)
    rows, cols = scene.depths.shape[1:]
    got = ops.tsdf_free_views(_dev(blocks), _dev(scene.cams), rows, cols, scene.voxel, scene.origin, scene.dims, scene.pixel_centre)
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(blocks), 1)
    want = scene.rule()
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want)
    n = len(scene.cams)
    assert 0 < CR.bits_set(want) < len(blocks) * n and (want >> np.uint64(n) == 0).all()          # a strict subset of all-ones
    again = ops.tsdf_free_views(_dev(blocks), _dev(scene.cams), rows, cols, scene.voxel, scene.origin, scene.dims, scene.pixel_centre)
    assert torch.equal(got, again)
    _check(ops, scene)


@pytest.mark.parametrize('name', ('views65', 'camera_inside', 'uneven'))
def test_the_free_views_elsewhere(ops, name):
    scene = {'views65': CR.views65, 'camera_inside': lambda: CR.Scene.of(TC.camera_inside()),
             'uneven': lambda: CR.Scene.of(TC.uneven(0.2))}[name]()
    blocks = CR.all_blocks(scene.dims)[::-1].copy()              # any order of blocks: a word belongs to its slot
    rows, cols = scene.depths.shape[1:]
    got = ops.tsdf_free_views(_dev(blocks), _dev(scene.cams), rows, cols, scene.voxel, scene.origin, scene.dims, scene.pixel_centre)
    assert np.array_equal(got.cpu().numpy().view(np.uint64), scene.rule()[::-1])
