"""-m gpu: ops.tsdf_integrate(weights=) against tests/tsdf_weighted_restated.py, bit for bit (np.array_equal everywhere, floats as
bits), `free` included, with and without carving: random non-dyadic weights, weights that are no weight (0, -0, -1, NaN, +-inf), the
inputs of tests/tsdf_cases.py, a second mask word, the gather.  The two identities of the definition: all-ones weights are the call
without weights, and a 0/1 weight plane is the depths zeroed by that mask -- with the mask ops.fusion_support makes."""
import numpy as np
import pytest
import torch

import tsdf_carve_restated as CR
import tsdf_cases as TC
import tsdf_weighted_restated as WR
from tsdf_cases import _volume_equal

pytestmark = pytest.mark.gpu

CARVE = (None, 0.5)


@pytest.fixture(scope='module')
def ops(cuda):
    from atvsnet_amd import ops as o
    return o


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _integrate(ops, scene, weights, cw, depths=None, **kw):
    return ops.tsdf_integrate(_dev(scene.depths if depths is None else depths), _dev(scene.cams), scene.voxel, scene.trunc, scene.origin,
                              scene.dims, images=_dev(scene.images), pixel_centre=scene.pixel_centre, carve_weight=cw,
                              weights=_dev(weights), **kw)


def _dense_free(vol):
    bx, by, bz = vol.dims
    b = vol.blocks.cpu().numpy().astype(np.int64)
    full = np.zeros((bz * by * bx, 8, 8, 8), np.float32)
    full[(b[:, 2] * by + b[:, 1]) * bx + b[:, 0]] = vol.free.cpu().numpy()
    return full.reshape(bz, by, bx, 8, 8, 8).transpose(0, 3, 1, 4, 2, 5).reshape(bz * 8, by * 8, bx * 8)


def _equal(vol, want):
    """_volume_equal (blocks, tsdf and colour as bits, weight, exactly the blocks with a voxel of weight > 0), weight as bits, free."""
    _volume_equal(vol, want)
    assert np.array_equal(vol.to_dense()[1].view(np.uint32), want['weight'].view(np.uint32))
    if want['free'] is None:
        assert vol.free is None
    else:
        assert vol.free is not None and tuple(vol.free.shape) == (vol.num_blocks, 8, 8, 8)
        assert np.array_equal(_dense_free(vol).view(np.uint32), want['free'].view(np.uint32))


def _same_bits(a, b):
    for name in ('blocks', 'tsdf', 'weight', 'color', 'free'):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), name
        if x is not None:
            assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)), name


def _check(ops, scene, weights, cw, **kw):
    vol = _integrate(ops, scene, weights, cw, **kw)
    _equal(vol, WR.integrate_scene(scene, weights, cw))
    return vol


# ----------------------------------------------------------------------------------------------------------------------- the ring
@pytest.mark.parametrize('cw', CARVE)
def test_random_weights_on_the_ring(ops, cw):
    scene = WR.ring()
    w = WR.random_weights(scene.depths.shape, 5)
    assert w.min() > 0 and w.max() <= 2 and (np.frexp(w)[0] * (1 << 12) % 1 != 0).mean() > 0.9       # hardly any is dyadic: w * x rounds
    vol = _check(ops, scene, w, cw)
    _same_bits(vol, _integrate(ops, scene, w, cw))                   # the same bits again
    plain = _integrate(ops, scene, None, cw)
    assert torch.equal(vol.blocks, plain.blocks) and not torch.equal(vol.weight, plain.weight) and not torch.equal(vol.tsdf, plain.tsdf)
    assert not torch.equal(vol.color, plain.color)
    if cw is not None:
        assert float(vol.free.max()) > 2 and not torch.equal(vol.free, plain.free)


@pytest.mark.parametrize('cw', CARVE)
def test_weights_that_are_no_weight(ops, cw):
    scene = WR.ring()
    w = WR.special_weights(scene.depths.shape, 11)
    assert np.isnan(w).any() and np.isposinf(w).any() and np.isneginf(w).any() and (w == -1).any() and (w == 0).any()
    vol = _check(ops, scene, w, cw)
    assert bool(torch.isfinite(vol.tsdf).all()) and bool(torch.isfinite(vol.weight).all()) and bool(torch.isfinite(vol.color).all())


def test_without_images(ops):
    scene = WR.ring()
    bare = CR.Scene(scene.depths, scene.cams, None)
    assert _check(ops, bare, WR.random_weights(scene.depths.shape, 6), 0.5).color is None


@pytest.mark.parametrize('cw', CARVE)
def test_all_ones_weights_are_the_call_without_weights(ops, cw):
    for scene in (WR.ring(), CR.Scene.of(TC.uneven(0.2))):
        ones = np.ones(scene.depths.shape, np.float32)
        _same_bits(_integrate(ops, scene, ones, cw), _integrate(ops, scene, None, cw))


# ------------------------------------------------------------------------------------------------------- the inputs of tsdf_cases
@pytest.mark.parametrize('cw', CARVE)
@pytest.mark.parametrize('trunc', TC.UNEVEN_TRUNCS)
def test_uneven_box_with_every_invalid_depth(ops, trunc, cw):
    scene = CR.Scene.of(TC.uneven(trunc))
    _check(ops, scene, WR.special_weights(scene.depths.shape, 3), cw)


@pytest.mark.parametrize('cw', CARVE)
def test_long_directory_through_the_gather(ops, cw):
    case = TC.long_directory()
    scene = CR.Scene.of(case)
    marked = TC.check_marking_is_a_strict_superset(case)
    w = WR.random_weights(scene.depths.shape, 8)
    vol = _check(ops, scene, w, cw, max_blocks=marked)
    assert vol.num_blocks < marked                                   # slots without a weight: gather compacts what was integrated


@pytest.mark.parametrize('cw', CARVE)
def test_65_views_need_a_second_word(ops, cw):
    scene = CR.views65()
    w = WR.random_weights(scene.depths.shape, 9)
    _check(ops, scene, w, cw)
    # the last view alone carries another weight: the second mask word reads its own pixels' weights
    w2 = w.copy()
    w2[64] = np.float32(1.7)
    assert not np.array_equal(WR.integrate_scene(scene, w2, cw)['weight'], WR.integrate_scene(scene, w, cw)['weight'])
    _check(ops, scene, w2, cw)


# -------------------------------------------------------------------------------------------------------------------- the identities
@pytest.mark.parametrize('cw', CARVE)
def test_a_mask_as_weights_is_the_depths_zeroed_by_the_mask(ops, cw):
    scene = WR.floater()
    cams28, nd, _ = WR.scene_count('floater')
    got = ops.fusion_support(_dev(cams28), _dev(nd), WR.DISP_THRESHOLD, WR.FAKE_NORMAL_THRESHOLD, 2, want=('count', 'depth'))
    mask = (got['count'] >= 2).to(torch.float32)
    assert 0 < int(mask.sum()) < mask.numel()
    by_weight = ops.tsdf_integrate(_dev(scene.depths), _dev(scene.cams), scene.voxel, scene.trunc, scene.origin, scene.dims,
                                   images=_dev(scene.images), carve_weight=cw, weights=mask)
    by_depth = ops.tsdf_integrate(got['depth'], _dev(scene.cams), scene.voxel, scene.trunc, scene.origin, scene.dims,
                                  images=_dev(scene.images), carve_weight=cw)
    _same_bits(by_weight, by_depth)
    assert by_weight.num_blocks < _integrate(ops, scene, None, cw).num_blocks        # the blob's blocks are gone


def test_a_block_whose_samples_all_have_weight_0_is_absent(ops):
    scene = WR.ring()
    w = np.ones(scene.depths.shape, np.float32)
    w[3] = 0
    w[:, :, :scene.depths.shape[2] // 2] = 0
    want = WR.integrate_scene(scene, w)
    assert 0 < len(want['blocks']) < len(scene.plain['blocks'])
    vol = _check(ops, scene, w, None)
    assert vol.num_blocks == len(want['blocks'])
    assert bool((vol.weight.reshape(vol.num_blocks, -1) > 0).any(dim=1).all())
    # every weight 0: no block at all, with the arrays a volume always has
    empty = _integrate(ops, scene, np.zeros(scene.depths.shape, np.float32), 0.5)
    assert empty.num_blocks == 0 and tuple(empty.free.shape) == (0, 8, 8, 8) and tuple(empty.color.shape) == (0, 8, 8, 8, 3)


def test_the_arguments_are_checked_before_any_launch(ops):
    scene = WR.ring()
    with pytest.raises(ValueError, match='weights'):
        _integrate(ops, scene, np.ones(scene.depths.shape[1:], np.float32), None)
    with pytest.raises(TypeError, match='weights'):
        _integrate(ops, scene, np.ones(scene.depths.shape, np.float64), None)
    with pytest.raises(RuntimeError, match='weights'):
        ops.tsdf_integrate(_dev(scene.depths), _dev(scene.cams), scene.voxel, scene.trunc, scene.origin, scene.dims,
                           weights=torch.ones(scene.depths.shape))
