"""CPU: what tests/test_gpu_real_cams.py relies on, pinned on the oracle alone -- that the reference's real 5-view cameras
(tests/real_cams.py), scaled to a 24x40 map with 16 planes, are the hard inputs they are meant to be, and that the checked-in
evaluation (tests/golden/make_real_cams_golden.py) is current and a float64-class reference.
"""
import numpy as np
import pytest
import torch

import real_cams as RC
from oracle import homography_warping as G
from oracle import model as OM
from oracle import nets

SCENES = (0, 1)


def _nontrivial(t, what):
    bad = int(((t == 0) | (t == 1)).sum())
    assert bad == 0, '%s has %d entries that are exactly 0 or 1' % (what, bad)


@pytest.fixture(scope='module')
def forced():
    """{scene: (images, cams, fixture, (depth_agg_init, depth_views, prob_volume_agg, cost_volume_agg) as the oracle takes them)}"""
    out = {}
    for s in SCENES:
        imgs, cams = RC.inputs(s)
        fx = RC.load(s)
        t = lambda k: torch.from_numpy(fx[k])                            # noqa: E731
        dv = [t('depth_views')[i][None, ..., None] for i in range(cams.shape[1] - 1)]
        out[s] = (imgs, cams, fx, (t('depth_agg_init')[None, ..., None], dv, t('prob_volume_agg')[None], t('cost_volume_agg')[None]))
    return out


@pytest.mark.parametrize('scene', SCENES)
def test_the_cameras_are_the_shipped_ones_scaled(scene):
    raw = RC.raw_cams(scene)
    assert raw.shape == (5, 2, 4, 4) and raw.dtype == np.float64
    c = RC.cams(scene, RC.H, RC.W, RC.D, RC.VIEWS[scene])
    ids = RC.VIEWS[scene] or list(range(5))
    assert c.shape == (1, len(ids), 2, 4, 4) and c.dtype == torch.float32
    for i, v in enumerate(ids):
        assert torch.equal(c[0, i, 0], torch.from_numpy(raw[v, 0].astype(np.float32)))            # the pose is untouched
        K = c[0, i, 1, :3, :3].double().numpy()
        assert np.allclose(K[0], raw[v, 1, 0, :3] * RC.W / 240.0, rtol=1e-6) and np.allclose(K[1], raw[v, 1, 1, :3] * RC.H / 160.0, rtol=1e-6)
        assert K[0, 0] != K[1, 1]                                                               # fx != fy after scaling
        assert np.isclose(float(c[0, i, 1, 3, 1]) * RC.D, raw[v, 1, 3, 1] * 128.0, rtol=1e-6)   # D planes span the scene's range
    starts = [float(raw[v, 1, 3, 0]) for v in range(5)]
    assert len(set(starts)) == 5 and max(starts) > 1.3 * min(starts)                            # a depth_start per view (C11)
    # unscaled: the cameras' own grid
    own = RC.cams(scene, 160, 240, 128)
    assert torch.equal(own[0], torch.from_numpy(raw.astype(np.float32)))
    # a selection reorders
    sel = RC.cams(scene, RC.H, RC.W, RC.D, [0, 3, 4])
    assert torch.equal(sel[0, 1], RC.cams(scene, RC.H, RC.W, RC.D)[0, 3])


@pytest.mark.parametrize('scene', SCENES)
def test_homographies_are_full_and_the_sweeps_leave_the_image(scene):
    """No structural 0 or 1 in any homography of any pair, either direction; per source a share of valid warp samples between 0.3
    and 0.8 (synthetic.make_cams: 0.91 to 0.93), all five views of the scene."""
    h, w, D = RC.H, RC.W, RC.D
    cams = RC.cams(scene, h, w, D)
    ds, di = OM.depth_start_interval(cams)
    for a in range(5):
        for b in range(5):
            if a != b:
                _nontrivial(G.get_homographies(cams[:, a], cams[:, b], D, ds, di), 'scene %d H %d->%d' % (scene, a, b))
    src = torch.randn(1, h, w, 1, generator=torch.Generator().manual_seed(1))
    for v in range(1, 5):
        H = G.get_homographies(cams[:, 0], cams[:, v], D, ds, di)
        m = torch.stack([G.homography_warping(src, H[:, d], output_mask=True)[1] for d in range(D)])
        share = float(m.float().mean())
        print('scene %d source %d: valid warp samples %.3f' % (scene, v, share))
        assert 0.3 < share < 0.8, (scene, v, share)
    from atvsnet_amd import synthetic
    syn = torch.from_numpy(synthetic.make_cams(5, 4 * h, 4 * w, D))[None]
    sds, sdi = OM.depth_start_interval(syn)
    for v in range(1, 5):
        H = G.get_homographies(syn[:, 0], syn[:, v], D, sds, sdi)
        m = torch.stack([G.homography_warping(src, H[:, d], output_mask=True)[1] for d in range(D)])
        assert float(m.float().mean()) > 0.8


@pytest.mark.parametrize('scene', SCENES)
def test_refinement_inputs_hold_zeros_and_a_mixed_hull(forced, weights, scene):
    """On the fixture's forced stage inputs, per source: exact zeros in 0.2 to 0.7 of photo_group[..., :16] (masked samples); a hull
    that holds each of its values (0, 1/2, 1: behind the surface of neither, one or both of its two views) and marks 0.6 to 0.85
    of the voxels (non-zero; 0.47 to 0.51 of them are exactly 1); and for a source >= 2 the hull is not the one its own camera
    gives."""
    imgs, cams, fx, (dinit, dviews, prob, _) = forced[scene]
    D = RC.D
    ds, di = OM.depth_start_interval(cams)
    n = cams.shape[1]
    shallow = [nets.resnet_ds2_spp_shallow_f16(imgs[:, v], weights) for v in range(n)]
    for v in range(1, n):
        init = torch.stack([dinit, dviews[v - 1]], 1)
        inp = OM.refinement_inputs(init, cams, D, ds, di, None, prob, None, 0, v, shallow=(shallow[0], shallow[v]))
        zeros = float((inp['photo_group'][..., :16] == 0).float().mean())
        hull = inp['vis_hull']
        marked, ones = float((hull > 0).float().mean()), float((hull == 1).float().mean())
        print('scene %d source %d: photo zeros %.3f, hull marked %.3f, exactly one %.3f' % (scene, v, zeros, marked, ones))
        assert 0.2 < zeros < 0.7, (scene, v, zeros)
        assert sorted(set(hull.reshape(-1).tolist())) == [0.0, 0.5, 1.0]
        assert 0.6 < marked < 0.85, (scene, v, marked, ones)
        if v >= 2:
            own = torch.stack([cams[:, 0], cams[:, v]], 1)
            h_own = G.get_visual_hull(init.squeeze(-1), own, D, ds, di, ref_id=0, view_num=2)
            assert not torch.equal(h_own, hull), (scene, v)


@pytest.mark.parametrize('scene', SCENES)
def test_fixture_is_current_and_its_float64_values_are_a_reference(forced, weights, scene):
    """Re-running the float32 oracle's forced refinement of the last source (a source >= 2) reproduces the stored evaluation: it is
    within 1e-5 of the stored float64 volume, the bar of every e32 below, and so within 2e-5 of the stored float32 one (a stale
    fixture -- other cameras, weights, images or stage inputs -- is off by 1e-2 and more).  Not bit for bit: the oracle's
    convolutions sum in an order that depends on the CPU thread count (2e-6 to 5e-6 of these volumes between 1, 3 and 8 threads).
    The float32 oracle is within 1e-5 of every stored float64 volume and 1e-6 of the forced final depth (measured: 3e-6 and
    3e-7), so the float64 values are what float32-class evaluations scatter around."""
    imgs, cams, fx, inputs = forced[scene]
    n = cams.shape[1]
    rc, _, _, _ = RC.forced_refinement(imgs, cams, weights, RC.D, *inputs, sources=[n - 1])
    again64 = RC.vol_dist(rc[0][0], fx['refined_cost64_%d' % (n - 1)])
    again32 = RC.vol_dist(rc[0][0], fx['refined_cost32_%d' % (n - 1)])
    print('scene %d re-run of source %d: %.3e from the stored float64 volume, %.3e from the stored float32 one' % (scene, n - 1, again64, again32))
    assert again64 <= 1e-5 and again32 <= 2e-5
    vols = ['cost_volume_agg', 'prob_volume_agg', 'refined_cost_volume_agg', 'refined_prob_volume_agg'] + \
        ['refined_cost_%d' % v for v in range(1, n)]
    for k in vols:
        print('scene %d e32_%s %.3e' % (scene, k, float(fx['e32_' + k])))
        assert 0.0 < float(fx['e32_' + k]) <= 1e-5, k
    assert 0.0 < float(fx['e32_depth_final']) <= 1e-6
    for k in ['depth_agg_init', 'depth_views'] + ['depth_views_%d' % v for v in range(1, n)]:
        assert 0.0 < float(fx['e32_' + k]) <= 1e-5, k
    # the stored float32 stage is within its own e32 of the stored float64 one (the file is consistent with itself)
    for k in ('cost_volume_agg', 'prob_volume_agg'):
        assert abs(RC.vol_dist(fx[k], fx[k + '64']) - float(fx['e32_' + k])) <= 1e-7
    assert fx['depth_final64'].shape == (4 * RC.H, 4 * RC.W) and fx['depth_views'].shape == (n - 1, RC.H, RC.W)
