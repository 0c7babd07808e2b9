"""CPU: the conditions tests/test_gpu_geometry.py relies on, pinned on the oracle alone, so that an edit of
tests/geometry_cases.py cannot hollow the GPU tests out; and the oracle's metric-depth branch (INVERSE_DEPTH = False) held
against its inverse-depth one in float64 before any kernel is compared with it.
"""
import pytest
import torch

import geometry_cases as GC
from oracle import homography_warping as G
from oracle import model as OM


def _feat(h, w, C, seed):
    return torch.randn(1, h, w, C, generator=torch.Generator().manual_seed(seed))


def _nontrivial(t, what):
    bad = int(((t == 0) | (t == 1)).sum())
    assert bad == 0, '%s has %d entries that are exactly 0 or 1' % (what, bad)


def _pose_nontrivial(left, right, what):
    mat, vec = G._relative_pose(left, right)
    _nontrivial(mat[:, :2], what + ' mat')
    # K's last row (0, 0, 1) makes mat's last row R_r R_l^T K_l^-1's: still full, since K^-1 has a full last column
    _nontrivial(mat[:, 2], what + ' mat row 2')
    _nontrivial(vec, what + ' vec')


@pytest.mark.parametrize('h,w,D', GC.WARP_SHAPES)
def test_general_cams_fill_every_entry_and_both_mask_values(h, w, D):
    """No entry of H[d] or of (mat, vec) is exactly 0 or 1, for every pair of the four views and both directions; the bilinear,
    nearest and per-pixel-depth masks of the pair (0, 1) hold valid and invalid samples (0.05 < share < 1) in both directions."""
    cams = GC.general_cams(4, h, w, D)
    ds, di = OM.depth_start_interval(cams)
    for a in range(4):
        for b in range(4):
            if a != b:
                _nontrivial(G.get_homographies(cams[:, a], cams[:, b], D, ds, di), 'H %d->%d' % (a, b))
                _pose_nontrivial(cams[:, a], cams[:, b], 'pose %d->%d' % (a, b))
    src = _feat(h, w, 1, 1)
    depth = GC.inverse_map(h, w, 3)[None, ..., None]
    for a, b in ((0, 1), (1, 0)):
        H = G.get_homographies(cams[:, a], cams[:, b], D, ds, di)
        for method in ('bilinear', 'nearest'):
            m = torch.stack([G.homography_warping(src, H[:, d], method=method, output_mask=True)[1] for d in range(D)])
            assert 0.05 < float(m.float().mean()) < 1.0, (a, b, method)
        m = G.homography_warping_by_depth(src, cams[:, a], cams[:, b], depth, output_mask=True)[1]
        assert 0.05 < float(m.float().mean()) < 1.0, (a, b)


@pytest.mark.parametrize('h,w,D', GC.METRIC_SHAPES)
def test_metric_range_keeps_both_mask_values(monkeypatch, h, w, D):
    assert (h, w, D) in GC.WARP_SHAPES
    cams = GC.general_cams(2, h, w, D)
    ds, di = GC.metric_range(*OM.depth_start_interval(cams), D)
    # the sweep covers the inverse one's scene range: 1 / (ds + D di) .. 1 / ds
    ids, idi = OM.depth_start_interval(cams)
    assert torch.allclose(ds + D * di, 1.0 / ids, rtol=1e-6) and torch.allclose(ds, 1.0 / (ids + D * idi), rtol=1e-6)
    monkeypatch.setattr(G, 'INVERSE_DEPTH', False)
    src = _feat(h, w, 1, 1)
    depth = GC.metric_map(GC.inverse_map(h, w, 3))[None, ..., None]
    for a, b in ((0, 1), (1, 0)):
        H = G.get_homographies(cams[:, a], cams[:, b], D, ds, di)
        _nontrivial(H, 'metric H %d->%d' % (a, b))
        m = torch.stack([G.homography_warping(src, H[:, d], output_mask=True)[1] for d in range(D)])
        assert 0.05 < float(m.float().mean()) < 1.0, (a, b)
        m = G.homography_warping_by_depth(src, cams[:, a], cams[:, b], depth, output_mask=True)[1]
        assert 0.05 < float(m.float().mean()) < 1.0, (a, b)


@pytest.mark.parametrize('h,w', GC.TRANSFORM_SIZES)
def test_transform_sizes_have_full_poses(h, w):
    """pose[6..8] and pose[11] of transform_depth (and the rest of the pose) are non-trivial at every size, and the transformed
    map keeps valid and masked pixels."""
    cams = GC.general_cams(2, h, w, 2)
    _pose_nontrivial(cams[:, 1], cams[:, 0], 'pose 1->0')
    d = GC.transform_map(h, w, 5)
    assert bool((d > 0).any())
    fwd = G.transform_depth(d[None, ..., None], cams[:, 1], cams[:, 0])
    assert bool(torch.isfinite(fwd).all()) and float(fwd.max()) > 0.0
    assert bool((fwd[0, ..., 0] == 0).eq(d == 0).all())


@pytest.mark.parametrize('h,w', GC.BACKWARDS_SIZES)
def test_a_backwards_camera_sees_negative_depths_only(monkeypatch, h, w):
    """Into backwards_cam every transformed z is negative, so its maximum is (the unsigned-atomicMin branch of the kernels' float
    maximum, a negative upper bound in the clip), and the inverse-mode output is finite and nowhere positive."""
    cams = GC.general_cams(2, h, w, 2)
    back = GC.backwards_cam(cams[:, 0])
    assert (h, w) in GC.TRANSFORM_SIZES
    _pose_nontrivial(cams[:, 1], back, 'pose 1->backwards')
    d = GC.transform_map(h, w, 5)
    out = G.transform_depth(d[None, ..., None], cams[:, 1], back)
    assert bool(torch.isfinite(out).all()) and float(out.max()) <= 0.0 and -100.0 < float(out.min()) < -10.0
    # the transformed z itself: the metric branch is the bare transform (no clip, no mask), here of the reciprocals
    monkeypatch.setattr(G, 'INVERSE_DEPTH', False)
    z = G.transform_depth(torch.where(d > 0, 1.0 / d, torch.zeros(()))[None, ..., None], cams[:, 1], back)
    assert float(z.max()) < 0.0


def test_degenerate_homographies_hit_the_zero_guard_the_sign_change_and_the_overflow():
    """The table of the planes' properties at 17 x 23, on the oracle."""
    h, w = GC.DEGENERATE_HW
    H = GC.degenerate_homographies()
    assert H.shape == (1, 4, 3, 3) and H.dtype == torch.float32
    px, py = G.get_pixel_grids(h, w)
    src = _feat(h, w, 4, 2)
    #        dv == 0, dv < 0 share, valid share, bilinear NaN
    table = [(17, 0.435, 0.281, False), (23, 0.471, 0.322, False), (0, 0.0, 0.0, True), (0, 0.0, 0.857, False)]
    for p, (zeros, neg, valid, nan) in enumerate(table):
        r = H[0, p, 2]
        dv = (r[0] * px + r[1] * py) + r[2]
        assert int((dv == 0).sum()) == zeros
        assert abs(float((dv < 0).float().mean()) - neg) < 5e-4
        ob, mb = G.homography_warping(src, H[:, p], output_mask=True)
        on, mn = G.homography_warping(src, H[:, p], method='nearest', output_mask=True)
        assert torch.equal(mb, mn) and abs(float(mb.float().mean()) - valid) < 5e-4
        assert bool(torch.isnan(ob).all()) if nan else bool(torch.isfinite(ob).all())
        assert bool(torch.isfinite(on).all())
    dv0 = ((H[0, 0, 2, 0] * px + H[0, 0, 2, 1] * py) + H[0, 0, 2, 2]).reshape(h, w)
    assert bool((dv0[:, 10] == 0).all()) and bool((dv0[:, :10] < 0).all()) and bool((dv0[:, 11:] > 0).all())
    dv1 = ((H[0, 1, 2, 0] * px + H[0, 1, 2, 1] * py) + H[0, 1, 2, 2]).reshape(h, w)
    assert bool((dv1[8] == 0).all()) and bool((dv1[9:] < 0).all()) and bool((dv1[:8] > 0).all())
    on = G.homography_warping(src, H[:, 2], method='nearest')
    assert torch.equal(on[0], src[0, 0, 0].expand(h, w, 4))          # every pixel invalid -> pixel (0,0), not masked


def _f64(*ts):
    return [t.double() for t in ts]


@pytest.mark.parametrize('h,w', [(24, 40), (9, 11)])
def test_oracle_metric_branch_is_the_inverse_one_on_reciprocal_depths(monkeypatch, h, w):
    """INVERSE_DEPTH = False against INVERSE_DEPTH = True on the reciprocal depths, float64 inputs, 1e-12 relative (float64
    rounding of a handful of operations; a wrong branch is off by O(1)): get_homographies plane by plane, the sampling
    coordinates of homography_warping_by_depth, transform_depth (reciprocal of the inverse-mode output; every depth valid and
    inside the clip range, so the inverse-mode clips are the identity).  The four `if FLAGS.inverse_depth` sites of the reference
    (homography_warping.py:149, 215, 301 / 321, 369 / 378) read against the oracle: multiply <-> divide at the first two, the
    clip / reciprocal / mask blocks skipped at the third; the fourth (the hull's comparison direction) is a comparison, checked
    by its truth table below."""
    D = 6
    cams = GC.general_cams(2, h, w, D)
    ds, di = OM.depth_start_interval(cams)
    ds_m, di_m = GC.metric_range(ds, di, D)
    c0, c1, ds_m, di_m = _f64(cams[:, 0], cams[:, 1], ds_m, di_m)
    inv = GC.inverse_map(h, w, 3).double()[None, ..., None]
    met = 1.0 / inv
    src = _feat(h, w, 2, 4).double()
    seen = []
    real = G.interpolate

    def spy(image, x, y, **kw):
        seen.append((x, y))
        return real(image, x, y, **kw)
    monkeypatch.setattr(G, 'interpolate', spy)

    def rel(a, b):
        r = float(((a - b).abs() / b.abs()).max())
        return r

    assert G.INVERSE_DEPTH is True
    planes = [ds_m + k * di_m for k in range(D)]
    H_inv = [G.get_homographies(c0, c1, 1, 1.0 / p, di_m)[0, 0] for p in planes]
    G.homography_warping_by_depth(src, c0, c1, inv)
    td_inv = G.transform_depth(inv, c1, c0)
    assert bool((td_inv > 0).all())
    monkeypatch.setattr(G, 'INVERSE_DEPTH', False)
    H_met = G.get_homographies(c0, c1, D, ds_m, di_m)[0]
    G.homography_warping_by_depth(src, c0, c1, met)
    td_met = G.transform_depth(met, c1, c0)
    for k in range(D):
        assert rel(H_met[k], H_inv[k]) < 1e-12
    (xi, yi), (xm, ym) = seen
    assert rel(xm, xi) < 1e-12 and rel(ym, yi) < 1e-12
    assert rel(td_met, 1.0 / td_inv) < 1e-12
    # and the metric branch is not the inverse one applied to the same numbers (the check above can tell them apart)
    monkeypatch.setattr(G, 'INVERSE_DEPTH', True)
    assert rel(G.get_homographies(c0, c1, D, ds_m, di_m)[0], H_met) > 1e-3


def test_oracle_hull_compares_towards_the_camera_in_both_parameterisations(monkeypatch):
    """get_visual_hull's two comparisons (reference :369-372, :378-381): a voxel counts for a view when it lies BEHIND that view's
    surface -- depth > surface in metric depth, inverse depth < the surface's.  The same scene in both parameterisations,
    planes strictly between the map's values, gives the same hull."""
    h, w, D = 8, 10, 5
    cams = GC.general_cams(2, h, w, D)
    inv = torch.stack([GC.inverse_map(h, w, 1), GC.inverse_map(h, w, 2)])[None]
    ds, di = torch.tensor([0.0613]), torch.tensor([0.0571])
    hull_i = G.get_visual_hull(inv, cams, D, ds, di, view_num=1)
    assert 0.0 < float(hull_i.mean()) < 1.0
    monkeypatch.setattr(G, 'INVERSE_DEPTH', False)
    for d in range(D):
        plane = 1.0 / (ds + d * di)
        hull_m = G.get_visual_hull(1.0 / inv, cams, 1, plane, di, view_num=1)
        assert torch.equal(hull_m[:, 0], hull_i[:, d])
