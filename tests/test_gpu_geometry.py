"""-m gpu: geometry + soft-argmin HIP kernels (through the C-ABI) vs the CPU oracle.

Geometry is integer/index work plus fixed-order fp32 arithmetic -> BIT-EXACT bar
(built with -ffp-contract=off; oracle uses the same operation order).
Camera families: 'synthetic' (synthetic.make_cams: identity reference camera, rotation about y, shift along x, fx = fy, no skew --
half of every homography and pose is exact zeros and ones), 'example2' (the golden cameras, homographies only) and 'general'
(tests/geometry_cases.py: every entry of H and of the relative pose in play); hand-made degenerate homographies (an exactly zero
and a sign-changing denominator, an overflow) go straight to the launches.  Depth parameterisations: inverse depth (the path's
setting) and metric depth (inverse_depth=False against the oracle under INVERSE_DEPTH = False).  transform_depth: the
one-workgroup kernel at its item, carry and width edges, and the general path above 32,768 pixels.
tests/test_geometry_cases_host.py pins what these inputs must have (on the CPU oracle) and the oracle's metric branch.
Soft-argmin uses expf -> tolerance 2e-6 relative, here against the FLOAT32 oracle (which is itself up to 1.6e-6
from a float64 evaluation at these depth counts) and at a few shapes; tests/test_gpu_depth_regression.py holds the
same kernels element by element to a float64 reference (2e-6 * sum_d p_d |v_d|), at every chunk, tile and scale edge.
"""
import numpy as np
import pytest
import torch

import geometry_cases as GC
import numerics as N
from oracle import homography_warping as G
from oracle import model as OM

pytestmark = pytest.mark.gpu


def _example_cams(views=2):
    from atvsnet_amd import synthetic
    cams = synthetic.make_cams(views, 128, 160, 32)
    return torch.from_numpy(cams)[None]          # (1,N,2,4,4)


def _golden_cams():
    import os
    d = os.path.join(os.path.dirname(__file__), 'golden')
    c = np.stack([np.load(os.path.join(d, 'example2_%d_cam.npy' % i)) for i in range(2)]).astype(np.float32)
    return torch.from_numpy(c)[None]


def _cams(family, h, w, D, views=2):
    """The camera family of a test: (1, views, 2, 4, 4).  The synthetic intrinsics are for 32x40 whatever the map's size."""
    if family == 'synthetic':
        return _example_cams(views)
    assert (h, w, D) in GC.WARP_SHAPES            # pinned by tests/test_geometry_cases_host.py
    return GC.general_cams(views, h, w, D)


def _both(shapes):
    """Every shape with both camera families; the synthetic cases keep the ids they had before the family was a parameter."""
    out = []
    for s in shapes:
        tag = '-'.join(str(v) for v in s)
        out += [pytest.param('synthetic', *s, id=tag), pytest.param('general', *s, id='general-' + tag)]
    return out


def _same(got, want):
    """Bit equality where NaN can occur: equal, or NaN on both sides (inf * 0 of tf.multiply)."""
    got, want = got.cpu(), want.cpu()
    return got.shape == want.shape and bool(((got == want) | (torch.isnan(got) & torch.isnan(want))).all())


@pytest.mark.parametrize('which', ['synthetic', 'example2', 'general'])
@pytest.mark.parametrize('D', [1, 32, 192])
def test_homographies_bit_exact(cuda, which, D):
    from atvsnet_amd import ops
    cams = _golden_cams() if which == 'example2' else _cams(which, 32, 40, D)
    ds, di = OM.depth_start_interval(cams)
    for a, b in ((0, 1), (1, 0)):
        want = G.get_homographies(cams[:, a], cams[:, b], D, ds, di)[0]
        got = ops.get_homographies(cams[0, a].to(cuda).contiguous(), cams[0, b].to(cuda).contiguous(),
                                   ds.to(cuda), di.to(cuda), D).cpu()
        assert torch.equal(got, want)


def _feat(h, w, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, h, w, C, generator=g)


@pytest.mark.parametrize('cams,h,w,C,D', _both([(32, 40, 32, 32), (30, 36, 16, 8), (17, 23, 4, 5), (32, 40, 1, 16), (9, 11, 3, 4)]))
def test_warp_planes_bit_exact(cuda, cams, h, w, C, D):
    from atvsnet_amd import ops
    cams = _cams(cams, h, w, D)
    # intrinsics are for 32x40; other sizes simply sample more out-of-range pixels (exercises the masks)
    ds, di = OM.depth_start_interval(cams)
    H = G.get_homographies(cams[:, 0], cams[:, 1], D, ds, di)
    src = _feat(h, w, C, 1)
    want = torch.stack([G.homography_warping(src, H[:, d])[0] for d in range(D)])
    wm = torch.stack([G.homography_warping(src, H[:, d], output_mask=True)[1][0, ..., 0] for d in range(D)])
    got, mask = ops.warp_planes(src[0].to(cuda), H[0].to(cuda), want_mask=True)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(mask.cpu(), wm.to(torch.float32))
    assert 0.05 < wm.float().mean() < 1.0          # both valid and invalid samples are present


@pytest.mark.parametrize('cams,h,w,C,D', _both([(32, 40, 32, 8), (17, 23, 4, 5), (32, 40, 1, 16), (9, 11, 3, 4)]))
def test_homography_warping_nearest_bit_exact(cuda, cams, h, w, C, D):
    """homography_warping(method='nearest') through the reference-named face (reference homography_warping.py:45-56,
    230-271): tf.round sampling, out-of-range pixels read pixel (0,0) and are NOT zeroed (quirk C4)."""
    from atvsnet_amd.atvsnet import homography_warping as HW
    cams = _cams(cams, h, w, D)
    ds, di = OM.depth_start_interval(cams)
    H = G.get_homographies(cams[:, 0], cams[:, 1], D, ds, di)
    src = _feat(h, w, C, 7)
    want = torch.stack([G.homography_warping(src, H[:, d], method='nearest')[0] for d in range(D)])
    wm = torch.stack([G.homography_warping(src, H[:, d], method='nearest', output_mask=True)[1][0] for d in range(D)])
    got, mask = HW.homography_warping(src.to(cuda), H.to(cuda), method='nearest', output_mask=True)
    assert got.shape == (1, D, h, w, C) and mask.shape == (1, D, h, w, 1) and mask.dtype == torch.bool
    assert torch.equal(got[0].cpu(), want)
    assert torch.equal(mask[0].cpu(), wm)
    inv = ~wm[..., 0]
    assert inv.any() and torch.equal(want[inv], src[0, 0, 0].expand_as(want[inv]))      # un-masked pixel (0,0)
    # single homography (B,3,3), no mask: the reference's plain call form
    one = HW.homography_warping(src.to(cuda), H[:, 1].to(cuda), method='nearest')
    assert torch.equal(one[0].cpu(), want[1])
    with pytest.raises(ValueError):
        HW.homography_warping(src.to(cuda), H[:, 1].to(cuda), method='cubic')


@pytest.mark.parametrize('cams', ['synthetic', 'general'])
def test_cost_volume_bit_exact(cuda, cams):
    from atvsnet_amd import ops
    D, h, w, C = 32, 32, 40, 32
    cams = _cams(cams, h, w, D)
    ds, di = OM.depth_start_interval(cams)
    rf, vf = _feat(h, w, C, 2), _feat(h, w, C, 3)
    want = OM.build_cost_volume(rf, vf, cams, D, ds, di, 0, 1)[0]
    H = ops.get_homographies(cams[0, 0].to(cuda), cams[0, 1].to(cuda), ds.to(cuda), di.to(cuda), D)
    got = ops.build_cost_volume(rf[0].to(cuda), vf[0].to(cuda), H)
    assert torch.equal(got.cpu(), want)
    # reverse direction (model.py:413, quirk C11)
    want = OM.build_cost_volume(vf, rf, cams, D, ds, di, 1, 0)[0]
    H = ops.get_homographies(cams[0, 1].to(cuda), cams[0, 0].to(cuda), ds.to(cuda), di.to(cuda), D)
    got = ops.build_cost_volume(vf[0].to(cuda), rf[0].to(cuda), H)
    assert torch.equal(got.cpu(), want)


def test_identity_camera_warp(cuda):
    """Known answer: identity pose -> identity away from the last row/col, which go to 0."""
    from atvsnet_amd import ops
    cams = _example_cams()
    ds, di = OM.depth_start_interval(cams)
    src = _feat(12, 20, 8, 5)[0]
    H = ops.get_homographies(cams[0, 0].to(cuda), cams[0, 0].to(cuda), ds.to(cuda), di.to(cuda), 3)
    out = ops.warp_planes(src.to(cuda), H).cpu()
    for d in range(3):
        assert torch.allclose(out[d, :-1, :-1], src[:-1, :-1], atol=1e-5)
        assert torch.all(out[d, -1] == 0) and torch.all(out[d, :, -1] == 0)


@pytest.mark.parametrize('cams', ['synthetic', 'general'])
def test_refinement_volumes_bit_exact(cuda, cams):
    """photo / geo / visual-hull volumes and the D-constant maps of model.py:270-336."""
    from atvsnet_amd import ops
    D, h, w = 16, 32, 40
    cams = _cams(cams, h, w, D)
    ds, di = OM.depth_start_interval(cams)
    g = torch.Generator().manual_seed(7)
    ref_f, view_f = _feat(h, w, 16, 11), _feat(h, w, 16, 12)
    d_ref = 0.05 + 0.3 * torch.rand(1, h, w, 1, generator=g)
    d_view = 0.05 + 0.3 * torch.rand(1, h, w, 1, generator=g)
    d_view[0, :3, :5] = 0.0                       # invalid depths exercise the 1e-10 clip / mask
    init = torch.stack([d_ref, d_view], 1)
    prob = torch.randn(1, D, h, w, generator=g)
    want = OM.refinement_inputs(init, cams, D, ds, di, None, prob, None, 0, 1, shallow=(ref_f, view_f))

    c = lambda t: t.to(cuda).contiguous()
    ref_cam, view_cam = c(cams[0, 0]), c(cams[0, 1])
    dsg, dig = c(ds), c(di)
    H = ops.get_homographies(ref_cam, view_cam, dsg, dig, D)
    vtrans = ops.transform_depth(c(d_view[0, ..., 0]), view_cam, ref_cam)
    assert torch.equal(vtrans.cpu(), G.transform_depth(d_view, cams[:, 1], cams[:, 0])[0, ..., 0])

    photo = torch.empty(D, h, w, 48, device=cuda)
    ops.warp_planes(c(view_f[0]), H, out=photo, c_off=0, mode=1, ref=c(ref_f[0]))
    wf, mp = ops.warp_by_depth(c(view_f[0]), ref_cam, view_cam, c(d_ref[0, ..., 0]))
    from atvsnet_amd import ops as O
    perr = O.absdiff_mask(wf, c(ref_f[0]), mp)
    ops.tile_planes(perr, photo, 16)
    ops.tile_planes(c(ref_f[0]), photo, 32)
    assert torch.equal(photo.cpu(), want['photo_group'][0])

    geo = torch.empty(D, h, w, 19, device=cuda)
    ops.geo_ref_planes(c(d_ref[0, ..., 0]), dsg, dig, geo, 0)
    ops.warp_planes(vtrans.reshape(h, w, 1), H, out=geo, c_off=1, mode=2, depth_start=dsg, depth_interval=dig, rep=16)
    wd, mg = ops.warp_by_depth(vtrans.reshape(h, w, 1), ref_cam, view_cam, c(d_ref[0, ..., 0]), method='nearest')
    gerr = O.absdiff_mask(wd, c(d_ref[0]), mg)
    ops.tile_planes(gerr, geo, 17)
    ops.tile_planes(c(d_ref[0]), geo, 18)
    assert torch.equal(geo.cpu(), want['geo_group'][0])

    hull = ops.visual_hull(c(d_ref[0, ..., 0]), vtrans, H, dsg, dig)
    assert torch.equal(hull.cpu(), want['vis_hull'][0, ..., 0])


@pytest.mark.parametrize('cams', ['synthetic', 'general'])
def test_refinement_glue_launches_equal_their_parts_bitwise(cuda, cams):
    """The refinement's fused / batched geometry launches (round 5) against the launches they replace, bit for bit:
    atvs_geo_volume = geo_ref_planes + warp_planes(mode 2) (reference atvsnet/model.py:285-300), rep 1 (one 8-byte store per voxel)
    and rep 16 (the reference's replicated channel, quirk C7); atvs_transform_depth_batch = n x transform_depth (:289,321-324) for
    more maps than one launch holds (18 > 16), distinct cameras per map, invalid depths; atvs_warp_by_depth_err with copy_ref =
    warp_by_depth + absdiff_mask + the tiled reference (:309-316,329-334).  The batched transform also against the oracle's
    transform_depth, map by map (with the general cameras every pose entry it reads is in play)."""
    from atvsnet_amd import ops
    D, h, w = 12, 24, 40
    cams = _cams(cams, h, w, D, views=4)
    ds, di = OM.depth_start_interval(cams)
    g = torch.Generator().manual_seed(17)
    c = lambda t: t.to(cuda).contiguous()                       # noqa: E731
    cam = [c(cams[0, i]) for i in range(4)]
    dsg, dig = c(ds), c(di)
    d_ref = c(0.05 + 0.3 * torch.rand(h, w, generator=g))
    maps = []
    for k in range(18):
        m = 0.05 + 0.3 * torch.rand(h, w, generator=g)
        m[k % h, : 1 + k % 5] = 0.0                              # invalid depths: the 1e-10 clip / mask
        maps.append(c(m))
    jobs = [(maps[k], cam[1 + k % 3], cam[(k // 3) % 4]) for k in range(18)]
    got = ops.transform_depth_batch(jobs)
    for (m, lc, rc), o in zip(jobs, got):
        assert torch.equal(o, ops.transform_depth(m, lc, rc))
    for k in range(18):
        want = G.transform_depth(maps[k].cpu()[None, ..., None], cams[:, 1 + k % 3], cams[:, (k // 3) % 4])[0, ..., 0]
        assert torch.equal(got[k].cpu(), want), k
    H = ops.get_homographies(cam[0], cam[1], dsg, dig, D)
    for ld, c_off, rep in ((2, 0, 1), (19, 0, 16), (4, 1, 2)):
        a = torch.zeros(D, h, w, ld, device=cuda)
        b = torch.zeros(D, h, w, ld, device=cuda)
        ops.geo_volume(d_ref, got[0], H, dsg, dig, a, c_off, rep)
        ops.geo_ref_planes(d_ref, dsg, dig, b, c_off)
        ops.warp_planes(got[0].reshape(h, w, 1), H, out=b, c_off=c_off + 1, mode=2, depth_start=dsg, depth_interval=dig, rep=rep)
        assert torch.equal(a, b), (ld, c_off, rep)
    for C, method in ((16, 'bilinear'), (1, 'nearest')):
        src, ref = c(torch.randn(h, w, C, generator=g)), c(torch.randn(h, w, C, generator=g))
        out = torch.zeros(h, w, 2 * C + 3, device=cuda)
        ops.warp_by_depth_err(src, ref, cam[0], cam[1], d_ref, out, 1, method, True, copy_ref=True)
        wf, mask = ops.warp_by_depth(src, cam[0], cam[1], d_ref, method=method)
        assert torch.equal(out[..., 1:1 + C], ops.absdiff_mask(wf, ref, mask))
        assert torch.equal(out[..., 1 + C:1 + 2 * C], ref)
        assert float(out[..., 0].abs().max()) == 0.0 and float(out[..., 1 + 2 * C:].abs().max()) == 0.0


@pytest.mark.parametrize('D,h,w', [(32, 32, 40), (192, 16, 24), (1, 5, 7), (7, 3, 130)])
def test_softargmin(cuda, D, h, w):
    from atvsnet_amd import ops
    g = torch.Generator().manual_seed(D)
    cost = 6.0 * torch.randn(1, D, h, w, generator=g)
    ds, di = torch.tensor([0.05]), torch.tensor([0.31 / max(D, 1)])
    want = OM.prob2depth(cost, D, ds, di)[0, ..., 0]
    got = ops.softargmin(cost[0].to(cuda), ds.to(cuda), di.to(cuda)).cpu()
    assert torch.allclose(got, want, rtol=2e-6, atol=1e-8)
    _, want_up = OM.prob2depth_upsample(cost, D, ds, di)
    got_up = ops.upsample_softargmin(cost[0].to(cuda), ds.to(cuda), di.to(cuda)).cpu()
    assert got_up.shape == (4 * h, 4 * w)
    assert torch.allclose(got_up, want_up[0, ..., 0], rtol=2e-6, atol=1e-8)


def test_softargmin_known_answers(cuda):
    """one-hot minimum -> that plane's delta; constant cost -> mid-range."""
    from atvsnet_amd import ops
    D, h, w = 16, 4, 6
    ds, di = torch.tensor([0.1], device=cuda), torch.tensor([0.02], device=cuda)
    cost = torch.full((D, h, w), 50.0, device=cuda)
    cost[5] = -50.0
    assert torch.allclose(ops.softargmin(cost, ds, di).cpu(), torch.full((h, w), 0.1 + 5 * 0.02), rtol=1e-6)
    flat = torch.zeros(D, h, w, device=cuda)
    assert torch.allclose(ops.softargmin(flat, ds, di).cpu(), torch.full((h, w), 0.1 + 7.5 * 0.02), rtol=1e-6)


def _query_points(h, w, n, seed):
    """Texture coordinates around and beyond the image, with exact half-integers (tf.round ties), the borders of the
    valid range and non-finite values."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, generator=g) * (w + 6) - 3).float()
    y = (torch.rand(n, generator=g) * (h + 6) - 3).float()
    special = torch.tensor([0.5, 1.0, 1.5, 2.0, 2.5, w - 1.0, w - 0.5, w - 0.5 - 1e-4, 0.0, 0.49999, float('nan'),
                            float('inf'), -float('inf')])
    k = special.numel()
    x[:k] = special
    y[k:2 * k] = torch.where(special == w - 1.0, torch.tensor(h - 1.0), special)
    y[2 * k] = h - 0.5
    return x, y


@pytest.mark.parametrize('method', ['bilinear', 'nearest'])
@pytest.mark.parametrize('h,w,C', [(32, 40, 32), (17, 23, 3), (9, 11, 1)])
def test_interpolate_bit_exact(cuda, method, h, w, C):
    """interpolate with caller-supplied coordinates (reference homography_warping.py:31-104) against the oracle."""
    from atvsnet_amd.atvsnet import homography_warping as HW
    img = _feat(h, w, C, 5)
    x, y = _query_points(h, w, h * w, 7)
    want, wm = G.interpolate(img, x, y, output_mask=True, method=method)
    got, gm = HW.interpolate(img.to(cuda), x.to(cuda), y.to(cuda), output_mask=True, method=method)
    assert gm.dtype == torch.bool and torch.equal(gm.cpu(), wm)
    got, want = got.cpu(), want
    same = (got == want) | (torch.isnan(got) & torch.isnan(want))      # inf * 0 = NaN on both sides (tf.multiply)
    assert bool(same.all())
    only = HW.interpolate(img.to(cuda), x.to(cuda), y.to(cuda), method=method).cpu()
    assert bool(((only == want) | (torch.isnan(only) & torch.isnan(want))).all())


def test_interpolate_on_the_pixel_grid_is_the_identity_warp(cuda):
    """get_pixel_grids -> interpolate = the image away from the last row / column (SURVEY 8c known answer 2)."""
    from atvsnet_amd.atvsnet import homography_warping as HW
    h, w, C = 12, 20, 4
    img = _feat(h, w, C, 9)
    grid = HW.get_pixel_grids(h, w)
    gx, gy = G.get_pixel_grids(h, w)
    assert grid.shape == (3 * h * w,)
    assert torch.equal(grid.cpu(), torch.cat([gx, gy, torch.ones(h * w)]))
    out = HW.interpolate(img.to(cuda), grid[:h * w], grid[h * w:2 * h * w]).cpu().reshape(h, w, C)
    assert torch.equal(out[:-1, :-1], img[0, :-1, :-1])
    assert bool((out[-1] == 0).all()) and bool((out[:, -1] == 0).all())
    near = HW.interpolate(img.to(cuda), grid[:h * w], grid[h * w:2 * h * w], method='nearest').cpu().reshape(h, w, C)
    assert torch.equal(near[:-1, :-1], img[0, :-1, :-1])
    assert torch.equal(near[-1, 3], img[0, 0, 0])                      # invalid -> pixel (0,0), not masked


def test_interpolate_refuses_what_the_reference_cannot_mean(cuda):
    from atvsnet_amd.atvsnet import homography_warping as HW
    img = _feat(4, 5, 2, 1).to(cuda)
    z = torch.zeros(20, device=cuda)
    with pytest.raises(ValueError):
        HW.interpolate(img, z, z, method='bicubic')
    with pytest.raises(ValueError):
        HW.interpolate(img, z, z[:7])
    with pytest.raises(RuntimeError):
        HW.interpolate(img.cpu(), z.cpu(), z.cpu())


# ---------------------------------------------------------------------------
# atvs_warp_planes instantiations and grids that no other test launches (general cameras)
# ---------------------------------------------------------------------------
def _oracle_planes(src, H, ref=None, method='bilinear'):
    """The oracle's warp of src (1,h,w,C) onto every plane of H (1,D,3,3) -> (values (D,h,w,C), mask (D,h,w) float32); with ref,
    the photo volume |warp - ref| * mask (reference model.py:272-279)."""
    vals, masks = [], []
    for d in range(H.shape[1]):
        v, m = G.homography_warping(src, H[:, d], method=method, output_mask=True)
        if ref is not None:
            v = torch.abs(v - ref) * m.to(v.dtype)
        vals.append(v[0])
        masks.append(m[0, ..., 0].to(torch.float32))
    return torch.stack(vals), torch.stack(masks)


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('C,D', [(16, 3), (64, 2)])
def test_warp_planes_shared_kernel_over_two_rounds_of_the_xcd_dealing(cuda, C, D, mode):
    """warp_planes_shared_kernel at 48 x 64 = 3,072 pixels: 12 workgroups of 256 pixels padded to 16, so the second round of the
    dealing over the 8 XCDs (blockIdx.x >> 3) is live -- workgroup b takes pixel block (b & 7) * 2 + (b >> 3) -- and four
    workgroups (blocks 12..15) are empty.  Plain warp and photo volume, values and mask against the oracle; for C = 16 the
    chunk-planar form and its fp16 pieces against the channel-last result, as tests/test_gpu_conv.py holds them."""
    from atvsnet_amd import ops
    h, w = 48, 64
    N.poison_allocator(cuda)                      # a pixel block no workgroup writes must not find an earlier test's values
    cams = _cams('general', h, w, D)
    ds, di = OM.depth_start_interval(cams)
    H = G.get_homographies(cams[:, 0], cams[:, 1], D, ds, di)
    src, ref = _feat(h, w, C, 21), _feat(h, w, C, 22)
    want, wm = _oracle_planes(src, H, ref if mode == 1 else None)
    assert 0.05 < float(wm.mean()) < 1.0
    kw = dict(mode=mode, ref=ref[0].to(cuda)) if mode == 1 else {}
    got, mask = ops.warp_planes(src[0].to(cuda), H[0].to(cuda), want_mask=True, **kw)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(mask.cpu(), wm)
    if C == 16:
        pl = ops.warp_planes(src[0].to(cuda), H[0].to(cuda), planar=True, **kw)
        assert tuple(pl.shape) == (C // 8, ops.planar_stride(D, h, w))
        x = ops.planar_view(pl, D, h, w)                                            # (K, D, h, w, 8)
        assert torch.equal(x.permute(1, 2, 3, 0, 4).reshape(D, h, w, C), got)
        pc = ops.warp_planes(src[0].to(cuda), H[0].to(cuda), planar=True, pieces=True, **kw)
        assert pc.shape == pl.shape and pc.dtype == torch.float32
        x = x.cpu().numpy()
        halves = pc[..., :D * h * w * 8].contiguous().view(torch.float16).cpu().numpy().reshape(C // 8, 2, D, h, w, 8)
        h0 = x.astype(np.float16)
        h1 = ((x - h0.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
        assert np.array_equal(halves[:, 0].view(np.uint16), h0.view(np.uint16))
        assert np.array_equal(halves[:, 1].view(np.uint16), h1.view(np.uint16))


@pytest.mark.parametrize('h,w,C,D', [(17, 23, 8, 5), (9, 11, 3, 4)])
def test_photo_volume_gather_kernels_bit_exact(cuda, h, w, C, D):
    """Mode 1 outside the shared kernel: warp_planes_kernel<1,4> (C % 4 == 0, C not in {16, 32, 64}) and <1,1> (C % 4 != 0)."""
    from atvsnet_amd import ops
    cams = _cams('general', h, w, D)
    ds, di = OM.depth_start_interval(cams)
    H = G.get_homographies(cams[:, 0], cams[:, 1], D, ds, di)
    src, ref = _feat(h, w, C, 23), _feat(h, w, C, 24)
    want, wm = _oracle_planes(src, H, ref)
    assert 0.05 < float(wm.mean()) < 1.0
    got, mask = ops.warp_planes(src[0].to(cuda), H[0].to(cuda), mode=1, ref=ref[0].to(cuda), want_mask=True)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(mask.cpu(), wm)


def test_photo_volume_at_an_odd_channel_offset_takes_the_scalar_kernel(cuda):
    """Mode 1, C = 16 written at c_off = 2 of an ld = 20 buffer: the offset is no multiple of 4, so the launch is
    warp_planes_kernel<1,1> although C alone would take the shared kernel.  The channels outside [2, 18) keep their bits."""
    from atvsnet_amd import ops
    h, w, C, D = 17, 23, 16, 5
    cams = _cams('general', h, w, D)
    ds, di = OM.depth_start_interval(cams)
    H = G.get_homographies(cams[:, 0], cams[:, 1], D, ds, di)
    src, ref = _feat(h, w, C, 25), _feat(h, w, C, 26)
    want, wm = _oracle_planes(src, H, ref)
    out = N.nan_output((D, h, w, 20), cuda)
    _, mask = ops.warp_planes(src[0].to(cuda), H[0].to(cuda), out=out, c_off=2, mode=1, ref=ref[0].to(cuda), want_mask=True)
    assert torch.equal(out[..., 2:18].cpu(), want)
    assert torch.equal(mask.cpu(), wm)
    N.assert_bits_kept(out, 2, 18)


def test_cost_volume_small_odd_map_bit_exact(cuda):
    """cost_volume_kernel at 17 x 23, C = 4, D = 5: two lanes per pixel (one copies ref, one warps), a ragged last workgroup."""
    from atvsnet_amd import ops
    h, w, C, D = 17, 23, 4, 5
    cams = _cams('general', h, w, D)
    ds, di = OM.depth_start_interval(cams)
    rf, vf = _feat(h, w, C, 27), _feat(h, w, C, 28)
    for a, b in ((0, 1), (1, 0)):
        want = OM.build_cost_volume(rf, vf, cams, D, ds, di, a, b)[0]
        H = G.get_homographies(cams[:, a], cams[:, b], D, ds, di)[0]
        got = ops.build_cost_volume(rf[0].to(cuda), vf[0].to(cuda), H.to(cuda))
        assert torch.equal(got.cpu(), want)


# ---------------------------------------------------------------------------
# Degenerate homographies straight into the launches
# ---------------------------------------------------------------------------
def _oracle_hull(ref_depth, view_trans, H, ds, di, inverse=True):
    """get_visual_hull's plane loop (reference homography_warping.py:363-385, view_num = 2) for GIVEN homographies, from the
    oracle's nearest warp: ([ref > 0][ref > delta_d] + [wd > 0][wd > delta_d]) / 2."""
    out = []
    for d in range(H.shape[1]):
        cur = ds + di * float(d)
        wd = G.homography_warping(view_trans[None, ..., None], H[:, d], method='nearest')[0, ..., 0]
        s = 0.0
        for m in (ref_depth, wd):
            behind = (m > cur) if inverse else (cur > m)
            s = s + (m > 0).to(torch.float32) * behind.to(torch.float32)
        out.append(s)
    return torch.stack(out) / 2.0


def test_degenerate_homographies_bit_exact(cuda):
    """geometry_cases.degenerate_homographies at 17 x 23 through every launch that applies a homography: a denominator that is
    exactly 0 (the reference's + 1e-7, homography_warping.py:251-252) on a whole column / row, one that changes sign inside the
    image, and a coordinate that overflows to inf -- invalid, and inf * 0 stays NaN in the bilinear output (tf.multiply, :64-65)
    while the nearest warp reads pixel (0,0).  Values equal or NaN on both sides; masks equal."""
    from atvsnet_amd import ops
    h, w = GC.DEGENERATE_HW
    H = GC.degenerate_homographies()
    D = H.shape[1]
    Hg = H[0].to(cuda)
    c = lambda t: t.to(cuda).contiguous()                       # noqa: E731
    for C in (4, 16):                                           # gather kernel <0,4>, shared kernel <0>
        src = _feat(h, w, C, 31)
        want, wm = _oracle_planes(src, H)
        assert bool(torch.isnan(want[2]).all()) and bool(torch.isfinite(want[[0, 1, 3]]).all())
        got, mask = ops.warp_planes(c(src[0]), Hg, want_mask=True)
        assert _same(got, want) and torch.equal(mask.cpu(), wm), C
    src, ref = _feat(h, w, 16, 32), _feat(h, w, 16, 33)         # shared kernel <1>
    want, wm = _oracle_planes(src, H, ref)
    got, mask = ops.warp_planes(c(src[0]), Hg, mode=1, ref=c(ref[0]), want_mask=True)
    assert _same(got, want) and torch.equal(mask.cpu(), wm)
    # mode 2 (one channel, rep 2) and the fused geo volume around it
    ds, di = torch.tensor([0.05]), torch.tensor([0.04])
    dn = torch.tensor(float(D))
    vt, d_ref = GC.inverse_map(h, w, 34), GC.inverse_map(h, w, 35)
    wd, wm = _oracle_planes(vt[None, ..., None], H)
    val = (ds + torch.arange(D, dtype=torch.float32) * di).reshape(D, 1, 1)
    geo_view = (torch.abs(wd[..., 0] - val) / di / dn) * wm
    geo_ref = torch.abs(d_ref[None] - val) / di / dn
    got, mask = ops.warp_planes(c(vt.reshape(h, w, 1)), Hg, mode=2, depth_start=c(ds), depth_interval=c(di), rep=2, want_mask=True)
    assert _same(got, torch.stack([geo_view, geo_view], -1)) and torch.equal(mask.cpu(), wm)
    for ld, c_off, rep in ((2, 0, 1), (5, 1, 2)):               # the 8-byte store, the scalar stores
        out = N.nan_output((D, h, w, ld), cuda)
        ops.geo_volume(c(d_ref), c(vt), Hg, c(ds), c(di), out, c_off, rep)
        assert _same(out[..., c_off:c_off + 1 + rep], torch.stack([geo_ref] + [geo_view] * rep, -1)), (ld, c_off, rep)
        N.assert_bits_kept(out, c_off, c_off + 1 + rep)
    # nearest (mode 3), cost volume, visual hull
    src = _feat(h, w, 4, 36)
    want, wm = _oracle_planes(src, H, method='nearest')
    assert torch.equal(want[2], src[0, 0, 0].expand(h, w, 4))
    got, mask = ops.warp_planes(c(src[0]), Hg, mode=ops.WARP_NEAREST, want_mask=True)
    assert torch.equal(got.cpu(), want) and torch.equal(mask.cpu(), wm)
    rf = _feat(h, w, 4, 37)
    want, _ = _oracle_planes(src, H)
    got = ops.build_cost_volume(c(rf[0]), c(src[0]), Hg)
    assert _same(got, torch.cat([rf.expand(D, -1, -1, -1), want], -1))
    hull = ops.visual_hull(c(d_ref), c(vt), Hg, c(ds), c(di))
    want = _oracle_hull(d_ref, vt, H, ds, di)
    assert torch.equal(hull.cpu(), want) and 0.0 < float(want.mean()) < 1.0


# ---------------------------------------------------------------------------
# Metric depth: every inverse_depth == 0 branch against the oracle under INVERSE_DEPTH = False
# ---------------------------------------------------------------------------
def _metric_scene(monkeypatch, h, w, D, views=2):
    monkeypatch.setattr(G, 'INVERSE_DEPTH', False)
    assert (h, w, D) in GC.METRIC_SHAPES
    cams = GC.general_cams(views, h, w, D)
    ds, di = GC.metric_range(*OM.depth_start_interval(cams), D)
    return cams, ds, di


@pytest.mark.parametrize('D', [1, 8])
def test_metric_homographies_bit_exact(cuda, monkeypatch, D):
    """homographies_kernel's e - tv / depth (reference homography_warping.py:218)."""
    from atvsnet_amd import ops
    cams, ds, di = _metric_scene(monkeypatch, 24, 40, D)
    for a, b in ((0, 1), (1, 0)):
        want = G.get_homographies(cams[:, a], cams[:, b], D, ds, di)[0]
        got = ops.get_homographies(cams[0, a].to(cuda).contiguous(), cams[0, b].to(cuda).contiguous(), ds.to(cuda), di.to(cuda), D,
                                   inverse_depth=False)
        assert torch.equal(got.cpu(), want)
        inv = ops.get_homographies(cams[0, a].to(cuda).contiguous(), cams[0, b].to(cuda).contiguous(), ds.to(cuda), di.to(cuda), D)
        assert not torch.equal(inv.cpu(), want)                 # the flag reaches the kernel


def test_metric_warp_by_depth_bit_exact(cuda, monkeypatch):
    """warp_by_depth_kernel's vec / depth (reference :152), plain and ERR, bilinear (C = 16) and nearest (C = 1)."""
    from atvsnet_amd import ops
    h, w = 24, 40
    cams, _, _ = _metric_scene(monkeypatch, h, w, 6)
    c = lambda t: t.to(cuda).contiguous()                       # noqa: E731
    depth = GC.metric_map(GC.inverse_map(h, w, 41))
    for C, method in ((16, 'bilinear'), (1, 'nearest')):
        src, ref = _feat(h, w, C, 42), _feat(h, w, C, 43)
        want, wm = G.homography_warping_by_depth(src, cams[:, 0], cams[:, 1], depth[None, ..., None], output_mask=True, method=method)
        assert 0.05 < float(wm.float().mean()) < 1.0
        got, mask = ops.warp_by_depth(c(src[0]), c(cams[0, 0]), c(cams[0, 1]), c(depth), method=method, inverse_depth=False)
        assert torch.equal(got.cpu(), want[0]) and torch.equal(mask.cpu(), wm[0, ..., 0].to(torch.float32))
        out = N.nan_output((h, w, 2 * C + 3), cuda)
        ops.warp_by_depth_err(c(src[0]), c(ref[0]), c(cams[0, 0]), c(cams[0, 1]), c(depth), out, 1, method, False, copy_ref=True)
        assert torch.equal(out[..., 1:1 + C], ops.absdiff_mask(got, c(ref[0]), mask))
        assert torch.equal(out[..., 1:1 + C].cpu(), torch.abs(want[0] - ref[0]) * wm[0].to(torch.float32))
        assert torch.equal(out[..., 1 + C:1 + 2 * C].cpu(), ref[0])
        N.assert_bits_kept(out, 1, 1 + 2 * C)


@pytest.mark.parametrize('h,w', [(24, 40), (129, 256)])
def test_metric_transform_depth_bit_exact(cuda, monkeypatch, h, w):
    """The bare transform (no clip, no reciprocal, no mask: reference :301-305, :321-324 skipped) in the one-workgroup kernel and in
    transform_depth_kernel<0/1>, where the two maxima are still formed and must not reach the output."""
    from atvsnet_amd import ops
    monkeypatch.setattr(G, 'INVERSE_DEPTH', False)
    assert (h, w) in GC.TRANSFORM_SIZES
    cams = GC.general_cams(2, h, w, 2)
    depth = GC.metric_map(GC.inverse_map(h, w, 44))
    want = G.transform_depth(depth[None, ..., None], cams[:, 1], cams[:, 0])[0, ..., 0]
    got = ops.transform_depth(depth.to(cuda), cams[0, 1].to(cuda).contiguous(), cams[0, 0].to(cuda).contiguous(), inverse_depth=False)
    assert torch.equal(got.cpu(), want)


def test_metric_transform_depth_batch_bit_exact(cuda, monkeypatch):
    from atvsnet_amd import ops
    h, w = 24, 40
    cams, _, _ = _metric_scene(monkeypatch, h, w, 6, views=3)
    cam = [cams[0, i].to(cuda).contiguous() for i in range(3)]
    pairs = ((1, 0), (2, 0), (0, 2))
    maps = [GC.metric_map(GC.inverse_map(h, w, 45 + k)) for k in range(3)]
    got = ops.transform_depth_batch([(m.to(cuda), cam[a], cam[b]) for m, (a, b) in zip(maps, pairs)], inverse_depth=False)
    for m, (a, b), o in zip(maps, pairs, got):
        assert torch.equal(o.cpu(), G.transform_depth(m[None, ..., None], cams[:, a], cams[:, b])[0, ..., 0]), (a, b)


def test_metric_visual_hull_bit_exact(cuda, monkeypatch):
    """visual_hull_kernel's delta_d > depth comparisons (reference :372, :381) on metric homographies and a metric transform,
    against get_visual_hull(view_num=2)."""
    from atvsnet_amd import ops
    D, h, w = 6, 24, 40
    cams, ds, di = _metric_scene(monkeypatch, h, w, D)
    c = lambda t: t.to(cuda).contiguous()                       # noqa: E731
    maps = torch.stack([GC.metric_map(GC.inverse_map(h, w, 48)), GC.metric_map(GC.inverse_map(h, w, 49))])
    want = G.get_visual_hull(maps[None], cams, D, ds, di, ref_id=0, view_num=2)[0, ..., 0]
    assert sorted(set(want.reshape(-1).tolist())) == [0.0, 0.5, 1.0]
    H = ops.get_homographies(c(cams[0, 0]), c(cams[0, 1]), c(ds), c(di), D, inverse_depth=False)
    vt = ops.transform_depth(c(maps[1]), c(cams[0, 1]), c(cams[0, 0]), inverse_depth=False)
    got = ops.visual_hull(c(maps[0]), vt, H, c(ds), c(di), inverse_depth=False)
    assert torch.equal(got.cpu(), want)
    assert not torch.equal(ops.visual_hull(c(maps[0]), vt, H, c(ds), c(di)).cpu(), want)


# ---------------------------------------------------------------------------
# transform_depth sizes (inverse depth, general cameras)
# ---------------------------------------------------------------------------
def _transform_case(h, w, seed=5):
    assert (h, w) in GC.TRANSFORM_SIZES
    return GC.general_cams(2, h, w, 2), GC.transform_map(h, w, seed)


@pytest.mark.parametrize('h,w', [(128, 256), (37, 883), (3, 1500), (300, 7), (4099, 1), (1, 1), (129, 256), (181, 182)])
def test_transform_depth_sizes_bit_exact(cuda, h, w):
    """One-workgroup kernel (up to 32,768 pixels): (128,256) all 32 items of every thread, (37,883) a ragged last item, (3,1500)
    w > 1024 (sy = 0), (300,7) many row carries per step, (4099,1) sx = 0, (1,1) one pixel.  General path (fill, max_kernel,
    transform_depth_kernel<0/1>, the float atomic maximum): (129,256) the first size past the threshold, (181,182) a ragged last
    workgroup.  A zero patch (invalid depths: the 1e-10 clip and the mask) wherever the map holds more than 15 pixels.
    Out of scope: an all-invalid map.  Its intermediate is NaN (1 / 0 * 0), and what the reference's tf.maximum / tf.reduce_max
    make of that cannot be observed without TensorFlow; every map here keeps a valid pixel."""
    from atvsnet_amd import ops
    cams, d = _transform_case(h, w)
    assert bool((d > 0).any()) and (h * w <= 15 or bool((d == 0).any()))
    want = G.transform_depth(d[None, ..., None], cams[:, 1], cams[:, 0])[0, ..., 0]
    got = ops.transform_depth(d.to(cuda), cams[0, 1].to(cuda).contiguous(), cams[0, 0].to(cuda).contiguous())
    assert torch.equal(got.cpu(), want)


def test_transform_depth_into_a_backwards_camera_bit_exact(cuda):
    """(129,256) into geometry_cases.backwards_cam: every transformed z is negative, so the general path's maximum goes through the
    unsigned-atomicMin branch of atomic_max_float and the clip's upper bound is negative; the oracle's output is finite
    (1 / zmax, about -61, at every valid pixel).
    The order of the clip here is the oracle's, min(max(z, 1e-10), zmax).  TensorFlow's clip_by_value is, as far as its public
    source goes, max(min(z, zmax), 1e-10); the two differ only when zmax < 1e-10, i.e. only for a camera that sees nothing in front
    of it, and which of them TensorFlow 1.5 evaluates cannot be observed without it -- like the all-invalid map, that question is
    out of scope here: this test holds the kernels to the oracle as it stands."""
    from atvsnet_amd import ops
    h, w = 129, 256
    assert (h, w) in GC.BACKWARDS_SIZES
    cams, d = _transform_case(h, w)
    back = GC.backwards_cam(cams[:, 0])
    want = G.transform_depth(d[None, ..., None], cams[:, 1], back)[0, ..., 0]
    assert bool(torch.isfinite(want).all()) and float(want.max()) <= 0.0 and float(want.min()) < -10.0
    got = ops.transform_depth(d.to(cuda), cams[0, 1].to(cuda).contiguous(), back[0].to(cuda).contiguous())
    assert torch.equal(got.cpu(), want)
    assert torch.equal(torch.signbit(got.cpu()), torch.signbit(want))          # -0.0 at the masked pixels on both sides


def test_transform_depth_batch_of_16_full_maps_two_camera_pairs_bit_exact(cuda):
    """16 maps of (128,256) -- a whole launch, every thread at its 32 items -- over two camera pairs, one of them into the backwards
    camera (a negative maximum inside the one-workgroup kernel): each workgroup reads its own map and its own pose."""
    from atvsnet_amd import ops
    h, w = 128, 256
    assert (h, w) in GC.BACKWARDS_SIZES
    cams = GC.general_cams(2, h, w, 2)
    back = GC.backwards_cam(cams[:, 0])
    c1, c0, cb = (t.to(cuda).contiguous() for t in (cams[0, 1], cams[0, 0], back[0]))
    maps = [GC.transform_map(h, w, 60 + k) for k in range(16)]
    got = ops.transform_depth_batch([(m.to(cuda), c1, cb if k % 3 == 1 else c0) for k, m in enumerate(maps)])
    for k, (m, o) in enumerate(zip(maps, got)):
        want = G.transform_depth(m[None, ..., None], cams[:, 1], back if k % 3 == 1 else cams[:, 0])[0, ..., 0]
        assert torch.equal(o.cpu(), want), k
        assert (float(want.max()) <= 0.0) == (k % 3 == 1)
