"""-m gpu: the depth-map fusion kernel (csrc/fusion.hip, reference fusibile/fusibile.cu:138-277) against its oracle,
bit for bit, and the depth_fusion driver end to end.

The cases of tests/fusion_cases.py (pinned on the CPU by tests/test_fusion_cases_host.py): full cameras, occlusion, special depths
and normals, every reference camera; the four small pairs also against their known answers."""
import os

import numpy as np
import pytest
import torch

import fusion_cases as FC
import numerics
from fusion_scene import make_scene
from test_fusion import write_dense_folder

pytestmark = pytest.mark.gpu


def _operands(n_views, seed, noise):
    from atvsnet_amd.atvsnet import depth_fusion as DF
    Ps, depths, normals, images, _, _ = make_scene(n_views, rows=56, cols=72, seed=seed)
    rng = np.random.default_rng(seed)
    depths = depths * (1.0 + noise * rng.normal(size=depths.shape)).astype(np.float32)     # some views disagree
    depths[:, 3:9, 40:50] = 0                                                              # filtered pixels
    cams = DF.pack_cameras(Ps)
    nd = np.ascontiguousarray(np.concatenate([normals, depths[..., None]], -1).astype(np.float32))
    img4 = np.ascontiguousarray(np.concatenate([images.astype(np.float32), np.zeros(images.shape[:3] + (1,), np.float32)], -1))
    return Ps, depths, normals, images, cams, nd, img4


@pytest.mark.parametrize('n_views,noise,disp,nthr,ncons', [(4, 0.004, 0.01, 2 * np.pi, 2), (3, 0.0, 0.01, 0.08, 1),
                                                           (5, 0.01, 0.02, 2 * np.pi, 3)])
def test_fusion_kernel_bit_exact(cuda, n_views, noise, disp, nthr, ncons):
    from atvsnet_amd import ops
    from oracle import fusibile as F
    _, _, _, _, cams, nd, img4 = _operands(n_views, 7, noise)
    cd, ndd, imd = (torch.from_numpy(a).to(cuda) for a in (cams, nd, img4))
    some = 0
    for ref in range(n_views):
        X, nrm, tex, created = F.fuse_reference(cams, nd, img4, ref, disp, nthr, ncons)
        coord, normal, texture, cr = [t.cpu().numpy() for t in ops.fusibile(cd, ndd, imd, ref, disp, nthr, ncons)]
        assert np.array_equal(cr > 0, created), ref
        assert np.array_equal(coord[..., :3], X, equal_nan=True), ref
        assert np.array_equal(normal[..., :3], nrm, equal_nan=True), ref
        assert np.array_equal(texture[..., :3], tex[..., :3], equal_nan=True), ref
        some += int(created.sum())
    assert 0 < some < n_views * nd.shape[1] * nd.shape[2]          # the case decides something


# ------------------------------------------------------------------------------------------ the cases of fusion_cases.py

def _device_inputs(cuda, Ps, depths, normals, images):
    """(cams, nd, img4) on the host as the oracle takes them, and NaN-bordered on the device."""
    from atvsnet_amd.atvsnet import depth_fusion as DF
    nd, img4 = FC.textures(depths, normals, images)
    rows, cols = nd.shape[1:3]
    assert (rows, cols) in FC.FUSION_SHAPES['kernel'], 'shape %dx%d is not listed in fusion_cases.FUSION_SHAPES' % (rows, cols)
    cams = DF.pack_cameras(Ps)
    return (cams, nd, img4), tuple(numerics.nan_bordered(torch.from_numpy(a).to(cuda)) for a in (cams, nd, img4))


def _launch(cuda, dev, ref, disp, nthr, ncons):
    """One atvs_fusibile launch into outputs that were NaN before it: -> coord, normal, texture (rows,cols,4), created."""
    from atvsnet_amd import ops
    numerics.poison_allocator(cuda)
    return [t.cpu().numpy() for t in ops.fusibile(dev[0], dev[1], dev[2], ref, disp, nthr, ncons)]


def _assert_is_oracle(got, want, what):
    coord, normal, texture, created = got
    X, nrm, tex, want_created = want
    assert coord.shape == X.shape and normal.shape == nrm.shape and texture.shape == tex.shape and coord.shape[-1] == 4
    assert np.array_equal(created, want_created.astype(np.float32)), what           # 1.0 / 0.0, every pixel written
    assert np.array_equal(coord, X, equal_nan=True), what
    assert np.array_equal(normal, nrm, equal_nan=True), what
    assert np.array_equal(texture, tex, equal_nan=True), what


_oracle = {}


def _case_oracle(case):
    """fuse_reference of every reference camera of a case, four components each, computed once."""
    from oracle import fusibile as F
    if case not in _oracle:
        Ps, depths, normals, images, _ = FC.case_inputs(case)
        nd, img4 = FC.textures(depths, normals, images)
        cams = F.pack_cameras(Ps)
        _oracle[case] = [F.fuse_reference(cams, nd, img4, ref, case.thresholds[0], case.thresholds[1], case.ncons, full=True)
                         for ref in range(case.n)]
    return _oracle[case]


@pytest.mark.parametrize('case', FC.KERNEL_CASES, ids=FC.case_id)
def test_fusion_kernel_general_cases(cuda, case):
    """general_scene (hard_maps planted where the case says so): every reference camera, all four components of coord, normal and
    texture and the created map, equal to the oracle."""
    Ps, depths, normals, images, _ = FC.case_inputs(case)
    _, dev = _device_inputs(cuda, Ps, depths, normals, images)
    want = _case_oracle(case)
    for ref in range(case.n):
        got = _launch(cuda, dev, ref, case.thresholds[0], case.thresholds[1], case.ncons)
        _assert_is_oracle(got, want[ref], 'ref %d' % ref)
        assert (got[0][..., 3] == 0).all() and (got[1][..., 3] == 0).all() and (got[2][..., 3] == 0).all()


def _pair_against_oracle(cuda, pair, ncons):
    """Both reference cameras of a two-view case at (0.01, 2 pi) against the oracle: -> [(got, trace of the other view)]."""
    from oracle import fusibile as F
    host, dev = _device_inputs(cuda, *pair)
    out = []
    for ref in (0, 1):
        trace = {}
        want = F.fuse_reference(host[0], host[1], host[2], ref, 0.01, FC.TWO_PI, ncons, full=True, trace=trace)
        got = _launch(cuda, dev, ref, 0.01, FC.TWO_PI, ncons)
        _assert_is_oracle(got, want, 'ref %d' % ref)
        out.append((got, trace['views'][1 - ref]))
    return host, out


def test_facing_away_pair_creates_the_in_bounds_pixels(cuda):
    """tz < 0 everywhere: the relative disparity difference is negative and passes, so created == projects inside the image."""
    _, out = _pair_against_oracle(cuda, FC.facing_away_pair(), 1)
    for got, other in out:
        assert (other['tz'] < 0).all()
        assert np.array_equal(got[3] > 0, other['inb'])
        assert 0.9 * other['inb'].size < (got[3] > 0).sum() < other['inb'].size


def test_side_by_side_holes_divide_by_zero(cuda):
    """A hole of depth 0 is its camera's centre, tz == 0 in the other view: not created, and nothing read outside the maps."""
    pair = FC.side_by_side_holes()
    host, out = _pair_against_oracle(cuda, pair, 1)
    for ref, (got, other) in enumerate(out):
        hole = pair[1][ref] == 0
        assert hole.sum() > 60 and (other['tz'][hole] == 0).all()
        assert not (got[3][hole] > 0).any() and (got[3][~hole] > 0).sum() > 0.5 * (~hole).sum()
        assert (got[0][hole][:, :3] == host[0][ref, 21:24]).all()
    _pair_against_oracle(cuda, pair, 0)


def test_zero_baseline_pair_creates_nothing(cuda):
    """base = 0: both disparities are 0, 0 / 0 is NaN and no view agrees; at num_consistent = 0 every pixel is created."""
    pair = FC.zero_baseline_pair()
    _, out = _pair_against_oracle(cuda, pair, 1)
    for got, other in out:
        assert other['inb'].mean() > 0.8 and not (got[3] > 0).any()
    _, out = _pair_against_oracle(cuda, pair, 0)
    assert all((got[3] > 0).all() for got, _ in out)


@pytest.mark.parametrize('rows,cols,sx,sy', FC.EXACT_CASES)
def test_exact_projections_blend_by_hand(cuda, rows, cols, sx, sy):
    """px = x + sx, py = y + sy exactly: the texture is the hand-written blend (clamped second texel, 8-bit weights with ties
    rounded up, weight 1.0), created is the hand-written inside test (0 and cols - 2^-10 in, cols and -2^-10 out).  Also on
    one-row, one-column and one-pixel maps, where both texels of a footprint clamp to the same row or column."""
    pair = FC.exact_projections(sx, sy, (rows, cols))
    _, out = _pair_against_oracle(cuda, pair, 1)
    (coord, normal, texture, created), _ = out[0]
    want_tex, want_created = FC.expected_exact(pair[3], sx, sy)
    assert np.array_equal(created > 0, want_created)
    assert np.array_equal(texture[..., :3].astype(np.float64), want_tex)
    ys, xs = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing='ij')
    assert np.array_equal(coord[..., :3].astype(np.float64), np.stack([(xs - 32) / 16, (ys - 32) / 16, np.full_like(xs, 4.0)], -1))
    assert np.array_equal(normal[..., :3], pair[2][0])


def test_depth_fusion_driver_end_to_end(cuda, tmp_path):
    """probability filter -> gipuma files -> fusion on the GPU -> PLY, against the oracle on the same files."""
    from atvsnet_amd.atvsnet import depth_fusion as DF
    from atvsnet_amd.tools import ply
    from oracle import fusibile as F
    root = str(tmp_path)
    _, _, _, _, n, d0 = write_dense_folder(root, n_views=4)
    DF.main(['--dense_folder', root, '--prob_threshold', '0.8', '--disp_threshold', '0.01', '--num_consistent', '2'])
    pts, cols = ply.read_ply(os.path.join(root, 'final3d_model.ply'))
    assert len(pts) > 0.6 * 4 * 48 * 64
    assert float(np.abs(pts.astype(np.float64) @ n + d0).max()) < 5e-3
    # the oracle on exactly what the driver read back from disk
    pf = os.path.join(root, 'points_atvsnet')
    names = ['%08d' % i for i in range(4)]
    Ps = [DF.read_p_file(os.path.join(pf, 'cams', s + '.jpg.P')) for s in names]
    depths = np.stack([DF.read_gipuma_dmb(os.path.join(pf, '2333__' + s, 'disp.dmb')) for s in names])
    normals = np.stack([DF.read_gipuma_dmb(os.path.join(pf, '2333__' + s, 'normals.dmb')) for s in names])
    images = np.stack([DF._imread_bgr(os.path.join(pf, 'images', s + '.jpg')) for s in names])
    want_p, want_c = F.fuse(Ps, depths, normals, images, 0.01, 360 * np.pi / 180.0, 2)
    assert np.array_equal(pts, want_p) and np.array_equal(cols, want_c)
