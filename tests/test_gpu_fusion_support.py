"""-m gpu: ops.fusion_support (csrc/fusion_support.hip) against the oracle's fuse_reference(trace=)['count'] of every reference
camera: the count integer for integer, the masked depth plane and the weight plane bit for bit -- on the ring and the floater of the
TSDF tests under the fake normal, on the inputs of tests/fusion_cases.py that carry real normals and a normal threshold that rejects,
on a map that is no multiple of 256 pixels, with one camera alone, at num_consistent 0, 1, 2 and n, each output alone (a NULL pointer
for each of the others), each case twice for the same bits."""
import numpy as np
import pytest
import torch

import fusion_cases as FC
import tsdf_weighted_restated as WR

pytestmark = pytest.mark.gpu

OUTPUTS = ('count', 'depth', 'weight')


@pytest.fixture(scope='module')
def ops(cuda):
    from atvsnet_amd import ops as o
    return o


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _check(ops, cams28, nd, disp, ang, nc, want):
    """All three outputs at once, each alone, and all three again: `want`'s integers and bits every time."""
    cams_d, nd_d = _dev(cams28), _dev(nd)
    first = ops.fusion_support(cams_d, nd_d, disp, ang, nc)
    assert sorted(first) == sorted(OUTPUTS)
    for name in OUTPUTS:
        assert first[name].dtype == (torch.int32 if name == 'count' else torch.float32) and tuple(first[name].shape) == nd.shape[:3]
        assert np.array_equal(_bits(first[name]), _bits(want[name])), name
        alone = ops.fusion_support(cams_d, nd_d, disp, ang, nc, want=(name,))
        assert list(alone) == [name] and torch.equal(alone[name].view(torch.int32), first[name].view(torch.int32)), name
    again = ops.fusion_support(cams_d, nd_d, disp, ang, nc)
    for name in OUTPUTS:
        assert torch.equal(again[name].view(torch.int32), first[name].view(torch.int32)), name
    return first


@pytest.mark.parametrize('name', ('ring', 'floater'))
def test_the_tsdf_scenes_under_the_fake_normal(ops, name):
    cams28, nd, count = WR.scene_count(name)
    n = len(nd)
    assert nd.shape[1:3] == (37, 53) and (37 * 53) % 256 != 0 and count.max() >= 2
    for nc in (0, 1, 2, n):
        got = _check(ops, cams28, nd, WR.DISP_THRESHOLD, WR.FAKE_NORMAL_THRESHOLD, nc, WR.scene_support(name, nc))
        kept = int((got['depth'] > 0).sum())
        valid = int((nd[..., 3] > 0).sum())
        # 0 masks nothing, n everything (a count is at most n - 1), 1 and 2 a part
        assert kept == valid if nc == 0 else kept == 0 if nc == n else 0 < kept < valid
    # the weight is written for every pixel whatever the mask says: 1 / (1 + nc) where nothing agrees
    got = ops.fusion_support(_dev(cams28), _dev(nd), WR.DISP_THRESHOLD, WR.FAKE_NORMAL_THRESHOLD, 2, want=('weight',))['weight']
    assert torch.equal(got[_dev(count == 0)], torch.full((int((count == 0).sum()),), float(np.float32(1.0) / np.float32(3.0)), device='cuda'))


REAL_NORMAL_CASES = tuple(c for c in FC.SCENE_CASES if c.thresholds[1] in FC.FINITE_NORMAL_THRESHOLDS and c.rows == 67)


@pytest.mark.parametrize('case', REAL_NORMAL_CASES, ids=FC.case_id)
def test_real_normals_and_a_threshold_that_rejects(ops, case):
    from oracle import fusibile as F
    Ps, depths, normals, images, _ = FC.case_inputs(case)
    nd, _ = FC.textures(depths, normals, images)
    cams28 = F.pack_cameras(Ps)
    disp, ang = case.thresholds
    want = WR.support(cams28, nd, disp, ang, case.ncons)
    # the normal test decides some pixels: under a threshold that rejects nothing the count is another
    loose = WR.support(cams28, nd, disp, FC.TWO_PI, case.ncons)['count']
    assert (loose > want['count']).any() and (want['count'] > 0).any()
    _check(ops, cams28, nd, disp, ang, case.ncons, want)
    other = (case.ncons + 1) % (case.n + 1)
    _check(ops, cams28, nd, disp, ang, other, dict(count=want['count'], **WR.planes(want['count'], nd[..., 3], other)))


def test_one_camera_alone_agrees_with_nothing(ops):
    cams28, nd, _ = WR.scene_count('ring')
    cams28, nd = cams28[4:5], nd[4:5]
    for nc in (0, 1):
        want = dict(count=np.zeros(nd.shape[:3], np.int32), **WR.planes(np.zeros(nd.shape[:3], np.int32), nd[..., 3], nc))
        got = _check(ops, cams28, nd, WR.DISP_THRESHOLD, WR.FAKE_NORMAL_THRESHOLD, nc, want)
        assert int(got['count'].abs().sum()) == 0
        assert torch.equal(got['depth'], _dev(nd[..., 3])) if nc == 0 else int((got['depth'] != 0).sum()) == 0


def test_the_outputs_it_was_not_asked_for_stay_untouched_and_the_slab_is_only_read(ops):
    cams28, nd, _ = WR.scene_count('ring')
    cams_d, nd_d = _dev(cams28), _dev(nd)
    before = nd_d.clone()
    ops.fusion_support(cams_d, nd_d, WR.DISP_THRESHOLD, WR.FAKE_NORMAL_THRESHOLD, 2)
    assert torch.equal(nd_d.view(torch.int32), before.view(torch.int32))
    with pytest.raises(ValueError, match='num_consistent'):
        ops.fusion_support(cams_d, nd_d, WR.DISP_THRESHOLD, WR.FAKE_NORMAL_THRESHOLD, -1)
    with pytest.raises(ValueError, match='want'):
        ops.fusion_support(cams_d, nd_d, WR.DISP_THRESHOLD, WR.FAKE_NORMAL_THRESHOLD, 2, want=())
