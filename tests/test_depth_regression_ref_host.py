"""CPU: the float64 reference of the depth regression and confidence kernels (tests/depth_regression_ref.py) checked against the
float32 oracle, so that the bar tests/test_gpu_depth_regression.py holds the kernels to is itself held where no GPU exists."""
import pytest
import torch

import depth_regression_ref as R
from oracle import model as OM
from oracle import tf_ops as T


@pytest.mark.parametrize('D', [1, 2, 5, 63, 64, 65, 130, 192, 257])
@pytest.mark.parametrize('regime', R.REGIMES)
def test_depths_are_the_oracles_linspace(D, regime):
    ds, di = R.sweep(regime, D)
    end = ds + (float(D) - 1.0) * di
    assert torch.equal(R.depths(ds, di, D), T.linspace(ds[0], end[0], D))
    assert R.depths(ds, di, D).dtype == torch.float32


def test_upsampled_is_the_identity_at_scale_one_and_keeps_the_corners():
    cost = R.costs('typical', (5, 3, 4), 1)
    assert torch.equal(R.upsampled(cost, 1), cost)
    up = R.upsampled(cost, 3)
    assert up.shape == (5, 9, 12) and up.dtype == torch.float32
    assert torch.equal(up[:, ::8, ::11], cost[:, ::2, ::3])
    one = R.upsampled(cost[:, :1, :1].contiguous(), 4)                  # extents of 1: scale 0, every output is the one input
    assert torch.equal(one, cost[:, :1, :1].expand(5, 4, 4))


@pytest.mark.parametrize('D,h,w,up', [(1, 1, 1, 1), (5, 1, 7, 1), (65, 9, 21, 1), (192, 3, 130, 1), (63, 6, 1, 2), (65, 7, 11, 3),
                                       (192, 7, 11, 4), (130, 1, 9, 5), (64, 7, 11, 8)])
@pytest.mark.parametrize('regime', R.REGIMES)
def test_soft_argmin_reference_agrees_with_the_float32_oracle(D, h, w, up, regime):
    """|oracle - want| <= 2e-6 * cond at every pixel: a correct float32 evaluation meets the bar the kernels are held to."""
    cost = R.costs(regime, (D, h, w), 1000 * D + 10 * h + w + up)
    ds, di = R.sweep(regime, D)
    vol = R.upsampled(cost, up)
    want, cond = R.softargmin64(vol, R.depths(ds, di, D))
    oracle = OM.prob2depth(vol[None], D, ds, di)[0, ..., 0]
    ratio = ((oracle.double() - want).abs() / cond).max()
    assert float(ratio) <= R.REL, float(ratio)
    if up == 4:
        _, o_up = OM.prob2depth_upsample(cost[None], D, ds, di)
        assert torch.equal(o_up[0, ..., 0], oracle)                    # the oracle's own x4 path is the same interpolation


@pytest.mark.parametrize('D,h,w,up', [(2, 6, 67, 1), (5, 3, 23, 3), (64, 2, 17, 4), (192, 5, 3, 3), (192, 1, 4, 4)])
@pytest.mark.parametrize('regime', R.REGIMES)
def test_confidence_reference_agrees_with_the_float32_oracle(D, h, w, up, regime):
    """At the finite depths (the oracle takes a non-finite one through a cast; R.planes states those planes instead)."""
    cost = R.costs(regime, (D, h, w), 7 * D + h + w + up)
    ds, di = R.sweep(regime, D)
    vol = R.upsampled(cost, up)
    H, W = vol.shape[1:]
    depth = R.depth_map(H, W, ds, di, D, D + up)
    fin = torch.isfinite(depth)
    assert int((~fin).sum()) == 3
    p32 = torch.softmax(-vol, 0)
    oracle = OM.get_propability_map(p32[None], depth.reshape(1, H, W, 1), ds, di).reshape(H, W)
    soft = R.probmap64(vol, depth, ds, di, True)
    assert float((oracle.double() - soft)[fin].abs().max()) <= R.PROB_ABS
    assert torch.equal(R.probmap32_plain(p32, depth, ds, di)[fin], oracle[fin])
    plain = R.probmap64(p32, depth, ds, di, False)
    assert float((oracle.double() - plain)[fin].abs().max()) <= 3 * 2.0 ** -24 * 2.0      # three float32 additions of a sum <= 2


def test_planes_at_the_edges():
    D = 5
    ds, di = torch.tensor([0.5]), torch.tensor([2.0 ** -6])
    v = R.depths(ds, di, D)
    inf = float('inf')
    depth = torch.tensor([float(v[0]), float(v[3]), float(v[4]), float(v[3]) + 2.0 ** -8, 0.0, 9.0, float('nan'), inf, -inf])
    l0, l1, r0, r1 = [t.tolist() for t in R.planes(depth, ds, di, D)]
    assert l0 == [0, 3, 4, 3, 0, 4, 0, 4, 0]
    assert l1 == [0, 2, 3, 2, 0, 3, 0, 3, 0]
    assert r0 == [0, 3, 4, 4, 0, 4, 0, 4, 0]
    assert r1 == [1, 4, 4, 4, 1, 4, 1, 4, 1]
    assert [t.tolist() for t in R.planes(torch.tensor([float('nan'), inf, 0.7]), ds, di, 1)] == [[0, 0, 0]] * 4
    # a decreasing sweep turns the infinities round: the planes follow the sign of the plane coordinate
    l0, _, _, r1 = R.planes(torch.tensor([inf, -inf]), torch.tensor([0.5]), torch.tensor([-0.1]), D)
    assert l0.tolist() == [0, 4] and r1.tolist() == [1, 4]


@pytest.mark.parametrize('D', [5, 64, 65, 130, 192])
def test_one_hot_known_answer_is_exact_in_the_oracle(D):
    """cost +-100: every plane is the minimum of some pixel and the oracle returns its hypothesis bit for bit."""
    h, w = 3, 130
    k = torch.arange(h * w) % D
    assert sorted(set(k.tolist())) == list(range(D))
    assert set(R.boundary_planes(D)) <= set(k.tolist())
    cost = R.one_hot(D, h, w, k)
    for regime in ('typical', 'decreasing'):
        ds, di = R.sweep(regime, D)
        v = R.depths(ds, di, D)
        assert torch.equal(OM.prob2depth(cost[None], D, ds, di)[0, ..., 0], v[k].reshape(h, w))
        want, cond = R.softargmin64(cost, v)
        assert torch.equal(want.float(), v[k].reshape(h, w))


def test_flat_regime_gives_every_plane_weight():
    """The flat regime is there so that ONE plane lost or counted twice moves the result: every plane of every pixel carries at
    least 1 / (8 D)."""
    worst = 1e9
    for D, h, w in [(2, 1, 7), (5, 5, 1), (63, 3, 130), (64, 9, 21), (65, 9, 21), (130, 3, 130), (192, 9, 21), (192, 3, 130)]:
        for up in (1, 4):
            cost = R.costs('flat', (D, h, w), 1000 * D + 10 * h + w + up)
            p = torch.softmax(-R.upsampled(cost, up).double(), 0)
            worst = min(worst, float(p.min()) * 8 * D)
            assert float(p.min()) >= 1.0 / (8 * D), (D, h, w, up, float(p.min()) * D)
