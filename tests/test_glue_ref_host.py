"""CPU: the float64 references of tests/glue_ref.py agree with oracle.tf_ops at float32 within the bars the GPU tests use, and
those bars FAIL a subtly wrong kernel: each defect below is applied to a float32 restatement of the kernel's own decomposition
(pooling: windows, SL slices of partial sums, a finishing pass) or to the float64 formula (AANet), and must miss the bar.
"""
import pytest
import torch

import glue_ref as G
import numerics as N
from oracle import tf_ops as T


def _gen(seed):
    return torch.Generator().manual_seed(seed)


POOL_SHAPES = [(1, 32, 40, 128, 64, 64), (5, 16, 20, 128, 8, 8), (2, 30, 45, 32, 8, 8), (3, 9, 11, 12, 4, 4), (2, 7, 5, 3, 2, 2),
               (1, 5, 6, 7, 3, 2), (2, 12, 6, 16, 4, 4), (1, 3, 3, 8, 64, 64), (4, 1, 1, 4, 2, 2), (2, 36, 36, 64, 8, 2)]


def _ints(shape, seed):
    return torch.randint(-8, 9, shape, generator=_gen(seed)).float()


def _normal(shape, seed):
    return torch.randn(shape, generator=_gen(seed)) * 3 + 5


# --------------------------------------------------------------------------------------------- references against the oracle

@pytest.mark.parametrize('shape', POOL_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_avg_pool64_agrees_with_the_oracle(shape):
    """avg_pool64 (plain loops) and oracle.tf_ops.avg_pool2d_same (padded sums / padded counts) are written independently: the
    oracle at float32 has the exact row's bits and is within the random row's bar; the counts are the oracle's counts."""
    Gn, H, W, C, pool, stride = shape
    xi, xr = _ints((Gn, H, W, C), 1), _normal((Gn, H, W, C), 2)
    mean64, count, _ = G.avg_pool64(xi, pool, stride)
    assert torch.equal(T.avg_pool2d_same(xi, pool, stride), G.pool_exact(mean64))
    assert int(count.min()) >= 1 and int(count.max()) <= min(pool, H) * min(pool, W)
    mean64, count, sabs = G.avg_pool64(xr, pool, stride)
    G.assert_within(T.avg_pool2d_same(xr, pool, stride), mean64, G.pool_bar(count, sabs), 'oracle fp32')
    # the float64 oracle is the reference to rounding
    assert float((T.avg_pool2d_same(xr.double(), pool, stride) - mean64).abs().max()) < 1e-13


def test_avg_pool64_counts_by_hand():
    """H = 5, k = 3, s = 2: Ho = 3, pad = 2, one row in front -> windows [0,2) [1,4) [3,5); W = 6: Wo = 3, pad = 1, none in
    front -> [0,3) [2,5) [4,6)."""
    ys, xs = G.pool_windows(5, 6, 3, 2)
    assert ys == [(0, 2), (1, 4), (3, 5)] and xs == [(0, 3), (2, 5), (4, 6)]
    _, count, _ = G.avg_pool64(torch.zeros(5, 6, 1), 3, 2)
    assert count.tolist() == [[6, 6, 4], [9, 9, 6], [6, 6, 4]]


@pytest.mark.parametrize('shape', [(5, 2, 3, 32, 16, 20), (1, 1, 1, 8, 4, 6), (2, 9, 13, 3, 9, 13), (1, 16, 20, 4, 5, 7),
                                   (1, 6, 7, 1, 24, 28), (1, 5, 9, 2, 1, 1), (1, 5, 9, 2, 1, 17)])
def test_resize64_agrees_with_the_oracle(shape):
    Gn, H, W, C, Ho, Wo = shape
    x = torch.randn((Gn, H, W, C), generator=_gen(3))
    y64, corners = G.resize64(x, (Ho, Wo))
    G.assert_within(T.resize_bilinear_align_corners(x, (Ho, Wo)), y64, G.resize_bar(corners), 'oracle fp32')
    if (H, W) == (Ho, Wo):
        assert torch.equal(y64, x.double())
    # a scale of H / Ho instead of (H - 1) / (Ho - 1) misses the bar wherever both have more than one pixel and the sizes differ
    if Ho > 1 and Wo > 1 and (H, W) != (1, 1) and (H, W) != (Ho, Wo):
        wrong = torch.nn.functional.interpolate(x.permute(0, 3, 1, 2), size=(Ho, Wo), mode='bilinear', align_corners=False)
        with pytest.raises(AssertionError):
            G.assert_within(wrong.permute(0, 2, 3, 1), y64, G.resize_bar(corners), 'half-pixel centres')


# ------------------------------------------------------------------------------------------------ pooling: emulated defects

def pool_emulated(x, pool, stride, defect=None):
    """csrc/pool.hip restated in float32 on the CPU: per image, per window, SL slices [n sl / SL, n (sl + 1) / SL) of the
    window's pixels in row-major order -> workspace (G, Ho, Wo, SL, C); then the slices summed in order and divided by the
    valid count.  (A slice is summed in float64 and rounded: one of the orders the bar allows.)  defect: None, or
      'row' / 'col'  the window one row / column too large (where the image has one)
      'kk'           divided by k * k instead of the valid count
      'slice'        the last of the SL partial slices dropped
      'ws'           image 0 finished from image 1's workspace"""
    Gn, H, W, C = x.shape
    ys, xs = G.pool_windows(H, W, pool, stride)
    Ho, Wo = len(ys), len(xs)
    SL = G.pool_slices(Ho, Wo)
    ws = torch.full((Gn, Ho, Wo, SL, C), float('nan'))
    for oy, (y0, y1) in enumerate(ys):
        for ox, (x0, x1) in enumerate(xs):
            ye = min(y1 + 1, H) if defect == 'row' else y1
            xe = min(x1 + 1, W) if defect == 'col' else x1
            px = x[:, y0:ye, x0:xe, :].reshape(Gn, -1, C)
            n = px.shape[1]
            for sl in range(SL):
                ws[:, oy, ox, sl] = px[:, n * sl // SL:n * (sl + 1) // SL].double().sum(1).float()
    out = torch.zeros((Gn, Ho, Wo, C))
    for g in range(Gn):
        src = ws[1 if (defect == 'ws' and g == 0) else g]
        v = torch.zeros((Ho, Wo, C))
        for sl in range(SL - 1 if defect == 'slice' else SL):
            v = v + src[:, :, sl]
        for oy, (y0, y1) in enumerate(ys):
            for ox, (x0, x1) in enumerate(xs):
                div = pool * pool if defect == 'kk' else (y1 - y0) * (x1 - x0)
                out[g, oy, ox] = v[oy, ox] / torch.tensor(float(div))
    return out


DEFECT_SHAPES = [(2, 30, 45, 32, 8, 8), (2, 32, 40, 16, 64, 64), (2, 5, 6, 7, 3, 2)]


@pytest.mark.parametrize('shape', DEFECT_SHAPES + [(3, 9, 11, 12, 4, 4), (1, 3, 3, 8, 64, 64)],
                         ids=lambda s: 'x'.join(str(v) for v in s))
def test_pool_emulation_without_defect_meets_both_bars(shape):
    Gn, H, W, C, pool, stride = shape
    xi, xr = _ints((Gn, H, W, C), 4), _normal((Gn, H, W, C), 5)
    assert torch.equal(pool_emulated(xi, pool, stride), G.pool_exact(G.avg_pool64(xi, pool, stride)[0]))
    mean64, count, sabs = G.avg_pool64(xr, pool, stride)
    G.assert_within(pool_emulated(xr, pool, stride), mean64, G.pool_bar(count, sabs))


@pytest.mark.parametrize('shape,defect', [(s, d) for s in DEFECT_SHAPES for d in ('row', 'col', 'kk', 'slice', 'ws')
                                          if not (d in ('row', 'col') and s[4] > max(s[1], s[2]))],
                         ids=lambda v: 'x'.join(str(i) for i in v) if isinstance(v, tuple) else v)
def test_pool_defect_fails_both_bars(shape, defect):
    """Ragged 8 x 8 windows (SL = 26), 64 x 64 windows larger than the map (SL = 64: one dropped slice is 1 / 64 of a window) and
    overlapping 3 x 3 windows of stride 2 (SL = 64, mostly empty slices): the exact row loses its bits and the random row
    misses n * 2^-24 * mean|x| under every defect.  (A window larger than the map has no further row or column to take in:
    there the 'row' and 'col' defects change nothing and are no rows of this test.)"""
    Gn, H, W, C, pool, stride = shape
    xi, xr = _ints((Gn, H, W, C), 4), _normal((Gn, H, W, C), 5)
    assert not torch.equal(pool_emulated(xi, pool, stride, defect), G.pool_exact(G.avg_pool64(xi, pool, stride)[0]))
    mean64, count, sabs = G.avg_pool64(xr, pool, stride)
    with pytest.raises(AssertionError):
        G.assert_within(pool_emulated(xr, pool, stride, defect), mean64, G.pool_bar(count, sabs))


# -------------------------------------------------------------------------------------------------- AANet: emulated defects

AANET_ROWS = [(nv, regime) for nv in (2, 3, 5, 8, 9, 16) for regime in G.REGIMES]


def _parts(srs, xs):
    sr = torch.stack(srs, 0).double()
    S, R = sr[..., :8], sr[..., 8:]
    return S, R, torch.stack(xs, 0).double()


def test_rel_is_what_the_docstring_says():
    """REL is at most 8 x the largest err / cond measured on the GPU, and at most a tenth of the mildest defect's."""
    assert 0 < G.REL <= 8 * G.AANET_MEASURED
    assert G.AANET_DEFECT >= 10 * G.REL


@pytest.mark.parametrize('nv,regime', [(1, 'normal')] + AANET_ROWS)
def test_aanet_float32_formula_meets_the_bar(nv, regime):
    """The module's formula in float32 torch (oracle.tf_ops.softmax: max-subtracted) is within REL * cond of aanet_combine64."""
    srs, xs = G.aanet_case(nv, 129, regime)
    sr, X = torch.stack(srs, 0), torch.stack(xs, 0)
    S, R = sr[..., :8], sr[..., 8:]
    y = (T.softmax((R - S) + S.sum(0, keepdim=True), 0) * X).sum(0)
    N.assert_elementwise(y, G.aanet_combine64(srs, xs), G.aanet_combine_cond(srs, xs), G.REL, 0.0, 'float32 formula')


@pytest.mark.parametrize('nv,regime', AANET_ROWS)
def test_aanet_softmax_without_s_sum_passes(nv, regime):
    """What the bar CANNOT see: the softmax is shift invariant, so scores without the S_sum term give the same map."""
    srs, xs = G.aanet_case(nv, 129, regime)
    S, R, X = _parts(srs, xs)
    y = (torch.softmax(R - S, 0) * X).sum(0)
    N.assert_elementwise(y, G.aanet_combine64(srs, xs), G.aanet_combine_cond(srs, xs), G.REL, 0.0, 'no S_sum')


def _neighbour_ratio(nv, regime, V=129):
    srs, xs = G.aanet_case(nv, V, regime)
    S, R, X = _parts(srs, xs)
    p = torch.softmax((R - S) + S.sum(0, keepdim=True), 0)
    y = (torch.roll(p, 1, 0) * X).sum(0)                       # view n weighted with view n - 1's score
    err = (y - G.aanet_combine64(srs, xs)).abs()
    return float((err / G.aanet_combine_cond(srs, xs)).max()), y, srs, xs


@pytest.mark.parametrize('nv,regime', AANET_ROWS)
def test_aanet_neighbouring_score_fails(nv, regime):
    """View n weighted with view n - 1's score: the mildest defect here.  Its worst element is at least 10 x REL over, in
    every regime and view count, and no row is milder than the recorded AANET_DEFECT (16 views, N(0,1))."""
    ratio, y, srs, xs = _neighbour_ratio(nv, regime)
    assert ratio >= 10 * G.REL and ratio >= 0.99 * G.AANET_DEFECT, 'err / cond %.3e' % ratio
    with pytest.raises(AssertionError):
        N.assert_elementwise(y, G.aanet_combine64(srs, xs), G.aanet_combine_cond(srs, xs), G.REL, 0.0)


def test_aanet_recorded_defect_ratio():
    ratio = _neighbour_ratio(16, 'normal')[0]
    assert abs(ratio - G.AANET_DEFECT) <= 0.01 * G.AANET_DEFECT, 'measured here %.4e' % ratio


@pytest.mark.parametrize('nv', [2, 5, 16])
def test_aanet_no_max_shift_fails_at_spread_200(nv):
    """A weight e^U / sum e^U in float32 without the max shift overflows at a spread of 200: not finite, which the bar counts
    as a miss."""
    srs, xs = G.aanet_case(nv, 129, 'spread200')
    sr, X = torch.stack(srs, 0), torch.stack(xs, 0)
    S, R = sr[..., :8], sr[..., 8:]
    e = torch.exp((R - S) + S.sum(0, keepdim=True))
    y = (e * X).sum(0) / e.sum(0)
    assert not bool(torch.isfinite(y).all())
    with pytest.raises(AssertionError):
        N.assert_elementwise(y, G.aanet_combine64(srs, xs), G.aanet_combine_cond(srs, xs), G.REL, 0.0)
