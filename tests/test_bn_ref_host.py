"""The batch-norm bar of tests/bn_ref.py is sound and strong enough: a float32 emulation of the kernels' two fused multiply-adds
passes 2u * bn_cond in every regime; and each defect a kernel could have -- a 16-bit shift, a mean short of two bits,
another sample's parameter block, beta lost on the channels a float4 loop leaves over -- fails it where the channel means are
large.  No GPU."""
import pytest
import torch

import bn_ref as B
import numerics as N

DRAWS = 20
SHAPE = (2, 4099, 27)            # two samples with their own parameters; C mod 4 = 3


def _ratio(raw, par, relu, defect=None, rel=B.APPLY_REL):
    got = B.emulate_fma(raw, par, relu, defect)
    return N.assert_elementwise(got, B.bn64(raw, par, relu), B.bn_cond(raw, par), rel, 0.0, str(defect))


@pytest.mark.parametrize('regime', B.REGIMES)
def test_the_fma_form_passes_the_bar_with_room(regime):
    worst = 0.0
    for d in range(DRAWS):
        raw, par = B.operand(regime, SHAPE, 100 + d)
        for relu in (False, True):
            worst = max(worst, _ratio(raw, par, relu))
    print('%s: fma form, largest err/cond %.3f u over %d draws' % (regime, worst / B.U, DRAWS))
    # randn and small: where |x s| is far below |b| the value IS the shift, rounded twice, and both roundings can come close to
    # u |shift| = u * cond; offset: x s and m s nearly cancel, so the result's own rounding is small beside u |m s| <= cond / 2
    assert worst <= (B.APPLY_REL / 2 if regime == 'offset' else B.APPLY_REL)


def test_the_offset_regime_is_what_it_says():
    raw, par = B.operand('offset', SHAPE, 100)
    x = raw.double()
    ratio = x.mean(1).abs() / x.std(1, unbiased=False)
    print('offset: |mean| / std from %.0f to %.0f' % (float(ratio.min()), float(ratio.max())))
    assert 40 <= float(ratio.min()) and float(ratio.max()) <= 2.1e4 and float(ratio.max()) >= 1e3
    # the parameters are the sample's own float64 moments, rounded once
    assert torch.equal(par[:, 0], x.mean(1).float())
    n = B.bn64(raw, par, False)
    assert float(n.mean(1).sub(par[:, 2].double()).abs().max()) <= 2.0 ** -24 * float((par[:, 0] * par[:, 1]).abs().max())
    assert float((n.std(1, unbiased=False) - 1).abs().max()) < 3e-3          # var / (var + 1e-3), var >= 0.25


@pytest.mark.parametrize('defect', B.DEFECTS)
def test_each_planted_defect_fails_the_bar_in_the_offset_regime(defect):
    """Three of the defects fail the bar in every draw, by a factor of 100 and more.  mean_22_bits sits AT the bar and is the
    measure of what the bar resolves: a mean rounded to 22 bits is off by at most 2^-22 |m| = 4u |m| (only where the two
    dropped bits are a tie and the mantissa is near 1), and at x ~ m the bar is 2u (|x s| + |m s|) ~ 4u |m s|.  The regime fails
    it (the largest ratio over the draws, reached in about three draws of four); a draw whose 54 means all round by less than
    that passes, as it must: such a mean is a correct float32 mean of slightly different data."""
    ratios, good = [], 0.0
    for d in range(DRAWS):
        raw, par = B.operand('offset', SHAPE, 100 + d)
        good = max(good, _ratio(raw, par, False))
        ratios.append(_ratio(raw, par, False, defect, rel=float('inf')))
    failing = [r for r in ratios if r > B.APPLY_REL]
    assert failing, '%s passes the bar in every draw (largest err/cond %.2f u)' % (defect, max(ratios) / B.U)
    print('%s: fails %d of %d draws, smallest failing err/cond %.2f u, largest %.2f u; the fma form %.3f u; the bar 2 u'
          % (defect, len(failing), DRAWS, min(failing) / B.U, max(ratios) / B.U, good / B.U))
    raw, par = B.operand('offset', SHAPE, 100 + ratios.index(max(ratios)))
    with pytest.raises(AssertionError, match='err/cond'):
        _ratio(raw, par, False, defect)
    if defect != 'mean_22_bits':
        assert len(failing) == DRAWS and min(failing) >= 100 * B.APPLY_REL


def test_sum_bound_holds_for_the_emulated_chain():
    """(a + b) + c in emulated float32 of two pending terms and a dense one stays within 4u * sum of conds."""
    from atvsnet_amd import ops
    worst = 0.0
    for regime in B.REGIMES:
        (ra, pa), (rb, pb) = B.operand(regime, SHAPE, 7), B.operand(regime, SHAPE, 8)
        c = B.dense(regime, SHAPE, 9)
        items = [ops.PendingBN(ra, pa, True), c, ops.PendingBN(rb, pb, False)]
        want, cnd = B.sum64(items)
        a, b = B.emulate_fma(ra, pa, True), B.emulate_fma(rb, pb, False)
        got = ((a + c.double()).float().double() + b).float().double()
        worst = max(worst, N.assert_elementwise(got, want, cnd, B.ADD_REL, 0.0, 'sum ' + regime))
    print('three-term sum: largest err/cond %.3f u; the bar 4 u' % (worst / B.U))
    assert worst <= B.ADD_REL


def test_the_on_load_bar_passes_the_transform_and_fails_a_16_bit_shift():
    """The offset regime of tests/test_gpu_split_precision.py: a convolution (float64 accumulation here) of the emulated on-load
    transform stays within 2^-22 * cond_on_load by itself, and with the kernels' own bar on top a shift rounded to fp16 fails."""
    from atvsnet_amd import ops
    from oracle import tf_ops as T
    raw, par = B.operand('offset', (2, 9, 13, 16), 3)
    w = torch.randn((3, 3, 16, 8), generator=torch.Generator().manual_seed(4)) * (2.0 / 144) ** 0.5
    pend = ops.PendingBN(raw, par, True)

    def op(x, w):
        return T.conv(x, w, 1, 'SAME')
    want, cnd = N.ref64(op, pend, w), N.cond_on_load(op, pend, w)
    assert bool((cnd >= N.cond(op, pend, w)).all())
    good = op(B.emulate_fma(raw, par, True), w.double())
    r = N.assert_elementwise(good, want, cnd, 2.0 ** -22, 0.0, 'on-load transform')
    print('on-load 3x3 convolution, offset: the fma form err/cond %.3f u; the bar %.1f u' % (r / B.U, (N.SPLIT.rel + 2.0 ** -22) / B.U))
    with pytest.raises(AssertionError, match='err/cond'):
        N.assert_elementwise(op(B.emulate_fma(raw, par, True, 'shift_fp16'), w.double()), want, cnd, N.SPLIT.rel + 2.0 ** -22,
                             N.floor_of(w, N.SPLIT), 'shift_fp16')
