"""-m gpu: the depth regression and confidence kernels (csrc/softargmin.hip) held element by element to a float64 reference
(tests/depth_regression_ref.py; the reference is itself checked on the CPU by tests/test_depth_regression_ref_host.py).

    atvs_softargmin            softargmin_kernel: the depth axis split over four wavefronts, partials merged through LDS
    atvs_upsample_softargmin   up_scale 1, 2: upsample_softargmin_kernel (one thread per output pixel, D sequential pushes)
                               up_scale >= 3: upsample_softargmin_tile_kernel (taps staged in LDS in chunks of 64 planes)
    atvs_probability_map       probability_map_kernel<SOFTMAX, UP>, all four instantiations

Bars.  A depth: |got - want| <= 2e-6 * cond, want = sum_d p_d v_d and cond = sum_d p_d |v_d| with p the float64 soft-max of the
float32 (interpolated) cost -- the project's soft-argmin tolerance, unchanged; the float32 oracle meets it against the same
reference (host test).  One-hot costs (+-100): v_k bit for bit.  The plain confidence: bit for bit (a gather and three float32
additions in a stated order, through an interpolation that is the oracle's operations in its order).  The soft-max confidence:
2e-6 absolute against float64, the number tests/test_gpu_probmap.py states for this form.

Every case runs with its volume and depth map inside NaN borders and its output taken from a NaN-poisoned allocator, and every
output element is compared: a tap read outside the volume or a pixel left unwritten fails.  Shapes are the smallest that reach
each branch: depth counts around the 64-plane chunk (63, 64, 65, 130 = two chunks and a remainder of 2, 192), extents of 1,
output sizes that end in a partial tile and cross several (33, 35, 36, 390 wide), up_scale 3 where 16 outputs span the most taps
of the 8-wide window.  Four cost regimes (depth_regression_ref.costs): in `flat` every plane carries at least 1 / (8 D), so one
plane lost or counted twice at a wavefront or chunk boundary moves the depth by ~1e-3 relative, 500 x the bar.

Largest err / cond per kernel and depth count on an MI355X (u = 2^-24 = 5.96e-8; the bar is 2e-6 = 33.6 u): not measured -- no
GPU run could be obtained while this module was written.  Every test prints its figure (`DEPTHREG <kernel> D=.. up=.. <regime>
err/cond ..` under pytest -s); the table belongs here after the first run.  What is known without a GPU: the float32 oracle is
at most 19 u from the reference on these cases (host test), and a float32 restatement of the kernels' order of operations on
the CPU (numpy's expf, not the GPU's) gives at D = 192 at most 12 u for the four-way split of softargmin_kernel and 29 u for the
single pass of the two x-up kernels (typical and decreasing regimes, 390 x 12 pixels): most of it is the float32 rounding of
x - max in front of expf (2^-22 absolute for 4 <= |x - max| < 8), which the float64 soft-max does not have.  Should a single-pass
kernel exceed 2e-6 at D = 192 on the GPU by that rounding alone (_hold names the pixel and its plane weights: a lost plane is an
error of a whole weight, ~1e-3 in the flat regime), the worst case of a D-term sum of non-negative terms caps what that kernel's
bar at that D may become: (2 D + 16) u single pass, (D / 2 + 16) u four-way split.  The bar is not moved towards a measurement.

Sensitivity (mutations of csrc/softargmin.hip on a scratch copy, never committed), and the tests each must fail: not run on a
GPU either.  On the CPU, with a float32 stand-in carrying the mutation in each kernel's place, the tests named below fail and
no other does (the x1 clamp was not emulated; its row is by reading).
    the tile kernel skips its remainder chunk            test_upsample_softargmin at up >= 3 with D = 65, 130; both test_one_hot_* at D = 65, 130
    a wavefront's plane range starts one plane late      test_softargmin at every D >= 5, test_one_hot_is_the_hypothesis_bit_for_bit at every D
    x1 clamped to w - 2                                  test_upsample_softargmin (every w > 1), test_probability_map_plain / _softmax
    the clipping of l1 and r1 swapped                    test_probability_map_plain at every (up, D), test_probability_map_softmax at D >= 5
    the last output row left unwritten                   every test of the family (NaN from the poisoned allocator)
"""
import ctypes

import pytest
import torch

import depth_regression_ref as R
import numerics as N
from oracle import model as OM

pytestmark = pytest.mark.gpu


def _in(t, cuda):
    return N.nan_bordered(t.contiguous().to(cuda))


def _note(kernel, D, up, regime, ratio):
    print('DEPTHREG %-28s D=%-3d up=%d %-10s err/cond %.3e' % (kernel, D, up, regime, ratio))


def _softargmin(cuda, cost, ds, di, groups=None):
    from atvsnet_amd import ops
    c, s, i = _in(cost, cuda), _in(ds, cuda), _in(di, cuda)
    N.poison_allocator(cuda)
    return ops.softargmin(c, s, i, groups=groups).cpu()


def _upsample_softargmin(cuda, cost, ds, di, up):
    from atvsnet_amd import ops
    c, s, i = _in(cost, cuda), _in(ds, cuda), _in(di, cuda)
    N.poison_allocator(cuda)
    got = ops.upsample_softargmin(c, s, i, up).cpu()
    assert got.shape == (cost.shape[1] * up, cost.shape[2] * up)
    return got


def _probability_map(cuda, vol, depth, ds, di, up, softmax):
    from atvsnet_amd import ops
    v, d, s, i = _in(vol, cuda), _in(depth, cuda), _in(ds, cuda), _in(di, cuda)
    N.poison_allocator(cuda)
    return ops.probability_map(v, d, s, i, up, softmax).cpu()


def _hold(got, want, cond, vol, what):
    """assert_elementwise at the 2e-6 bar; a failure also names the plane weights of the worst pixel (the five largest and the
    smallest), from which a lost plane (an error of about one weight times the sweep) and rounding can be told apart."""
    try:
        return N.assert_elementwise(got, want, cond, R.REL, 0.0, what)
    except AssertionError as e:
        ratio = (got.double() - want).abs() / cond
        ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float('inf')))
        y, x = divmod(int(ratio.argmax()), ratio.shape[-1])
        p = torch.softmax(-vol[:, y, x].double(), 0)
        top = p.topk(min(5, p.numel()))
        raise AssertionError('%s; plane weights at (%d, %d): largest %s at planes %s, smallest %.3e' % (
            e, y, x, ['%.3e' % t for t in top.values.tolist()], top.indices.tolist(), float(p.min())))


def _seed(D, h, w, up):
    return 1000 * D + 10 * h + w + up


# ------------------------------------------------------------------------------------------------------- 1. soft-argmin

SOFTARGMIN_SHAPES = [(1, 1, 1), (2, 1, 7), (5, 5, 1), (63, 3, 130), (64, 9, 21), (65, 9, 21), (130, 3, 130), (192, 9, 21),
                     (192, 3, 130), (65, 1, 1), (130, 5, 1), (2, 9, 21)]


@pytest.mark.parametrize('D,h,w', SOFTARGMIN_SHAPES)
def test_softargmin(cuda, D, h, w):
    """atvs_softargmin in every regime, then three volumes of three regimes as groups of one launch (on an increasing and on a
    decreasing sweep).  D < 4 leaves wavefronts without a plane; 3 x 130 = 390 pixels are seven workgroups, the last partial."""
    vols = {}
    for regime in R.REGIMES:
        cost = vols[regime] = R.costs(regime, (D, h, w), _seed(D, h, w, 0) + R.REGIMES.index(regime))
        ds, di = R.sweep(regime, D)
        want, cond = R.softargmin64(cost, R.depths(ds, di, D))
        got = _softargmin(cuda, cost, ds, di)
        _note('softargmin', D, 1, regime, _hold(got, want, cond, cost, 'softargmin %s' % regime))
    cost3 = torch.stack([vols['flat'], vols['typical'], vols['peaked']])
    for regime in ('typical', 'decreasing'):
        ds, di = R.sweep(regime, D)
        ref = [R.softargmin64(c, R.depths(ds, di, D)) for c in cost3]
        got = _softargmin(cuda, cost3, ds, di, groups=3)
        assert got.shape == (3, h, w)
        r = N.assert_elementwise(got, torch.stack([a for a, _ in ref]), torch.stack([b for _, b in ref]), R.REL, 0.0,
                                 'softargmin groups=3 %s' % regime)
        _note('softargmin groups=3', D, 1, regime, r)


# ----------------------------------------------------------------------------------------------------- 2. x up soft-argmin

UPSAMPLE_CASES = (
    [(4, D, h, w) for D, h, w in [(1, 1, 1), (5, 1, 9), (63, 6, 1), (64, 7, 11), (65, 3, 130), (130, 7, 11), (192, 3, 130),
                                  (65, 1, 9), (192, 7, 11)]] +
    [(1, 1, 1, 1), (1, 5, 6, 1), (1, 65, 7, 11), (1, 192, 3, 130), (1, 64, 1, 9)] +
    [(2, 63, 6, 1), (2, 130, 7, 11), (2, 64, 1, 9), (2, 5, 1, 1), (2, 192, 3, 130)] +
    [(3, 1, 1, 1), (3, 5, 1, 9), (3, 130, 6, 1), (3, 65, 7, 11), (3, 192, 3, 130), (3, 63, 7, 11)] +
    [(5, 64, 7, 11), (5, 130, 1, 9), (5, 5, 6, 1), (5, 65, 3, 130)] +
    [(8, 65, 7, 11), (8, 192, 1, 9), (8, 63, 6, 1), (8, 1, 1, 1)])


@pytest.mark.parametrize('up,D,h,w', UPSAMPLE_CASES)
def test_upsample_softargmin(cuda, up, D, h, w):
    """atvs_upsample_softargmin against softargmin64 of the float32 interpolated cost: the scalar kernel at up 1, 2, the tile
    kernel from 3 on.  D = 65, 130 end in a remainder chunk; widths 33, 35, 36, 390 end in a partial tile."""
    kernel = 'upsample_softargmin' + ('_tile' if up >= 3 else '')
    for regime in R.REGIMES:
        cost = R.costs(regime, (D, h, w), _seed(D, h, w, up) + R.REGIMES.index(regime))
        ds, di = R.sweep(regime, D)
        vol = R.upsampled(cost, up)
        want, cond = R.softargmin64(vol, R.depths(ds, di, D))
        got = _upsample_softargmin(cuda, cost, ds, di, up)
        _note(kernel, D, up, regime, _hold(got, want, cond, vol, '%s x%d %s' % (kernel, up, regime)))


# ------------------------------------------------------------------------------------------------------- 3. known answers

@pytest.mark.parametrize('D', [5, 64, 65, 130, 192])
def test_one_hot_is_the_hypothesis_bit_for_bit(cuda, D):
    """cost +100, -100 at plane k: exp(-200) is 0 in float32, so the regression returns v_k itself.  k = pixel index mod D makes
    every plane the minimum somewhere (atvs_softargmin, and atvs_upsample_softargmin at up 1).  Through an interpolation the
    volume is constant in x and y so that no planes mix: every k up to D = 65 and the planes where wavefronts and chunks change
    hands beyond, at up 2 (scalar kernel) and 3, 4, 5 (tile kernel)."""
    h, w = 3, 130
    k = torch.arange(h * w) % D
    cost = R.one_hot(D, h, w, k)
    for regime in ('typical', 'decreasing'):
        ds, di = R.sweep(regime, D)
        v = R.depths(ds, di, D)
        want = v[k].reshape(h, w)
        assert torch.equal(_softargmin(cuda, cost, ds, di), want), 'softargmin %s' % regime
        assert torch.equal(_upsample_softargmin(cuda, cost, ds, di, 1), want), 'upsample_softargmin x1 %s' % regime
    ds, di = R.sweep('typical', D)
    v = R.depths(ds, di, D)
    ks = range(D) if D <= 65 else sorted(set(R.boundary_planes(D)) | set(range(0, D, 5)))
    for up, (h, w) in ((2, (2, 3)), (3, (2, 3)), (4, (1, 1)), (5, (1, 2))):
        for kk in ks:
            cost = R.one_hot(D, h, w, torch.full((h * w,), kk, dtype=torch.int64))
            got = _upsample_softargmin(cuda, cost, ds, di, up)
            assert torch.equal(got, v[kk].expand(h * up, w * up)), 'x%d plane %d' % (up, kk)


@pytest.mark.parametrize('D', [5, 64, 65, 130, 192])
def test_one_hot_rows_through_the_interpolation(cuda, D):
    """The same costs with k depending on the low-resolution row only, at up 4: output rows between two low-resolution rows mix
    two planes.  Against the oracle's float32 result and against float64, both at the float64 bar."""
    ks = torch.tensor(R.boundary_planes(D))
    h, w = ks.numel(), 5
    cost = R.one_hot(D, h, w, ks.reshape(h, 1).expand(h, w).contiguous())
    for regime in ('typical', 'decreasing'):
        ds, di = R.sweep(regime, D)
        want, cond = R.softargmin64(R.upsampled(cost, 4), R.depths(ds, di, D))
        _, oracle = OM.prob2depth_upsample(cost[None], D, ds, di)
        got = _upsample_softargmin(cuda, cost, ds, di, 4)
        N.assert_elementwise(got, oracle[0, ..., 0].double(), cond, R.REL, 0.0, 'one-hot rows vs the oracle, %s' % regime)
        r = N.assert_elementwise(got, want, cond, R.REL, 0.0, 'one-hot rows vs float64, %s' % regime)
        _note('upsample_softargmin_tile 1hot', D, 4, regime, r)
        assert torch.equal(got[0], R.depths(ds, di, D)[ks[0]].expand(4 * w))        # output row 0 is low-resolution row 0 alone


# ----------------------------------------------------------------------------------------------------------- 4, 5. confidence

PROB_SHAPES = {1: [(6, 67), (1, 13), (13, 1)], 3: [(3, 23), (5, 1), (1, 2)], 4: [(2, 17), (1, 4), (3, 1)]}
PROB_CASES = [(up, D) for up in (1, 3, 4) for D in (2, 5, 64, 192)]


@pytest.mark.parametrize('up,D', PROB_CASES)
def test_probability_map_plain(cuda, up, D):
    """softmax = 0 (probability_map_kernel<false, *>): the volume is a soft-max computed on the CPU, the depth map holds values
    inside and outside the sweep, exactly on hypotheses 0, 3 and D-1, one ulp to either side of them, NaN, +inf and -inf.
    Expected: the oracle fed the same depth map and the interpolated volume, bit for bit.  At the three non-finite depths the
    oracle's planes would come from a cast of NaN / inf to an integer; there the planes are stated (depth_regression_ref.planes):
        plane coordinate NaN, -inf -> (l0, l1, r0, r1) = (0, 0, 0, min(1, D-1));   +inf -> (D-1, max(D-2, 0), D-1, D-1)."""
    for regime in R.REGIMES:
        ds, di = R.sweep(regime, D)
        for h, w in PROB_SHAPES[up]:
            probs = torch.softmax(-R.costs(regime, (D, h, w), _seed(D, h, w, up)), 0)
            vol = R.upsampled(probs, up)
            H, W = h * up, w * up
            depth = R.depth_map(H, W, ds, di, D, _seed(D, h, w, up) + 1)
            fin = torch.isfinite(depth)
            want = OM.get_propability_map(vol[None], depth.reshape(1, H, W, 1), ds, di).reshape(H, W)
            stated = R.probmap32_plain(vol, depth, ds, di)
            assert torch.equal(want[fin], stated[fin])
            want = torch.where(fin, want, stated)
            got = _probability_map(cuda, probs, depth, ds, di, up, False)
            bad = (got != want).nonzero()
            assert torch.equal(got, want), 'plain x%d D=%d %s (%d,%d): %d differ, first at %s' % (
                up, D, regime, h, w, len(bad), bad[:1].tolist())


@pytest.mark.parametrize('up,D', PROB_CASES)
def test_probability_map_softmax(cuda, up, D):
    """softmax = 1 (probability_map_kernel<true, *>): the same depth maps on pre-soft-max costs of every regime, every pixel
    within 2e-6 absolute of the four terms gathered from the float64 soft-max (the planes chosen in float32, as the kernel must)."""
    for regime in R.REGIMES:
        ds, di = R.sweep(regime, D)
        for h, w in PROB_SHAPES[up]:
            cost = R.costs(regime, (D, h, w), _seed(D, h, w, up) + 2)
            H, W = h * up, w * up
            depth = R.depth_map(H, W, ds, di, D, _seed(D, h, w, up) + 3)
            want = R.probmap64(R.upsampled(cost, up), depth, ds, di, True)
            got = _probability_map(cuda, cost, depth, ds, di, up, True)
            err = N.assert_elementwise(got, want, torch.ones_like(want), R.PROB_ABS, 0.0,
                                       'soft-max confidence x%d D=%d %s (%d,%d)' % (up, D, regime, h, w))
            _note('probability_map softmax', D, up, regime, err)


# ------------------------------------------------------------------------------------------------------------- 6. arguments

def test_arguments_are_refused_before_any_launch(cuda):
    """up_scale, D, h or w <= 0: ATVS_ERR_SHAPE; a null pointer: ATVS_ERR_NULL; the output keeps its bytes either way."""
    from atvsnet_amd import _lib, ops
    lib = _lib.lib()
    ERR_NULL, ERR_SHAPE = -1, -2
    buf = torch.full((64,), 7.0, device=cuda)
    out = torch.full((64,), -3.0, device=cuda)
    p, o, null = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = (2, 1, 1, 1)                                       # D, h, w, up_scale
    for pos in range(4):
        for bad in (0, -1):
            dims = list(good)
            dims[pos] = bad
            assert lib.atvs_upsample_softargmin(p, p, p, o, *dims, stream) == ERR_SHAPE, dims
            for softmax in (0, 1):
                assert lib.atvs_probability_map(p, p, p, p, o, *dims, softmax, stream) == ERR_SHAPE, dims
    for pos in range(4):
        ptrs = [p, p, p, o]
        ptrs[pos] = null
        assert lib.atvs_upsample_softargmin(*ptrs, *good, stream) == ERR_NULL, pos
    for pos in range(5):
        ptrs = [p, p, p, p, o]
        ptrs[pos] = null
        assert lib.atvs_probability_map(*ptrs, *good, 1, stream) == ERR_NULL, pos
    vol = torch.zeros(4, 3, 5, device=cuda)
    one = torch.ones(1, device=cuda)
    for shape, up in (((3, 4), 1), ((5, 3), 1), ((3, 5), 2), ((12, 20), 3), ((15,), 1)):
        with pytest.raises(ValueError):
            ops.probability_map(vol, torch.zeros(shape, device=cuda), one, one, up, True)
    torch.cuda.synchronize()
    assert bool((out == -3.0).all()) and bool((buf == 7.0).all())
