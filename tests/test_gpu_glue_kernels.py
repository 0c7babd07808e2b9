"""-m gpu: the small kernels between the convolutions -- SAME average pooling, align-corners resize, channel copy / stack /
concat / add (csrc/pool.hip, csrc/norm.hip) and the cross-view softmax + weighted sum (csrc/aanet.hip) -- element by element
against the float64 references and bars of tests/glue_ref.py, on the code paths the networks take (groups = views, channel
slices of a wider buffer, views sharded over ranks).  tests/test_glue_ref_host.py shows on the CPU that each bar fails a
subtly wrong kernel.
"""
import pytest
import torch

import glue_ref as G
import numerics as N
from oracle import model as OM
from oracle import tf_ops as T

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits_equal(got, want, what=''):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert tuple(got.shape) == tuple(want.shape), '%s: shape %s, expected %s' % (what, tuple(got.shape), tuple(want.shape))
    bad = got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)
    assert not bool(bad.any()), '%s: %d of %d values differ in their bits, first at %s' % (
        what, int(bad.sum()), bad.numel(), tuple(int(v) for v in torch.nonzero(bad)[0]))


# ------------------------------------------------------------------------------------------------------------------ pooling

POOL_SHAPES = [
    # G, H, W, C, pool, stride
    (1, 32, 40, 128, 64, 64),     # window larger than the map, SL = 64, 1280 pixels: 20 per slice
    (5, 16, 20, 128, 8, 8),       # the production form: groups = views; SL = 64 of one pixel each
    (2, 30, 45, 32, 8, 8),        # ragged SAME padding on both axes (pad 2 and 3), SL = 26
    (3, 9, 11, 12, 4, 4),         # C / 4 = 3 channel groups: 85 pixel lanes, lane 255 idle
    (2, 7, 5, 3, 2, 2),           # C % 4 != 0: the scalar branch
    (1, 5, 6, 7, 3, 2),           # the scalar branch with stride != pool: overlapping windows
    (2, 12, 6, 16, 4, 4),         # 64 pixel lanes against a 4-wide window: the `while (xx >= x1)` wrap
    (2, 36, 36, 64, 8, 2),        # 18 x 18 outputs: SL = 1; 16 lanes step four times through windows 5 .. 8 wide
    (1, 3, 3, 8, 64, 64),         # 9 pixels over SL = 64 slices: most slices are empty
    (4, 1, 1, 4, 2, 2),           # a single-pixel map
]


def _pool_input(kind, shape, seed):
    g = _gen(seed)
    if kind == 'exact':
        return torch.randint(-8, 9, shape, generator=g).float()
    if kind == 'normal':
        return torch.randn(shape, generator=g) * 3 + 5
    mag = torch.exp2(torch.rand(shape, generator=g) * 20 - 10)
    return torch.where(torch.rand(shape, generator=g) < 0.5, -mag, mag)


@pytest.mark.parametrize('kind', ['exact', 'normal', 'loguniform'])
@pytest.mark.parametrize('shape', POOL_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_avg_pool_per_window(cuda, shape, kind):
    """avg_pool_partial_kernel + avg_pool_finish_kernel against avg_pool64, every window on its own.

    exact rows (integers in [-8, 8]): float32(sum64 / count) bit for bit -- a dropped, doubled or foreign element, a window one
    pixel too large, a count that includes the padding all change the bits.  random rows (N(0,1) * 3 + 5; log-uniform
    2^-10 .. 2^10 with mixed signs): |got - mean64| <= n * 2^-24 * (sum|x| / n).

    Branches of avg_pool_partial_kernel and the row that reaches each:
      the scalar branch, C % 4 != 0                      2x7x5x3x2x2, 1x5x6x7x3x2
      a channel-group count that does not divide 256     3x9x11x12x4x4 (cw = 3, 85 lanes, one idle)
      more pixel lanes than the window is wide           2x12x6x16x4x4 (64 lanes, ww = 4: a slice holds one pixel at most, so the
                                                         `while (xx >= x1)` wrap runs but no later step reads its result) and
                                                         2x36x36x64x8x2 (SL = 1, 16 lanes, windows 5 .. 8 wide, up to 64 pixels:
                                                         every lane takes up to four steps, each wrapping over two or three rows);
                                                         1x32x40x128x64x64 (8 lanes, 20 pixels per slice: a wrap in mid-slice)
      empty slices (fewer pixels than SL)                1x3x3x8x64x64 (9 pixels, SL = 64), 4x1x1x4x2x2
      stride != pool                                     1x5x6x7x3x2 (scalar branch), 2x36x36x64x8x2 (float4 branch)
      groups > 1, workspace and image offsets            every row with G > 1: each image has its own data and must equal the
                                                         single-image call on it bit for bit
      64 slices of a 64 x 64 window                      1x32x40x128x64x64
    The workspace and the output come out of a NaN-poisoned allocator: a slice that is never written is a NaN in its window."""
    from atvsnet_amd import ops
    Gn, H, W, C, pool, stride = shape
    x = _pool_input(kind, (Gn, H, W, C), 100 + H * W + C)
    mean64, count, sabs = G.avg_pool64(x, pool, stride)
    xd = x.to(cuda)
    N.poison_allocator(cuda)
    got = ops.avg_pool_same(xd, pool, stride, groups=Gn)
    assert tuple(got.shape) == (Gn,) + tuple(mean64.shape[1:])
    if kind == 'exact':
        _bits_equal(got, G.pool_exact(mean64), 'grouped')
    else:
        r = G.assert_within(got, mean64, G.pool_bar(count, sabs), 'grouped')
        print('avg_pool %s %s: largest err / bar %.3f' % (shape, kind, r))
    for g in range(Gn):
        N.poison_allocator(cuda)
        one = ops.avg_pool_same(xd[g], pool, stride)
        _bits_equal(one, got[g], 'image %d alone' % g)


# ------------------------------------------------------------------------------------------------------------------- resize

RESIZE_SHAPES = [
    # G, H, W, C, Ho, Wo
    (5, 2, 3, 32, 16, 20),        # an SPP branch: into c_off = 192 of the 320-wide concat buffer
    (1, 1, 1, 8, 4, 6),           # single-pixel source
    (2, 9, 13, 3, 9, 13),         # identity
    (1, 16, 20, 4, 5, 7),         # down-sampling
    (1, 6, 7, 1, 24, 28),         # the upsample_prob_vol form: C = 1
    (1, 5, 9, 2, 1, 1),           # single-pixel target
    (1, 5, 9, 2, 1, 17),          # one output row
]


@pytest.mark.parametrize('shape', RESIZE_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_resize_bits_of_the_oracle(cuda, shape):
    """resize_bilinear_kernel: the bits of oracle.tf_ops.resize_bilinear_align_corners (the kernel is built with
    -ffp-contract=off; same float32 scale, same operation order), and within 4 * 2^-24 * (|tl| + |tr| + |bl| + |br|) of
    resize64.  The first row is ResNetDS2SPP's call: groups = views, written into channels [192, 224) of a NaN-filled buffer
    with ld = 320, whose other channels must keep their bits (numerics.assert_bits_kept)."""
    from atvsnet_amd import ops
    Gn, H, W, C, Ho, Wo = shape
    x = torch.randn((Gn, H, W, C), generator=_gen(200 + H * W + C))
    want = T.resize_bilinear_align_corners(x, (Ho, Wo))
    y64, corners = G.resize64(x, (Ho, Wo))
    xd = x.to(cuda)
    if C == 32:
        buf = N.nan_output((Gn, Ho, Wo, 320), cuda)
        ops.resize_bilinear(xd, (Ho, Wo), out=buf, c_off=192, groups=Gn)
        N.assert_bits_kept(buf, 192, 224)
        got = buf[..., 192:224]
    elif Gn > 1:
        N.poison_allocator(cuda)
        got = ops.resize_bilinear(xd, (Ho, Wo), groups=Gn)
    else:
        N.poison_allocator(cuda)
        got = ops.resize_bilinear(xd[0], (Ho, Wo))[None]
    _bits_equal(got, want, 'resize')
    G.assert_within(got, y64, G.resize_bar(corners), 'resize')


def test_upsample_prob_vol_bits_of_the_oracle(cuda):
    """model.upsample_prob_vol (the resize at C = 1, plane by plane into the planes of one buffer) on a (1, 5, 6, 7) volume:
    the oracle's bits."""
    from atvsnet_amd.atvsnet import model
    vol = torch.randn((1, 5, 6, 7), generator=_gen(230))
    N.poison_allocator(cuda)
    _bits_equal(model.upsample_prob_vol(vol.to(cuda)), OM.upsample_prob_vol(vol), 'upsample_prob_vol')


# ------------------------------------------------------------------------------------------- copy, stack, concat, add: bitwise

@pytest.mark.parametrize('rows', [1, 257])
@pytest.mark.parametrize('C', [1, 3, 32])
def test_copy_channels_both_offsets(cuda, C, rows):
    """copy_channels_kernel with src_off > 0 and dst_off > 0 together; C = 1, 3, 32; 1 row and 257 rows (more than one
    workgroup at every C but 1 x 1); the destination NaN-filled, its other channels untouched."""
    from atvsnet_amd import ops
    src = torch.randn((rows, C + 7), generator=_gen(300 + C))
    dst = N.nan_output((rows, C + 9), cuda)
    ops.copy_channels(src.to(cuda), dst, C, src_off=5, dst_off=3)
    N.assert_bits_kept(dst, 3, 3 + C)
    _bits_equal(dst[:, 3:3 + C], src[:, 5:5 + C], 'copy_channels')


@pytest.mark.parametrize('n,shape,dim', [(2, (3, 5, 8), 0), (16, (6, 10), 0), (3, (4,), 0),      # stack_kernel
                                         (17, (2, 6), 0), (3, (5, 3), 0),                          # the copy_channels fallback
                                         (2, (1, 6, 8, 1), 1), (2, (1, 6, 7, 1), 1)])              # model.py's dim = 1 form
def test_stack_bits(cuda, n, shape, dim):
    """ops.stack against torch.stack, bit for bit, into a NaN-poisoned allocation.  atvs_stack (one launch): 2 tensors, 16
    tensors (every pointer slot), numel = 4 (one float4).  The fallback through copy_channels: 17 tensors (more than the
    16 slots), numel % 4 != 0 (15).  dim = 1 behind a unit axis: init_depth_images of model.py, on the kernel (48 values) and
    on the fallback (42)."""
    from atvsnet_amd import ops
    ts = [torch.randn(shape, generator=_gen(400 + i)) for i in range(n)]
    td = [t.to(cuda) for t in ts]
    N.poison_allocator(cuda)
    _bits_equal(ops.stack(td, dim), torch.stack(ts, dim), 'stack')


def test_concat_channels_bits(cuda):
    """concat_channels of widths (8, 3, 1, 32): every dst_off, bit for bit against torch.cat."""
    from atvsnet_amd import ops
    ts = [torch.randn((3, 5, 7, c), generator=_gen(500 + c)) for c in (8, 3, 1, 32)]
    td = [t.to(cuda) for t in ts]
    N.poison_allocator(cuda)
    _bits_equal(ops.concat_channels(td), torch.cat(ts, -1), 'concat_channels')


@pytest.mark.parametrize('n', [1029, 1030, 1031, 3, 1])
def test_add_n_scalar_tail(cuda, n):
    """add_n_kernel's scalar tail: n % 4 = 1, 2, 3 behind whole float4s (and a second workgroup), and n < 4 where the tail is
    all there is; two and three tensors; bit for bit (a + b) + c."""
    from atvsnet_amd import ops
    a, b, c = [torch.randn((n,), generator=_gen(600 + i)) for i in range(3)]
    ad, bd, cd = a.to(cuda), b.to(cuda), c.to(cuda)
    N.poison_allocator(cuda)
    _bits_equal(ops.add_n([ad, bd]), a + b, 'a + b')
    _bits_equal(ops.add_n([ad, bd, cd]), (a + b) + c, '(a + b) + c')


def test_add_n_four_tensors_chain(cuda):
    """Four tensors: one launch for (a + b) + c, a second for + d; into a NaN-filled `out` as well."""
    from atvsnet_amd import ops
    ts = [torch.randn((5, 6, 7), generator=_gen(610 + i)) for i in range(4)]
    td = [t.to(cuda) for t in ts]
    want = ((ts[0] + ts[1]) + ts[2]) + ts[3]
    N.poison_allocator(cuda)
    _bits_equal(ops.add_n(td), want, 'add_n of four')
    out = N.nan_output((5, 6, 7), cuda)
    assert ops.add_n(td, out=out) is out
    _bits_equal(out, want, 'add_n of four into out')


# -------------------------------------------------------------------------------------------------------------------- AANet

AANET_VIEWS = [1, 2, 3, 5, 8, 9, 12, 16]       # aanet_combine_kernel<1 .. 8> | aanet_combine_generic_kernel
AANET_VOXELS = [1, 127, 129, 6 * 8 * 10]       # one lane pair; odd counts either side of half a workgroup; the old test's


def _dev(ts, cuda):
    return [t.to(cuda) for t in ts]


@pytest.mark.parametrize('regime', G.REGIMES)
@pytest.mark.parametrize('nv', AANET_VIEWS)
def test_aanet_combine_per_element(cuda, nv, regime):
    """atvs_aanet_combine, |got - y64| <= REL * cond per element (glue_ref.aanet_combine_cond): 1, 2, 3, 5, 8 views on the
    templated kernel, 9, 12, 16 on aanet_combine_generic_kernel; V = 1, 127, 129 (odd voxel counts: the last workgroup is
    ragged) and 480; scores N(0,1), spread over 30, spread over 200 (a saturated softmax on the hardware exp2 and rcp), and
    log-uniform X over 2^-20 .. 2^10 with mixed signs.  S, R >= 0 as after the ReLU."""
    from atvsnet_amd import ops
    worst = 0.0
    for V in AANET_VOXELS:
        srs, xs = G.aanet_case(nv, V, regime)
        N.poison_allocator(cuda)
        got = ops.aanet_combine(_dev(srs, cuda), _dev(xs, cuda))
        r = N.assert_elementwise(got, G.aanet_combine64(srs, xs), G.aanet_combine_cond(srs, xs), G.REL, 0.0,
                                 'aanet_combine %d views V=%d %s' % (nv, V, regime))
        worst = max(worst, r)
    print('aanet_combine %d views %s: largest err / cond %.3e' % (nv, regime, worst))


def _known_cases(nv, V, seed):
    """(srs, xs, want, what) with exact answers.  Scores N(0,1) clamped at 0; the chosen views get R + 200."""
    out = []
    g = _gen(seed)
    srs, xs = G.aanet_case(nv, V, 'normal', seed)
    X = torch.stack(xs, 0)
    # one winner per element: every other view is at least 180 below it, e^-180 = 0 in fp32
    win = torch.randint(0, nv, (V, 8), generator=g)
    sat = [t.clone() for t in srs]
    for n in range(nv):
        sat[n][:, 8:] += 200.0 * (win == n)
    out.append((sat, xs, torch.gather(X, 0, win[None])[0], 'saturated'))
    if nv >= 2:
        # two distinct views a, b with the same S and R (+ 200), the rest 200 below: (x_a + x_b) / 2
        a = torch.randint(0, nv, (V, 8), generator=g)
        b = (a + torch.randint(1, nv, (V, 8), generator=g)) % nv
        SR = torch.stack(srs, 0).clone()                               # (nv, V, 16)
        shared = SR[0].clone()
        shared[:, 8:] += 200.0
        for n in range(nv):
            pick = ((a == n) | (b == n))
            SR[n] = torch.where(torch.cat([pick, pick], -1), shared, SR[n])
        xa, xb = torch.gather(X, 0, a[None])[0], torch.gather(X, 0, b[None])[0]
        out.append(([SR[n].contiguous() for n in range(nv)], xs, (xa + xb) * 0.5, 'tie'))
    return out


@pytest.mark.parametrize('nv', AANET_VIEWS)
def test_aanet_combine_known_answers(cuda, nv):
    """Exact answers, bit for bit, V = 129.  One view: out == X in every regime (the softmax of one score is 1).  A saturated
    softmax (one view 200 above the rest): out == the winning view's X.  Two views with equal scores, the rest 200 below:
    out == float32(x_a + x_b) * 0.5 -- an exact tie gives two weights of exactly one half."""
    from atvsnet_amd import ops
    V = 129
    if nv == 1:
        for regime in G.REGIMES:
            srs, xs = G.aanet_case(1, V, regime)
            N.poison_allocator(cuda)
            _bits_equal(ops.aanet_combine(_dev(srs, cuda), _dev(xs, cuda)), xs[0], 'one view, %s' % regime)
    for srs, xs, want, what in _known_cases(nv, V, 3):
        N.poison_allocator(cuda)
        _bits_equal(ops.aanet_combine(_dev(srs, cuda), _dev(xs, cuda)), want, '%s, %d views' % (what, nv))


def _sharded(ops, srs, xs, parts):
    """Stages 0, 1, 2 per part (rank), the partials combined as an all-reduce would (SUM, MAX, SUM), then the division ->
    (out, per-part stage 0, total, per-part stage 1)."""
    lo = [sum(parts[:i]) for i in range(len(parts))]
    sl = [slice(a, a + n) for a, n in zip(lo, parts)]
    s0 = [ops.aanet_partial(srs[s], xs[s], 0) for s in sl]
    ssum = torch.stack(s0, 0).sum(0)
    s1 = [ops.aanet_partial(srs[s], xs[s], 1, ssum=ssum) for s in sl]
    umax = torch.stack(s1, 0).max(0).values
    acc = torch.stack([ops.aanet_partial(srs[s], xs[s], 2, ssum=ssum, umax=umax) for s in sl], 0).sum(0)
    return ops.divide(acc[1].contiguous(), acc[0].contiguous()), s0, ssum, s1, sl


@pytest.mark.parametrize('regime', G.REGIMES)
@pytest.mark.parametrize('parts', [(2, 3), (9, 7)])
def test_aanet_sharded_over_ranks(cuda, parts, regime):
    """aanet_partial_kernel with the views split over two ranks, 5 = 2 + 3 and 16 = 9 + 7; V = 127 and 480.  Stage 0 (sum of
    the local S) and stage 1 (max of the local (R - S) + S_sum) are the torch fp32 results in view order, bit for bit; the final
    map, after torch's sum / max / sum over the ranks and ops.divide, is within REL * cond of float64 (the ranks' S_sum differs
    from the single-rank one in its last bit: a shift of every score alike)."""
    from atvsnet_amd import ops
    worst = 0.0
    for V in (127, 480):
        srs, xs = G.aanet_case(sum(parts), V, regime, seed=1)
        N.poison_allocator(cuda)
        got, s0, ssum, s1, sl = _sharded(ops, _dev(srs, cuda), _dev(xs, cuda), parts)
        for k, s in enumerate(sl):
            a = torch.zeros(V, 8)
            for t in srs[s]:
                a = a + t[:, :8]
            _bits_equal(s0[k], a, 'stage 0 of rank %d' % k)
            m = torch.full((V, 8), float('-inf'))
            for t in srs[s]:
                m = torch.maximum(m, (t[:, 8:] - t[:, :8]) + ssum.cpu())
            _bits_equal(s1[k], m, 'stage 1 of rank %d' % k)
        r = N.assert_elementwise(got, G.aanet_combine64(srs, xs), G.aanet_combine_cond(srs, xs), G.REL, 0.0,
                                 'sharded %s V=%d %s' % (parts, V, regime))
        worst = max(worst, r)
    print('aanet sharded %s %s: largest err / cond %.3e' % (parts, regime, worst))


def test_aanet_sharded_known_answers(cuda):
    """The exact answers of test_aanet_combine_known_answers through the sharded form, 5 views as 2 + 3: a denominator of
    exactly 1 or 2 divides exactly."""
    from atvsnet_amd import ops
    for srs, xs, want, what in _known_cases(5, 129, 4):
        N.poison_allocator(cuda)
        got = _sharded(ops, _dev(srs, cuda), _dev(xs, cuda), (2, 3))[0]
        _bits_equal(got, want, 'sharded, %s' % what)


@pytest.mark.parametrize('n', [4, 1028, 8 * 480])
def test_divide_bits(cuda, n):
    """divide_kernel: the correctly rounded fp32 quotient, bit for bit; magnitudes 2^-20 .. 2^20, both signs; one float4, a
    ragged second workgroup, the production form."""
    from atvsnet_amd import ops
    g = _gen(700 + n)
    num = torch.randn((n,), generator=g) * torch.exp2(torch.rand((n,), generator=g) * 40 - 20)
    den = (torch.rand((n,), generator=g) + 0.5) * torch.exp2(torch.rand((n,), generator=g) * 40 - 20)
    den = torch.where(torch.rand((n,), generator=g) < 0.5, -den, den)
    N.poison_allocator(cuda)
    _bits_equal(ops.divide(num.to(cuda), den.to(cuda)), num / den, 'divide')
