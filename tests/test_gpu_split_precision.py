"""-m gpu: every launch form of the convolution kernels held element by element to a float64 evaluation (tests/numerics.py):
|got - ref64| <= rel * cond + floor, at the SPLIT bar for the split-operand kernels and at the FP32_MFMA bar for
their fp32 forms -- the kernels the overflow recompute falls back to.

One row per launch form; each row asserts the kernel family it reaches (ops.conv_plan, or the entry point's predicate) and
runs six operand regimes: randn, post-ReLU, scale 1e-3, log-uniform 1e-4 ... 1e2 per channel, below 2^-14 (both fp16 pieces
subnormal), and a few entries near 6e4 with finite outputs.  Every run is under poison_allocator with NaN-bordered inputs:
a read past an input, an unwritten output or statistics row, or a write outside the output's channel slice turns up as a
NaN or a changed bit.  The batch-norm moments of each output are checked against float64 moments of what was written, and
must not raise the sticky non-finite flag.  Rows with G = 3 scale the samples 1e-3, 1, 1e3 (where the range allows).

Rows whose input is lazy (a pending batch norm, or a sum of two, formed while the kernel stages it) run a seventh regime,
`offset` (tests/bn_ref.py): raw inputs whose channel means are 50 to 2e4 standard deviations, with each sample's own batch
moments as parameters.  There the rounding of the on-load transform, about u |mean * rstd| and not u |value|, is what dominates,
so cond is numerics.cond_on_load -- the same operator on bn_cond = |x s| + |m s| + |b| of each lazy term -- and rel is the row's
own plus 2^-22: the transform moves a normalised input by at most 2u * bn_cond, a two-term sum adds u (cond_a + cond_b), and
3u < 2^-22.

79 rows: 35 at the SPLIT bar and 44 at FP32_MFMA, of which 31 run under cfg=FP32 -- a twin of every split row whose fp32 form the
fp32 path launches (tests/golden/conv_dispatch.json's split16=0 cases; tests/test_numerics_bar.py checks that each of their
events has a row), the three-launch residual unit, and the AANet module as score convolutions + ops.aanet_combine / the
ops.aanet_partial stages.  The one fp32 twin that is refused, a lazy input to conv2d_lds, is asserted below the table."""
import collections

import numpy as np
import pytest
import torch

from oracle import nets
from oracle import tf_ops as T

import bn_ref
import numerics as N
from numerics import FP32_MFMA, SPLIT

pytestmark = pytest.mark.gpu

REGIMES = ('randn', 'relu', 'small', 'loguniform', 'subnormal', 'near_max')
OFFSET = 'offset'                  # the seventh regime, of the rows with a lazy input only
OFFSET_REL = 2.0 ** -22
_SCALE = {'randn': 1.0, 'relu': 1.0, 'small': 1e-3, 'loguniform': 1.0, 'subnormal': 2.0 ** -16, 'near_max': 1.0, OFFSET: 1.0}
SAMPLE_SCALES = (1e-3, 1.0, 1e3)

# family: what the row asserts it reaches; split: its split-operand family (the ops.split_on names, xb = conv_xb.hip,
# aanet_b = aanet_b.hip) or None; cfg: the ops.configure switches it runs under
# maker: the function that built the row (tests/test_numerics_bar.py maps the entry points of conv_dispatch.json to it)
Row = collections.namedtuple('Row', 'name family split bar run cfg lazy maker')
Row.__new__.__defaults__ = (False, None)             # lazy: the input is formed on load, the row runs the offset regime too
FP32 = {'split16': False}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _input(shape, seed, regime, grouped=False):
    """A CPU float32 operand (channel-last, channels on the last axis) of the regime; grouped: samples scaled 1e-3, 1, 1e3."""
    g = _gen(seed)
    x = torch.randn(shape, generator=g)
    if regime == 'relu':
        x = x.clamp(min=0)
    elif regime == 'small':
        x = x * 1e-3
    elif regime == 'loguniform':
        x = x * 10.0 ** (torch.rand(shape[-1], generator=g) * 6 - 4)
    elif regime == 'subnormal':
        x = (x * 2.0 ** -16).clamp(-2.0 ** -14 * 0.99, 2.0 ** -14 * 0.99)
    elif regime == 'near_max':
        flat = x.view(-1)
        idx = torch.randperm(flat.numel(), generator=g)[:6]
        flat[idx] = torch.tensor([6.0e4, -6.0e4, 5.9e4, -5.95e4, 6.05e4, 6.1e4])[:idx.numel()]
    if grouped and shape[0] == 3 and regime in ('randn', 'relu', 'small'):
        x = x * torch.tensor(SAMPLE_SCALES).reshape((3,) + (1,) * (len(shape) - 1))
    return x


def _weights(shape, seed):
    fan = int(np.prod(shape[:-1]))
    return torch.randn(shape, generator=_gen(seed)) * (2.0 / fan) ** 0.5


def _params(G, C, seed, regime):
    """(G,3,C) batch-norm parameters (mean, rstd, beta) of a lazy input; rstd <= 1 keeps a near-6e4 raw value in range."""
    g, s = _gen(seed), _SCALE[regime]
    return torch.stack([torch.randn(G, C, generator=g) * 0.1 * s, torch.rand(G, C, generator=g) * 0.5 + 0.5,
                        torch.randn(G, C, generator=g) * 0.1 * s], 1).contiguous()


def _dev(t, dev):
    return N.nan_bordered(t.to(dev))


def _pending(shape, seed_x, seed_p, regime, dev, relu):
    """A lazy input of the regime: the operand and parameters of _input / _params, or in the offset regime a raw tensor with
    large channel means and its own batch moments (bn_ref.operand)."""
    from atvsnet_amd import ops
    if regime == OFFSET:
        x, par = bn_ref.operand(OFFSET, shape, seed_x)
    else:
        x, par = _input(shape, seed_x, regime, grouped=True), _params(shape[0], shape[-1], seed_p, regime)
    return ops.PendingBN(_dev(x, dev), par.to(dev), relu=relu)


def _cond(regime):
    return N.cond_on_load if regime == OFFSET else N.cond


def _relu(t, on=True):
    return t.clamp(min=0) if on else t


def _winograd_cond(x, w):
    """cond of conv_xw.hip's Winograd F(2,3) along y (its fp32 form): the products are U_p * t_p with U_p sums of the three y
    taps and t_p sums of two of the four input rows of an output-row pair, so an accumulation error scales with
    sum_(kd,kx,ci) (sum_ky |w|) * (sum of |x| over the rows y-2 .. y+2), not with sum |x||w|."""
    k5 = w.double().abs().sum(1, keepdim=True).expand(-1, 5, -1, -1, -1)
    return T.conv(x.double().abs(), k5, 1, 'SAME')


def _winograd_cond_terms(terms, w, regime):
    """_winograd_cond of an input that is the sum of `terms` (tensors, or lazy inputs formed on load): |x| of a tensor, |its
    float64 normalised value| of a lazy term, and in the offset regime its bn_cond (numerics.cond_on_load's rule)."""
    def mag(t):
        if not N._is_pending(t):
            return t.double().abs()
        return bn_ref.bn_cond(t.raw, t.params) if regime == OFFSET else N.term64(t).abs()
    return _winograd_cond(sum(mag(t) for t in terms), w)


class Case(object):
    """One launch's result: got (CPU) against want64 / cond64, the absolute floor, and what to check beside the values."""

    def __init__(self, got, want64, cond64, floor, stats=None, kept=None, fold=(1,)):
        self.got, self.want64, self.cond64, self.floor = got, want64, cond64, floor
        self.stats = stats            # (Stats, device output of the same values, channels) or None
        self.fold = fold              # the column folds the launch form may report (Stats.fold)
        self.kept = kept              # (NaN-filled device buffer, lo, hi) or None


def _check_stats(st, y, C, what, fold=(1,)):
    """The per-sample moments the launch wrote (all rows, the first C channels) against float64 moments of y; then
    bn_params must not raise the sticky non-finite flag."""
    from atvsnet_amd import ops
    G = st.groups
    part = st.partial.detach().cpu()
    # every launch form in this table but one writes its rows unfolded; fold > 1 is the tiled transposed-convolution fallback
    # (the fp32 64 -> 32 layer), whose column k * C + c holds the share of parity class k in channel c
    assert st.fold in fold, '%s: statistics folded by %d' % (what, st.fold)
    assert bool(torch.isfinite(part[..., :st.fold * C]).all()), '%s: a statistics row holds a non-finite value' % what
    s = part.reshape(G, -1, 2, st.cpad).sum(1)[..., :st.fold * C].reshape(G, 2, st.fold, C).sum(2)
    v = y.detach().cpu().double().reshape(G, -1, C)
    for k, want in ((0, v.sum(1)), (1, (v * v).sum(1))):
        tol = 1e-5 * (v.abs() if k == 0 else v * v).sum(1) + 1e-30
        bad = (s[:, k] - want).abs() > tol
        assert not bool(bad.any()), '%s: moment %d of sample/channel %s: %.9e vs %.9e' % (
            what, k, tuple(bad.nonzero()[0].tolist()), float(s[:, k][bad][0]), float(want[bad][0]))
    ops.bn_params(st, C, torch.empty(1, device=y.device))
    assert not ops.nonfinite_seen(y.device), '%s: bn_params raised the non-finite flag' % what


# ------------------------------------------------------------------------------------------------------- ops.conv rows

def conv_row(name, family, split, bar, G, sp, cin, cout, stride=1, k=3, dilation=1, explicit_pad=None, lazy=None, bias=True,
             relu=True, cfg=None, slice_out=True, winograd=False, residual=False):
    """residual: a tensor of the output's shape added in the epilogue (a residual unit's conv3); it stays out of cond and the
    floor gains the rounding of that add (_residual_floor)."""
    nsp = len(sp)
    ks = (k,) * nsp

    def run(dev, regime):
        from atvsnet_amd import ops
        x = None if lazy else _input((G,) + sp + (cin,), 1, regime, grouped=True)
        w = _weights(ks + (cin, cout), 2)
        b = torch.randn(cout, generator=_gen(3)) * 0.1 * _SCALE[regime] if bias else None
        padding = 'SAME' if explicit_pad is None else 'VALID'
        out_spec = (cout + 8, 4) if slice_out else None
        plan = ops.conv_plan(sp, k, cin, cout, stride, dilation, padding if explicit_pad is None else explicit_pad,
                             bias, residual, False, out_spec, lazy)
        assert plan.family == family, '%s: conv_plan chose %s' % (name, plan.family)
        assert plan.on_load == bool(lazy), '%s: the lazy input is not formed on load' % name
        if family in ('conv2d_lds', 'conv1x1'):
            pk = (ops.pack_conv2d_lds if family == 'conv2d_lds' else
                  (lambda kk, ww, dd: ops.pack_conv1x1(kk, ww, cin, dd)))((name, 'probe'), w.numpy(), dev)
            assert (pk.kind in ('b', '_b')) == (bar is SPLIT), '%s: packed for %r' % (name, pk.kind)
        if family == 'xp':
            assert ops.pack_conv_xp((name, 'probe'), w.numpy(), dev).kind == ('xb' if bar is SPLIT else 'xw')
        kw = dict(stride=stride, dilation=dilation, explicit_pad=explicit_pad, relu=relu, want_stats=True, groups=G,
                  bias=None if b is None else b.to(dev))
        terms = []
        if lazy is None:
            xin = _dev(x, dev)
            terms = [x]
        else:
            pa = _pending((G,) + sp + (cin,), 1, 4, regime, dev, True)
            kw.update(in_params=pa.params, in_relu=True)
            xin, terms = pa.raw, [pa]
            if lazy == 'sum':
                pb = _pending((G,) + sp + (cin,), 5, 6, regime, dev, False)
                kw.update(in_sum=(pb.raw, pb.params, False))
                terms.append(pb)
        buf = None
        if slice_out:
            buf = N.nan_output((G,) + plan.outs[3 - nsp:] + (cout + 8,), dev)
            kw.update(out=buf, y_coff=4)
        res = None
        if residual:
            res = _input((G,) + plan.outs[3 - nsp:] + (cout,), 7, regime, grouped=True)
            kw.update(residual=_dev(res, dev))
        y, st = ops.conv(xin, name, w.numpy(), **kw)
        ys = buf[..., 4:4 + cout] if slice_out else y

        def op(*a):
            xs, (wt, bt) = a[:-2], a[-2:]
            s = xs[0] if len(xs) == 1 else xs[0] + xs[1]
            return _relu(T.conv(s, wt, stride, padding, dilation, bias=bt, explicit_pad=explicit_pad), relu)
        bb = b if b is not None else torch.zeros(cout)
        cnd = _winograd_cond(x, w) + bb.double().abs() if winograd else _cond(regime)(op, *terms, w, bb)
        want, floor = N.ref64(op, *terms, w, bb), N.floor_of(w, bar)
        if residual:
            want = want + res.double()
            floor = _residual_floor(want, w, bar=bar)
        return [Case(ys.cpu(), want, cnd, floor, stats=(st, ys, cout), kept=(buf, 4, 4 + cout) if slice_out else None)]
    return Row(name, family, split, bar, run, cfg or {}, bool(lazy), 'conv_row')


# ------------------------------------------------------------------------------------------------ the other entry points

def _residual_floor(want, *ws, bar=SPLIT):
    """The floor of a residual unit: the weights' floors plus the fp32 rounding of the final residual add (2^-23 |y|).
    The residual itself (exact fp32) stays out of cond, so a defect in the branch is measured against the branch alone."""
    return sum(N.floor_of(w, bar) for w in ws) + 2.0 ** -23 * want.abs()


def tail_row(name, G, H, W, C, dil):
    def run(dev, regime):
        from atvsnet_amd import ops
        assert ops.conv2d_tail_ok(C, dil, H, W)
        x = _input((G, H, W, C), 11, regime, grouped=True)
        res = _input((G, H, W, C), 12, regime, grouped=True)
        w2, w3 = _weights((3, 3, C, C), 13), _weights((1, 1, C, C), 14)
        b2, b3 = (torch.randn(C, generator=_gen(s)) * 0.1 * _SCALE[regime] for s in (15, 16))
        y, st = ops.conv2d_tail(_dev(x, dev), ((name, 2), (name, 3)), w2.numpy(), b2.to(dev), w3.numpy(), b3.to(dev),
                                residual=_dev(res, dev), dilation=dil)

        def branch(x, w2, b2, w3, b3):
            return T.conv(_relu(T.conv(x, w2, 1, 'SAME', dil, bias=b2)), w3, 1, 'SAME', bias=b3)
        a = (x, w2, b2, w3, b3)
        want = N.ref64(branch, *a) + res.double()
        return [Case(y.cpu(), want, N.cond(branch, *a), _residual_floor(want, w2, w3), stats=(st, y, C))]
    return Row(name, 'conv2d_tail', 'btl', SPLIT, run, {}, False, 'tail_row')


def bottleneck_row(name, G, H, W, C):
    def run(dev, regime):
        from atvsnet_amd import ops
        assert ops.bottleneck_ok(C, 1, H, W)
        pend = _pending((G, H, W, C), 21, 22, regime, dev, True)
        x = pend.raw.cpu()
        ws = [_weights(s, 23 + i) for i, s in enumerate(((1, 1, C, C), (3, 3, C, C), (1, 1, C, C)))]
        bs = [torch.randn(C, generator=_gen(26 + i)) * 0.1 * _SCALE[regime] for i in range(3)]
        y, st = ops.bottleneck(pend.raw, pend.params, tuple((name, i) for i in range(3)), ws[0].numpy(), bs[0].to(dev),
                               ws[1].numpy(), bs[1].to(dev), ws[2].numpy(), bs[2].to(dev))

        def branch(xn, w1, b1, w2, b2, w3, b3):
            r = _relu(T.conv(xn, w1, 1, 'SAME', bias=b1))
            r = _relu(T.conv(r, w2, 1, 'SAME', bias=b2))
            return T.conv(r, w3, 1, 'SAME', bias=b3)
        a = (pend, ws[0], bs[0], ws[1], bs[1], ws[2], bs[2])
        want = N.ref64(branch, *a) + x.double()
        return [Case(y.cpu(), want, _cond(regime)(branch, *a), _residual_floor(want, *ws), stats=(st, y, C))]
    return Row(name, 'bottleneck', 'btl', SPLIT, run, {}, True, 'bottleneck_row')


def residual_unit_row(name, G, H, W, C, dil):
    """The identity-shortcut residual unit as the fp32 path runs it (cnn_wrapper/network.py bottleneck), three launches where the
    split path runs ops.bottleneck (dil 1) or conv1 + ops.conv2d_tail (the 128-channel dilated units): conv1 1x1 with the
    pre-activation batch norm formed on load, conv2 3x3 on conv2d_lds, conv3 1x1 with residual=.  bottleneck_row's operands and
    float64 reference (with the dilation); r1 and r2 pass through memory as fp32, which the propagated cond covers as it does
    the fused unit's registers."""
    def run(dev, regime):
        from atvsnet_amd import ops
        assert not ops.bottleneck_ok(C, dil, H, W) and not ops.conv2d_tail_ok(C, dil, H, W)
        assert ops.conv_plan((H, W), 1, C, C, bias=True, lazy='bn')[:2] == ('conv1x1', True)
        assert ops.conv_plan((H, W), 3, C, C, dilation=dil, bias=True)[:2] == ('conv2d_lds', False)
        assert ops.conv_plan((H, W), 1, C, C, bias=True, residual=True)[:2] == ('conv1x1', False)
        assert ops.pack_conv1x1((name, 'probe1'), np.zeros((C, C), np.float32), C, dev).kind == ''
        assert ops.pack_conv2d_lds((name, 'probe2'), np.zeros((3, 3, C, C), np.float32), dev).kind == 'lds'
        pend = _pending((G, H, W, C), 21, 22, regime, dev, True)
        x = pend.raw.cpu()
        ws = [_weights(s, 23 + i) for i, s in enumerate(((1, 1, C, C), (3, 3, C, C), (1, 1, C, C)))]
        bs = [torch.randn(C, generator=_gen(26 + i)) * 0.1 * _SCALE[regime] for i in range(3)]
        r1 = ops.conv(pend.raw, (name, 0), ws[0].numpy(), bias=bs[0].to(dev), relu=True, groups=G, in_params=pend.params,
                      in_relu=True)
        r2 = ops.conv(r1, (name, 1), ws[1].numpy(), dilation=dil, bias=bs[1].to(dev), relu=True, groups=G)
        y, st = ops.conv(r2, (name, 2), ws[2].numpy(), bias=bs[2].to(dev), residual=pend.raw, want_stats=True, groups=G)

        def branch(xn, w1, b1, w2, b2, w3, b3):
            r = _relu(T.conv(xn, w1, 1, 'SAME', bias=b1))
            r = _relu(T.conv(r, w2, 1, 'SAME', dil, bias=b2))
            return T.conv(r, w3, 1, 'SAME', bias=b3)
        a = (pend, ws[0], bs[0], ws[1], bs[1], ws[2], bs[2])
        want = N.ref64(branch, *a) + x.double()
        return [Case(y.cpu(), want, _cond(regime)(branch, *a), _residual_floor(want, *ws, bar=FP32_MFMA), stats=(st, y, C))]
    return Row(name, 'residual_unit', None, FP32_MFMA, run, FP32, True, 'residual_unit_row')


def siblings_row(name, G, D, H, W, cin, bar, cfg=None, lazy=None):
    """lazy='bn': the input is one pending batch norm + ReLU, normalised while it is staged (Cin % 16 == 0); lazy='sum': the sum
    of two pending batch norms, formed while it is staged (Cin == 8, the U-Net's stack inputs)."""
    def run(dev, regime):
        from atvsnet_amd import ops
        assert ops.siblings_ok((D, H, W), cin, 8, 16)
        w1, w2 = _weights((3, 3, 3, cin, 8), 32), _weights((3, 3, 3, cin, 16), 33)
        assert ops.pack_conv_xp((name, 'probe'), w1.numpy(), dev).kind == ('xb' if bar is SPLIT else 'xw')
        if lazy is None:
            x = _input((G, D, H, W, cin), 31, regime, grouped=True)
            src, terms = _dev(x, dev), [x]
        else:
            terms = [_pending((G, D, H, W, cin), 31, 34, regime, dev, True)]
            if lazy == 'sum':
                terms.append(_pending((G, D, H, W, cin), 35, 36, regime, dev, False))
            src = terms[0] if lazy == 'bn' else ops.PendingSum(terms)
            assert ops.siblings_prologue_ok(src)
        (y, st), (y2, st2) = ops.conv_siblings(src, (name, 1), w1.numpy(), (name, 2), w2.numpy(), groups=G)
        assert all(t._final is None for t in terms if lazy), '%s: the lazy input was materialised' % name
        out = []
        for yy, s, w, stride, c in ((y, st, w1, 1, 8), (y2, st2, w2, 2, 16)):
            def op(*a, stride=stride):
                xs, w = a[:-1], a[-1]
                return T.conv(xs[0] if len(xs) == 1 else xs[0] + xs[1], w, stride, 'SAME')
            cnd = _winograd_cond_terms(terms, w, regime) if (stride == 1 and bar is FP32_MFMA) else \
                _cond(regime)(op, *terms, w)
            out.append(Case(yy.cpu(), N.ref64(op, *terms, w), cnd, N.floor_of(w, bar), stats=(s, yy, c)))
        return out
    return Row(name, 'xp_siblings', 'xb' if bar is SPLIT else None, bar, run, cfg or {}, bool(lazy), 'siblings_row')


def plane_row(name, G, D, H, W, cv, cc, bar, cfg=None):
    """conv_split: the D-varying channels on the x-pair kernel, the D-constant ones as a depth-plane bias (2-D convolution)."""
    def run(dev, regime):
        from atvsnet_amd import ops
        var = _input((G, D, H, W, cv), 41, regime, grouped=True)
        const = _input((G, H, W, cc), 42, regime, grouped=True)
        cmap = [('c', i) for i in range(cc)] + [('v', i) for i in range(cv)]
        w = _weights((3, 3, 3, cc + cv, 8), 43)
        plan = ops.conv_plan((D, H, W), 3, cv, 8, plane_bias=True)
        assert plan.family == 'xp'
        assert ops.pack_conv_xp((name, 'probe'), w[..., cc:, :].numpy(), dev).kind == ('xb' if bar is SPLIT else 'xw')
        sv = ops.SplitVolume(_dev(var, dev), _dev(const, dev), cmap)
        y, st = ops.conv_split(sv, name, w.numpy(), want_stats=True)

        def op(var, const, w):
            dense = torch.cat([const[:, None].expand(-1, D, -1, -1, -1), var], -1)
            return T.conv(dense, w, 1, 'SAME')
        cnd = N.cond(op, var, const, w)
        if bar is FP32_MFMA:
            # conv_xw.hip's Winograd products for the D-varying channels (_winograd_cond), sum |x||w| for the plane bias
            cnd = _winograd_cond(var, w[..., cc:, :]) + N.cond(op, torch.zeros_like(var), const, w)
        return [Case(y.cpu(), N.ref64(op, var, const, w), cnd, N.floor_of(w, bar), stats=(st, y, 8))]
    return Row(name, 'xp_plane_bias', 'xb' if bar is SPLIT else None, bar, run, cfg or {}, False, 'plane_row')


def into_plane_row(name, G, D, H, W, cv, cc, pieces, plane=2):
    """conv_split_into_plane: the photo stem written into one plane of the chunk-planar concat (B, 4, planar_stride).  With
    pieces the D-varying input is the chunk-planar fp16 pieces warp_planes writes (built here from DESIGN.md 8's split)."""
    def run(dev, regime):
        from atvsnet_amd import ops
        var = _input((G, D, H, W, cv), 101, regime, grouped=True)
        const = _input((G, H, W, cc), 102, regime, grouped=True)
        cmap = [('c', i) for i in range(cc)] + [('v', i) for i in range(cv)]
        w = _weights((3, 3, 3, cc + cv, 8), 103)
        assert ops._xkind() == 'xb'
        ps, n, K = ops.planar_stride(D, H, W), D * H * W * 8, cv // 8
        if pieces:
            h0, h1 = N.emulate_split(var.reshape(G, D, H, W, K, 8).permute(0, 4, 1, 2, 3, 5))     # (G, K, D, H, W, 8)
            pc = torch.full((G, K, ps), float('nan'))
            pc[..., :n] = torch.stack([h0.half(), h1.half()], 2).reshape(G, K, -1).view(torch.float32)
            sv = ops.SplitVolume(_dev(pc, dev), _dev(const, dev), cmap, planar=(D, H, W), pieces=True)
        else:
            sv = ops.SplitVolume(_dev(var, dev), _dev(const, dev), cmap)
        buf = N.nan_output((G, 4, ps), dev)
        st = ops.conv_split_into_plane(sv, name, w.numpy(), buf, plane, (D, H, W))
        got = ops.planar_view(buf, D, H, W)[:, plane]
        # everything but the plane's n values (the other planes, the padding behind every plane) keeps its NaN bits
        bits = buf.cpu().view(torch.int32).clone()
        bits[:, plane, :n] = torch.full((), float('nan')).view(torch.int32)
        assert bool((bits == torch.full((), float('nan')).view(torch.int32)).all()), '%s: wrote outside its plane' % name

        def op(var, const, w):
            dense = torch.cat([const[:, None].expand(-1, D, -1, -1, -1), var], -1)
            return T.conv(dense, w, 1, 'SAME')
        return [Case(got.cpu(), N.ref64(op, var, const, w), N.cond(op, var, const, w), N.floor_of(w, SPLIT),
                     stats=(st, got, 8))]
    return Row(name, 'xp_into_plane', 'xb', SPLIT, run, {}, False, 'into_plane_row')


def deconv_row(name, family, split, bar, G, D, H, W, cin, cout, summed=False, cfg=None):
    def run(dev, regime):
        from atvsnet_amd import ops
        w = _weights((3, 3, 3, cout, cin), 52)
        lib = ops._lib.lib()
        fold = (1,)
        if family == 'deconv_halves':
            assert not ops.deconv_up_ok(cin, cout) and cout == 32 and bool(lib.atvs_deconv_up_b_supported(cin, 16))
        elif family in ('deconv_tiled', 'deconv_gather'):
            # the fp32 64 -> 32 layer (no deconv_up form, and deconv_halves is the split path's): W >= 12 runs all parity classes
            # of a class group from one staged tile of conv_tiled (its statistics folded by the classes per launch), a narrower
            # map one gather launch per class
            assert not ops.deconv_up_ok(cin, cout) and bar is FP32_MFMA and cout % 4 == 0 and cout <= 64
            assert (W >= 12) == (family == 'deconv_tiled')
            if family == 'deconv_tiled':
                fold = (min(8, 128 // cout),)
        else:
            assert ops.deconv_up_ok(cin, cout) and bool(lib.atvs_deconv_up_b_supported(cin, cout))
        assert ops.split_on('upb') == (bar is SPLIT)
        if summed:
            a = _pending((G, D, H, W, cin), 51, 53, regime, dev, True)
            b = _pending((G, D, H, W, cin), 54, 55, regime, dev, False)
            src = ops.PendingSum([a, b])
            assert ops.deconv_sum_ok(src, cout, G)
            terms = [a, b]
        else:
            x = _input((G, D, H, W, cin), 51, regime, grouped=True)
            terms, src = [x], _dev(x, dev)
        y, st = ops.conv3d_transpose_s2(src, name, w.numpy(), relu=True, want_stats=True, groups=G)

        def op(*a):
            xs, w = a[:-1], a[-1]
            s = xs[0] if len(xs) == 1 else xs[0] + xs[1]
            return _relu(T.conv3d_transpose_same(s, w))
        return [Case(y.cpu(), N.ref64(op, *terms, w), _cond(regime)(op, *terms, w), N.floor_of(w.permute(0, 1, 2, 4, 3), bar),
                     stats=(st, y, cout), fold=fold)]
    return Row(name, family, split, bar, run, cfg or {}, summed, 'deconv_row')


def aanet_row(name, nv, D, H, W):
    def run(dev, regime):
        from atvsnet_amd import ops
        X = _input((nv, D, H, W, 8), 61, regime)
        ws, wu = _weights((3, 3, 3, 8, 8), 62), _weights((3, 3, 3, 8, 8), 63)
        xs = [_dev(X[n], dev) for n in range(nv)]
        assert ops.aanet_fused_ok(xs)
        y = ops.aanet_fused(xs, name, ws.numpy(), wu.numpy())
        Wd = {'a/attention_activation/weight_unique': wu.double(), 'a/attention_activation/weight_shared': ws.double()}
        want = nets.attention_aggregation(X.double().permute(1, 2, 3, 4, 0).unsqueeze(0), Wd, 'a')[0]
        # the linearised bound of the score convolutions' errors through the softmax (numerics.aanet_cond); with one view the
        # softmax is identically 1 and the row checks the pass-through of X alone
        cnd, spread = N.aanet_cond(X, ws, wu)
        return [Case(y.cpu(), want, cnd, 2.0 * N.floor_of(torch.cat([ws, wu], -1), SPLIT) * spread)]
    return Row(name, 'aanet_b', 'aanet_b', SPLIT, run, {}, False, 'aanet_row')


def aanet_fp32_row(name, nv, D, H, W, parts=None):
    """The AANet module as the fp32 path runs it (cnn_wrapper/network.py attention_aggregation): the shared | unique 8 -> 16
    score convolution of every view on conv_c16, then ops.aanet_combine (csrc/aanet.hip).  atvs_aanet_combine launches
    aanet_combine_kernel<nv> (every operand read once, kept in registers) for nv <= 8 and aanet_combine_generic_kernel (the
    operands re-read per pass) for 9 <= nv <= 16; neither the ABI nor a predicate says which ran, so the rows' view counts
    1, 2, 5, 8 | 16 straddle that switch statement.  parts: the same views split over ranks, the three ops.aanet_partial
    stages reduced as the all-reduces would (SUM, MAX, SUM) and ops.divide, held to the same bound."""
    def run(dev, regime):
        from atvsnet_amd import ops
        X = _input((nv, D, H, W, 8), 61, regime)
        ws, wu = _weights((3, 3, 3, 8, 8), 62), _weights((3, 3, 3, 8, 8), 63)
        w16 = torch.cat([ws, wu], -1)
        xs = [_dev(X[n], dev) for n in range(nv)]
        assert not ops.aanet_fused_ok(xs)
        assert ops.conv_plan((D, H, W), 3, 8, 16)[:2] == ('c16', False)
        srs = [ops.conv(x, name, w16.numpy(), relu=True) for x in xs]
        y = ops.aanet_combine(srs, xs)
        Wd = {'a/attention_activation/weight_unique': wu.double(), 'a/attention_activation/weight_shared': ws.double()}
        want = nets.attention_aggregation(X.double().permute(1, 2, 3, 4, 0).unsqueeze(0), Wd, 'a')[0]
        cnd, spread = N.aanet_cond(X, ws, wu)
        floor = 2.0 * N.floor_of(w16, FP32_MFMA) * spread
        out = [Case(y.cpu(), want, cnd, floor)]
        if parts:
            assert sum(parts) == nv
            sl = [slice(sum(parts[:i]), sum(parts[:i + 1])) for i in range(len(parts))]
            ssum = torch.stack([ops.aanet_partial(srs[s], xs[s], 0) for s in sl], 0).sum(0)
            umax = torch.stack([ops.aanet_partial(srs[s], xs[s], 1, ssum=ssum) for s in sl], 0).max(0).values
            acc = torch.stack([ops.aanet_partial(srs[s], xs[s], 2, ssum=ssum, umax=umax) for s in sl], 0).sum(0)
            out.append(Case(ops.divide(acc[1].contiguous(), acc[0].contiguous()).cpu(), want, cnd, floor))
        return out
    return Row(name, 'aanet_combine', None, FP32_MFMA, run, FP32, False, 'aanet_fp32_row')


def stem_row(name, G, D, H, W, cin):
    def run(dev, regime):
        from atvsnet_amd import ops
        x = _input((G, D, H, W, cin), 71, regime, grouped=True)
        w = _weights((3, 3, 3, cin, 8), 72)
        assert ops.conv_plan((D, H, W), 3, cin, 8).family == 'stem'
        y, st = ops.conv(_dev(x, dev), name, w.numpy(), want_stats=True, groups=G)

        def op(x, w):
            return T.conv(x, w, 1, 'SAME')
        return [Case(y.cpu(), N.ref64(op, x, w), N.cond(op, x, w), N.floor_of(w, FP32_MFMA), stats=(st, y, 8))]
    return Row(name, 'stem', None, FP32_MFMA, run, {}, False, 'stem_row')


def refine_stems_row(name, G, D, H, W):
    def run(dev, regime):
        from atvsnet_amd import ops
        photo = _input((G, D, H, W, 8), 81, regime, grouped=True)
        geo, prob, hull = (_input((G, D, H, W, c), 82 + i, regime, grouped=True) for i, c in enumerate((2, 1, 1)))
        wg, wp, wh = _weights((3, 3, 3, 2, 8), 85), _weights((3, 3, 3, 1, 8), 86), _weights((3, 3, 3, 1, 8), 87)
        buf, st = ops.refine_stems(_dev(photo, dev), _dev(geo, dev), None, _dev(prob, dev), _dev(hull, dev), name,
                                   wg.numpy(), wp.numpy(), wh.numpy())
        assert torch.equal(buf[..., :8].cpu(), photo)

        def op(geo, prob, hull, wg, wp, wh):
            return torch.cat([T.conv(geo, wg, 1, 'SAME'), T.conv(prob, wp, 1, 'SAME'), T.conv(hull, wh, 1, 'SAME')], -1)
        a = (geo, prob, hull, wg, wp, wh)
        return [Case(buf[..., 8:].cpu(), N.ref64(op, *a), N.cond(op, *a), N.floor_of(wg, FP32_MFMA),
                     stats=(st, buf[..., 8:], 24))]
    return Row(name, 'refine_stems', None, FP32_MFMA, run, {}, False, 'refine_stems_row')


def head_row(name, G, D, H, W, summed=False):
    def run(dev, regime):
        from atvsnet_amd import ops
        w = _weights((3, 3, 3, 8, 1), 92)
        if summed:
            a = _pending((G, D, H, W, 8), 91, 93, regime, dev, True)
            b = _pending((G, D, H, W, 8), 94, 95, regime, dev, True)
            src = ops.PendingSum([a, b])
            assert src.two_pending() is not None and ops.cfg.head_sum and ops.cfg.sum_on_load
            terms = [a, b]
        else:
            x = _input((G, D, H, W, 8), 91, regime, grouped=True)
            terms, src = [x], _dev(x, dev)
        y = ops.conv3d_8to1(src, w.reshape(-1).to(dev), groups=G)

        def op(*a):
            xs, w = a[:-1], a[-1]
            return T.conv(xs[0] if len(xs) == 1 else xs[0] + xs[1], w, 1, 'SAME')
        return [Case(y.cpu(), N.ref64(op, *terms, w), _cond(regime)(op, *terms, w), N.floor_of(w, FP32_MFMA))]
    return Row(name, '8to1', None, FP32_MFMA, run, {}, summed, 'head_row')


ROWS = [
    # ---- split-operand forms (the default configuration)
    conv_row('c16b_cin16_G3_D2', 'c16b', 'c16b', SPLIT, 3, (2, 9, 13), 16, 16),
    conv_row('c16b_cin8_D1_W12', 'c16b', 'c16b', SPLIT, 1, (1, 7, 12), 8, 16),
    conv_row('c16b_sum', 'c16b_sum', 'c16b', SPLIT, 2, (3, 8, 14), 16, 16, lazy='sum'),
    conv_row('c3b_cin48_G3', 'c3b', 'c3b', SPLIT, 3, (2, 9, 13), 48, 32),
    conv_row('c3b_cin32_64', 'c3b', 'c3b', SPLIT, 1, (4, 6, 17), 32, 64),
    conv_row('c3b_norm', 'c3b_norm', 'c3b', SPLIT, 2, (3, 7, 12), 32, 32, lazy='bn'),
    conv_row('s2b_cin16_G3_Wo8', 's2b', 's2b', SPLIT, 3, (4, 9, 15), 16, 32, stride=2),
    conv_row('s2b_cin48_64', 's2b', 's2b', SPLIT, 1, (3, 8, 17), 48, 64, stride=2),
    conv_row('s2b_norm', 's2b_norm', 's2b', SPLIT, 2, (5, 6, 16), 32, 32, stride=2, lazy='bn'),
    conv_row('c2b_G3', 'conv2d_lds', 'c2b', SPLIT, 3, (8, 16), 32, 32),
    conv_row('c2b_ragged', 'conv2d_lds', 'c2b', SPLIT, 1, (9, 37), 64, 64),
    conv_row('c2b_dil2', 'conv2d_lds', 'c2b', SPLIT, 1, (10, 18), 128, 128, dilation=2),
    conv_row('c2b_tiny', 'conv2d_lds', 'c2b', SPLIT, 2, (3, 5), 32, 32),
    conv_row('c2b_on_load', 'conv2d_lds', 'c2b', SPLIT, 2, (8, 20), 32, 64, lazy='bn'),
    conv_row('c2b_stride2', 'conv2d_b_s2', 'c2b', SPLIT, 1, (16, 32), 32, 64, stride=2, explicit_pad=((1, 1), (1, 1)),
             slice_out=False),
    tail_row('c2b_tail_dil2', 1, 8, 16, 128, 2),
    conv_row('c1b_G3', 'conv1x1', 'c1b', SPLIT, 3, (5, 13), 64, 32, k=1),
    conv_row('c1b_on_load', 'conv1x1', 'c1b', SPLIT, 1, (7, 9), 32, 128, k=1, lazy='bn'),
    bottleneck_row('btl_G2', 2, 8, 16, 32),
    conv_row('xb_cin24_G2_W24', 'xp', 'xb', SPLIT, 2, (2, 5, 24), 24, 8),
    conv_row('xb_cin8_D1', 'xp', 'xb', SPLIT, 1, (1, 4, 25), 8, 8),
    siblings_row('xb_siblings', 2, 3, 6, 24, 16, SPLIT),
    siblings_row('xb_siblings_norm', 2, 3, 6, 24, 16, SPLIT, lazy='bn'),
    siblings_row('xb_siblings_sum', 2, 3, 5, 25, 8, SPLIT, lazy='sum'),
    plane_row('xb_plane_bias', 2, 3, 5, 26, 8, 3, SPLIT),
    into_plane_row('xb_into_plane', 2, 3, 5, 26, 16, 3, False),
    into_plane_row('xb_into_plane_pieces', 2, 3, 5, 26, 16, 3, True),
    deconv_row('upb_cin16', 'deconv_up_b', 'upb', SPLIT, 2, 3, 4, 6, 16, 8),
    deconv_row('upb_cin32_16_G3', 'deconv_up_b', 'upb', SPLIT, 3, 2, 3, 5, 32, 16),
    deconv_row('upb_halves_64_32', 'deconv_halves', 'upb', SPLIT, 1, 2, 3, 4, 64, 32),
    deconv_row('upb_sum', 'deconv_up_b_sum', 'upb', SPLIT, 2, 3, 4, 6, 16, 8, summed=True),
    aanet_row('aanet_b_nv1', 1, 2, 5, 12),
    aanet_row('aanet_b_nv2', 2, 3, 4, 13),
    aanet_row('aanet_b_nv5', 5, 2, 3, 12),
    aanet_row('aanet_b_nv8', 8, 2, 3, 14),
    # ---- just below a split family's threshold: another (fp32) family takes the shape
    conv_row('below_c16_W11_gather', 'gather', None, FP32_MFMA, 1, (3, 9, 11), 16, 16),
    conv_row('tiled_cin24_16', 'tiled', None, FP32_MFMA, 2, (3, 9, 14), 24, 16),
    conv_row('below_s2b_Wo7_gather', 'gather', None, FP32_MFMA, 1, (3, 6, 13), 16, 32, stride=2),
    conv_row('below_xp_cin19_xpair_tiled', 'xpair_tiled', None, FP32_MFMA, 1, (3, 8, 24), 19, 8),
    conv_row('below_xp_W23_tiled', 'tiled', None, FP32_MFMA, 2, (2, 5, 23), 24, 8),
    conv_row('below_c2b_s2_H14_gather', 'gather', None, FP32_MFMA, 1, (14, 32), 32, 64, stride=2,
             explicit_pad=((1, 1), (1, 1)), slice_out=False),
    conv_row('below_c2b_s2_W30_gather', 'gather', None, FP32_MFMA, 1, (16, 30), 32, 64, stride=2,
             explicit_pad=((1, 1), (1, 1)), slice_out=False),
    conv_row('gather_cin24_W10', 'gather', None, FP32_MFMA, 2, (3, 5, 10), 24, 8),
    # ---- the fp32 forms (ops.configure(split16=False)): what the overflow recompute runs
    conv_row('fp32_c16_G3', 'c16', None, FP32_MFMA, 3, (2, 9, 13), 16, 16, cfg=FP32),
    conv_row('fp32_c16_cin48', 'c16', None, FP32_MFMA, 1, (2, 9, 13), 48, 32, cfg=FP32),
    conv_row('fp32_tiled_64', 'tiled', None, FP32_MFMA, 1, (4, 6, 17), 32, 64, cfg=FP32),
    conv_row('fp32_gather_s2', 'gather', None, FP32_MFMA, 3, (4, 9, 15), 16, 32, stride=2, cfg=FP32),
    conv_row('fp32_conv2d_lds', 'conv2d_lds', None, FP32_MFMA, 3, (8, 16), 32, 32, cfg=FP32),
    conv_row('fp32_conv1x1', 'conv1x1', None, FP32_MFMA, 3, (5, 13), 64, 32, k=1, cfg=FP32),
    conv_row('fp32_xw', 'xp', None, FP32_MFMA, 2, (2, 5, 24), 24, 8, cfg=FP32, winograd=True),
    siblings_row('fp32_xw_siblings', 2, 3, 6, 24, 16, FP32_MFMA, cfg=FP32),
    deconv_row('fp32_deconv_up', 'deconv_up', None, FP32_MFMA, 2, 3, 4, 6, 16, 8, cfg=FP32),
    # the fp32 twins of the split rows above, at their shapes.  Where the fp32 plan sends a shape to another family than its
    # split twin's (the tiny map and the strided conv2 go to gather: their conv2d_lds / conv2d_b_s2 forms are split-operand
    # only), the row asserts the family the fp32 path launches
    conv_row('fp32_conv1x1_on_load', 'conv1x1', None, FP32_MFMA, 1, (7, 9), 32, 128, k=1, lazy='bn', cfg=FP32),
    conv_row('fp32_conv1x1_on_load_G3', 'conv1x1', None, FP32_MFMA, 3, (5, 13), 64, 32, k=1, lazy='bn', cfg=FP32),
    conv_row('fp32_conv1x1_residual', 'conv1x1', None, FP32_MFMA, 2, (8, 16), 32, 32, k=1, relu=False, residual=True,
             slice_out=False, cfg=FP32),          # the kernel takes a residual only with the output at channel 0
    conv_row('fp32_conv2d_lds_dil2', 'conv2d_lds', None, FP32_MFMA, 1, (10, 18), 128, 128, dilation=2, cfg=FP32),
    conv_row('fp32_conv2d_lds_ragged', 'conv2d_lds', None, FP32_MFMA, 1, (9, 37), 64, 64, cfg=FP32),
    conv_row('fp32_tiny_gather', 'gather', None, FP32_MFMA, 2, (3, 5), 32, 32, cfg=FP32),
    conv_row('fp32_stride2_gather', 'gather', None, FP32_MFMA, 1, (16, 32), 32, 64, stride=2, explicit_pad=((1, 1), (1, 1)),
             slice_out=False, cfg=FP32),
    conv_row('fp32_c16_cin8_16', 'c16', None, FP32_MFMA, 1, (2, 5, 12), 8, 16, cfg=FP32),
    conv_row('fp32_c16_G3_D1', 'c16', None, FP32_MFMA, 3, (1, 7, 13), 16, 16, cfg=FP32),
    deconv_row('fp32_deconv_up_32_16_G3', 'deconv_up', None, FP32_MFMA, 3, 2, 3, 5, 32, 16, cfg=FP32),
    deconv_row('fp32_deconv_64_32', 'deconv_gather', None, FP32_MFMA, 1, 2, 3, 4, 64, 32, cfg=FP32),
    deconv_row('fp32_deconv_64_32_W12', 'deconv_tiled', None, FP32_MFMA, 1, 2, 3, 12, 64, 32, cfg=FP32),
    plane_row('fp32_xw_plane_bias', 2, 3, 5, 26, 8, 3, FP32_MFMA, cfg=FP32),
    siblings_row('fp32_xw_siblings_norm', 2, 3, 6, 24, 16, FP32_MFMA, cfg=FP32, lazy='bn'),
    siblings_row('fp32_xw_siblings_sum', 2, 3, 5, 25, 8, FP32_MFMA, cfg=FP32, lazy='sum'),
    residual_unit_row('fp32_unit_G2', 2, 8, 16, 32, 1),
    residual_unit_row('fp32_unit_dil2', 1, 8, 16, 128, 2),
    aanet_fp32_row('fp32_aanet_nv1', 1, 2, 5, 12),
    aanet_fp32_row('fp32_aanet_nv2', 2, 3, 4, 13),
    aanet_fp32_row('fp32_aanet_nv5', 5, 2, 3, 12, parts=(2, 3)),
    aanet_fp32_row('fp32_aanet_nv8', 8, 2, 3, 14, parts=(4, 4)),
    aanet_fp32_row('fp32_aanet_nv16', 16, 2, 3, 13),
    stem_row('stem_cin2_G3', 3, 3, 5, 12, 2),
    stem_row('stem_cin1', 1, 2, 9, 33, 1),
    refine_stems_row('refine_stems_G2', 2, 3, 9, 35),
    head_row('8to1_G3', 3, 3, 5, 9),
    head_row('8to1_sum', 2, 4, 6, 10, summed=True),
]
_WORST = {}


@pytest.mark.parametrize('row', ROWS, ids=[r.name for r in ROWS])
def test_elementwise_against_float64(cuda, row):
    from atvsnet_amd import ops
    with ops.configure(clear_pack_cache=True, **row.cfg):
        ops.nonfinite_seen(cuda)                           # reset the sticky flag
        for regime in REGIMES + ((OFFSET,) if row.lazy else ()):
            N.poison_allocator(cuda)
            cases = row.run(cuda, regime)
            torch.cuda.synchronize()
            for i, c in enumerate(cases):
                what = '%s[%s]#%d' % (row.name, regime, i)
                rel = row.bar.rel * (N.NEAR_MAX if regime == 'near_max' else 1.0) + (OFFSET_REL if regime == OFFSET else 0.0)
                r = N.assert_elementwise(c.got, c.want64, c.cond64, rel, c.floor, what)
                key = (row.family, 'split' if row.bar is SPLIT else 'fp32', regime)
                _WORST[key] = max(_WORST.get(key, 0.0), r)
                print('%-28s %-10s err/cond %.2e' % (row.name, regime, r))
                if c.kept is not None:
                    N.assert_bits_kept(*c.kept)
                if c.stats is not None:
                    _check_stats(c.stats[0], c.stats[1], c.stats[2], what, c.fold)
    ops.clear_pack_cache()


def test_fp32_conv2d_lds_refuses_a_lazy_input(cuda):
    """The fp32 twin of c2b_on_load, (8, 20), 32 -> 64: conv2d_lds.hip has no on-load form (conv2d_b.hip's is split-operand
    only), so the plan keeps the family and says so, norm_on_load_2d_ok sends the network to a bn_apply pass, and ops.conv
    refuses the pending input instead of convolving the raw one."""
    from atvsnet_amd import ops
    with ops.configure(clear_pack_cache=True, **FP32):
        pend = _pending((2, 8, 20, 32), 1, 4, 'randn', cuda, True)
        assert ops.conv_plan((8, 20), 3, 32, 64, bias=True, lazy='bn')[:2] == ('conv2d_lds', False)
        assert not ops.norm_on_load_2d_ok(pend, 3, 64)
        with pytest.raises(ValueError, match='no normalise-on-load form'):
            ops.conv(pend.raw, 'fp32_conv2d_lds_on_load', _weights((3, 3, 32, 64), 2).numpy(), groups=2,
                     in_params=pend.params, in_relu=True)
    ops.clear_pack_cache()


@pytest.fixture(scope='module', autouse=True)
def _report():
    """After the rows: the largest err / cond per family and regime (what tests/numerics.py's constants were set from)."""
    yield
    for cls in ('split', 'fp32'):
        keys = sorted(k for k in _WORST if k[1] == cls)
        if not keys:
            continue
        print('\n%s: largest err/cond %.2e' % (cls, max(_WORST[k] for k in keys)))
        for fam in sorted({k[0] for k in keys}):
            print('  %-16s ' % fam + ' '.join('%s %.1e' % (reg, _WORST[(fam, cls, reg)]) for reg in REGIMES + (OFFSET,)
                                              if (fam, cls, reg) in _WORST))
