"""Float64 references and per-element bars of the small kernels between the convolutions: SAME average pooling and
align-corners resize (csrc/pool.hip), and the cross-view softmax + weighted sum of the AANet module (csrc/aanet.hip).  Shared
by tests/test_glue_ref_host.py (CPU) and tests/test_gpu_glue_kernels.py (-m gpu).

Pooling.  avg_pool64 restates TF SAME pooling as plain loops.  Two bars:
  exact rows   integer-valued inputs in [-8, 8]: a window has at most 64 * 64 = 4096 elements, so every partial sum is an
               integer below 2^15 and exact in fp32 in ANY order; the one division is IEEE (the build keeps the correctly
               rounded fp32 divide), so the kernel must give float32(sum64 / count) bit for bit (pool_exact).
  random rows  |got - mean64| <= n * 2^-24 * (sum|x| / n), n the window's valid count (pool_bar): summing n numbers in fp32
               in any order is off by at most (n - 1) u sum|x| to first order (u = 2^-24), the mean by that / n, and the
               division adds u |mean| <= u sum|x| / n.  Derived, not measured.

Resize.  The source coordinate oy * scale is part of the operation's DEFINITION (TF forms it in float32; the kernel and
oracle.tf_ops do the same), so resize64 takes the float32 scale and the float32 product, and then interpolates the four
corners in float64.  What remains in the kernel is the rounding of one difference, one product and one sum in each of three
lerps (the weights fy - floor(fy) are exact), each at most u times a value bounded by the corners it blends: within
4 u (|tl| + |tr| + |bl| + |br|) (resize_bar).  The GPU test also demands the oracle's bits.

AANet combine.  |got - y64| <= REL * cond with cond from aanet_combine_cond (derivation there).  Measured on one MI355X by
tests/test_gpu_glue_kernels.py (1, 2, 3, 5, 8, 9, 12, 16 views; V = 1, 127, 129, 480; the four regimes; the sharded form
included), largest err / cond: 3.004e-7 (12 views, scores spread over 30).  Before the winning view's exponent was made exact
(2^(u log2 e - round(max log2 e)) instead of 2^((u - max) log2 e), csrc/common.h) the same rows measured 3.170e-7 and the
known-answer rows failed: one view returned X in all but 8 of 1032 values, a saturated softmax the winning X in all but ~170.
The mildest defect tests/test_glue_ref_host.py emulates -- view n weighted with view n-1's score -- reaches err / cond 2.454e-1
at its worst element in its mildest row (16 views, N(0,1) scores, V = 129).  REL = 2.0e-6 is 6.7 x the measured maximum (at
most 8 x is allowed) and 1 / 122 700 of the defect (at least 10 x is asked); both factors are asserted on the CPU.
"""
import torch

U32 = 2.0 ** -24                    # unit round-off of fp32

AANET_MEASURED = 3.004e-7           # largest err / cond of the kernels on one MI355X
AANET_DEFECT = 2.454e-1             # err / cond of the neighbouring-score defect in its mildest row (CPU, float64)
REL = 2.0e-6


# ------------------------------------------------------------------------------------------------------------------ pooling

def pool_slices(Ho, Wo):
    """SL of csrc/pool.hip: the number of partial-sum slices of one window (about 640 workgroups per image, at most 64)."""
    return max(1, min(64, 640 // (Ho * Wo)))


def pool_windows(H, W, pool, stride):
    """TF SAME windows: ((y0, y1) per output row, (x0, x1) per output column), clipped to the image.
    pad = max((Ho - 1) * s + k - H, 0), pad // 2 of it in front."""
    def axis(n):
        no = -(-n // stride)
        pad = max((no - 1) * stride + pool - n, 0)
        lo = [o * stride - pad // 2 for o in range(no)]
        return [(max(a, 0), min(a + pool, n)) for a in lo]
    return axis(H), axis(W)


def avg_pool64(x, pool, stride):
    """x (..., H, W, C) -> (mean64 (..., Ho, Wo, C), count (Ho, Wo) int64, sum|x| per window (..., Ho, Wo, C) float64):
    the mean over the in-image elements of each SAME window."""
    x = x.detach().cpu().double()
    H, W, C = x.shape[-3:]
    ys, xs = pool_windows(H, W, pool, stride)
    lead = tuple(x.shape[:-3])
    mean = torch.zeros(lead + (len(ys), len(xs), C), dtype=torch.float64)
    sabs = torch.zeros_like(mean)
    count = torch.zeros((len(ys), len(xs)), dtype=torch.int64)
    for oy, (y0, y1) in enumerate(ys):
        for ox, (x0, x1) in enumerate(xs):
            win = x[..., y0:y1, x0:x1, :].reshape(lead + (-1, C))
            n = win.shape[-2]
            count[oy, ox] = n
            mean[..., oy, ox, :] = win.sum(-2) / n
            sabs[..., oy, ox, :] = win.abs().sum(-2)
    return mean, count, sabs


def pool_exact(mean64):
    """The bits an exact row must have: float32(sum64 / count)."""
    return mean64.float()


def pool_bar(count, sabs):
    """n * 2^-24 * (sum|x| / n) per output element."""
    n = count.double().unsqueeze(-1)
    return n * U32 * (sabs / n)


def assert_within(got, want64, bar, what=''):
    """|got - want64| <= bar at every element, got finite; returns the largest err / bar."""
    got = got.detach().cpu().double()
    assert tuple(got.shape) == tuple(want64.shape), '%s: shape %s, reference %s' % (what, tuple(got.shape), tuple(want64.shape))
    err = (got - want64).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float('inf')))
    bad = err > bar
    if bool(bad.any()):
        i = int(torch.argmax((err / bar.clamp(min=1e-300)).reshape(-1)))
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), got.shape))
        raise AssertionError('%s: %d elements over the bar; element %s got %.9e, float64 %.9e, bar %.3e'
                             % (what, int(bad.sum()), idx, float(got[idx]), float(want64[idx]), float(bar[idx])))
    return float((err / bar.clamp(min=1e-300)).max())


# ------------------------------------------------------------------------------------------------------------------- resize

def _axis32(n_in, n_out):
    """(lo, hi, weight of hi) of every output coordinate: float32 scale and float32 product, as TF defines them."""
    scale = torch.tensor((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0, dtype=torch.float32)
    src = torch.arange(n_out, dtype=torch.float32) * scale
    lo = torch.floor(src).long()
    hi = torch.clamp(torch.ceil(src).long(), max=n_in - 1)
    return lo, hi, (src.double() - lo.double())


def resize64(x, size):
    """Align-corners bilinear resize of x (..., H, W, C) to (..., Ho, Wo, C) in float64 -> (y64, |tl| + |tr| + |bl| + |br|)."""
    x = x.detach().cpu().double()
    H, W, C = x.shape[-3:]
    ylo, yhi, ly = _axis32(H, int(size[0]))
    xlo, xhi, lx = _axis32(W, int(size[1]))
    ly, lx = ly.reshape(-1, 1, 1), lx.reshape(1, -1, 1)
    top, bot = x[..., ylo, :, :], x[..., yhi, :, :]
    tl, tr, bl, br = top[..., xlo, :], top[..., xhi, :], bot[..., xlo, :], bot[..., xhi, :]
    y = (1 - ly) * ((1 - lx) * tl + lx * tr) + ly * ((1 - lx) * bl + lx * br)
    return y, tl.abs() + tr.abs() + bl.abs() + br.abs()


def resize_bar(corners):
    return 4 * U32 * corners


# -------------------------------------------------------------------------------------------------------------------- AANet

def _sru(srs):
    sr = torch.stack([t.detach().cpu().double() for t in srs], 0)         # (nv, V.., 16)
    S, R = sr[..., :8], sr[..., 8:]
    return S, R, (R - S) + S.sum(0, keepdim=True)


def aanet_combine64(srs, xs):
    """The module's formula in float64: srs list of (V.., 16) [S | R], xs list of (V.., 8);
    U = (R - S) + sum_n S, p = softmax_n U, y = sum_n p_n X_n."""
    X = torch.stack([t.detach().cpu().double() for t in xs], 0)
    _, _, U = _sru(srs)
    return (torch.softmax(U, 0) * X).sum(0)


def aanet_combine_cond(srs, xs):
    """The linearised bound of the combine kernel alone (numerics.aanet_cond without the convolutions):

        cond = sum_n p_n |X_n|  +  sum_n p_n |X_n - y| (1 + |R_n - S_n| + |U_n| + |U_n - max_m U_m|)

    An error dU_n of a score moves y by sum_n p_n (X_n - y) dU_n.  An error of sum S, and the rounding of max * log2 e, shift
    every score alike and cancel (sum_n p_n (X_n - y) = 0).  What remains per view: the rounding of R - S (u |R - S|), of the
    add (u |U|), of the exponent's argument (u |U - max| times a constant near log2 e, formed as a product or as a fused
    multiply-add) and one ulp of exp2 (the 1).  The first term is the weighted sum's own rounding and the reciprocal."""
    X = torch.stack([t.detach().cpu().double() for t in xs], 0)
    S, R, U = _sru(srs)
    p = torch.softmax(U, 0)
    y = (p * X).sum(0)
    w = 1 + (R - S).abs() + U.abs() + (U - U.max(0, keepdim=True).values).abs()
    return (p * X.abs()).sum(0) + (p * (X - y).abs() * w).sum(0)


REGIMES = ('normal', 'spread30', 'spread200', 'loguniform_x')


def aanet_case(nv, V, regime, seed=0):
    """(srs, xs): nv views of [S | R] (V, 16) >= 0 (as after the ReLU) and X (V, 8), float32 on the CPU.
    normal: S, R = relu(N(0,1)), X = N(0,1).  spread30 / spread200: R uniform over [0, 30] / [0, 200] (the latter saturates
    the softmax).  loguniform_x: |X| = 2^uniform(-20, 10) with random signs, scores as normal."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * nv + V + 7 * REGIMES.index(regime))
    srs, xs = [], []
    for _ in range(nv):
        S = torch.randn(V, 8, generator=g).clamp(min=0)
        if regime in ('spread30', 'spread200'):
            R = torch.rand(V, 8, generator=g) * (30.0 if regime == 'spread30' else 200.0)
        else:
            R = torch.randn(V, 8, generator=g).clamp(min=0)
        if regime == 'loguniform_x':
            mag = torch.exp2(torch.rand(V, 8, generator=g) * 30.0 - 20.0)
            X = torch.where(torch.rand(V, 8, generator=g) < 0.5, -mag, mag)
        else:
            X = torch.randn(V, 8, generator=g)
        srs.append(torch.cat([S, R], -1).contiguous())
        xs.append(X.contiguous())
    return srs, xs
