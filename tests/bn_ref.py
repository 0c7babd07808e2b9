"""The float64 reference and the per-element bar of the batch-norm transform, shared by
tests/test_bn_ref_host.py (CPU), tests/test_gpu_batch_norm.py and tests/test_gpu_split_precision.py (-m gpu).

Every kernel that normalises computes, from float32 parameters (mean m, rstd s, beta b) of the value's sample and channel,

    shift = fl(fma(-m, s, b))        once per channel      (atvs_bn_shift, csrc/common.h)
    y     = fl(fma(x, s, shift))     once per value        (atvs_bn1)

The bound.  With u = 2^-24: shift is one rounding of b - m s, so |shift - (b - m s)| <= u |b - m s| <= u (|m s| + |b|).
y is one rounding of x s + shift, so |y - (x s + shift)| <= u |x s + shift| <= u (|x s| + |m s| + |b|) (1 + u).  Together

    |y - bn64| <= u (|x s| + 2 |m s| + 2 |b|)  <=  2 u * bn_cond,        bn_cond = |x s| + |m s| + |b|,

and a ReLU (max with 0 of both sides) does not enlarge the error.  The error is absolute in |m s|, not relative to |y|: where a
channel's mean is 1e4 standard deviations, a normalised value of size 1 may be off by 4e4 u = 2.4e-3 (a correct evaluation
measures a quarter of that).

The `offset` regime puts the operands there: raw = m_c + sigma_c * randn per channel with |m_c| log-uniform in [1e2, 1e4]
(random sign) and sigma_c uniform in [0.5, 2], so |m| / sigma runs from about 50 to 2e4; the parameters are the float32
roundings of each sample's float64 batch mean and of 1 / sqrt(var64 + float32(1e-3)), beta = 0.1 * randn.

An emulation of the two roundings (emulate_fma) on that regime gives at most 0.48 u * bn_cond (tests/test_bn_ref_host.py prints
it): there the bar of 2 u keeps a factor 4 over a correct float32 evaluation.  In the randn and small regimes (means near 0) a
value with |x s| far below |b| is its shift rounded twice, and the emulation reaches 1.9 u of the same bar.
"""
import torch

import numerics as N

U = 2.0 ** -24
APPLY_REL = 2.0 * U                  # bn_apply, and the on-load transform of one lazy convolution input
ADD_REL = 4.0 * U                    # bn_add / bn_add_plus: the transform's 2u, and u per add of the (a + b) + c chain
REGIMES = ('randn', 'small', 'offset')
EPS = 1e-3


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _full(params, raw):
    """(G,3,C) or (3,C) float parameters -> three float64 tensors broadcastable against raw (G, ..., C)."""
    par = params.detach().cpu().double()
    G, C = raw.shape[0], raw.shape[-1]
    if par.dim() == 2:
        par = par.unsqueeze(0).expand(G, -1, -1)
    bc = (G,) + (1,) * (raw.dim() - 2) + (C,)
    return par[:, 0].reshape(bc), par[:, 1].reshape(bc), par[:, 2].reshape(bc)


def bn64(raw, params, relu):
    """relu?((x - m) * s + b) in float64 from the float32 parameters (numerics.term64 of the pending batch norm)."""
    from atvsnet_amd import ops
    return N.term64(ops.PendingBN(raw.detach().cpu(), params.detach().cpu(), relu))


def bn_cond(raw, params):
    """|x s| + |m s| + |b| in float64: what the transform's rounding errors scale with."""
    x = raw.detach().cpu().double()
    m, s, b = _full(params, x)
    return (x * s).abs() + (m * s).abs() + b.abs()


def batch_params(raw, beta, eps=EPS):
    """(G,3,C) float32: per sample the roundings of the float64 batch mean and of 1 / sqrt(var64 + float32(eps)), and beta."""
    x = raw.double().reshape(raw.shape[0], -1, raw.shape[-1])
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)               # two-pass: a one-pass form cancels at |m| / sigma = 1e4
    rstd = 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))
    b = beta.double().reshape(1, -1).expand_as(mean)
    return torch.stack([mean, rstd, b], 1).float().contiguous()


def operand(regime, shape, seed):
    """(raw, params): a CPU float32 tensor (G, ..., C) of the regime and its (G,3,C) batch-norm parameters.
    randn: N(0,1); small: N(0,1) * 1e-3 (beta too); offset: see the module docstring."""
    g = _gen(seed)
    C = shape[-1]
    z = torch.randn(shape, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    if regime == 'randn':
        raw = z
    elif regime == 'small':
        raw, beta = z * 1e-3, beta * 1e-3
    elif regime == 'offset':
        mag = 10.0 ** (2.0 + 2.0 * torch.rand(C, generator=g, dtype=torch.float64))
        sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0).double()
        sigma = 0.5 + 1.5 * torch.rand(C, generator=g, dtype=torch.float64)
        raw = (mag * sign + sigma * z.double()).float()
    else:
        raise ValueError(regime)
    return raw.contiguous(), batch_params(raw, beta)


def dense(regime, shape, seed):
    """A finished (already normalised) tensor beside the pending ones: N(0,1), * 1e-3 in the small regime."""
    return torch.randn(shape, generator=_gen(seed)) * (1e-3 if regime == 'small' else 1.0)


# ------------------------------------------------------------------------------------------- the float32 arithmetic, emulated

def _fma32(a, b, c):
    """fl32(a * b + c) of float32 values held in float64: the product of two float32 is exact in float64, the sum rounds to 53
    bits and then to 24 (a double rounding that can move a result by 2^-53 relative past a tie: invisible at these bars)."""
    return (a * b + c).float().double()


def _round_bits(t, bits):
    """t (float64) rounded to `bits` significant bits, to nearest."""
    m, e = torch.frexp(t)
    return torch.ldexp(torch.round(m * 2.0 ** bits), e - bits)


DEFECTS = ('shift_fp16', 'mean_22_bits', 'sample_0_params', 'beta_dropped_on_tail')


def emulate_fma(raw, params, relu, defect=None):
    """The kernels' two fused multiply-adds in emulated float32 (float64 out), with an optional planted defect:
    shift_fp16: the shift rounded to fp16; mean_22_bits: the shift built from the mean rounded to 22 significant bits;
    sample_0_params: sample 1 normalised with sample 0's parameters; beta_dropped_on_tail: beta = 0 on the last C mod 4
    channels (the remainder a float4 loop would leave to a tail)."""
    x = raw.detach().cpu().float().double()
    par = params.detach().cpu().float().clone()
    if par.dim() == 2:
        par = par.unsqueeze(0).expand(x.shape[0], -1, -1).clone()
    C = x.shape[-1]
    if defect == 'sample_0_params':
        par[1] = par[0]
    elif defect == 'beta_dropped_on_tail':
        assert C % 4, 'the defect needs C mod 4 != 0'
        par[:, 2, C - C % 4:] = 0.0
    m, s, b = _full(par, x)
    if defect == 'mean_22_bits':
        m = _round_bits(m, 22)
    shift = _fma32(-m, s, b)
    if defect == 'shift_fp16':
        shift = shift.half().double()
    y = _fma32(x, s, shift)
    return y.clamp(min=0) if relu else y


# ---------------------------------------------------------------------------------------------------------------- sums

def term_cond(t):
    """cond of one term of a sum: bn_cond of a pending batch norm, |x| of a dense tensor."""
    from atvsnet_amd import ops
    if isinstance(t, ops.PendingBN):
        return bn_cond(t.raw, t.params)
    return t.detach().cpu().double().abs()


def sum64(items):
    """(the float64 sum of the items, the sum of their conds); items: PendingBN or dense tensors."""
    want = sum(N.term64(t) for t in items)
    return want, sum(term_cond(t) for t in items)

